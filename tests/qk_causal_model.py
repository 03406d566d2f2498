"""Host models of the causal Q/K statistic (mdg_qk_causal_accum), independent of the kernel.  Per sequence s of T rows, query head h,
kv = h / (n_heads / n_kv), with the prefix sums over the keys each query can see,

  K_i = sum_{j<=i} k_j k_j^T,   m_i = sum_{j<=i} k_j,   n_i = i + 1,   C_i = K_i / n_i - m_i m_i^T / n_i^2
  P_h = sum_s sum_i (q_i q_i^T) (.) C_i,        P_raw_h = sum_s sum_i (q_i q_i^T) (.) K_i / n_i

longdouble_causal   (P, P_raw, A) by that recurrence in numpy long double (x87: 64-bit mantissa); A is the scale of the header's bound,
                    A_h[a,b] = sum_s sum_i |q_ia q_ib| sqrt(K_i[a,a] K_i[b,b]) / n_i
exact_causal        on integer-valued rows: exact rational arithmetic (integers over the common denominators lcm(1..T)^2 and
                    lcm(1..T), as Python ints and Fractions), then the correctly rounded fp64 of the exact value
brute_force_causal  the explicit sums over (s, i, j <= i) of the variance / the mean square of e_ij = q_iD . k_jD, for a column set D
bound               the header's entry-wise bound (4T + B + 8) 2^-53 A
unit_scores         what mdg_qk_select ranks the rotary units by on (P, ones) with ridges 0: sum over the group of P[u,u] + P[u+ns,u+ns]
disagreement_rows   the rows of the case on which the causal and the full within-sequence rule select differently
"""
import math
from fractions import Fraction

import numpy as np
import torch

from tests.qk_pair_model import LD, U, as_ld, split_heads  # noqa: F401  (the sibling statistic's helpers: same row layout)


def longdouble_causal(q: torch.Tensor, k: torch.Tensor, B, T, n_heads, n_kv, hd):
    """(P, P_raw, A) in long double, each [n_heads, hd, hd]."""
    g = n_heads // n_kv
    Q, K = split_heads(as_ld(q), B, T, n_heads, hd), split_heads(as_ld(k), B, T, n_kv, hd)
    P = np.zeros((n_heads, hd, hd), dtype=LD)
    R = np.zeros_like(P)
    A = np.zeros_like(P)
    for s in range(B):
        for v in range(n_kv):
            Kp, m = np.zeros((hd, hd), dtype=LD), np.zeros(hd, dtype=LD)
            for i in range(T):
                n = LD(i + 1)
                kr = K[s, v, i]
                Kp = Kp + np.outer(kr, kr)
                m = m + kr
                Kn = Kp / n
                C = Kn - np.outer(m, m) / (n * n)
                d = np.sqrt(np.diagonal(Kp))
                kap = np.outer(d, d) / n
                for h in range(v * g, (v + 1) * g):
                    qq = np.outer(Q[s, h, i], Q[s, h, i])
                    P[h] += qq * C
                    R[h] += qq * Kn
                    A[h] += np.abs(qq) * kap
    return P, R, A


def bound(A, B, T):
    """The header's entry-wise bound on |pair - exact| (and on |pair_raw - exact|) for a pair that held zero."""
    return (4 * T + B + 8) * U * A


def exact_causal(q: torch.Tensor, k: torch.Tensor, B, T, n_heads, n_kv, hd):
    """Integer-valued rows: (P, P_raw) as fp64 tensors holding the CORRECTLY ROUNDED exact values.  With L = lcm(1 .. T),
    P = sum_n [ sum_s qq (n K - m m^T) ]_{i = n - 1} / n^2 and P_raw = sum_n [ sum_s qq K ] / n; the brackets are exact in int64, the
    sums over n are taken as Python ints over L^2 (L), and float(Fraction(numerator, denominator)) rounds once."""
    g = n_heads // n_kv
    qi, ki = (x.detach().cpu().to(torch.float64).numpy() for x in (q, k))
    assert (qi == np.rint(qi)).all() and (ki == np.rint(ki)).all(), "exact_causal takes integer-valued rows"
    assert np.abs(qi).max(initial=0) <= 64 and np.abs(ki).max(initial=0) <= 64 and T <= 4096 and B <= 64, "int64 brackets"
    Q = split_heads(qi.astype(np.int64), B, T, n_heads, hd)
    K = split_heads(ki.astype(np.int64), B, T, n_kv, hd)
    L = 1
    for n in range(1, T + 1):
        L = L * n // math.gcd(L, n)
    num = np.zeros((n_heads, hd, hd), dtype=object)
    num_raw = np.zeros((n_heads, hd, hd), dtype=object)
    Kp = np.zeros((B, n_kv, hd, hd), dtype=np.int64)
    m = np.zeros((B, n_kv, hd), dtype=np.int64)
    for i in range(T):
        n = i + 1
        kr = K[:, :, i]                                                     # [B, n_kv, hd]
        Kp += kr[..., :, None] * kr[..., None, :]
        m += kr
        cen = n * Kp - m[..., :, None] * m[..., None, :]                    # n^2 C_i, [B, n_kv, hd, hd]
        qr = Q[:, :, i]
        qq = qr[..., :, None] * qr[..., None, :]                            # [B, n_heads, hd, hd]
        s_c = (qq * np.repeat(cen, g, axis=1)).sum(0)                       # the bracket of n, [n_heads, hd, hd]
        s_r = (qq * np.repeat(Kp, g, axis=1)).sum(0)
        num = num + s_c.astype(object) * ((L // n) ** 2)
        num_raw = num_raw + s_r.astype(object) * (L // n)
    out = []
    for M_, den in ((num, L * L), (num_raw, L)):
        vals = [float(Fraction(int(v), den)) for v in M_.reshape(-1)]
        out.append(torch.tensor(vals, dtype=torch.float64).reshape(n_heads, hd, hd))
    return out[0], out[1]


def exact_causal_fractions(q, k, B, T, n_heads, n_kv, hd):
    """The same values, token by token in Fractions (slow: small shapes only) -- the check of exact_causal's bookkeeping."""
    g = n_heads // n_kv
    Q = split_heads(q.detach().cpu().to(torch.float64).numpy().astype(np.int64), B, T, n_heads, hd)
    K = split_heads(k.detach().cpu().to(torch.float64).numpy().astype(np.int64), B, T, n_kv, hd)
    P = [[[Fraction(0)] * hd for _ in range(hd)] for _ in range(n_heads)]
    R = [[[Fraction(0)] * hd for _ in range(hd)] for _ in range(n_heads)]
    for s in range(B):
        for h in range(n_heads):
            Kp = [[0] * hd for _ in range(hd)]
            m = [0] * hd
            for i in range(T):
                n = i + 1
                kr, qr = [int(x) for x in K[s, h // g, i]], [int(x) for x in Q[s, h, i]]
                for a in range(hd):
                    m[a] += kr[a]
                for a in range(hd):
                    for b in range(hd):
                        Kp[a][b] += kr[a] * kr[b]
                        P[h][a][b] += Fraction(qr[a] * qr[b] * (n * Kp[a][b] - m[a] * m[b]), n * n)
                        R[h][a][b] += Fraction(qr[a] * qr[b] * Kp[a][b], n)
    f = lambda X: torch.tensor([[[float(v) for v in row] for row in mat] for mat in X], dtype=torch.float64)   # noqa: E731
    return f(P), f(R)


def brute_force_causal(q, k, B, T, n_heads, n_kv, hd, D):
    """Per query head: (sum_s sum_i Var_{j<=i}(e_ij), sum_s sum_i mean_{j<=i}(e_ij^2)), e_ij = q_iD . k_jD, in long double."""
    g = n_heads // n_kv
    Q, K = split_heads(as_ld(q), B, T, n_heads, hd), split_heads(as_ld(k), B, T, n_kv, hd)
    D = list(D)
    var, ms = np.zeros(n_heads, dtype=LD), np.zeros(n_heads, dtype=LD)
    for s in range(B):
        for h in range(n_heads):
            e = Q[s, h][:, D] @ K[s, h // g][:, D].T          # [i, j]
            for i in range(T):
                row = e[i, :i + 1]
                var[h] += ((row - row.mean()) ** 2).mean()
                ms[h] += (row ** 2).mean()
    return var, ms


def unit_scores(P, n_kv):
    """[n_kv, ns]: sum over the kv head's group of P_h[u,u] + P_h[u+ns,u+ns] -- mdg_qk_select's score of rotary unit u on (P, ones)
    with ridges 0, up to the monotone square root of the grouped mode."""
    H, hd = P.shape[0], P.shape[1]
    g, ns = H // n_kv, hd // 2
    d = np.stack([np.diagonal(P[h]) for h in range(H)])                     # [H, hd]
    unit = d[:, :ns] + d[:, ns:]
    return unit.reshape(n_kv, g, ns).sum(1)


# the disagreement case: B 2, T 24, 2 query heads on 1 kv head of 16, rotary units (u, u + 8); unit SPECIAL carries a key amplitude
# on a few tokens only
DIS = dict(B=2, T=24, H=2, KV=1, hd=16, special=3)


def disagreement_rows(where: str, amplitude: float, seed: int = 5, T: int = 0):
    """(q, k) bf16 rows [B*T, H*hd], [B*T, KV*hd].  Queries: unit Gaussians.  Keys: Gaussians of scale 4 on every unit but SPECIAL,
    whose two columns are 0.01-scale Gaussians except on the last two tokens of every sequence (where = "late": +amplitude, then
    -amplitude) or on token 0 (where = "first": +amplitude)."""
    B, H, KV, hd, sp = (DIS[n] for n in ("B", "H", "KV", "hd", "special"))
    T = T or DIS["T"]
    ns = hd // 2
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B * T, H * hd, generator=gen, dtype=torch.float64)
    k = 4.0 * torch.randn(B * T, KV * hd, generator=gen, dtype=torch.float64)
    for col in (sp, sp + ns):
        k[:, col] = 0.01 * torch.randn(B * T, generator=gen, dtype=torch.float64)
        for s in range(B):
            if where == "late":
                k[s * T + T - 2, col] = amplitude
                k[s * T + T - 1, col] = -amplitude
            elif where == "first":
                k[s * T, col] = amplitude
            else:
                raise ValueError(where)
    return q.to(torch.bfloat16), k.to(torch.bfloat16)


def margins(score, special, keep):
    """(rank of `special` in the descending order, score[special] / the best score among the other units that are dropped when
    special is kept, i.e. the keep-th best of the others, ... / the weakest kept of the others when special is dropped, the same
    unit): one ratio, >= 1 means special is among the `keep` kept, <= 1 among the dropped."""
    others = sorted((float(x) for u, x in enumerate(score) if u != special), reverse=True)
    rank = sorted(range(len(score)), key=lambda u: (-float(score[u]), u)).index(special)
    return rank, float(score[special]) / others[keep - 1]
