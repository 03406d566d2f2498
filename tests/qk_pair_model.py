"""Host models of the within-sequence Q/K statistic (mdg_qk_pair_accum), independent of the kernel:

  P_h     = sum_s G^q_{s,h} (.) (G^k_{s,kv} - m_s m_s^T / T),   P_raw_h = sum_s G^q_{s,h} (.) G^k_{s,kv},
  G^q = Q^T Q, G^k = K^T K, m = K^T 1 per sequence s, kv = h / (n_heads / n_kv)

longdouble_pair  the same expression in numpy long double (x87: 64-bit mantissa), plus the scale of the header's bound
exact_pair       on integer-valued rows: T P and P_raw as Python ints (no rounding anywhere), then the fp64 values
brute_force      the explicit sums over (s, i, j) of the variance / the mean square of e_ij = q_iD . k_jD, for a column set D
bound            the header's entry-wise bound (4T + B + 8) 2^-53 sum_s sqrt(G^q_aa G^q_bb) sqrt(G^k_aa G^k_bb)
"""
from fractions import Fraction

import numpy as np
import torch

LD = np.longdouble
U = 2.0 ** -53


def as_ld(x: torch.Tensor):
    """bf16 / f16 / f32 tensor -> long double array, exactly."""
    return x.detach().cpu().to(torch.float64).numpy().astype(LD)


def split_heads(x, B, T, heads, hd):
    """[B*T, heads*hd] -> [B, heads, T, hd]"""
    return x.reshape(B, T, heads, hd).transpose(0, 2, 1, 3)


def longdouble_pair(q: torch.Tensor, k: torch.Tensor, B, T, n_heads, n_kv, hd):
    """(P, P_raw, scale) in long double, each [n_heads, hd, hd]; scale = sum_s sqrt(G^q_aa G^q_bb) sqrt(G^k_aa G^k_bb)."""
    g = n_heads // n_kv
    Q, K = split_heads(as_ld(q), B, T, n_heads, hd), split_heads(as_ld(k), B, T, n_kv, hd)
    P = np.zeros((n_heads, hd, hd), dtype=LD)
    R = np.zeros_like(P)
    S = np.zeros_like(P)
    for s in range(B):
        gk, mk = [], []
        for v in range(n_kv):
            gk.append(K[s, v].T @ K[s, v])
            mk.append(K[s, v].sum(0))
        for h in range(n_heads):
            gq = Q[s, h].T @ Q[s, h]
            kk, m = gk[h // g], mk[h // g]
            P[h] += gq * (kk - np.outer(m, m) / LD(T))
            R[h] += gq * kk
            dq, dk = np.sqrt(np.diagonal(gq)), np.sqrt(np.diagonal(kk))
            S[h] += np.outer(dq, dq) * np.outer(dk, dk)
    return P, R, S


def bound(scale, B, T):
    """The header's entry-wise bound on |pair - exact| (and on |pair_raw - exact|) for a pair that held zero."""
    return (4 * T + B + 8) * U * scale


def exact_pair(q: torch.Tensor, k: torch.Tensor, B, T, n_heads, n_kv, hd):
    """Integer-valued rows: (P, P_raw) as fp64 tensors holding the EXACT values (asserted representable), from T P and P_raw in
    Python ints."""
    g = n_heads // n_kv
    qi, ki = (x.detach().cpu().to(torch.float64).numpy() for x in (q, k))
    assert (qi == np.rint(qi)).all() and (ki == np.rint(ki)).all(), "exact_pair takes integer-valued rows"
    Q = split_heads(qi.astype(np.int64), B, T, n_heads, hd)
    K = split_heads(ki.astype(np.int64), B, T, n_kv, hd)
    TP = np.zeros((n_heads, hd, hd), dtype=object)
    R = np.zeros((n_heads, hd, hd), dtype=object)
    for s in range(B):
        for h in range(n_heads):
            gq = (Q[s, h].T @ Q[s, h]).astype(object)
            kv = K[s, h // g]
            gk, m = (kv.T @ kv).astype(object), kv.sum(0).astype(object)
            TP[h] = TP[h] + gq * (gk * int(T) - np.outer(m, m))
            R[h] = R[h] + gq * gk
    out = []
    for M, den in ((TP, int(T)), (R, 1)):
        flat = [int(v) for v in M.reshape(-1)]
        vals = [float(v) / den for v in flat]
        assert all(abs(v) < 2 ** 53 for v in flat) and all(Fraction(x) * den == v for x, v in zip(vals, flat)), "not exact in fp64"
        out.append(torch.tensor(vals, dtype=torch.float64).reshape(n_heads, hd, hd))
    return out[0], out[1]


def brute_force(q, k, B, T, n_heads, n_kv, hd, D):
    """Per query head: (sum_s sum_i sum_j (e_ij - mean_j e_ij)^2, sum_s sum_i sum_j e_ij^2), e_ij = q_iD . k_jD, in long double."""
    g = n_heads // n_kv
    Q, K = split_heads(as_ld(q), B, T, n_heads, hd), split_heads(as_ld(k), B, T, n_kv, hd)
    D = list(D)
    var, ms = np.zeros(n_heads, dtype=LD), np.zeros(n_heads, dtype=LD)
    for s in range(B):
        for h in range(n_heads):
            e = Q[s, h][:, D] @ K[s, h // g][:, D].T          # [i, j]
            var[h] += ((e - e.mean(1, keepdims=True)) ** 2).sum()
            ms[h] += (e ** 2).sum()
    return var, ms


def lattice_rows(B, T, heads, hd, seed, offset=0):
    """Integer rows with |x| <= 8 (plus a constant offset), bf16: exact in every format the kernel takes."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (B * T, heads * hd), generator=gen).to(torch.float32) + float(offset)
    return x.to(torch.bfloat16)


def generic_rows(B, T, heads, hd, seed, dtype, mean_sigmas=0.0):
    """Gaussian rows whose column scales span four decades; mean_sigmas: a constant mean of that many sigma on every fourth
    column of a head (the key rows of the cancellation case)."""
    gen = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(heads * hd, generator=gen, dtype=torch.float64) * 4 - 2)
    x = torch.randn(B * T, heads * hd, generator=gen, dtype=torch.float64)
    if mean_sigmas:
        x[:, torch.arange(heads * hd) % 4 == 1] += mean_sigmas
    return (x * scale).to(dtype)
