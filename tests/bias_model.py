"""Host model of the projection biases through the V/O truncation ("Projection biases"): numpy, sums in long
double, eigen-decompositions by numpy's fp64 eigh on matrices built to be well conditioned.  The oracle has no notion of a bias; the
tests of mdg_vo_bias (tests/test_gpu_vo_bias.py) and of the identities (tests/test_bias_model_host.py) stand on this file.

Notation: W_v [n_kv hd, d], W_o [d, n_heads hd], C = sigma_x + ridge I, query head h reads kv head g = h // (n_heads // n_kv).
P_g [r, hd] and Q_g [hd, r] are the factors of the truncation, W_v,g' = P_g W_v,g and W_o,h' = W_o,h Q_g, Pi_g = Q_g P_g.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def ld(a):
    return np.asarray(a, dtype=LD)


def bf16_round(a):
    """fp64 / fp32 array -> the nearest bf16 values (round to nearest even through fp32, as torch does), returned as fp64."""
    f = np.asarray(a, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def expand_bias(b_v, n_heads, n_kv, hd):
    """b_v [n_kv hd] -> the [n_heads hd] vector a token's v carries into W_o (query heads of a group share their kv head's entries)."""
    g = n_heads // n_kv
    return np.concatenate([np.asarray(b_v)[(h // g) * hd:(h // g + 1) * hd] for h in range(n_heads)])


def _eigh_desc(G):
    lam, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    order = np.argsort(-lam, kind="stable")
    return lam[order], V[:, order]


def factors(Wv, Wo, C, n_heads, n_kv, hd, rank):
    """[(P_g, Q_g, lam_g)] per kv head, fp64; lam_g the spectrum the truncation cuts (descending): the Gram matrix's for the grouped
    variant, the second decomposition's for the two-SVD MHA variant (n_kv == n_heads), as mdg_vo_compress computes them."""
    out = []
    for g in range(n_kv):
        Wg = ld(Wv[g * hd:(g + 1) * hd])
        lam, V = _eigh_desc(Wg @ ld(C) @ Wg.T)
        S = np.sqrt(np.maximum(lam, 0.0))
        if n_kv != n_heads:
            out.append((V[:, :rank].T / S[:rank, None], V[:, :rank] * S[None, :rank], lam))
            continue
        Wh = ld(Wo[:, g * hd:(g + 1) * hd])
        Y = S[:, None] * V.T                                      # S V^T
        lam2, Up = _eigh_desc(ld(Y) @ (Wh.T @ Wh) @ ld(Y).T)      # B B^T, B = S V^T W_o,h^T
        P = Up[:, :rank].T @ (V.T / S[:, None])
        Q = (V * S[None, :]) @ Up[:, :rank]
        out.append((P, Q, lam2))
    return out


def sigma_ratio(lam, rank):
    """sigma_r / sigma_r+1 of a descending spectrum lam = sigma^2 (inf at full rank)."""
    if rank >= len(lam):
        return float("inf")
    return float(np.sqrt(max(lam[rank - 1], 0.0) / max(lam[rank], 1e-300)))


def fold(Wo, b_v, b_o, n_heads, n_kv, hd):
    """(o_bias, absolute) in long double: o_bias_i = b_o,i + sum_j W_o,ij b_j and absolute_i = |b_o,i| + sum_j |W_o,ij b_j|, b the expanded
    v bias; b_o may be None (zeros)."""
    b = ld(expand_bias(b_v, n_heads, n_kv, hd))
    W = ld(Wo)
    bo = np.zeros(W.shape[0], dtype=LD) if b_o is None else ld(b_o)
    return bo + W @ b, np.abs(bo) + np.abs(W) @ np.abs(b)


def projected_bias(facs, b_v, hd):
    """v_bias [n_kv r]: P_g b_v,g per kv head, long double."""
    return np.concatenate([ld(P) @ ld(b_v[g * hd:(g + 1) * hd]) for g, (P, _, _) in enumerate(facs)])


def kept_part(facs, b_v, hd):
    """Pi_g b_v,g per kv head, [n_kv hd], long double."""
    return np.concatenate([ld(Q) @ (ld(P) @ ld(b_v[g * hd:(g + 1) * hd])) for g, (P, Q, _) in enumerate(facs)])


def residual(Wo, facs, b_v, n_heads, n_kv, hd):
    """(rho, absolute): rho_i = sum_j W_o,ij (b - Pi b)_j, absolute_i = sum_j |W_o,ij| (|b_j| + |(Pi b)_j|), long double."""
    b = ld(expand_bias(b_v, n_heads, n_kv, hd))
    kb = ld(expand_bias(kept_part(facs, b_v, hd), n_heads, n_kv, hd))
    W = ld(Wo)
    return W @ (b - kb), np.abs(W) @ (np.abs(b) + np.abs(kb))


# ---- inputs whose truncated spectrum has a step at `rank` and whose eigenproblems are well conditioned ----
def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))[None, :]


def stepped_spectrum(rng, n, rank, top=(1.0, 2.0), low=(0.02, 0.1)):
    """n values, the first `rank` in `top`, the rest in `low`, descending: sigma_r / sigma_r+1 >= sqrt(top[0] / low[1]) = 3.16."""
    hi = np.sort(rng.uniform(*top, size=rank))[::-1]
    lo = np.sort(rng.uniform(*low, size=n - rank))[::-1]
    return np.concatenate([hi, lo])


def make_case(n_heads, n_kv, hd, d, rank, seed, bf16=True):
    """(Wv, Wo, C, b_v, b_o), fp64 arrays; bf16: Wv / Wo / biases hold bf16 values (sums of their products are then EXACT in fp64: 16-bit
    products of similar exponents), else full fp64 values, whose sums round.
    Grouped (n_kv hd <= d required): the rows of W_v are orthonormal up to bf16 rounding and sigma_x = W_v^+ D W_v^+T + 0.01 (I -
    W_v^+ W_v) with D = blockdiag(R_g diag(lam) R_g^T), R_g random orthogonal and lam = stepped_spectrum: every head's Gram matrix is
    a dense matrix with that spectrum.  MHA: every head's W_v,g has orthonormal rows and sigma_x = I, so the first decomposition is
    flat; the step sits in W_o,h = U_h diag(s) R_h^T, s^2 = stepped_spectrum, which the second decomposition cuts."""
    rng = np.random.default_rng(seed)
    a = n_kv * hd
    rnd = bf16_round if bf16 else (lambda x: np.asarray(x, dtype=np.float64))
    if n_kv != n_heads:
        assert a <= d
        Wv = rnd(_orthogonal(rng, d)[:a])
        D = np.zeros((a, a))
        for g in range(n_kv):
            R = _orthogonal(rng, hd)
            D[g * hd:(g + 1) * hd, g * hd:(g + 1) * hd] = (R * stepped_spectrum(rng, hd, rank)[None, :]) @ R.T
        Wp = np.linalg.pinv(Wv)
        C = Wp @ D @ Wp.T + 0.01 * (np.eye(d) - Wp @ Wv)
        C = (C + C.T) / 2
        Wo = rnd(rng.standard_normal((d, n_heads * hd)) * 0.15)
    else:
        assert hd <= d
        Wv = rnd(np.concatenate([_orthogonal(rng, d)[:hd] for _ in range(n_kv)]))
        C = np.eye(d)
        Wo = rnd(np.concatenate(
            [(_orthogonal(rng, d)[:, :hd] * np.sqrt(stepped_spectrum(rng, hd, rank))[None, :]) @ _orthogonal(rng, hd).T
             for _ in range(n_heads)], axis=1))
    b_v = rnd(rng.standard_normal(a) * 0.15)
    b_o = rnd(rng.standard_normal(d) * 0.15)
    return Wv, Wo, C, b_v, b_o
