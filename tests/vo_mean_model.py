"""Long double host model of the mean-aware V/O truncation ("The V/O intercept"): the head vectors a_g = W_v,g mu
+ b_v,g and a'_g = v^_g mu, the intercept delta of STORED factors, the two norms mdg_vo_intercept reports, the a priori bound the GPU
tests hold the kernel to, and the truncation itself (grouped and two-SVD MHA variant) on any statistic -- centred or not.  Plain numpy
in np.longdouble on top of tests/mean_model.py and the long double Jacobi solver of tests/eig_ref.py; nothing here touches a GPU."""
import numpy as np

from tests import eig_ref as E
from tests import mean_model as M

LD = M.LD
U = 2.0 ** -53
ld = M.ld
bf16_round = M.bf16_round


def head_vectors(W_v, v_hat, mu, n_kv, hd, rank, b_v=None):
    """(a [n_kv, hd], a' [n_kv, rank]): a_g = W_v,g mu + b_v,g, a'_g = v^_g mu."""
    mu = ld(mu)
    a = (ld(W_v) @ mu).reshape(n_kv, hd)
    if b_v is not None:
        a = a + ld(b_v).reshape(n_kv, hd)
    a2 = (ld(v_hat) @ mu).reshape(n_kv, rank) if rank else np.zeros((n_kv, 0), dtype=LD)
    return a, a2


def delta(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v=None):
    """(delta [d], const [d]): const_i = sum_h W_o,h[i, :] a_kv(h) -- the constant the uncompressed attention adds to its output --
    and delta_i = const_i - sum_h o^_h[i, :] a'_kv(h)."""
    a, a2 = head_vectors(W_v, v_hat, mu, n_kv, hd, rank, b_v)
    g = n_heads // n_kv
    const = ld(W_o) @ np.repeat(a, g, axis=0).reshape(-1)
    dl = const - ld(o_hat) @ np.repeat(a2, g, axis=0).reshape(-1) if rank else const.copy()
    return dl, const


def intercept(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v=None, b_o=None):
    """(bias, ||delta||^2, ||const||^2): bias = b_o + delta for the factors that are stored."""
    dl, const = delta(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v)
    return (dl if b_o is None else ld(b_o) + dl), (dl * dl).sum(), (const * const).sum()


def delta_bound(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v=None):
    """Entry-wise bound of delta: (d + n_heads (hd + rank) + 8) 2^-53 A_i,
    A_i = sum_h |W_o,h[i, :]| (|W_v,g| |mu| + |b_v,g|) + |o^_h[i, :]| (|v^_g| |mu|).
    The head vectors are sums of d exact products (+ one addition of b_v), the rows sums of n_heads hd and n_heads rank exact products
    of them, then one subtraction; every partial sum is bounded by its sum of absolute terms, in whatever order they are added."""
    d = np.shape(W_v)[1]
    return (d + n_heads * (hd + rank) + 8) * LD(U) * magnitude(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v)


def magnitude(W_v, W_o, v_hat, o_hat, mu, n_heads, n_kv, hd, rank, b_v=None):
    """A_i of delta_bound."""
    am = np.abs(ld(mu))
    a = (np.abs(ld(W_v)) @ am).reshape(n_kv, hd)
    if b_v is not None:
        a = a + np.abs(ld(b_v)).reshape(n_kv, hd)
    g = n_heads // n_kv
    A = np.abs(ld(W_o)) @ np.repeat(a, g, axis=0).reshape(-1)
    if rank:
        a2 = (np.abs(ld(v_hat)) @ am).reshape(n_kv, rank)
        A = A + np.abs(ld(o_hat)) @ np.repeat(a2, g, axis=0).reshape(-1)
    return A


# ---------------------------------------------------------------- the truncation on a statistic (compress_vo.py:112-223 on the Gram matrix)
def _eigh(G):
    lam, V, sweeps = E.jacobi_eigh(G, dtype=LD, update="rutishauser")
    assert sweeps <= E.MAX_SWEEPS
    return lam, V


def truncate(stat, W_v, W_o, n_heads, n_kv, hd, rank, ridge=0.0):
    """(v^ [n_kv rank, d], o^ [d, n_heads rank], Pi [n_kv, hd, hd]) in long double, unrounded: the factors mdg_vo_compress computes from
    the statistic `stat` (+ ridge I), and per kv head the map Pi_g = Q_g P_g its value stream passes through (v^_g = P_g W_v,g,
    o^_h = W_o,h Q_g).  Grouped: Pi_g = V_r V_r^T, the projector on the leading eigenvectors of G = W_v,g stat W_v,g^T.  MHA
    (n_kv == n_heads), the two-SVD variant: Pi = V S U_r U_r^T S^-1 V^T, U the eigenvectors of (S V^T) W_o,h^T W_o,h (V S)."""
    Wv, Wo = ld(W_v), ld(W_o)
    d = Wv.shape[1]
    Cm = ld(stat) + LD(ridge) * np.eye(d, dtype=LD)
    g = n_heads // n_kv
    v_hat = np.zeros((n_kv * rank, d), dtype=LD)
    o_hat = np.zeros((d, n_heads * rank), dtype=LD)
    Pi = np.zeros((n_kv, hd, hd), dtype=LD)
    for k in range(n_kv):
        Wk = Wv[k * hd:(k + 1) * hd]
        lam, V = _eigh(Wk @ Cm @ Wk.T)
        s = np.sqrt(np.maximum(lam, 0))
        if g > 1:
            P = (V[:, :rank] / s[:rank]).T                        # [rank, hd]
            Q = V[:, :rank] * s[:rank]                            # [hd, rank]
        else:
            Wh = Wo[:, k * hd:(k + 1) * hd]
            Y = (V * s).T                                         # S V^T
            _, Up = _eigh(Y @ (Wh.T @ Wh) @ Y.T)
            P = Up[:, :rank].T @ (V / s).T
            Q = (V * s) @ Up[:, :rank]
        Pi[k] = Q @ P
        v_hat[k * rank:(k + 1) * rank] = P @ Wk
        for j in range(g):
            h = k * g + j
            o_hat[:, h * rank:(h + 1) * rank] = Wo[:, h * hd:(h + 1) * hd] @ Q
    return v_hat, o_hat, Pi


def head_maps(W_v, W_o, v_hat, o_hat, n_heads, n_kv, hd, rank):
    """Delta_h [n_heads, d, d] = W_o,h W_v,kv(h) - o^_h v^_kv(h): what query head h's linear map x -> W_o,h W_v x loses."""
    Wv, Wo, vh, oh = ld(W_v), ld(W_o), ld(v_hat), ld(o_hat)
    g = n_heads // n_kv
    out = []
    for h in range(n_heads):
        k = h // g
        D = Wo[:, h * hd:(h + 1) * hd] @ Wv[k * hd:(k + 1) * hd]
        if rank:
            D = D - oh[:, h * rank:(h + 1) * rank] @ vh[k * rank:(k + 1) * rank]
        out.append(D)
    return np.stack(out)


def output_errors(X, Dh, bias=None):
    """From the token matrix, in long double: the error of the layer's summed per-head linear maps, e_t = sum_h Delta_h x_t - bias.
    Returns (mean_t e_t [d], sum over heads and tokens of ||Delta_h x_t - Delta_h mean||^2 with bias given / ||Delta_h x_t||^2 without):
    with an intercept every head's map is affine and its optimal constant is its own mean, the bias being their sum."""
    X = ld(X)
    per_head = np.einsum("hij,tj->hti", ld(Dh), X)                # [n_heads, tokens, d]
    e = per_head.sum(axis=0)
    if bias is not None:
        e = e - ld(bias)
        per_head = per_head - per_head.mean(axis=1, keepdims=True)
    return e.mean(axis=0), (per_head * per_head).sum()


def value_stream_error(X, W_v, Pi, n_kv, hd, a=None):
    """sum_t ||(I - Pi_g)(W_v,g x_t) - (I - Pi_g) a_g||^2 summed over the kv heads (a None: nothing subtracted)."""
    X, Wv = ld(X), ld(W_v)
    total = LD(0)
    for k in range(n_kv):
        R = np.eye(hd, dtype=LD) - ld(Pi[k])
        y = X @ Wv[k * hd:(k + 1) * hd].T
        if a is not None:
            y = y - ld(a)[k]
        z = y @ R.T
        total = total + (z * z).sum()
    return total


def moments(X):
    """(C, mu) of the token matrix in long double: C = X^T X / T, mu = mean_t x_t."""
    X = ld(X)
    T = LD(X.shape[0])
    return X.T @ X / T, X.sum(axis=0) / T


def make_tokens(tokens, d, seed=0, mean_scale=8.0):
    """X [tokens, d], bf16-valued: Gaussian with a per-channel spread in [1/4, 4] plus a per-channel mean of up to mean_scale spreads
    (a few channels carry a large, nearly constant value, as real hidden states do).  Every entry sits on the grid spread / 16 with at
    most 255 grid units, so it is a bf16 value, and the column sums (2^17 units) and second moments (2^25 units of s_i s_j / 256) of up
    to 512 tokens are exact in fp64 -- with a power-of-two token count so are C and mu."""
    rng = np.random.default_rng(1013 * seed + d)
    spread = 2.0 ** rng.integers(-2, 3, size=d)
    mean = rng.uniform(-mean_scale, mean_scale, size=d) * spread
    units = np.clip(np.round((rng.standard_normal((tokens, d)) * spread + mean) / spread * 16.0), -255, 255)
    X = units / 16.0 * spread
    assert np.array_equal(bf16_round(X), X)
    return X


def make_weights(n_heads, n_kv, hd, d, seed=0, rank=0):
    """bf16-valued W_v [n_kv hd, d], W_o [d, n_heads hd], b_v [n_kv hd], b_o [d] (and, with rank, arbitrary factors v^, o^)."""
    rng = np.random.default_rng(7919 * seed + 31 * d + n_heads * hd)
    out = {"W_v": bf16_round(rng.standard_normal((n_kv * hd, d)) / np.sqrt(d)),
           "W_o": bf16_round(rng.standard_normal((d, n_heads * hd)) / np.sqrt(n_heads * hd)),
           "b_v": bf16_round(rng.standard_normal(n_kv * hd) * 0.1), "b_o": bf16_round(rng.standard_normal(d) * 0.1)}
    if rank:
        out["v_hat"] = bf16_round(rng.standard_normal((n_kv * rank, d)) / np.sqrt(d))
        out["o_hat"] = bf16_round(rng.standard_normal((d, n_heads * rank)) / np.sqrt(n_heads * rank))
    return out
