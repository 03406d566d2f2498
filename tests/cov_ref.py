"""References and input builders of the fp64 covariance tests (test_cov_ref_host.py on the CPU, test_gpu_cov.py on the GPU):
mdg_cov_accum, mdg_cov_accum_multi, mdg_cov_finalize and mdg_bi_accum of csrc/cov.hip.  No GPU, no library call.

Two kinds of reference.  EXACT ones, for inputs built on a lattice on which fp64 arithmetic cannot round, so that the kernel's
result is determined bit for bit whatever its summation order (exact_inputs / exact_cov, bi_exact_inputs); and LONG-DOUBLE ones for
generic data, with the quantity an a-priori rounding bound is stated in (longdouble_cov, longdouble_bi)."""
import numpy as np
import torch

LD = np.longdouble
TILE = 128                       # the kernel's output tile; a split-K partial is one TILE x TILE fp64 tile per (split, batch, tile)
BK = 16                          # tokens per staging step; a split's length is a multiple of it
MANT = 15                        # |m| <= MANT
EXP = 8                          # |e_j| <= EXP


def exact_inputs(tokens, width, dtype, seed):
    """x[t, j] = m[t, j] * 2**e[j] as a [tokens, width] tensor of `dtype`: m integers in [-15, 15] (about a quarter of them zero,
    both signs, and some of the zeros stored as -0.0), e[j] a per-column integer in [-8, 8].  Every value has at most 4 significant
    bits and lies in [2**-8, 15 * 2**8], so it is exact in bf16, fp16, fp32 and fp64 alike."""
    rng = np.random.default_rng([seed, tokens, width])
    m = rng.integers(-MANT, MANT + 1, size=(tokens, width)).astype(np.float64)
    m[rng.random((tokens, width)) < 0.22] = 0.0
    m[(m == 0.0) & (rng.random((tokens, width)) < 0.3)] = -0.0
    e = rng.integers(-EXP, EXP + 1, size=width)
    x = torch.from_numpy(m * np.exp2(e.astype(np.float64))[None, :])
    out = x.to(dtype)
    assert torch.equal(out.double(), x) and bool((torch.signbit(out) == torch.signbit(x)).all())
    return out


def _heads_f64(x, heads, relu):
    v = x.detach().cpu().double()
    tokens, width = v.shape
    assert width % heads == 0
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))            # max(m, 0): -0.0 and negatives give +0
    return v.reshape(tokens, heads, width // heads)


def exact_cov(x, heads=1, relu=False, sigma0=None):
    """sigma[h] = sigma0[h] + X_h^T X_h as a [heads, feat, feat] fp64 tensor (both triangles), the data widened to fp64 and multiplied
    in fp64 on the CPU.

    Exact, and independent of the order of summation, for data of exact_inputs: every product x_ti x_tj is an integer
    m_ti m_tj (|.| <= 225) times 2**(e_i + e_j), so every partial sum of sigma_ij, over any subset of the tokens, is an integer
    multiple of 2**(e_i + e_j) of magnitude at most 225 * tokens * 2**(e_i + e_j).  With 225 * tokens far below 2**53 such a number
    is an fp64 value, hence no fp64 addition or fused multiply-add ever rounds: any order, any split over tokens and any grouping
    inside a matrix instruction produce the same bits, and so does this plain product.  sigma0 (what the buffer held before) must
    come from the same lattice with the same column exponents, e.g. an earlier exact_cov of other tokens of the same columns; the
    argument then covers the total token count."""
    v = _heads_f64(x, heads, relu)
    assert 225 * max(v.shape[0], 1) < 2 ** 40
    s = torch.einsum("thi,thj->hij", v, v)
    return s if sigma0 is None else s + sigma0.reshape(s.shape)


def longdouble_cov(x, heads=1, relu=False):
    """(sigma, scale): sigma[h] = X_h^T X_h summed in np.longdouble (64-bit significand) over the exactly widened data, and
    scale[h]_ij = sqrt(sigma_ii sigma_jj), the quantity the a-priori bound of an fp64 sum of exact products is stated in
    (|x_i . x_j| <= |x_i| |x_j|).  Both [heads, feat, feat] np.longdouble arrays."""
    v = _heads_f64(x, heads, relu).numpy().astype(LD)
    s = np.einsum("thi,thj->hij", v, v)
    dg = np.sqrt(np.einsum("hii->hi", s))
    return s, dg[:, :, None] * dg[:, None, :]


def longdouble_abs_cov(x, heads=1):
    """sum_t |x_ti x_tj| in np.longdouble, [heads, feat, feat]: the scale of the bound when the products themselves round (fp64 input)."""
    v = np.abs(_heads_f64(x, heads, False).numpy().astype(LD))
    return np.einsum("thi,thj->hij", v, v)


def n_tri(n_feat):
    t = -(-n_feat // TILE)
    return t * (t + 1) // 2


def split_plan(ws_bytes, tokens, n_feat, batch):
    """(ksplit, tokens_per_split, last_split_tokens) of an mdg_cov_accum call, from what mdg_cov_accum_ws_bytes answers for it and
    nothing else: the workspace holds one 128 x 128 fp64 partial per (split, batch, lower tile), a split is ceil(tokens / ksplit)
    tokens rounded up to the 16-token stage, and the last one takes what is left."""
    per_split = batch * n_tri(n_feat) * TILE * TILE * 8
    if ws_bytes == 0:
        ksplit = 1
    else:
        assert ws_bytes % per_split == 0, (ws_bytes, per_split)
        ksplit = ws_bytes // per_split
    tps = -(-(-(-tokens // ksplit)) // BK) * BK
    last = tokens - (ksplit - 1) * tps
    assert 0 < last <= tps, "the workspace size does not describe a split of %d tokens into %d" % (tokens, ksplit)
    return ksplit, tps, last


def bi_exact_inputs(tokens, d, dtype, seed):
    """(x_in, x_out, total) for mdg_bi_accum: [tokens, d] tensors of `dtype` and the exact value of sum_t (1 - cos(x_in[t], x_out[t])).

    Row t of x_in is (3, 4) * 2**k_t at two random positions, zero elsewhere; x_out[t] is x_in[t], -x_in[t], (4, -3) * 2**k_t at
    the same positions (perpendicular) or zero.  Both norms are then exactly 5 * 2**k (25 * 4**k and its square root are exact), the
    dot product is exactly +-25 * 4**k or 0, and the term is exactly 0, 2, 1 or -- for the zero row, whose norm is clamped to 1e-8
    and whose dot product is 0 -- 1.  The total is a small integer: exact in any order of summation."""
    assert d >= 2
    rng = np.random.default_rng([seed, tokens, d])
    xin = np.zeros((tokens, d))
    xout = np.zeros((tokens, d))
    kind = rng.integers(0, 4, size=tokens)
    k = np.exp2(rng.integers(-4, 5, size=tokens).astype(np.float64))
    p = rng.integers(0, d, size=tokens)
    q = (p + 1 + rng.integers(0, d - 1, size=tokens)) % d
    t = np.arange(tokens)
    xin[t, p], xin[t, q] = 3 * k, 4 * k
    same, neg, perp = kind == 0, kind == 1, kind == 2
    xout[same] = xin[same]
    xout[neg] = -xin[neg]
    xout[t[perp], p[perp]], xout[t[perp], q[perp]] = 4 * k[perp], -3 * k[perp]
    total = float(2 * neg.sum() + perp.sum() + (kind == 3).sum())
    a, b = torch.from_numpy(xin).to(dtype), torch.from_numpy(xout).to(dtype)
    assert torch.equal(a.double(), torch.from_numpy(xin)) and torch.equal(b.double(), torch.from_numpy(xout))
    return a, b, total


def longdouble_bi(x_in, x_out):
    """sum_t (1 - x_in[t] . x_out[t] / (max(|x_in[t]|, 1e-8) max(|x_out[t]|, 1e-8))) in np.longdouble: the kernel's formula, each
    norm clamped separately (torch.cosine_similarity's eps)."""
    a = x_in.detach().cpu().double().numpy().astype(LD)
    b = x_out.detach().cpu().double().numpy().astype(LD)
    eps = LD(1e-8)
    dot = (a * b).sum(axis=1)
    den = np.maximum(np.sqrt((a * a).sum(axis=1)), eps) * np.maximum(np.sqrt((b * b).sum(axis=1)), eps)
    return (LD(1) - dot / den).sum()
