"""GPU: the mean-aware V/O truncation from a token matrix, through ops alone:
    col_sum_accum -> mean -> cov_accum / cov_finalize -> cov_center -> vo_compress(S) -> vo_intercept on the STORED bf16 factors
512 tokens, d = 128, 4 query heads of 32 over 2 (grouped) and 4 (MHA, two-SVD) kv heads, rank 22, ridge 0.  The token matrix
(vo_mean_model.make_tokens) is bf16-valued with channel means of up to 8 spreads; its column sums and second moments over 512 tokens
are exact in fp64, so the device and the long double model start from the same mu, and mean_t Delta x_t = Delta mu exactly.

  * the test that fails without the feature: the mean over the tokens of the output error of the stored factors, per channel, is
    within one bf16 rounding of the stored bias (2^-8 |bias_i|) plus the kernel's fp64 bound (tests/test_gpu_vo_intercept.py);
  * the host model's inequalities on the device's fp64 factors: MHA -- centring + intercept loses no more than the reference's route;
    grouped -- the same on the value stream, Pi_g recovered from o^_h = W_o,h Q_g by least squares (W_o,h has full column rank);
  * mu = 0 exactly (the second half of X is the negation of the first): S is C bit for bit, the centred path reproduces the
    uncentred factors bit for bit, and delta -- every a_g and a'_g being a sum of exact zeros -- is zero."""
import functools

import numpy as np
import pytest
import torch

from tests import vo_mean_model as V

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
TOKENS, D, HD, RANK = 512, 128, 32, 22
LAYOUTS = [(4, 2), (4, 4)]


@functools.lru_cache(maxsize=None)
def _chain(n_heads, n_kv, zero_mean=False):
    """Everything once per layout, shared by the tests below and left unchanged by them."""
    from modegpt_amd import ops
    dev = torch.device("cuda:0")
    X = V.make_tokens(TOKENS, D, seed=3)
    if zero_mean:
        X[TOKENS // 2:] = -X[:TOKENS // 2]
    w = V.make_weights(n_heads, n_kv, HD, D, seed=5)
    x = torch.from_numpy(X).to(dev).to(torch.bfloat16)
    assert np.array_equal(x.double().cpu().numpy(), X)
    Wv, Wo = (torch.from_numpy(w[k]).to(dev).to(torch.bfloat16) for k in ("W_v", "W_o"))
    sums = torch.zeros(D, dtype=torch.float64, device=dev)
    ops.col_sum_accum(sums, x)
    mu = sums / TOKENS                                          # (a power of two: exact)
    C = torch.zeros(D, D, dtype=torch.float64, device=dev)
    ops.cov_accum(C, x)
    ops.cov_finalize(C, 1.0 / TOKENS)
    S = ops.cov_center(C, mu)
    v, o, v64, o64 = ops.vo_compress(S, Wv, Wo, n_heads, n_kv, HD, RANK, 0.0, want_f64=True)
    bias, bias64, norms = ops.vo_intercept(Wv, Wo, v, o, mu, n_heads, n_kv, HD, RANK)
    bias64_f = ops.vo_intercept(Wv, Wo, v64, o64, mu, n_heads, n_kv, HD, RANK)[1]       # the fp64 factors go in unchanged
    vu, ou, vu64, ou64 = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, HD, RANK, 0.0, want_f64=True)
    torch.cuda.synchronize()
    out = {k: t.cpu() for k, t in dict(mu=mu, C=C, S=S, v=v, o=o, v64=v64, o64=o64, bias=bias, bias64=bias64, norms=norms,
                                       bias64_f=bias64_f, vu=vu, ou=ou, vu64=vu64, ou64=ou64).items()}
    return X, w, out


def _np(t):
    return t.double().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_moments_are_the_token_matrix_s(dev, layout):
    X, w, out = _chain(*layout)
    C, mu = V.moments(X)
    assert np.array_equal(_np(out["mu"]), mu.astype(np.float64)) and np.array_equal(V.ld(_np(out["mu"])), mu)      # exact
    assert np.array_equal(V.ld(_np(out["C"])), C)
    S = C - np.outer(mu, mu)
    assert np.all(np.abs(V.ld(_np(out["S"])) - S) <= U * np.abs(S))                     # one rounding per entry
    ratio = np.abs(X.mean(axis=0)) / X.std(axis=0)
    assert ratio.max() > 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stored_factors_leave_no_mean_error_on_the_tokens(dev, layout):
    n_heads, n_kv = layout
    X, w, out = _chain(*layout)
    mu = _np(out["mu"])
    v, o, bias = _np(out["v"]), _np(out["o"]), _np(out["bias"])
    assert out["bias"].dtype == torch.bfloat16 and torch.equal(out["bias"], out["bias64"].to(torch.bfloat16))
    args = (w["W_v"], w["W_o"], v, o, mu, n_heads, n_kv, HD, RANK)
    dl, const = V.delta(*args)
    fp64_bound = V.delta_bound(*args)
    assert np.all(np.abs(V.ld(_np(out["bias64"])) - dl) <= fp64_bound)
    Dh = V.head_maps(w["W_v"], w["W_o"], v, o, n_heads, n_kv, HD, RANK)
    mean_on, _ = V.output_errors(X, Dh, bias=bias)
    mean_off, _ = V.output_errors(X, Dh)
    model_noise = TOKENS * float(np.finfo(V.LD).eps) * 16 * V.magnitude(*args)          # the long double token sums' own rounding
    bound = 2.0 ** -8 * np.abs(bias) + fp64_bound + model_noise
    print(f"{layout}: |mean error| / bound max {float((np.abs(mean_on) / bound).max()):.3f}; without the bias "
          f"{float((np.abs(mean_off) / bound).max()):.3e}; ||delta||^2 / ||const||^2 = {float((dl * dl).sum() / (const * const).sum()):.3e}")
    assert np.all(np.abs(mean_on) <= bound)
    assert np.abs(mean_off).max() > 100 * bound.max()                                   # without the feature the mean error is delta
    n0, n1 = (float(x) for x in out["norms"])
    assert abs(n0 - float((dl * dl).sum())) <= 1e-9 * n0 and abs(n1 - float((const * const).sum())) <= 1e-9 * n1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_model_inequalities_on_the_fp64_factors(dev, layout):
    n_heads, n_kv = layout
    X, w, out = _chain(*layout)
    mu = _np(out["mu"])
    v_c, o_c, v_u, o_u = (_np(out[k]) for k in ("v64", "o64", "vu64", "ou64"))
    if n_heads == n_kv:
        dl, _ = V.delta(w["W_v"], w["W_o"], v_c, o_c, mu, n_heads, n_kv, HD, RANK)
        assert np.all(np.abs(V.ld(_np(out["bias64_f"])) - dl) <= V.delta_bound(w["W_v"], w["W_o"], v_c, o_c, mu, n_heads, n_kv, HD, RANK))
        _, sq_on = V.output_errors(X, V.head_maps(w["W_v"], w["W_o"], v_c, o_c, n_heads, n_kv, HD, RANK), bias=dl)
        _, sq_off = V.output_errors(X, V.head_maps(w["W_v"], w["W_o"], v_u, o_u, n_heads, n_kv, HD, RANK))
        print(f"MHA: summed squared output error, centred + intercept {float(sq_on):.6e}, reference route {float(sq_off):.6e}")
        assert sq_on <= sq_off
        return
    g = n_heads // n_kv

    def projections(v64, o64):
        Pi = np.zeros((n_kv, HD, HD))
        for k in range(n_kv):
            h = k * g
            Q, *_ = np.linalg.lstsq(w["W_o"][:, h * HD:(h + 1) * HD], o64[:, h * RANK:(h + 1) * RANK], rcond=None)     # [hd, rank]
            # v^_g = P W_v,g with W_v,g of full row rank: P = v^_g W_v,g^+
            P = v64[k * RANK:(k + 1) * RANK] @ np.linalg.pinv(w["W_v"][k * HD:(k + 1) * HD])
            Pi[k] = Q @ P
            assert np.abs(Pi[k] @ Pi[k] - Pi[k]).max() <= 1e-8 and np.abs(Pi[k] - Pi[k].T).max() <= 1e-8                # a projector
        return Pi

    a, _ = V.head_vectors(w["W_v"], None, mu, n_kv, HD, 0)
    on = V.value_stream_error(X, w["W_v"], projections(v_c, o_c), n_kv, HD, a=a)
    off = V.value_stream_error(X, w["W_v"], projections(v_u, o_u), n_kv, HD)
    print(f"grouped: value stream error, centred {float(on):.6e}, uncentred {float(off):.6e}")
    assert on <= off


@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_mean_reproduces_the_uncentred_factors_bit_for_bit(dev, layout):
    X, w, out = _chain(*layout, zero_mean=True)
    assert not out["mu"].any() and torch.equal(out["S"], out["C"])
    for a, b in (("v", "vu"), ("o", "ou")):
        assert torch.equal(out[a].view(torch.int16), out[b].view(torch.int16))
    for a, b in (("v64", "vu64"), ("o64", "ou64")):
        assert torch.equal(out[a].view(torch.int64), out[b].view(torch.int64))
    assert not out["bias64"].any() and not out["bias"].any() and not out["norms"].any()
