"""GPU: the mean-aware refit -- ops.cov_center -> ops.nystrom_down on S -> ops.nystrom_intercept -- and compress_weights(intercept=)
against the long double model of tests/mean_model.py.

Data (mean_model.make_case): h = |Gaussian| x a per-column power of two on a grid that makes C = H^T H / 512 and mu exact in fp64, so
the device and the model start from the same numbers; every mean is of the order of its standard deviation.  512 tokens keep the
model's S_kk well conditioned (asserted).  Checks, all a priori:
  D (fp64)        against the model, per entry relative to the largest entry of its column, 1e-7 (the Nystrom tests' tolerance)
  D^ (bf16)       at most one ulp off the rounded model on at most 0.1 % of the entries
  bias_f64        entry-wise within (n + r + 2) 2^-53 (|b_i| + sum_j |W_ij mu_j| + sum_p |D^_ip mu_p|)
  norms           within (d + 2) 2^-53 of the sums of squares of the rows the device itself produced
  from the TOKEN MATRIX and the stored tensors: the per-channel mean of y - y' is at most 2^-8 |delta_i| (one bf16 rounding of the
  bias) plus the bias bound; sum_t ||y - y'||^2 is strictly below the linear refit's and within rel 1e-3 of the model's.
The issue also expected the linear refit's per-channel mean to exceed four times that bound on these inputs, and asked for that to be
asserted on the host model before relying on it.  It does not hold there: 140 (257) non-negative features represent the constant up
to ||1_perp||^2 / T ~ 1 / (1 + 1.75 r) ~ 0.4 % of its energy, which is what the linear refit leaves of W_d mu -- the size of 2^-8
|delta| itself.  Host model, seed 0: |mean_off| / bound has median 0.99 and minimum 0.018 over the channels at (200, 140, 96), 0.61 and
0.009 at (385, 257, 40).  The test therefore asserts what the model supports (test_linear_refit_leaves_a_mean_the_intercept_removes):
the largest |mean| over the channels shrinks by more than the bf16 rounding allows the intercept to leave, and the squared error drops."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import mean_model as M
from tests import nystrom_split_ref as NS

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EPS = 1e-6
SIZES = [(200, 140, 96), (385, 257, 40)]


@functools.lru_cache(maxsize=None)
def _case(n, r, d):
    """The case, the model's fits and the device's outputs, computed once per size and shared (nothing below modifies them)."""
    from modegpt_amd import ops
    dev = torch.device("cuda")
    c = M.make_case(n, r, d, tokens=512, seed=0)
    H, W, C, mu, idx, b_d = (c[k] for k in ("H", "W", "C", "mu", "idx", "b_d"))
    S_model = M.center(C, mu).astype(np.float64)
    assert M.cond(S_model[np.ix_(idx, idx)]) < 1e4            # well conditioned: the refit is determined far below 1e-7
    D_model = M.refit(S_model, idx, W, EPS)                   # [d, r] long double
    Cd, mud = torch.from_numpy(C).to(dev), torch.from_numpy(mu).to(dev)
    Wd = torch.from_numpy(W).to(dev).to(torch.bfloat16)
    idxd = torch.from_numpy(idx).to(dev)
    bd = torch.from_numpy(b_d).to(dev).to(torch.bfloat16)
    Sd = ops.cov_center(Cd, mud)
    down, f64 = ops.nystrom_down(Sd, idxd, Wd, eps=EPS, want_f64=True)
    bias, bias64, norms = ops.nystrom_intercept(Wd, down, idxd, mud, b_d=bd)
    bias0, bias064, norms0 = ops.nystrom_intercept(Wd, down, idxd, mud)            # no b_d: bias_f64 IS delta
    down_lin = ops.nystrom_down(Cd, idxd, Wd, eps=EPS)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in dict(S=Sd, down=down, f64=f64, bias=bias, bias64=bias64, norms=norms, bias0=bias0, bias064=bias064,
                                       norms0=norms0, down_lin=down_lin).items()}
    assert torch.equal(Cd.cpu(), torch.from_numpy(C))         # cov[layer] is not modified
    return c, S_model, D_model, out, (Cd, mud, Wd, idxd, bd)


@pytest.mark.parametrize("size", SIZES)
def test_refit_on_the_centred_statistic_matches_the_model(size):
    c, S_model, D_model, out, _ = _case(*size)
    assert np.array_equal(out["S"].numpy(), S_model)          # (exact inputs, one rounding each: the same bits)
    err = NS.column_error(out["f64"].numpy(), D_model.T)
    print(f"{size}: D column error {err:.3e}")
    assert err <= 1e-7
    got = out["down"].to(torch.float64).numpy()
    want = M.bf16_round(D_model.astype(np.float64))
    off = got != want
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-300))) - 7)
    assert np.all(np.abs(got - want)[off] <= ulp[off] * 1.0000001)
    print(f"{size}: bf16 entries one ulp off: {off.mean():.2e}")
    assert off.mean() <= 1e-3


@pytest.mark.parametrize("size", SIZES)
def test_bias_and_norms_within_their_bounds(size):
    c, _, _, out, _ = _case(*size)
    n, r, d = size
    W, mu, idx, b_d = c["W"], c["mu"], c["idx"], c["b_d"]
    D_hat = out["down"].to(torch.float64).numpy()
    for got, b in ((out["bias64"], b_d), (out["bias064"], None)):
        ref, _, _ = M.intercept(W, D_hat, idx, mu, b)
        bound = M.bias_bound(W, D_hat, idx, mu, b)
        err = np.abs(M.ld(got.numpy()) - ref)
        print(f"{size}: bias err / bound max {float((err / bound).max()):.3e}")
        assert np.all(err <= bound)
    # the rounded output is the one rounding of bias_f64 torch's .to() makes
    assert torch.equal(out["bias"], out["bias64"].to(torch.bfloat16)) and torch.equal(out["bias0"], out["bias064"].to(torch.bfloat16))
    assert out["bias"].dtype == torch.bfloat16
    # norms: against the rows the device produced (bias_f64 without b_d is delta; with a zero D^ it is W_d mu)
    from modegpt_amd import ops
    _, mud, Wd, idxd, _ = _case(*size)[4]
    _, wmu, norms_z = ops.nystrom_intercept(Wd, torch.zeros_like(_case(*size)[3]["down"]).cuda(), idxd, mud)
    wmu, norms_z = M.ld(wmu.cpu().numpy()), norms_z.cpu().numpy()
    dl = M.ld(out["bias064"].numpy())
    for got, rows in ((out["norms0"][0].item(), dl), (out["norms0"][1].item(), wmu), (norms_z[0], wmu), (norms_z[1], wmu)):
        s = (rows * rows).sum()
        assert abs(M.LD(got) - s) <= (d + 2) * M.LD(U) * s
    assert torch.equal(out["norms"], out["norms0"])           # b_d does not enter the norms
    assert norms_z[0] == norms_z[1]


@pytest.mark.parametrize("size", SIZES)
def test_stored_tensors_leave_no_mean_error_on_the_tokens(size):
    """The test that fails without the feature: from the token matrix and the STORED tensors, in long double."""
    c, _, D_model, out, _ = _case(*size)
    H, W, mu, idx, b_d = c["H"], c["W"], c["mu"], c["idx"], c["b_d"]
    D_hat = out["down"].to(torch.float64).numpy()
    bias = out["bias"].to(torch.float64).numpy()
    dl, _ = M.delta(W, D_hat, idx, mu)
    # the bias is b_d + delta rounded once: 2^-8 of the stored value's magnitude, which is |delta| where there is no b_d
    for stored, b, mag in ((bias, b_d, np.abs(M.ld(b_d) + dl)), (out["bias0"].to(torch.float64).numpy(), None, np.abs(dl))):
        bound = 2.0 ** -8 * mag + M.bias_bound(W, D_hat, idx, mu, b)
        mean_on, sq_on = M.token_errors(H, W, idx, D_hat, bias=stored, b_d=b)
        print(f"{size}: |mean y - y'| / bound max {float((np.abs(mean_on) / bound).max()):.3f}")
        assert np.all(np.abs(mean_on) <= bound)
    # against the model's own stored pair
    D_m = M.bf16_round(D_model.astype(np.float64))
    b_m = M.bf16_round(M.intercept(W, D_m, idx, mu, b_d)[0].astype(np.float64))
    _, sq_model = M.token_errors(H, W, idx, D_m, bias=b_m, b_d=b_d)
    mean_on, sq_on = M.token_errors(H, W, idx, D_hat, bias=bias, b_d=b_d)
    assert abs(sq_on - sq_model) <= 1e-3 * sq_model
    # the linear refit (the switch off): the stored tensor of the refit on C, the bias unchanged
    D_lin = out["down_lin"].to(torch.float64).numpy()
    mean_off, sq_off = M.token_errors(H, W, idx, D_lin, bias=b_d, b_d=b_d)
    print(f"{size}: sum ||y - y'||^2 on {float(sq_on):.6e} off {float(sq_off):.6e};  max |mean| on {float(np.abs(mean_on).max()):.3e} "
          f"off {float(np.abs(mean_off).max()):.3e}")
    assert sq_on < sq_off


@pytest.mark.parametrize("size", SIZES)
def test_linear_refit_leaves_a_mean_the_intercept_removes(size):
    """Host model only (see the module docstring): what the linear refit leaves of the mean, against what one bf16 rounding of the
    intercept leaves.  Summed over the channels, the squared mean error of the linear refit exceeds the intercept's."""
    c = M.make_case(*size, tokens=512, seed=0)
    H, W, C, mu, idx = (c[k] for k in ("H", "W", "C", "mu", "idx"))
    D_on = M.bf16_round(M.refit(M.center(C, mu).astype(np.float64), idx, W, EPS).astype(np.float64))
    b_on = M.bf16_round(M.intercept(W, D_on, idx, mu)[0].astype(np.float64))
    D_off = M.bf16_round(M.refit(C, idx, W, EPS).astype(np.float64))
    mean_on, sq_on = M.token_errors(H, W, idx, D_on, bias=b_on)
    mean_off, sq_off = M.token_errors(H, W, idx, D_off)
    assert sq_on < sq_off and (mean_off ** 2).sum() > (mean_on ** 2).sum()


class _Lin:
    def __init__(self, w, b=None):
        self.weight, self.bias = w, b


@pytest.mark.parametrize("size", SIZES)
def test_compress_weights_switch_changes_down_and_down_bias_only(size):
    from modegpt_amd import ops
    from modegpt_amd.compression.compress_mlp import compress_weights
    n, r, d = size
    c, _, _, out, (Cd, mud, Wd, idxd, bd) = _case(*size)
    dev = Cd.device
    rows = torch.arange(n, device=dev)
    tag = torch.stack([rows // 16, rows % 16], dim=1).to(torch.bfloat16)          # row i of up / gate names i: the selection shows in them
    g = torch.Generator(device="cpu").manual_seed(1)
    W_u = torch.cat([tag, torch.randn(n, d - 2, generator=g).to(dev).to(torch.bfloat16)], dim=1)
    W_g = torch.cat([tag, torch.randn(n, d - 2, generator=g).to(dev).to(torch.bfloat16)], dim=1)
    keep = r / n + 1e-9
    assert int(n * keep) == r
    results = {}
    for name, bias in (("plain", None), ("biased", bd)):
        comps = types.SimpleNamespace(up_proj=_Lin(W_u), gate_proj=_Lin(W_g), down_proj=_Lin(Wd, bias))
        off_b, on_b, on_nc, norms = {}, {}, {}, []
        off = compress_weights(comps, Cd, keep, 0, 1e-2, bias_out=off_b)
        on = compress_weights(comps, Cd, keep, 0, 1e-2, bias_out=on_b, intercept=mud, intercept_out=norms)
        nc = compress_weights(comps, Cd, keep, 0, 1e-2, bias_out=on_nc, intercept=mud, carry_bias=False)
        torch.cuda.synchronize()
        assert off[3] == on[3] == r
        assert torch.equal(off[0], on[0]) and torch.equal(off[2], on[2])          # up, gate: the same bits
        sel = (on[0].T[:, 0].to(torch.int64) * 16 + on[0].T[:, 1].to(torch.int64))
        assert torch.equal(sel, ops.select_smallest_sorted(ops.ridge_scores(Cd, float(torch.tensor(1e-2, dtype=torch.float32))), r).to(torch.int64))
        # down: the refit on S for this selection, and its intercept
        S = ops.cov_center(Cd, mud)
        want = ops.nystrom_down(S, sel, Wd, eps=EPS)
        assert torch.equal(on[1].T, want) and torch.equal(off[1].T, ops.nystrom_down(Cd, sel, Wd, eps=EPS))
        wb, _, wn = ops.nystrom_intercept(Wd, want, sel, mud, b_d=bias)
        assert set(on_b) == {"down_bias"} and torch.equal(on_b["down_bias"], wb) and torch.equal(norms[0], wn)
        assert set(off_b) == (set() if bias is None else {"down_bias"})
        if bias is not None:
            assert torch.equal(off_b["down_bias"], bias)
        assert torch.equal(on_nc["down_bias"], ops.nystrom_intercept(Wd, want, sel, mud)[0]) and torch.equal(nc[1], on[1])
    with pytest.raises(ValueError):
        compress_weights(comps, Cd, keep, 0, 1e-2, intercept=mud)


def test_nan_in_one_row_of_the_weight_stays_in_that_rows_bias():
    from modegpt_amd import ops
    n, r, d = SIZES[0]
    c, _, _, out, (Cd, mud, Wd, idxd, bd) = _case(n, r, d)
    W2 = Wd.clone()
    W2[17, 33] = float("nan")
    down = out["down"].to(Cd.device)
    bias, bias64, norms = ops.nystrom_intercept(W2, down, idxd, mud, b_d=bd)
    torch.cuda.synchronize()
    bad = torch.isnan(bias64).cpu()
    assert bad[17] and int(bad.sum()) == 1 and bool(torch.isnan(bias[17])) and bool(torch.isnan(norms).all())
    keep = ~bad
    assert torch.equal(bias64.cpu()[keep], out["bias64"][keep])
    # ... and the fp64 weight path gives the same sums as the bf16 one (the same values, the same order of additions)
    b64 = ops.nystrom_intercept(Wd.to(torch.float64), down, idxd, mud, b_d=bd)[1]
    bound = M.bias_bound(c["W"], down.cpu().to(torch.float64).numpy(), c["idx"], c["mu"], c["b_d"])
    assert np.all(np.abs(M.ld(b64.cpu().numpy()) - M.ld(out["bias64"].numpy())) <= 2 * bound)
