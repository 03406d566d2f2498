"""GPU: mdg_vo_bias (the v_proj / o_proj biases through the V/O truncation) against the long double model of tests/bias_model.py.

Every case runs mdg_vo_compress and then mdg_vo_bias in both forms (b_o given: the fold; b_o NULL: the projected v bias) through the
raw C ABI, with a padded ld_wo and NaN-filled guard regions around every output.  The bounds are a priori (u = 2^-53, N = n_heads hd):
  o_bias_i            within (N + 1) u (|b_o,i| + sum_j |W_o,ij b_j|)            any summation order of N products and one more add
  resid               within (N + 2) u of the sum of absolute terms: sum_i (sum_j |W_o,ij b_j|)^2 for ||sum_h W_o,h b_v||^2 and
                      sum_i (sum_j |W_o,ij| (|b_j| + |(Pi b)_j|))^2 for ||rho||^2
  W_o,h' v_bias_g     against W_o,h Pi_g b_v,g to rel 1e-8, the tolerance the invariant per-head products are held to (DESIGN.md
                      section 2); it does not depend on the signs the eigensolvers pick
The inputs (bias_model.make_case) give the truncated spectrum a step sigma_r / sigma_r+1 >= 2 at the tested rank -- asserted on the
host model below, so a lost gap fails loudly -- and keep every eigenproblem well conditioned, so the host's fp64 eigh and the device's
Jacobi sweep agree on Pi far below these bounds.  bf16 cases hold bf16 values, whose products sum exactly in fp64 (those cases check
the indexing, not the rounding); the f64 cases hold full fp64 values."""
import functools

import numpy as np
import pytest
import torch

from tests import bias_model as B

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
GUARD = 16

# (n_heads, n_kv, hd, d): GQA, MHA two-SVD, the largest head; ranks hd, an even ~0.75 hd, 2
SHAPES = [(4, 2, 32, 64), (4, 4, 32, 64), (8, 2, 128, 256)]
CASES = [(s, r, w) for s in SHAPES for r in (s[2], (3 * s[2] // 4) & ~1, 2) for w in ("bf16", "f64")]
# beyond the issue's list: two column chunks of 2048 (N = 2560); rows that do not fill the last workgroup (d = 20) with the 16-byte
# loads; a row length that is no multiple of 8 (N = 18: scalar tail), MHA
EXTRA = [((20, 2, 128, 256), 96, "bf16"), ((4, 2, 8, 20), 6, "bf16"), ((3, 3, 6, 20), 4, "bf16"), ((4, 2, 8, 20), 6, "f64")]


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    host = buf.cpu()
    return bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + n:]).all())


def _run(dev, Wv, Wo, C, b_v, b_o, shape, rank, wdt, pad):
    """mdg_vo_compress + mdg_vo_bias in both forms through the C ABI.  Returns host arrays."""
    from modegpt_amd import _lib
    lib = _lib.load()
    n_heads, n_kv, hd, d = shape
    N = n_heads * hd
    tdt = torch.bfloat16 if wdt == "bf16" else torch.float64
    code = _lib.MDG_BF16 if wdt == "bf16" else _lib.MDG_F64
    ld_wo = N + pad
    Wo_buf = torch.full((d, ld_wo), float("nan"), dtype=tdt, device=dev)       # (the padding is never read: it would poison the sums)
    Wo_buf[:, :N] = torch.from_numpy(Wo).to(dev).to(tdt)
    Wv_d = torch.from_numpy(Wv).to(dev).to(tdt).contiguous()
    C_d = torch.from_numpy(C).to(dev).contiguous()
    bv_d = torch.from_numpy(b_v).to(dev).to(tdt)               # (biases in the weights' dtype: make_case gave them its values)
    bo_d = torch.from_numpy(b_o).to(dev).to(tdt)
    nbytes = lib.mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    v_out = torch.empty(n_kv * rank, d, dtype=torch.bfloat16, device=dev)
    o_out = torch.empty(d, n_heads * rank, dtype=torch.bfloat16, device=dev)
    v64 = torch.empty(n_kv * rank, d, dtype=torch.float64, device=dev)
    o64 = torch.empty(d, n_heads * rank, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _lib.check(lib.mdg_vo_compress(C_d.data_ptr(), d, d, Wv_d.data_ptr(), d, Wo_buf.data_ptr(), ld_wo, code, n_heads, n_kv, hd, rank,
                                       0.0, v_out.data_ptr(), d, o_out.data_ptr(), n_heads * rank, v64.data_ptr(), o64.data_ptr(),
                                       ws.data_ptr(), nbytes, st), "mdg_vo_compress")
        out = {}
        for form, bo in (("fold", bo_d), ("project", None)):
            ob_buf, ob = _guarded(d, dev)
            vb_buf, vb = _guarded(n_kv * rank, dev)
            rs_buf, rs = _guarded(2, dev)
            _lib.check(lib.mdg_vo_bias(ws.data_ptr(), nbytes, Wo_buf.data_ptr(), ld_wo, code, d, bv_d.data_ptr(),
                                       None if bo is None else bo.data_ptr(), code, n_heads, n_kv, hd, rank, ob.data_ptr(),
                                       vb.data_ptr(), rs.data_ptr(), st), "mdg_vo_bias")
            torch.cuda.synchronize(dev)
            assert _guards_intact(ob_buf, d) and _guards_intact(vb_buf, n_kv * rank) and _guards_intact(rs_buf, 2), form
            out[form] = {"o_bias": ob.cpu().numpy().copy(), "v_bias": vb.cpu().numpy().copy(), "resid": rs.cpu().numpy().copy()}
    out["o64"] = o64.cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _case(shape, rank, wdt, pad=8):
    n_heads, n_kv, hd, d = shape
    dev = torch.device("cuda:0")
    Wv, Wo, C, b_v, b_o = B.make_case(n_heads, n_kv, hd, d, rank, seed=1000 + 7 * rank + hd + n_kv, bf16=wdt == "bf16")
    got = _run(dev, Wv, Wo, C, b_v, b_o, shape, rank, wdt, pad)
    facs = B.factors(Wv, Wo, C, n_heads, n_kv, hd, rank)
    return (Wv, Wo, C, b_v, b_o), got, facs


def _ids(c):
    s, r, w = c
    return f"h{s[0]}kv{s[1]}hd{s[2]}d{s[3]}-r{r}-{w}"


@pytest.mark.parametrize("case", CASES + EXTRA, ids=_ids)
def test_fold_into_o_bias(dev, case):
    shape, rank, wdt = case
    n_heads, n_kv, hd, d = shape
    (Wv, Wo, C, b_v, b_o), got, _ = _case(shape, rank, wdt)
    want, absolute = B.fold(Wo, b_v, b_o, n_heads, n_kv, hd)
    o_bias = got["fold"]["o_bias"]
    err = np.abs(B.ld(o_bias) - want)
    bound = (n_heads * hd + 1) * U * absolute
    worst = float((err / bound).max())
    print(f"o_bias: worst error / bound = {worst:.3e}")
    assert np.all(np.isfinite(o_bias)) and np.all(err <= bound), worst
    # written only with b_o; the other form leaves it alone, and the fold leaves v_bias alone
    assert np.all(np.isnan(got["project"]["o_bias"])) and np.all(np.isnan(got["fold"]["v_bias"]))


@pytest.mark.parametrize("case", CASES + EXTRA, ids=_ids)
def test_projected_v_bias_through_the_sign_free_invariant(dev, case):
    shape, rank, wdt = case
    n_heads, n_kv, hd, d = shape
    (Wv, Wo, C, b_v, b_o), got, facs = _case(shape, rank, wdt)
    for _, _, lam in facs:
        assert B.sigma_ratio(lam, rank) >= 2.0, "the inputs lost the step of their truncated spectrum"
    v_bias = got["project"]["v_bias"]
    assert np.all(np.isfinite(v_bias))
    kept = B.kept_part(facs, b_v, hd)
    g = n_heads // n_kv
    worst = 0.0
    for h in range(n_heads):
        kv = h // g
        have = B.ld(got["o64"][:, h * rank:(h + 1) * rank]) @ B.ld(v_bias[kv * rank:(kv + 1) * rank])
        want = B.ld(Wo[:, h * hd:(h + 1) * hd]) @ kept[kv * hd:(kv + 1) * hd]
        worst = max(worst, float(np.abs(have - want).max() / np.abs(want).max()))
    print(f"W_o' v_bias against W_o Pi b_v: worst rel {worst:.3e}")
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("case", CASES + EXTRA, ids=_ids)
def test_residual_norms(dev, case):
    shape, rank, wdt = case
    n_heads, n_kv, hd, d = shape
    N = n_heads * hd
    (Wv, Wo, C, b_v, b_o), got, facs = _case(shape, rank, wdt)
    resid = got["project"]["resid"]
    assert np.array_equal(resid, got["fold"]["resid"])                          # both forms report the same two numbers
    const, abs_const = B.fold(Wo, b_v, None, n_heads, n_kv, hd)
    rho, abs_rho = B.residual(Wo, facs, b_v, n_heads, n_kv, hd)
    want = (float((rho * rho).sum()), float((const * const).sum()))
    tol = ((N + 2) * U * float((abs_rho * abs_rho).sum()), (N + 2) * U * float((abs_const * abs_const).sum()))
    print(f"||rho||^2: {resid[0]:.6e} (model {want[0]:.6e}, |diff| / tol {abs(resid[0] - want[0]) / tol[0]:.3e}); "
          f"||sum W_o b_v||^2: {resid[1]:.6e} (model {want[1]:.6e}, |diff| / tol {abs(resid[1] - want[1]) / tol[1]:.3e})")
    assert abs(resid[1] - want[1]) <= tol[1]
    assert abs(resid[0] - want[0]) <= tol[0]
    if rank == hd:
        # nothing is truncated: rho is the rounding of Q P against the identity.  ||rho|| <= ||W_o||_F ||(I - Q P) b||, and the
        # factors' P Q differs from I by the eigensolver's orthogonality error and one rounding per entry of hd-long sums, scaled by
        # the condition of S: taken as 16 hd kappa u
        kappa = max(float(np.sqrt(lam.max() / lam.min())) for _, _, lam in facs)
        b = B.expand_bias(b_v, n_heads, n_kv, hd)
        floor = (16 * hd * kappa * U) ** 2 * float((Wo * Wo).sum()) * float((b * b).sum())
        print(f"rank = hd: ||rho||^2 / ||sum W_o b_v||^2 = {resid[0] / resid[1]:.3e}")
        assert 0.0 <= resid[0] <= floor, (resid[0], floor)
    else:
        assert resid[0] > 1e-6 * resid[1]                                       # (the inputs can see the truncation)


@pytest.mark.parametrize("wdt,pad", [("bf16", 3), ("bf16", 0), ("f64", 1)])
def test_row_alignment_does_not_change_the_bits(dev, wdt, pad):
    """ld_wo that rules the 16-byte loads out (scalar loads in the same per-lane order would differ: the vector path sums eight
    neighbours per lane) still meets the bounds; an unpadded matrix gives the padded one's bits."""
    shape, rank = SHAPES[0], 24
    (Wv, Wo, C, b_v, b_o), ref, facs = _case(shape, rank, wdt)
    _, got, _ = _case(shape, rank, wdt, pad)
    n_heads, n_kv, hd, d = shape
    want, absolute = B.fold(Wo, b_v, b_o, n_heads, n_kv, hd)
    assert np.all(np.abs(B.ld(got["fold"]["o_bias"]) - want) <= (n_heads * hd + 1) * U * absolute)
    assert np.array_equal(got["project"]["v_bias"], ref["project"]["v_bias"])   # (P b_v never reads W_o)
    if pad == 0 or wdt == "f64":
        for form in ("fold", "project"):
            for k in ("o_bias", "v_bias", "resid"):
                assert np.array_equal(got[form][k], ref[form][k], equal_nan=True), (form, k)


def test_ops_front_end_gives_the_raw_call_and_repeats_bit_for_bit(dev):
    from modegpt_amd import ops
    shape, rank = SHAPES[0], 24
    n_heads, n_kv, hd, d = shape
    (Wv, Wo, C, b_v, b_o), ref, _ = _case(shape, rank, "bf16", 0)
    t = lambda a, dt: torch.from_numpy(a).to(dev).to(dt)      # noqa: E731
    args = (t(C, torch.float64), t(Wv, torch.bfloat16), t(Wo, torch.bfloat16), n_heads, n_kv, hd, rank, 0.0)
    plain = ops.vo_compress(*args)
    for _ in range(2):
        out = ops.vo_compress(*args, bias=(t(b_v, torch.bfloat16), t(b_o, torch.bfloat16)))
        assert len(out) == 3 and torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])      # the factors: same bits
        o_bias, v_bias, resid = out[2]
        assert v_bias is None and np.array_equal(o_bias.cpu().numpy(), ref["fold"]["o_bias"])
        assert np.array_equal(resid.cpu().numpy(), ref["fold"]["resid"])
    o_bias, v_bias, resid = ops.vo_compress(*args, want_f64=True, want_spectrum=True, want_curve=True,
                                            bias=(t(b_v, torch.bfloat16), None))[-1]
    assert o_bias is None and np.array_equal(v_bias.cpu().numpy(), ref["project"]["v_bias"])
    assert np.array_equal(resid.cpu().numpy(), ref["project"]["resid"])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]], ids=["gqa", "mha"])
def test_nan_in_one_heads_bias_stays_in_that_head(dev, shape):
    n_heads, n_kv, hd, d = shape
    rank = 24
    (Wv, Wo, C, b_v, b_o), ref, _ = _case(shape, rank, "bf16")
    bad = b_v.copy()
    bad[hd + 3] = float("nan")                                                    # kv head 1
    got = _run(torch.device("cuda:0"), Wv, Wo, C, bad, b_o, shape, rank, "bf16", 8)
    vb, clean = got["project"]["v_bias"], ref["project"]["v_bias"]
    assert np.all(np.isnan(vb[rank:2 * rank]))
    keep = np.r_[0:rank, 2 * rank:n_kv * rank]
    assert np.array_equal(vb[keep], clean[keep])                                  # the other heads: the clean run's bits
    # every output channel sums over all heads, so the fold and both norms carry the NaN; nothing else is touched (guards: _run)
    assert np.all(np.isnan(got["fold"]["o_bias"])) and np.all(np.isnan(got["project"]["resid"]))
