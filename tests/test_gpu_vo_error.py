"""mdg_vo_output_error (ops.vo_output_error) -- what the stored v_proj / o_proj lose of every output channel of every head on the
calibration statistic -- and mdg_vo_rank_curve (ops.vo_compress(want_curve=True)) against the long-double model
tests/vo_error_model.py, and MODEGPT_VO_ERROR=1 end to end.

Forward accuracy.  err = max |got - ref| / a with a[h][k] = (|y| |V_g|) |C| (|y| |V_g|)^T (for dnorm2: || |y| |V_g| ||^2); asserted is
err_kernel <= R * max(err_cpu, 64 (d + hd + r) 2^-53), err_cpu from the same route in plain fp64 numpy (vo_error_model.errors_fp64)
against the same long-double reference -- the criterion of tests/test_gpu_chol.py.  The curve: max_r |curve[r] - ref[r]| / ref[0]
with an R of its own, on inputs whose G has relative gaps >= 1e-3 (asserted on the host model).  Every R is fixed from the GPU run as
4 x the largest observed ratio rounded up to a power of two and may never exceed 32; a larger ratio is a finding, not a tolerance.

MEASURED on an MI355X (every test prints its figure before it asserts: lines FORWARD, CURVE, IDENTITY, E2E under pytest -s)
Forward ratios err_kernel / max(err_cpu, 64 (d + hd + r) u), 126 figures (e, dnorm2, q and its norm; bf16 and fp64 factors); err_kernel
and err_cpu themselves are 0 .. 4e-16 of a in every case, so the floor decides:
    largest for e / q:        3.95e-4  (acts d=70 4/2 hd=2 r=0 fp32 weights: err_kernel 2.0e-16, err_cpu 1.7e-16)
    largest for the norms:    6.30e-4  (the same case: err_kernel 3.2e-16, err_cpu 3.7e-16)
    hd = 128:                 1.8e-7 .. 8.0e-6 (d = 257 / 384, r = 1 / 88 / 128)
    -> 4 x 6.30e-4 = 2.5e-3 -> RATIO = 2^-8.
Curve ratios (err_kernel and err_cpu agree to 10 % everywhere: both carry the 1 / gap amplification of the eigenvectors):
    hd=16 d=70 4/2: 5.7e-3   hd=6 d=257 3/1: 2.4e-4   hd=64 d=70 2/2 (MHA): 3.8e-2   hd=128 d=257 3/1: 1.9e-2   hd=2 d=1: 3.7e-2
    -> 4 x 3.77e-2 = 0.15 -> CURVE_RATIO = 2^-2.
Identity on the device's fp64 factors, |objective - curve[r]| as a fraction of 64 (d + hd + r) u sum a (x cond for MHA):
    grouped 4/2 hd=16 r=11: 2.8e-6, 8.7e-6 (1.2e-16, 3.5e-16 of curve[0])   MHA 2/2: 7.5e-8, 7.3e-8 (cond 28, 19)   3/1 hd=64 r=40: 3.6e-8
    -> 4 x 8.72e-6 = 3.5e-5 -> IDENTITY_RATIO = 2^-14.   The bf16 artefact's excess_over_curve: 3.6e-6 .. 1.3e-5, positive everywhere.
End to end (tiny models, 4 heads of 32, ranks 22 / 16): relative_error 9.9e-2 / 2.1e-1 (llama_gqa) and 6.9e-2 / 1.1e-1 (opt),
excess_over_curve 4.7e-6 .. 1.4e-5, noise floor 1.3e-12 of the energy; the run from saved statistics gives the same report.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests import vo_error_model as VO
from tests.test_gpu_chol import matrix

pytestmark = pytest.mark.gpu
F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -53
RATIO = 2.0 ** -8                          # R of the forward criterion (module docstring: 4 x 6.30e-4 rounded up to a power of two)
CURVE_RATIO = 2.0 ** -2                    # R of the curve's criterion (4 x 3.77e-2 rounded up)
IDENTITY_RATIO = 2.0 ** -14                # R2 of the identity on the device (4 x 8.72e-6 rounded up)
RIDGE = 1e-5                               # ridge_vo of the end-to-end configurations


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def problem(kind, d, n_heads, n_kv, hd, wdt, grade=1.0):
    """(C, W_v, W_o) on the host, computed once, never modified."""
    Wv, Wo = VO.weights(d, n_heads, n_kv, hd, wdt, seed=len(kind), grade=grade)
    return matrix(kind, d)[0], Wv, Wo


@functools.lru_cache(maxsize=None)
def device_factors(kind, d, n_heads, n_kv, hd, r, wdt, grade=1.0):
    """(v bf16, o bf16, v_f64, o_f64, curve) of the device's own vo_compress, computed once per case, never modified."""
    from modegpt_amd import ops as _ops
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, wdt, grade)
    return _ops.vo_compress(C.to("cuda:0"), Wv.to("cuda:0"), Wo.to("cuda:0"), n_heads, n_kv, hd, r, RIDGE, want_f64=True, want_curve=True)


@functools.lru_cache(maxsize=None)
def model(kind, d, n_heads, n_kv, hd, r, wdt, form):
    """The long-double reference and the fp64 restatement for the device's factors of `form` (None: q)."""
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, wdt)
    vn = on = None
    if form is not None:
        f = device_factors(kind, d, n_heads, n_kv, hd, r, wdt)
        vn, on = (f[0].cpu(), f[1].cpu()) if form == "bf16" else (f[2].cpu(), f[3].cpu())
    return VO.errors(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on), VO.errors_fp64(C, Wv, Wo, n_heads, n_kv, hd, r, vn, on)


def check_forward(what, got, ref, cpu, a, size, ratio_max=None):
    """err <= RATIO * max(err_cpu, 64 size u), errors relative to a; where a = 0 the value itself must be 0.  Prints first."""
    got, cpu = R.ld(got), R.ld(cpu)
    live = a > 0
    assert bool((got[~live] == 0).all())
    err = float((np.abs(got - ref)[live] / a[live]).max()) if live.any() else 0.0
    err_cpu = float((np.abs(cpu - ref)[live] / a[live]).max()) if live.any() else 0.0
    ratio = err / max(err_cpu, 64 * size * U)
    print("FORWARD %-64s err_kernel %.3e err_cpu %.3e ratio %.2e" % (what, err, err_cpu, ratio))
    assert ratio <= (RATIO if ratio_max is None else ratio_max), "%s: err_kernel %.3e, err_cpu %.3e, ratio %.3g" % (what, err, err_cpu, ratio)
    return ratio


# ---------------------------------------------------------------- against the long-double model
# (hd, r): a stitch inside a 16-deep stage, n = hd + r exactly one tile, one past a tile, the production width, two full tiles.
# d: one element, below a tile, one past two tiles, three tiles.  hd = 128 only with n_heads <= 4 and d <= 384; d = 384 with at most
# two heads, so that the long-double model (d^3 per head) stays within seconds.
H11, H22, H42, H31, H41 = (1, 1), (2, 2), (4, 2), (3, 1), (4, 1)
MODEL_CASES = [
    (2, 1, 1, H11, "p3", BF16), (2, 1, 70, H42, "acts", torch.float32), (2, 1, 257, H31, "p6g3", BF16),
    (6, 5, 70, H31, "p3", torch.float32), (6, 5, 1, H22, "p6g3", BF16), (6, 5, 384, H11, "acts", BF16),
    (16, 11, 70, H42, "p6g3", BF16), (16, 11, 257, H41, "acts", torch.float32), (16, 11, 384, H22, "p3", BF16),
    (64, 64, 70, H41, "acts", BF16), (64, 64, 257, H22, "p3", torch.float32), (64, 64, 1, H31, "p6g3", BF16),
    (128, 1, 70, H31, "p6g3", torch.float32), (128, 1, 257, H42, "p3", BF16), (128, 1, 384, H11, "acts", BF16),
    (128, 88, 70, H42, "acts", BF16), (128, 88, 257, H22, "p6g3", torch.float32), (128, 88, 384, H22, "p3", BF16),
    (128, 128, 70, H41, "p3", BF16), (128, 128, 257, H11, "acts", torch.float32), (128, 128, 384, H22, "p6g3", BF16),
]


@pytest.mark.parametrize("form", ["bf16", "f64"])
@pytest.mark.parametrize("hd,r,d,heads,kind,wdt", MODEL_CASES,
                         ids=["hd%d-r%d-d%d-h%dkv%d-%s-%s" % (hd, r, d, h[0], h[1], k, str(w)[6:]) for hd, r, d, h, k, w in MODEL_CASES])
def test_error_against_long_double_model(ops, dev, hd, r, d, heads, kind, wdt, form):
    n_heads, n_kv = heads
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, wdt)
    f = device_factors(kind, d, n_heads, n_kv, hd, r, wdt)
    vn, on = (f[0], f[1]) if form == "bf16" else (f[2], f[3])
    (ref, ref_n, a, an), (cpu, cpu_n) = model(kind, d, n_heads, n_kv, hd, r, wdt, form)
    what = "%s d=%d %d/%d hd=%d r=%d %s %s" % (kind, d, n_heads, n_kv, hd, r, str(wdt)[6:], form)
    e, dn = ops.vo_output_error(C.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, hd, r, vn, on, want_dnorm2=True)
    assert e.shape == dn.shape == (n_heads, d) and e.dtype == dn.dtype == F64 and e.is_cuda
    size = d + hd + r
    check_forward(what + " e", e.cpu(), ref, cpu, a, size)
    check_forward(what + " dnorm2", dn.cpu(), ref_n, cpu_n, an, size)
    assert bool((R.ld(e.cpu()) >= -(RATIO * 64 * size * U) * a).all())                       # C is positive semidefinite
    assert same(ops.vo_output_error(C.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, hd, r, vn, on), e)      # want_dnorm2 does not change e
    if form == "bf16":                                                                       # q once per case
        (qref, qref_n, qa, qan), (qcpu, qcpu_n) = model(kind, d, n_heads, n_kv, hd, 0, wdt, None)
        q, qn = ops.vo_output_error(C.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, hd, 0, None, None, want_dnorm2=True)
        check_forward(what + " q", q.cpu(), qref, qcpu, qa, d + hd)
        check_forward(what + " qnorm2", qn.cpu(), qref_n, qcpu_n, qan, d + hd)


# ---------------------------------------------------------------- exact properties
@pytest.mark.parametrize("hd,r,d,heads,kind,wdt", [(16, 11, 70, H42, "p6g3", BF16), (128, 88, 257, H22, "p6g3", torch.float32)])
def test_exact_properties(ops, dev, hd, r, d, heads, kind, wdt):
    n_heads, n_kv = heads
    C, Wv, Wo = (t.to(dev) for t in problem(kind, d, n_heads, n_kv, hd, wdt))
    vb, ob, v64, o64, _ = device_factors(kind, d, n_heads, n_kv, hd, r, wdt)
    call = lambda *a, **kw: ops.vo_output_error(C, Wv, Wo, n_heads, n_kv, hd, *a, **kw)       # noqa: E731
    # v_new = None and rank = 0 are the same call
    q, qn = call(0, None, None, want_dnorm2=True)
    q1, qn1 = call(r, None, None, want_dnorm2=True)
    q2, qn2 = call(0, vb[:0], ob[:, :0], want_dnorm2=True)
    assert same(q, q1) and same(qn, qn1) and same(q, q2) and same(qn, qn2)
    assert bool((q > 0).all()) and bool((qn > 0).all())
    for vn, on in ((vb, ob), (v64, o64)):
        a, an = call(r, vn, on, want_dnorm2=True)
        b, bn = call(r, vn, on, want_dnorm2=True)
        with ops.DeferredStatus(dev) as st:
            c, cn = call(r, vn, on, want_dnorm2=True)
        st.check()
        assert same(a, b) and same(an, bn) and same(a, c) and same(an, cn)                    # two runs; inside and outside
        assert same(call(r, vn, on), a)                                                       # want_dnorm2 does not change e
        assert bool(torch.isfinite(a).all()) and float(a.sum()) < float(q.sum())              # the truncation loses less than everything


@pytest.mark.parametrize("heads", [H42, H22], ids=["grouped", "mha"])
def test_curve_exact_properties(ops, dev, heads):
    n_heads, n_kv = heads
    hd, r, d, kind = 16, 11, 70, "acts"
    C, Wv, Wo = (t.to(dev) for t in problem(kind, d, n_heads, n_kv, hd, BF16))
    plain = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, hd, r, RIDGE, want_f64=True)
    with_curve = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, hd, r, RIDGE, want_f64=True, want_curve=True)
    again = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, hd, r, RIDGE, want_f64=True, want_spectrum=True, want_curve=True)
    with ops.DeferredStatus(dev) as st:
        inside = ops.vo_compress(C, Wv, Wo, n_heads, n_kv, hd, r, RIDGE, want_f64=True, want_curve=True)
    st.check()
    for i in range(2):
        assert torch.equal(plain[i].view(torch.int16), with_curve[i].view(torch.int16))       # the factors: the same bits
    for i in (2, 3):
        assert same(plain[i], with_curve[i])
    curve = with_curve[-1]
    assert curve.shape == (n_kv, hd + 1) and curve.dtype == F64 and curve.is_cuda
    assert same(curve, again[-1]) and same(curve, inside[-1]) and again[-2].shape == (n_kv, 8)
    assert bool((bits(curve[:, hd]) == 0).all())                                              # +0.0
    assert bool((curve[:, 1:] <= curve[:, :-1]).all()) and bool((curve[:, 0] > 0).all())


# ---------------------------------------------------------------- the curve against the model
CURVE_CASES = [(16, 70, H42, "acts", BF16, 0.8), (6, 257, H31, "p6g3", torch.float32, 0.7), (64, 70, H22, "p3", BF16, 0.93),
               (128, 257, H31, "acts", BF16, 0.96), (2, 1, H11, "p3", BF16, 0.5)]


@pytest.mark.parametrize("hd,d,heads,kind,wdt,grade", CURVE_CASES,
                         ids=["hd%d-d%d-h%dkv%d-%s" % (hd, d, h[0], h[1], k) for hd, d, h, k, w, g in CURVE_CASES])
def test_curve_against_long_double_model(ops, dev, hd, d, heads, kind, wdt, grade):
    n_heads, n_kv = heads
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, wdt, grade)
    spec = VO.spectra(C, RIDGE, Wv, Wo, n_heads, n_kv, hd)
    for lam, _, lam2, _ in spec:                                 # the reference is itself determined
        assert VO.min_relative_gap(lam) >= 1e-3 and (lam2 is None or VO.min_relative_gap(lam2) >= 1e-3)
    ref = VO.curve(C, RIDGE, Wv, Wo, n_heads, n_kv, hd, spec=spec)
    cpu = R.ld(VO.curve(C, RIDGE, Wv, Wo, n_heads, n_kv, hd, dtype=np.float64))
    got = R.ld(device_factors(kind, d, n_heads, n_kv, hd, max(1, hd // 2), wdt, grade)[-1].cpu())
    err = float((np.abs(got - ref).max(axis=1) / ref[:, 0]).max())
    err_cpu = float((np.abs(cpu - ref).max(axis=1) / ref[:, 0]).max())
    ratio = err / max(err_cpu, 64 * (d + hd) * U)
    print("CURVE %s d=%d %d/%d hd=%d: err_kernel %.3e err_cpu %.3e ratio %.2e" % (kind, d, n_heads, n_kv, hd, err, err_cpu, ratio))
    assert ratio <= CURVE_RATIO
    assert bool((got[:, hd] == 0).all()) and bool((np.diff(got, axis=1) <= 0).all())


# ---------------------------------------------------------------- the identity on the device
@pytest.mark.parametrize("hd,r,d,heads,kind", [(16, 11, 70, H42, "acts"), (16, 11, 70, H22, "p3"), (64, 40, 70, H31, "p6g3")],
                         ids=["grouped", "mha", "grouped-hd64"])
def test_identity_on_the_device(ops, dev, hd, r, d, heads, kind):
    """vo_compress's own fp64 factors: |sum_{h in g} sum_k (e + rho dnorm2) - curve[g][r]| <= R2 64 (d + hd + r) u sum a; the MHA slack
    times max(1, lambda_1 / lambda_hd) of the first spectrum (host model), because S^-1 sits in those factors.  The bf16 artefact's
    excess_over_curve is >= minus that slack (as a fraction of curve[g][0])."""
    n_heads, n_kv = heads
    group = n_heads // n_kv
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, BF16)
    vb, ob, v64, o64, curve = device_factors(kind, d, n_heads, n_kv, hd, r, BF16)
    Cd, Wvd, Wod = C.to(dev), Wv.to(dev), Wo.to(dev)
    q = ops.vo_output_error(Cd, Wvd, Wod, n_heads, n_kv, hd, 0, None, None)
    e, dn = ops.vo_output_error(Cd, Wvd, Wod, n_heads, n_kv, hd, r, v64, o64, want_dnorm2=True)
    eb, dnb = ops.vo_output_error(Cd, Wvd, Wod, n_heads, n_kv, hd, r, vb, ob, want_dnorm2=True)
    a = model(kind, d, n_heads, n_kv, hd, r, BF16, "f64")[0][2]
    spec = VO.spectra(C, RIDGE, Wv, Wo, n_heads, n_kv, hd) if n_kv == n_heads else None
    rho, cv = R.LD(np.float64(RIDGE)), R.ld(curve.cpu())
    decoded = ops.decode_vo_output_error(eb.cpu(), q.cpu(), dnb.cpu(), RIDGE, r, n_kv, curve=curve.cpu())
    for g in range(n_kv):
        rows = slice(g * group, (g + 1) * group)
        objective = (R.ld(e.cpu())[rows] + rho * R.ld(dn.cpu())[rows]).sum()
        cond = max(1.0, float(spec[g][0][0] / spec[g][0][-1])) if spec else 1.0
        unit = 64 * (d + hd + r) * U * float(a[rows].sum()) * cond
        ratio = float(abs(objective - cv[g, r])) / unit
        excess = decoded["heads"][g]["excess_over_curve"]
        print("IDENTITY %s %d/%d hd=%d r=%d kv head %d: |objective - curve[r]| / curve[0] %.3e, ratio to the unit slack %.2e (cond %.2e); "
              "bf16 artefact excess_over_curve %.3e" % (kind, n_heads, n_kv, hd, r, g, float(abs(objective - cv[g, r]) / cv[g, 0]), ratio,
                                                        cond, excess))
        assert ratio <= IDENTITY_RATIO
        assert excess >= -IDENTITY_RATIO * unit / float(cv[g, 0])
        assert decoded["heads"][g]["predicted_objective"] == float(curve[g, r])


# ---------------------------------------------------------------- layout
def padded(A, fill, dev, rows, cols, col0):
    buf = torch.full((A.shape[0] + rows, A.shape[1] + cols), fill, dtype=A.dtype, device=dev)
    view = buf[:A.shape[0], col0:col0 + A.shape[1]]
    view.copy_(A)
    return buf, view


@pytest.mark.parametrize("form", ["bf16", "f64"])
@pytest.mark.parametrize("wdt", [BF16, torch.float32], ids=["bf16", "f32"])
def test_leading_dimensions(ops, dev, form, wdt):
    """ldc > d, ld_wv > d, ld_v > d, W_o / o_new as column-block views of wider NaN-filled buffers (data pointers off the 16-byte
    boundary): the contiguous call bit for bit, the inputs and their surroundings unchanged."""
    hd, r, d, (n_heads, n_kv), kind = 16, 11, 70, H42, "acts"
    C, Wv, Wo = problem(kind, d, n_heads, n_kv, hd, wdt)
    Wv, Wo = (Wv, Wo) if wdt == BF16 else (Wv.double(), Wo.double())                    # (what _as_weight hands the library)
    f = device_factors(kind, d, n_heads, n_kv, hd, r, wdt)
    vn, on = (f[0], f[1]) if form == "bf16" else (f[2], f[3])
    want, want_n = ops.vo_output_error(C.to(dev), Wv.to(dev), Wo.to(dev), n_heads, n_kv, hd, r, vn, on, want_dnorm2=True)
    nan = float("nan")
    bufs, views = zip(*(padded(t, nan, dev, *pad) for t, pad in ((C, (3, 37, 5)), (Wv, (2, 11, 3)), (Wo, (2, 9, 1)), (vn, (3, 5, 1)),
                                                                 (on, (1, 7, 3)))))
    Cd, Wvd, Wod, vd, od = views
    assert Cd.stride(0) == d + 37 and Wvd.stride(0) == d + 11 and vd.stride(0) == d + 5 and Wod.stride(0) == n_heads * hd + 9
    assert all(v.data_ptr() % 16 for v in views)
    before = [b.clone() for b in bufs]
    got, got_n = ops.vo_output_error(Cd, Wvd, Wod, n_heads, n_kv, hd, r, vd, od, want_dnorm2=True)
    assert same(got, want) and same(got_n, want_n)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_n).all())
    raw = lambda t: t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int64)      # noqa: E731
    for b, b0 in zip(bufs, before):
        assert torch.equal(raw(b), raw(b0))


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("form", ["bf16", "f64"])
def test_nan_containment(ops, dev, form):
    hd, r, d, (n_heads, n_kv), kind = 16, 11, 70, H42, "acts"
    C, Wv, Wo = (t.to(dev) for t in problem(kind, d, n_heads, n_kv, hd, BF16))
    f = device_factors(kind, d, n_heads, n_kv, hd, r, BF16)
    vn, on = (f[0], f[1]) if form == "bf16" else (f[2], f[3])
    call = lambda wv, wo, v, o: ops.vo_output_error(C, wv, wo, n_heads, n_kv, hd, r, v, o, want_dnorm2=True)      # noqa: E731
    clean, clean_n = call(Wv, Wo, vn, on)

    def only(mask, e, dn):
        assert torch.equal(torch.isnan(e), mask) and torch.equal(torch.isnan(dn), mask)
        assert torch.equal(bits(e)[~mask], bits(clean)[~mask]) and torch.equal(bits(dn)[~mask], bits(clean_n)[~mask])

    def poisoned(t, i, j):
        t = t.clone()
        t[i, j] = float("nan")
        return t
    cell = torch.zeros(n_heads, d, dtype=torch.bool, device=dev)
    one = cell.clone()
    one[2, 5] = True                                             # row 5 of head 2's W_o / o': e[2][5] alone
    only(one, *call(Wv, poisoned(Wo, 5, 2 * hd + 3), vn, on))
    only(one, *call(Wv, Wo, vn, poisoned(on, 5, 2 * r + 10)))
    grp = cell.clone()
    grp[2:4] = True                                              # kv head 1's W_v / v': heads 2 and 3, every channel; group 0 keeps its bits
    only(grp, *call(poisoned(Wv, hd + 7, 9), Wo, vn, on))
    only(grp, *call(Wv, Wo, poisoned(vn, r + 4, 60), on))
    q = ops.vo_output_error(C, poisoned(Wv, 3, 0), Wo, n_heads, n_kv, hd, 0, None, None)
    assert torch.equal(torch.isnan(q), ~grp)
    again, again_n = call(Wv, Wo, vn, on)                        # and a good call passes afterwards
    assert same(again, clean) and same(again_n, clean_n)


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    hd, r, d, (n_heads, n_kv), kind = 16, 11, 70, H42, "p3"
    C, Wv, Wo = (t.to(dev) for t in problem(kind, d, n_heads, n_kv, hd, BF16))
    vb, ob, v64, o64, _ = device_factors(kind, d, n_heads, n_kv, hd, r, BF16)
    e = torch.full((n_heads, d), -1.0, dtype=F64, device=dev)
    nbytes = lib.mdg_vo_output_error_ws_bytes(d, n_heads, n_kv, hd, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(c=C.data_ptr(), d_=d, ldc=d, wv=Wv.data_ptr(), ldwv=d, wo=Wo.data_ptr(), ldwo=n_heads * hd, wdt=_lib.MDG_BF16, nh=n_heads,
             nkv=n_kv, hd_=hd, r_=r, v=vb.data_ptr(), ldv=d, o=ob.data_ptr(), ldo=n_heads * r, ndt=_lib.MDG_BF16, out=e.data_ptr(),
             w=ws.data_ptr(), nb=nbytes):
        return lib.mdg_vo_output_error(c, d_, ldc, wv, ldwv, wo, ldwo, wdt, nh, nkv, hd_, r_, v, ldv, o, ldo, ndt, out, None, w, nb, None)

    bad = [dict(c=None), dict(wv=None), dict(wo=None), dict(out=None), dict(w=None), dict(nb=nbytes - 1), dict(d_=0), dict(ldc=d - 1),
           dict(ldwv=d - 1), dict(ldwo=n_heads * hd - 1), dict(ldv=d - 1), dict(ldo=n_heads * r - 1), dict(wdt=_lib.MDG_F32),
           dict(ndt=_lib.MDG_F16), dict(v=None), dict(o=None), dict(r_=-1), dict(r_=hd + 1), dict(nkv=3), dict(nkv=0), dict(hd_=15),
           dict(hd_=130)]
    for kw in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        with pytest.raises(RuntimeError):                            # what every ops front end turns the status into
            _lib.check(call(**kw), "mdg_vo_output_error")
    assert call(nb=nbytes - 1) == _lib.MDG_ERR_BAD_ARG and b"workspace" in lib.mdg_last_error()
    torch.cuda.synchronize()
    assert bool((e == -1.0).all())                                  # nothing was enqueued
    assert call() == _lib.MDG_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(e).all())
    assert call(r_=0, v=None, o=None) == _lib.MDG_OK                # q
    torch.cuda.synchronize()
    assert bool((e > 0).all())
    # the curve: null pointers, layout, dtype, leading dimension, short workspaces
    vbytes, cbytes = lib.mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd), lib.mdg_vo_rank_curve_ws_bytes(d, n_heads, n_kv, hd)
    vws = torch.zeros(vbytes, dtype=torch.uint8, device=dev)
    cws = torch.empty(cbytes, dtype=torch.uint8, device=dev)
    curve = torch.full((n_kv, hd + 1), -1.0, dtype=F64, device=dev)

    def ccall(vw=vws.data_ptr(), vb_=vbytes, wo=Wo.data_ptr(), ldwo=n_heads * hd, wdt=_lib.MDG_BF16, d_=d, nkv=n_kv, hd_=hd,
              out=curve.data_ptr(), w=cws.data_ptr(), nb=cbytes):
        return lib.mdg_vo_rank_curve(vw, vb_, wo, ldwo, wdt, d_, n_heads, nkv, hd_, out, w, nb, None)

    for kw in [dict(vw=None), dict(wo=None), dict(out=None), dict(w=None), dict(vb_=vbytes - 1), dict(nb=cbytes - 1), dict(ldwo=n_heads * hd - 1),
               dict(wdt=_lib.MDG_F32), dict(d_=0), dict(nkv=3), dict(hd_=15)]:
        assert ccall(**kw) == _lib.MDG_ERR_BAD_ARG, kw
    torch.cuda.synchronize()
    assert bool((curve == -1.0).all())
    assert ccall() == _lib.MDG_OK                                   # (a zeroed workspace: every eigenvalue 0, the curve all +0.0)
    torch.cuda.synchronize()
    assert bool((bits(curve) == 0).all())
    with pytest.raises(RuntimeError):
        ops.vo_output_error(C.cpu(), Wv.cpu(), Wo.cpu(), n_heads, n_kv, hd, 0, None, None)     # no CPU fallback
    with pytest.raises(ValueError):
        ops.vo_output_error(C, Wv, Wo, n_heads, n_kv, hd, r, vb[:-1], ob)


# ---------------------------------------------------------------- end to end: MODEGPT_VO_ERROR=1
@pytest.mark.parametrize("kind", ["llama_gqa", "opt"])
def test_model_end_to_end(dev, kind, tmp_path, monkeypatch):
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_vo import compress_vo, vo_rank_rule
    from tests.test_gpu_e2e import _tiny_model

    model_ = _tiny_model(kind, dev)
    conf = lambda name: CompressionConfig(temp_storage_dir=str(tmp_path / name), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=RIDGE,      # noqa: E731
                                          dataset="synthetic", calib_size=6, calibs_batch_size=4, compression_ratio=0.3,
                                          order="mlp,qk,vo")
    ad = ModelAdapter.from_model(model_, None)
    ad.config = conf("off")
    stats = str(tmp_path / "stats")
    cov_x = load_calibs(ad, n_samples=6, batch_size=4, dataset="synthetic", calibs_save_path=stats, target_layers=[])[3]
    layers = list(range(ad.n_layers))
    keep = [0.7, 0.5][:ad.n_layers] + [0.6] * max(0, ad.n_layers - 2)

    monkeypatch.delenv("MODEGPT_VO_ERROR", raising=False)
    compress_vo(ad, [c.clone() for c in cov_x], keep, target_layers=layers)
    assert ad.report_vo_errors() == {}
    assert "vo_output_error" not in ad.metrics and not getattr(ad, "vo_errors", None)

    def check_on(ad, name):
        report = ad.report_vo_errors()
        assert sorted(report) == layers and sorted(ad.metrics["vo_output_error"]) == [str(l) for l in layers]
        for l in layers:
            m = ad.metrics["vo_output_error"][str(l)]
            q, e, dn, curve = ad.vo_errors[l]
            rank = vo_rank_rule(ad.head_dim, keep[l], ad.arch)
            assert m == report[l] and m["rank"] == rank and m["n_kv"] == ad.n_kv_heads == len(m["heads"])
            assert all(not t.is_cuda and t.dtype == F64 for t in (q, e, dn, curve))
            assert q.shape == e.shape == dn.shape == (ad.n_heads, q.shape[1]) and curve.shape == (ad.n_kv_heads, ad.head_dim + 1)
            assert 0.0 < m["relative_error"] < 1.0 and m["error"] <= m["energy"]
            for g, hm in enumerate(m["heads"]):
                assert hm["predicted_objective"] == float(curve[g, rank])
                assert 0.0 < hm["relative_error"] < 1.0 and hm["error"] <= hm["energy"]
            print("E2E %s %s layer %d: rank %d of %d, relative_error %.3e, worst head %d at %.3e, excess_over_curve %.3e, noise floor %.1e "
                  "of the energy" % (kind, name, l, rank, ad.head_dim, m["relative_error"], m["worst_head"], m["worst_head_relative_error"],
                                     m["excess_over_curve"], m["noise_floor"] / m["energy"]))
        assert ad.report_vo_errors() == {}                          # read once
        return report

    monkeypatch.setenv("MODEGPT_VO_ERROR", "1")
    ad.config = conf("on")
    compress_vo(ad, [c.clone() for c in cov_x], keep, target_layers=layers)
    report = check_on(ad, "on")

    # once through saved statistics: a fresh adapter, no forward pass
    ad2 = ModelAdapter.from_model(model_, None)
    ad2.config = conf("loaded")
    fired = []
    hook = model_.register_forward_pre_hook(lambda *a: fired.append(1))
    try:
        cov_x2 = load_calibs(ad2, n_samples=6, batch_size=4, dataset="synthetic", load_calibs_from=stats, target_layers=[])[3]
    finally:
        hook.remove()
    assert not fired, "the model ran"
    compress_vo(ad2, cov_x2, keep, target_layers=layers)
    assert check_on(ad2, "loaded") == report

    for l in layers:
        off = torch.load(os.path.join(str(tmp_path / "off"), f"layer_{l}_vo"), map_location="cpu")
        for name in ("on", "loaded"):
            on = torch.load(os.path.join(str(tmp_path / name), f"layer_{l}_vo"), map_location="cpu")
            assert sorted(off) == sorted(on)
            for k in off:
                assert torch.equal(off[k].contiguous().view(torch.int16), on[k].contiguous().view(torch.int16)), (l, name, k)
