"""mdg_nystrom_rank_curve (ops.nystrom_rank_curve) -- the MLP refit's residual energy at every rank from one factorisation -- against
the long-double model tests/rank_curve_model.py, and MODEGPT_RANK_CURVE=1 end to end.

Forward accuracy (sections "model", "outer panel", "sandwich").  e = max_r |curve[r] - ref[r]| / ref[0]; asserted is
e_kernel <= R * max(e_cpu, 64 n 2^-53), e_cpu from the same algorithm in plain fp64 numpy / LAPACK (rank_curve_model.curve_fp64)
against the same long-double reference -- the criterion of tests/test_gpu_chol.py.  R was fixed once from the GPU run as 4 x the
largest observed ratio rounded up to a power of two and may never exceed 32; a ratio above 32 is a finding, not a tolerance.

Exact properties (section "exact"): curve[n] is +0.0 bit for bit, the curve is non-increasing entry by entry (a suffix sum of
squares accumulated from the tail), two runs agree bit for bit, and so do a call inside and one outside ops.DeferredStatus.

MEASURED on an MI355X (every test prints its figure before it asserts: lines FORWARD, SANDWICH under pytest -s)
Forward ratios e_kernel / max(e_cpu, 64 n u); e_kernel and e_cpu themselves are 1e-16 .. 8e-16 in every case, so the floor decides:
    n = 1    (d = 1)      p3 0.047    p6g3 0.014    acts 0.030          <- largest: the floor is only 64 u there
    n = 16   (d = 70)     p3 0.0010   p6g3 0.0012   acts 0.0026
    n = 129  (d = 1)      p3 2.1e-4   p6g3 2.9e-4   acts 4.4e-4         (d = 257)  1.8e-4   1.2e-4   1.1e-4
    n = 385  (d = 70)     p3 1.6e-4   p6g3 1.2e-4   acts 1.4e-4
    n = 640  (d = 70)     p3 4.0e-5   p6g3 5.5e-5   acts 6.1e-5         (d = 257)  5.6e-5   3.6e-5   7.4e-5
    n = 2304 (d = 64, p6g3, against the fp64 CPU restatement)  4.8e-5
    largest 0.047 -> 4 x 0.047 = 0.19 -> R = 0.25.
Sandwich on the device's refit (keep 0.7, d = 70), as fractions of q = curve[0]:
    n = 385: width 1.30e-06, hi - curve 1.55e-11, curve - lo 1.30e-06      n = 640: width 1.32e-06, hi - curve 1.23e-11, curve - lo 1.32e-06
    (the slack R 64 n u is 6.8e-13 / 1.1e-12 of q: the curve sits inside the sandwich without it)
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests import rank_curve_model as RC
from tests.test_gpu_chol import matrix

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
RATIO = 0.25                               # R of the forward criterion (module docstring: 4 x 0.047 rounded up to a power of two)
EPS = 1e-6                                 # the Nystrom ridge of compress_mlp.py:52,56
RIDGE = float(torch.tensor(1e-4, dtype=torch.float32).double())      # the ridge of the scores that give the order


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def weight(n, d, wdt):
    gen = torch.Generator().manual_seed(1000 * n + d)
    return (torch.randn(d, n, generator=gen) * 0.05).to(wdt)


@functools.lru_cache(maxsize=None)
def ridge_order(kind, n):
    """The ridge-score order of matrix(kind, n), from the device's own scores (so that ties, if any, are the device's)."""
    from modegpt_amd import ops as _ops
    scores = _ops.ridge_scores(matrix(kind, n)[0].to("cuda:0"), RIDGE)
    return torch.argsort(scores, stable=True).cpu()


def order_for(which, kind, n):
    if which == "identity":
        return torch.arange(n)
    if which == "reversed":
        return torch.arange(n - 1, -1, -1)
    return ridge_order(kind, n)


@functools.lru_cache(maxsize=None)
def references(kind, n, d, which, wdt):
    """(long-double curve, fp64 numpy / LAPACK curve) of one case: computed once, never modified."""
    C, W, order = matrix(kind, n)[0], weight(n, d, wdt), order_for(which, kind, n).numpy()
    return RC.curve(C, order, W, EPS), RC.curve_fp64(C, order, W, EPS)


def curve_error(got, ref):
    return float((np.abs(R.ld(got) - ref) / ref[0]).max())


def check_forward(what, e_kernel, e_cpu, n):
    base = max(float(e_cpu), 64 * n * U)
    ratio = float(e_kernel) / base
    print("FORWARD %-52s e_kernel %.3e e_cpu %.3e ratio %.2e" % (what, float(e_kernel), float(e_cpu), ratio))
    assert ratio <= RATIO, "%s: e_kernel %.3e, e_cpu %.3e, ratio %.3g > %g" % (what, e_kernel, e_cpu, ratio, RATIO)


# ---------------------------------------------------------------- against the long-double model
# n: one, below a block, one past a block, three blocks and one row, five blocks; d: one row, below a tile, two tiles and one row.
SHAPES = [(1, 1), (16, 70), (129, 1), (129, 257), (385, 70), (640, 70), (640, 257)]
KINDS = ["p3", "p6g3", "acts"]
ORDERS = ["identity", "reversed", "ridge"]
WDTS = [torch.bfloat16, torch.float32]     # (fp32 is widened exactly to fp64 by _as_weight)
# every shape with every matrix kind; order and weight type follow (i + k) mod 3 and mod 2, i.e. (i + k) mod 6 walks all six
# (order, weight type) pairs: a shape meets three consecutive values (every order, both types), a kind seven (every pair)
MODEL_CASES = [(n, d, kind, ORDERS[(i + k) % 3], WDTS[(i + k) % 2])
               for i, (n, d) in enumerate(SHAPES) for k, kind in enumerate(KINDS)]


@pytest.mark.parametrize("n,d,kind,which,wdt", MODEL_CASES,
                         ids=["n%d-d%d-%s-%s-%s" % (n, d, k, o, str(w)[6:]) for n, d, k, o, w in MODEL_CASES])
def test_curve_against_long_double_model(ops, dev, n, d, kind, which, wdt):
    C, W, order = matrix(kind, n)[0], weight(n, d, wdt), order_for(which, kind, n)
    ref, cpu = references(kind, n, d, which, wdt)
    got = ops.nystrom_rank_curve(C.to(dev), order.to(dev), W.to(dev), eps=EPS).cpu()
    assert got.shape == (n + 1,) and got.dtype == F64
    check_forward("%s n=%d d=%d %s %s" % (kind, n, d, which, str(wdt)[6:]), curve_error(got, ref), curve_error(cpu, ref), n)
    assert bits(got)[n].item() == 0 and bool((got[:-1] >= got[1:]).all())


def padded(A, fill, dev, rows, cols, col0):
    buf = torch.full((A.shape[0] + rows, A.shape[1] + cols), fill, dtype=A.dtype, device=dev)
    view = buf[:A.shape[0], col0:col0 + A.shape[1]]
    view.copy_(A)
    return buf, view


@pytest.mark.parametrize("strided", ["C", "W"])
@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f32"])
def test_leading_dimensions(ops, dev, strided, wdt):
    """ldc > n / ld_wd > n (column slices of wider NaN-filled buffers, data pointers off the 16-byte boundary): the curve of the
    contiguous call bit for bit, which the model test covers; the inputs and their surroundings unchanged.  Above the diagonal C
    holds NaN as well: only the lower triangle is read."""
    n, d, kind = 385, 70, "acts"
    C, order = matrix(kind, n)[0], ridge_order(kind, n).to(dev)
    W = weight(n, d, wdt)
    W = W if wdt == torch.bfloat16 else W.double()                     # (what _as_weight hands the library)
    want = ops.nystrom_rank_curve(C.to(dev), order, W.to(dev), eps=EPS)
    Cd, Wd = C.to(dev), W.to(dev)
    if strided == "C":
        Cl = torch.tril(C)
        Cl[torch.triu(torch.ones(n, n, dtype=torch.bool), 1)] = float("nan")
        buf, Cd = padded(Cl, float("nan"), dev, 3, 37, 5)
        assert Cd.stride(0) == n + 37
    else:
        buf, Wd = padded(W, float("nan"), dev, 2, 11, 3)
        assert Wd.stride(0) == n + 11
    before = buf.clone()
    got = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS)
    assert torch.equal(bits(got), bits(want))
    assert bool(torch.isfinite(got).all())
    raw = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int64)
    assert torch.equal(raw(buf), raw(before))


# ---------------------------------------------------------------- beyond the 2048-row outer panel of the factorisation
def test_curve_beyond_the_outer_panel(ops, dev):
    """n = 2304: the factorisation's lower-only outer update and two blocks behind it, 18 tile columns of the triangular product.
    The long-double factorisation is too slow here: the reference is the fp64 CPU restatement and the floor alone decides --
    e_kernel against the CPU value <= R * 64 n 2^-53."""
    n, d, kind = 2304, 64, "p6g3"
    C, W, order = matrix(kind, n)[0], weight(n, d, torch.bfloat16), ridge_order(kind, n)
    cpu = RC.curve_fp64(C, order.numpy(), W, EPS)
    got = ops.nystrom_rank_curve(C.to(dev), order.to(dev), W.to(dev), eps=EPS).cpu()
    check_forward("%s n=%d d=%d ridge bfloat16 (against fp64 CPU)" % (kind, n, d), curve_error(got, cpu.astype(R.LD)), 0.0, n)
    assert bits(got)[n].item() == 0 and bool((got[:-1] >= got[1:]).all())


# ---------------------------------------------------------------- the sandwich on the device's own refit
@pytest.mark.parametrize("n", [385, 640])
def test_sandwich_on_the_device_refit(ops, dev, n):
    """lo <= curve[r] <= hi (rank_curve_model.sandwich) with D the refit mdg_nystrom_down computes at the selection
    mdg_select_smallest_sorted makes, E_D, ||U||^2 and ||W_S||^2 in long double from that D; slack s = R 64 n 2^-53 curve[0], the
    forward criterion's floor.  The scores carry a planted tie across the selection threshold: the order's prefix is the
    selection all the same."""
    d, keep, kind = 70, 0.7, "acts"
    r = int(n * keep)
    C, W = matrix(kind, n)[0], weight(n, d, torch.bfloat16)
    Cd, Wd = C.to(dev), W.to(dev)
    scores = ops.ridge_scores(Cd, RIDGE)
    o0 = torch.argsort(scores, stable=True)
    scores[o0[r]] = scores[o0[r - 1]]                       # the r-th and (r+1)-th smallest now tie: the lower index is selected
    idx = ops.select_smallest_sorted(scores, r)
    order = torch.argsort(scores, stable=True)
    assert torch.equal(torch.sort(order[:r]).values, idx)
    assert int(min(o0[r], o0[r - 1])) in idx.tolist() and int(max(o0[r], o0[r - 1])) not in idx.tolist()
    _, D = ops.nystrom_down(Cd, idx, Wd, eps=EPS, want_f64=True)
    curve = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS).cpu()
    lo, hi = RC.sandwich(C, W, idx.cpu().numpy(), D, EPS)
    q, got = float(curve[0]), float(curve[r])
    s = RATIO * 64 * n * U * q
    print("SANDWICH n=%d r=%d width/q %.3e (hi - curve)/q %.3e (curve - lo)/q %.3e slack/q %.3e" % (
        n, r, float((hi - lo) / q), float((hi - got) / q), float((got - lo) / q), s / q))
    assert lo - s <= got <= hi + s


# ---------------------------------------------------------------- exact properties
@pytest.mark.parametrize("n,d,kind,wdt", [(385, 70, "acts", torch.bfloat16), (640, 257, "p6g3", torch.float32)])
def test_exact_properties(ops, dev, n, d, kind, wdt):
    Cd, Wd, order = matrix(kind, n)[0].to(dev), weight(n, d, wdt).to(dev), ridge_order(kind, n).to(dev)
    a = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS)
    b = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS)
    with ops.DeferredStatus(dev) as st:
        c = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS)
    st.check()
    assert bits(a)[n].item() == 0                                   # +0.0, not -0.0
    assert bool((a[:-1] >= a[1:]).all()) and bool(torch.isfinite(a).all()) and float(a[0]) > 0
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(a), bits(c))


# ---------------------------------------------------------------- failure paths (none of them leaves its buffers)
def order_of(exc):
    m = re.search(r"leading minor of order (\d+) is not positive-definite", str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


@pytest.mark.parametrize("first,second", [(10, 11), (10, 200), (127, 384)])
def test_repeated_index_is_not_positive_definite(ops, dev, first, second):
    """order[second] = order[first]: M[pi, pi] is singular, and the report names the first position of the repeated index --
    at once, and from the deferred status."""
    n, d, kind = 385, 70, "acts"
    Cd, Wd = matrix(kind, n)[0].to(dev), weight(n, d, torch.bfloat16).to(dev)
    order = ridge_order(kind, n).clone()
    order[second] = order[first]
    with pytest.raises(torch.linalg.LinAlgError) as now:
        ops.nystrom_rank_curve(Cd, order.to(dev), Wd, eps=EPS)
    assert order_of(now) == first + 1
    with ops.DeferredStatus(dev) as st:
        ops.nystrom_rank_curve(Cd, order.to(dev), Wd, eps=EPS)      # does not raise here
    with pytest.raises(torch.linalg.LinAlgError) as deferred:
        st.check()
    assert order_of(deferred) == first + 1
    good = ops.nystrom_rank_curve(Cd, ridge_order(kind, n).to(dev), Wd, eps=EPS)     # and a good call passes afterwards
    assert bool(torch.isfinite(good).all())


def test_out_of_range_entries_are_clamped(ops, dev):
    """Entries outside 0 .. n-1 are clamped to the ends (memory safety only): here they then repeat an index -> not PD."""
    n, d, kind = 385, 70, "acts"
    Cd, Wd = matrix(kind, n)[0].to(dev), weight(n, d, torch.bfloat16).to(dev)
    order = torch.arange(n)
    order[5], order[300] = n + 7, -2                                 # -> n - 1 (repeats position n - 1) and 0 (repeats position 0)
    with pytest.raises(torch.linalg.LinAlgError) as exc:
        ops.nystrom_rank_curve(Cd, order.to(dev), Wd, eps=EPS)
    assert order_of(exc) == 1


@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f32"])
def test_nan_weight_gives_nan_curve(ops, dev, wdt):
    n, d, kind, p = 385, 70, "acts", 200
    Cd, order = matrix(kind, n)[0].to(dev), ridge_order(kind, n)
    W = weight(n, d, wdt)
    W[3, int(order[p])] = float("nan")                               # the column at position p of the order
    curve = ops.nystrom_rank_curve(Cd, order.to(dev), W.to(dev), eps=EPS)       # MDG_OK: does not raise
    assert bool(torch.isnan(curve[:p + 1]).all())
    assert bits(curve)[n].item() == 0
    m = ops.decode_rank_curve(curve.cpu(), 269)
    assert m["rel_error"] is None and m["rank_for_rel_error"]["0.01"] is None


def test_bad_arguments(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    n, d = 129, 4
    Cd, Wd = matrix("p3", n)[0].to(dev), weight(n, d, torch.bfloat16).to(dev)
    order = torch.arange(n, device=dev)
    curve = torch.full((n + 1,), -1.0, dtype=F64, device=dev)
    nbytes = lib.mdg_nystrom_rank_curve_ws_bytes(n, d)
    assert nbytes >= 8 * (n * n + 2 * d * n) + lib.mdg_potrf_inv_diag_elems(n) * 8
    assert lib.mdg_nystrom_rank_curve_ws_bytes(n, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(n_=n, d_=d, ldc=n, ldw=n, wdt=_lib.MDG_BF16, nb=nbytes, c=Cd.data_ptr(), o=order.data_ptr()):
        return lib.mdg_nystrom_rank_curve(c, n_, ldc, o, Wd.data_ptr(), d_, ldw, wdt, EPS, curve.data_ptr(), ws.data_ptr(), nb, None)

    assert call(nb=nbytes - 1) == _lib.MDG_ERR_BAD_ARG and b"workspace" in lib.mdg_last_error()
    assert call(d_=0) == _lib.MDG_ERR_BAD_ARG
    assert call(n_=0) == _lib.MDG_ERR_BAD_ARG
    assert call(ldc=n - 1) == _lib.MDG_ERR_BAD_ARG
    assert call(ldw=n - 1) == _lib.MDG_ERR_BAD_ARG
    assert call(wdt=_lib.MDG_F32) == _lib.MDG_ERR_BAD_ARG and b"bf16 or f64" in lib.mdg_last_error()
    assert call(c=None) == _lib.MDG_ERR_BAD_ARG
    assert call(o=None) == _lib.MDG_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((curve == -1.0).all())                              # nothing was enqueued
    assert call() == _lib.MDG_OK
    torch.cuda.synchronize()
    assert float(curve[n]) == 0.0 and float(curve[0]) > 0


# ---------------------------------------------------------------- end to end: MODEGPT_RANK_CURVE=1
@pytest.mark.parametrize("kind", ["llama_gqa", "opt"])
def test_model_end_to_end(dev, kind, tmp_path, monkeypatch):
    from modegpt_amd import ops
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression_utils import allocate_global_sparsity
    from tests.test_gpu_e2e import _tiny_model

    ad = ModelAdapter.from_model(_tiny_model(kind, dev), None)
    conf = lambda name: CompressionConfig(temp_storage_dir=str(tmp_path / name), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5,
                                          dataset="synthetic", calib_size=6, calibs_batch_size=4, compression_ratio=0.3,
                                          order="mlp,qk,vo")
    ad.config = conf("off")
    cov_mlp, _, _, _, bi = load_calibs(ad, n_samples=6, batch_size=4, dataset="synthetic", target_layers=[])
    keep = allocate_global_sparsity(bi, 0.3, smoothing=0.15, max_sparsity=0.8, adapter=ad)
    layers, n = list(range(ad.n_layers)), ad.get_n_inner()

    monkeypatch.delenv("MODEGPT_RANK_CURVE", raising=False)
    compress_nystrom(ad, cov_mlp, keep, layers)
    assert ad.report_rank_curves() == {}
    assert "mlp_rank_curve" not in ad.metrics and not getattr(ad, "rank_curves", None)

    monkeypatch.setenv("MODEGPT_RANK_CURVE", "1")
    ad.config = conf("on")
    compress_nystrom(ad, cov_mlp, keep, layers)
    report = ad.report_rank_curves()
    assert sorted(report) == layers and sorted(ad.metrics["mlp_rank_curve"]) == [str(l) for l in layers]
    for l in layers:
        m, curve = ad.metrics["mlp_rank_curve"][str(l)], ad.rank_curves[l]
        assert m == report[l]
        assert not curve.is_cuda and curve.shape == (n + 1,) and curve.dtype == F64
        assert m["n"] == n and m["rank"] == int(n * keep[l]) and m["energy"] == float(curve[0]) > 0
        assert 0.0 <= m["rel_error"] <= 1.0
        assert m["rel_error"] == float(curve[m["rank"]]) / float(curve[0])
        assert m["rel_error_at_keep"][-1] == 0.0
        assert all(a >= b for a, b in zip(m["rel_error_at_keep"], m["rel_error_at_keep"][1:]))
        print("E2E %s layer %d: rank %d of %d, rel_error %.3e, rank for 1e-2: %s" % (
            kind, l, m["rank"], n, m["rel_error"], m["rank_for_rel_error"]["0.01"]))
        off = torch.load(os.path.join(str(tmp_path / "off"), f"layer_{l}_mlp"), map_location="cpu")
        on = torch.load(os.path.join(str(tmp_path / "on"), f"layer_{l}_mlp"), map_location="cpu")
        assert sorted(off) == sorted(on)
        for k in off:
            assert torch.equal(off[k].contiguous().view(torch.int16), on[k].contiguous().view(torch.int16)), (l, k)
    assert ad.report_rank_curves() == {}                            # read once
