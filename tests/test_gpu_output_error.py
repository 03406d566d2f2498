"""mdg_mlp_output_error (ops.mlp_output_error) -- what a stored down projection loses of every output channel on the calibration
statistic, e_k = u_k C u_k^T -- against the long-double model tests/output_error_model.py, and MODEGPT_OUTPUT_ERROR=1 end to end.

Forward accuracy (sections "model", "index handling", "sandwich").  err = max_k |e_k - ref_k| / a_k with a_k = |u_k| |C| |u_k|^T
(for unorm2: a_k = ||u_k||^2); asserted is err_kernel <= R * max(err_cpu, 64 n 2^-53), err_cpu from the same algorithm in plain
fp64 numpy (output_error_model.errors_fp64) against the same long-double reference -- the criterion of tests/test_gpu_chol.py.
R was fixed once from the GPU run as 4 x the largest observed ratio rounded up to a power of two and may never exceed 32; a ratio
above 32 is a finding, not a tolerance.

Exact properties (section "exact"): r = 0 is the down=None call bit for bit, down = W[:, idx] at r = n gives +0.0 everywhere,
two runs agree bit for bit and so do a call inside and one outside ops.DeferredStatus; e_k >= -(R 64 n u a_k).

MEASURED on an MI355X (every test prints its figure before it asserts: lines FORWARD, SANDWICH, E2E under pytest -s)
Forward ratios err_kernel / max(err_cpu, 64 n u) of e with the bf16 [d, r] artefact (the fp64 [r, d] solution through the strides and
unorm2 read alike); err_kernel and err_cpu themselves are 0 .. 3e-16 in every case, so the floor decides:
    n = 1    (d = 1)      p3 r=0 0        p6g3 r=1 0 (fp64 solution: 6.1e-3)    acts r=0 3.0e-3      <- largest: the floor is only 64 u there
    n = 16   (d = 70)     p3 r=16 1.2e-3  p6g3 r=11 5.5e-4                      acts r=0 1.3e-3      (unorm2: up to 2.2e-3)
    n = 129  (d = 1)      p3 r=90 2.2e-5  p6g3 r=0 8.6e-6   acts r=129 0        (d = 257)  r=0 4.0e-5   r=129 3.2e-5   r=90 5.4e-5
    n = 385  (d = 70)     p3 r=385 3.6e-5 p6g3 r=269 4.3e-6 acts r=0 2.5e-5     index rule (clamped, repeated) 9.4e-5
    n = 640  (d = 257)    p3 r=448 1.8e-6 p6g3 r=0 9.2e-6   acts r=640 1.4e-5
    largest over e and unorm2, both forms of down: 6.1e-3 -> 4 x 6.1e-3 = 0.024 -> R = 2^-5.
Sandwich on the device's refit (keep 0.7, d = 70), as fractions of q = curve[0]:
    n = 385: width 1.30e-06, hi - curve 1.55e-11, curve - lo 1.30e-06, objective(bf16 artefact) - curve 2.72e-06
    n = 640: width 1.32e-06, hi - curve 1.23e-11, curve - lo 1.32e-06, objective(bf16 artefact) - curve 2.68e-06
    (the slack R 64 n u is 6.8e-13 / 1.1e-12 of q: both ends hold without it)
End to end (tiny models, 320 inner features): relative_error 8.7e-2 / 2.2e-2 (llama_gqa, ranks 190 / 257) and 2.2e-3 / 2.7e-2 (opt, ranks
294 / 153); worst channel 1.3e-1 / 4.1e-2 / 6.2e-3 / 8.0e-2; excess_over_optimum 3.1e-3 / 6.1e-3 / 3.5e-5 / 1.1e-5.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests import output_error_model as OE
from tests.test_gpu_chol import matrix

pytestmark = pytest.mark.gpu
F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -53
RATIO = 2.0 ** -5                          # R of the forward criterion (module docstring: 4 x 6.1e-3 rounded up to a power of two)
RC_RATIO = 0.25                            # the R of tests/test_gpu_rank_curve.py: the slack of the sandwich is its R 64 n u q
EPS = 1e-6                                 # the Nystrom ridge of compress_mlp.py:52,56
RIDGE = float(torch.tensor(1e-4, dtype=torch.float32).double())      # the ridge of the scores that give the selection


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
def device_refit(kind, n, d, r, wdt):
    """(idx, down bf16 [d, r], D fp64 [r, d]) on the device: the device's own selection from its own ridge scores and its own refit.
    Computed once per case, never modified."""
    from modegpt_amd import ops as _ops
    Cd, Wd = matrix(kind, n)[0].to("cuda:0"), weight(n, d, wdt).to("cuda:0")
    if r == 0:
        empty = lambda *shape, dt: torch.empty(*shape, dtype=dt, device=Cd.device)        # noqa: E731
        return empty(0, dt=torch.int64), empty(d, 0, dt=BF16), empty(0, d, dt=F64)
    idx = _ops.select_smallest_sorted(_ops.ridge_scores(Cd, RIDGE), r)
    down, D = _ops.nystrom_down(Cd, idx, Wd, eps=EPS, want_f64=True)
    return idx, down, D


def check_forward(what, got, ref, cpu, a, n):
    """err <= RATIO * max(err_cpu, 64 n u), errors relative to a_k; where a_k = 0 the value itself must be 0.  Prints first."""
    got, cpu = R.ld(got), R.ld(cpu)
    live = a > 0
    assert bool((got[~live] == 0).all())
    err = float((np.abs(got - ref)[live] / a[live]).max()) if live.any() else 0.0
    err_cpu = float((np.abs(cpu - ref)[live] / a[live]).max()) if live.any() else 0.0
    ratio = err / max(err_cpu, 64 * n * U)
    print("FORWARD %-58s err_kernel %.3e err_cpu %.3e ratio %.2e" % (what, err, err_cpu, ratio))
    assert ratio <= RATIO, "%s: err_kernel %.3e, err_cpu %.3e, ratio %.3g > %g" % (what, err, err_cpu, ratio, RATIO)
    return ratio


def check_both(what, e, u2, C, W, idx, down, n):
    """e and unorm2 of one call against the model evaluated on the same (idx, down); and e_k >= -(R 64 n u a_k)."""
    ref, a = OE.errors(C, W, idx, down)
    check_forward(what + " e", e.cpu(), ref, OE.errors_fp64(C, W, idx, down), a, n)
    assert bool((R.ld(e.cpu()) >= -(RATIO * 64 * n * U) * a).all())            # C is positive semidefinite
    ref_u = OE.unorm2(W, idx, down)
    check_forward(what + " unorm2", u2.cpu(), ref_u, OE.unorm2(W, idx, down, np.float64), ref_u, n)


# ---------------------------------------------------------------- against the long-double model
# (n, d): one element, below a tile, one past a tile edge in either dimension, three tiles and one row, five tiles.
SHAPES = [(1, 1), (16, 70), (129, 1), (129, 257), (385, 70), (640, 257)]
KINDS = ["p3", "p6g3", "acts"]
RANKS = ["0", "n", "0.7n"]
WDTS = [torch.bfloat16, torch.float32]     # (fp32 is widened exactly to fp64 by _as_weight)
# every shape with every matrix kind; rank and weight type follow (i + k) mod 3 and mod 2, i.e. (i + k) mod 6 walks all six
# (rank, weight type) pairs: a shape meets three consecutive values (every rank, both types).  Every case runs BOTH forms of down.
MODEL_CASES = [(n, d, kind, RANKS[(i + k) % 3], WDTS[(i + k) % 2])
               for i, (n, d) in enumerate(SHAPES) for k, kind in enumerate(KINDS)]


def rank_of(which, n):
    return {"0": 0, "n": n, "0.7n": int(0.7 * n)}[which]


@pytest.mark.parametrize("n,d,kind,which,wdt", MODEL_CASES,
                         ids=["n%d-d%d-%s-r%s-%s" % (n, d, k, r, str(w)[6:]) for n, d, k, r, w in MODEL_CASES])
def test_error_against_long_double_model(ops, dev, n, d, kind, which, wdt):
    r = rank_of(which, n)
    C, W = matrix(kind, n)[0], weight(n, d, wdt)
    idx, down, D = device_refit(kind, n, d, r, wdt)
    Cd, Wd = C.to(dev), W.to(dev)
    what = "%s n=%d d=%d r=%d %s" % (kind, n, d, r, str(wdt)[6:])
    # the stored [d, r] bf16 artefact
    e, u2 = ops.mlp_output_error(Cd, Wd, idx, down, want_unorm2=True)
    assert e.shape == u2.shape == (d,) and e.dtype == u2.dtype == F64 and e.is_cuda
    check_both(what + " bf16[d,r]", e, u2, C, W, idx.cpu(), down.cpu() if r else None, n)
    assert torch.equal(bits(ops.mlp_output_error(Cd, Wd, idx, down)), bits(e))          # without unorm2: the same e
    # the fp64 solution [r, d] through the strides, no transpose
    DT = D.T
    assert r == 0 or d == 1 or r == 1 or (DT.stride(0) == 1 and DT.stride(1) == d)
    e, u2 = ops.mlp_output_error(Cd, Wd, idx, DT, want_unorm2=True)
    check_both(what + " f64[r,d]^T", e, u2, C, W, idx.cpu(), DT.cpu() if r else None, n)


# ---------------------------------------------------------------- exact properties
@pytest.mark.parametrize("n,d,kind,wdt", [(385, 70, "acts", torch.bfloat16), (640, 257, "p6g3", torch.float32)])
def test_exact_properties(ops, dev, n, d, kind, wdt):
    r = int(0.7 * n)
    Cd, Wd = matrix(kind, n)[0].to(dev), weight(n, d, wdt).to(dev)
    idx, down, D = device_refit(kind, n, d, r, wdt)
    # r = 0 is the down=None call
    q, qu = ops.mlp_output_error(Cd, Wd, None, None, want_unorm2=True)
    q0, qu0 = ops.mlp_output_error(Cd, Wd, idx[:0], down[:, :0], want_unorm2=True)
    assert torch.equal(bits(q), bits(q0)) and torch.equal(bits(qu), bits(qu0))
    assert bool((q > 0).all()) and bool((qu > 0).all())
    # two runs; inside and outside a deferred status
    for dn in (down, D.T):
        a, au = ops.mlp_output_error(Cd, Wd, idx, dn, want_unorm2=True)
        b, bu = ops.mlp_output_error(Cd, Wd, idx, dn, want_unorm2=True)
        with ops.DeferredStatus(dev) as st:
            c, cu = ops.mlp_output_error(Cd, Wd, idx, dn, want_unorm2=True)
        st.check()
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(au), bits(bu))
        assert torch.equal(bits(a), bits(c)) and torch.equal(bits(au), bits(cu))
        assert bool(torch.isfinite(a).all()) and float(a.sum()) < float(q.sum())      # the refit loses less than dropping everything


@pytest.mark.parametrize("n,d,kind", [(129, 257, "p3"), (385, 70, "acts")])
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_nothing_left_gives_plus_zero(ops, dev, n, d, kind, shuffled):
    """down = W[:, idx] with r = n: U = 0, and every e_k and unorm2_k is +0.0 bit for bit."""
    Cd, Wd = matrix(kind, n)[0].to(dev), weight(n, d, BF16).to(dev)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(dev) if shuffled else torch.arange(n, device=dev)
    e, u2 = ops.mlp_output_error(Cd, Wd, idx, Wd[:, idx].contiguous(), want_unorm2=True)
    assert bool((bits(e) == 0).all()) and bool((bits(u2) == 0).all())
    e, u2 = ops.mlp_output_error(Cd, Wd.double(), idx, Wd[:, idx].double().T.contiguous().T, want_unorm2=True)    # fp64, column-major
    assert bool((bits(e) == 0).all()) and bool((bits(u2) == 0).all())


# ---------------------------------------------------------------- layout
def padded(A, fill, dev, rows, cols, col0):
    buf = torch.full((A.shape[0] + rows, A.shape[1] + cols), fill, dtype=A.dtype, device=dev)
    view = buf[:A.shape[0], col0:col0 + A.shape[1]]
    view.copy_(A)
    return buf, view


@pytest.mark.parametrize("form", ["bf16", "f64"])
@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f32"])
def test_leading_dimensions(ops, dev, form, wdt):
    """ldc > n, ld_wd > n and a strided down (column slices of wider NaN-filled buffers, data pointers off the 16-byte boundary), NaN
    above the diagonal of C: the contiguous call bit for bit, the inputs and their surroundings unchanged."""
    n, d, kind = 385, 70, "acts"
    r = int(0.7 * n)
    C = matrix(kind, n)[0]
    W = weight(n, d, wdt)
    W = W if wdt == BF16 else W.double()                               # (what _as_weight hands the library)
    idx, down, D = device_refit(kind, n, d, r, wdt)
    dn = down if form == "bf16" else D.T
    want, want_u = ops.mlp_output_error(C.to(dev), W.to(dev), idx, dn, want_unorm2=True)
    Cl = torch.tril(C)
    Cl[torch.triu(torch.ones(n, n, dtype=torch.bool), 1)] = float("nan")
    cbuf, Cd = padded(Cl, float("nan"), dev, 3, 37, 5)
    wbuf, Wd = padded(W, float("nan"), dev, 2, 11, 3)
    if form == "bf16":
        dbuf, Dd = padded(down, float("nan"), dev, 2, 9, 1)           # [d, r] inside [d + 2, r + 9]
    else:
        dbuf, Dv = padded(D, float("nan"), dev, 3, 5, 1)              # [r, d] inside [r + 3, d + 5]; handed over transposed
        Dd = Dv.T
    assert Cd.stride(0) == n + 37 and Wd.stride(0) == n + 11 and Cd.data_ptr() % 16 and Wd.data_ptr() % 16 and Dd.data_ptr() % 16
    before = [b.clone() for b in (cbuf, wbuf, dbuf)]
    got, got_u = ops.mlp_output_error(Cd, Wd, idx, Dd, want_unorm2=True)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got_u), bits(want_u))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_u).all())
    raw = lambda t: t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int64)
    for b, b0 in zip((cbuf, wbuf, dbuf), before):
        assert torch.equal(raw(b), raw(b0))


# ---------------------------------------------------------------- index handling
def test_shuffled_index_same_bits(ops, dev):
    n, d, kind = 385, 70, "acts"
    r = int(0.7 * n)
    Cd, Wd = matrix(kind, n)[0].to(dev), weight(n, d, BF16).to(dev)
    idx, down, D = device_refit(kind, n, d, r, BF16)
    perm = torch.randperm(r, generator=torch.Generator().manual_seed(3)).to(dev)
    for dn in (down, D.T):
        a, au = ops.mlp_output_error(Cd, Wd, idx, dn, want_unorm2=True)
        b, bu = ops.mlp_output_error(Cd, Wd, idx[perm], dn[:, perm], want_unorm2=True)
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(au), bits(bu))


def test_out_of_range_and_repeated_entries(ops, dev):
    """MDG_OK (ops raises nothing), and the documented rule -- clamped; the highest position of a repeated index wins -- as the
    model evaluates it."""
    n, d, kind = 385, 70, "acts"
    r = int(0.7 * n)
    C, W = matrix(kind, n)[0], weight(n, d, BF16)
    idx, down, D = device_refit(kind, n, d, r, BF16)
    bad = idx.clone()
    bad[5], bad[40] = n + 7, -2                  # -> n - 1 and 0
    bad[200] = bad[17]                           # one index at three positions: the highest of them, r - 1, is the one subtracted
    bad[r - 1] = bad[17]
    assert OE.inverse_map(bad.cpu(), n)[int(bad[17])] == r - 1
    for name, dn in (("bf16[d,r]", down), ("f64[r,d]^T", D.T)):
        e, u2 = ops.mlp_output_error(C.to(dev), W.to(dev), bad, dn, want_unorm2=True)
        check_both("index rule " + name, e, u2, C, W, bad.cpu(), dn.cpu(), n)
        clean = ops.mlp_output_error(C.to(dev), W.to(dev), idx, dn)
        assert not torch.equal(bits(e), bits(clean))


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f32"])
def test_nan_stays_in_its_row(ops, dev, wdt):
    n, d, kind = 385, 70, "acts"
    r = int(0.7 * n)
    Cd = matrix(kind, n)[0].to(dev)
    W = weight(n, d, wdt)
    idx, down, D = device_refit(kind, n, d, r, wdt)
    clean, clean_u = ops.mlp_output_error(Cd, W.to(dev), idx, down, want_unorm2=True)
    one = lambda k: torch.arange(d, device=dev) == k
    Wn = W.clone()
    Wn[3, 300] = float("nan")
    e, u2 = ops.mlp_output_error(Cd, Wn.to(dev), idx, down, want_unorm2=True)             # MDG_OK: does not raise
    assert torch.equal(torch.isnan(e), one(3)) and torch.equal(torch.isnan(u2), one(3))
    assert torch.equal(bits(e)[~one(3)], bits(clean)[~one(3)])
    q = ops.mlp_output_error(Cd, Wn.to(dev), None, None)
    assert torch.equal(torch.isnan(q), one(3))
    for dn in (down.clone(), D.T.clone()):
        dn[5, 2] = float("nan")
        e, u2 = ops.mlp_output_error(Cd, W.to(dev), idx, dn, want_unorm2=True)
        assert torch.equal(torch.isnan(e), one(5)) and torch.equal(torch.isnan(u2), one(5))
    assert torch.equal(bits(ops.mlp_output_error(Cd, W.to(dev), idx, down)), bits(clean))   # and a good call passes afterwards


# ---------------------------------------------------------------- the sandwich on the device
@pytest.mark.parametrize("n", [385, 640])
def test_sandwich_on_the_device(ops, dev, n):
    """E_D + eps sum unorm2 from THIS kernel on the device's fp64 refit, and the device's own rank curve:
    hi - eps ||W_S||^2 - s <= curve[r] <= hi + s, s = R 64 n u q with the R of tests/test_gpu_rank_curve.py; and the bf16 artefact's
    objective >= curve[r] - s (the curve is the minimum over all refits)."""
    d, keep, kind = 70, 0.7, "acts"
    r = int(n * keep)
    C, W = matrix(kind, n)[0], weight(n, d, BF16)
    Cd, Wd = C.to(dev), W.to(dev)
    scores = ops.ridge_scores(Cd, RIDGE)
    idx = ops.select_smallest_sorted(scores, r)
    order = torch.argsort(scores, stable=True)
    assert torch.equal(torch.sort(order[:r]).values, idx)
    down, D = ops.nystrom_down(Cd, idx, Wd, eps=EPS, want_f64=True)
    curve = ops.nystrom_rank_curve(Cd, order, Wd, eps=EPS).cpu()
    q, got = float(curve[0]), float(curve[r])
    s = RC_RATIO * 64 * n * U * q
    eps = R.LD(np.float64(EPS))
    total = lambda t: R.ld(t.cpu()).sum()
    e, u2 = ops.mlp_output_error(Cd, Wd, idx, D.T, want_unorm2=True)
    hi = total(e) + eps * total(u2)
    ws = R.ld(W.double())[:, idx.cpu().numpy()]
    lo = hi - eps * (ws * ws).sum()
    eb, ub = ops.mlp_output_error(Cd, Wd, idx, down, want_unorm2=True)
    objective = total(eb) + eps * total(ub)
    print("SANDWICH n=%d r=%d width/q %.3e (hi - curve)/q %.3e (curve - lo)/q %.3e (objective(bf16) - curve)/q %.3e slack/q %.3e" % (
        n, r, float((hi - lo) / q), float((hi - got) / q), float((got - lo) / q), float((objective - got) / q), s / q))
    assert lo - s <= got <= hi + s
    assert objective >= got - s


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    n, d, r = 129, 4, 90
    Cd, Wd = matrix("p3", n)[0].to(dev), weight(n, d, BF16).to(dev)
    idx = torch.arange(r, device=dev)
    down = Wd[:, :r].contiguous()
    e = torch.full((d,), -1.0, dtype=F64, device=dev)
    nbytes = lib.mdg_mlp_output_error_ws_bytes(n, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(n_=n, d_=d, ldc=n, ldw=n, wdt=_lib.MDG_BF16, r_=r, dn=down.data_ptr(), ddt=_lib.MDG_BF16, nb=nbytes, c=Cd.data_ptr(),
             ix=idx.data_ptr(), out=e.data_ptr()):
        return lib.mdg_mlp_output_error(c, n_, ldc, Wd.data_ptr(), d_, ldw, wdt, ix, r_, dn, r, 1, ddt, out, None, ws.data_ptr(), nb, None)

    bad = [dict(nb=nbytes - 1), dict(n_=0), dict(d_=0), dict(r_=-1), dict(r_=n + 1), dict(ldc=n - 1), dict(ldw=n - 1),
           dict(wdt=_lib.MDG_F32), dict(ddt=_lib.MDG_F16), dict(dn=None), dict(ix=None), dict(c=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        with pytest.raises(RuntimeError):                            # what every ops front end turns the status into
            _lib.check(call(**kw), "mdg_mlp_output_error")
    assert call(nb=nbytes - 1) == _lib.MDG_ERR_BAD_ARG and b"workspace" in lib.mdg_last_error()
    torch.cuda.synchronize()
    assert bool((e == -1.0).all())                                  # nothing was enqueued
    assert call() == _lib.MDG_OK
    assert call(r_=0, dn=None, ix=None) == _lib.MDG_OK              # U = W_d
    torch.cuda.synchronize()
    assert bool((e > 0).all())
    with pytest.raises(RuntimeError):
        ops.mlp_output_error(Cd.cpu(), Wd.cpu(), None, None)        # no CPU fallback
    with pytest.raises(ValueError):
        ops.mlp_output_error(Cd, Wd, idx, down[:, :-1])


# ---------------------------------------------------------------- end to end: MODEGPT_OUTPUT_ERROR=1
@pytest.mark.parametrize("kind", ["llama_gqa", "opt"])
def test_model_end_to_end(dev, kind, tmp_path, monkeypatch):
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

    monkeypatch.delenv("MODEGPT_OUTPUT_ERROR", raising=False)
    monkeypatch.delenv("MODEGPT_RANK_CURVE", raising=False)
    compress_nystrom(ad, cov_mlp, keep, layers)
    assert ad.report_output_errors() == {}
    assert "mlp_output_error" not in ad.metrics and not getattr(ad, "output_errors", None)

    monkeypatch.setenv("MODEGPT_OUTPUT_ERROR", "1")
    ad.config = conf("on")
    compress_nystrom(ad, cov_mlp, keep, layers)
    report = ad.report_output_errors()
    assert sorted(report) == layers and sorted(ad.metrics["mlp_output_error"]) == [str(l) for l in layers]
    for l in layers:
        m = ad.metrics["mlp_output_error"][str(l)]
        q, e, u2 = ad.output_errors[l]
        assert m == report[l] and "predicted_objective" not in m and "excess_over_optimum" not in m
        assert all(not t.is_cuda and t.dtype == F64 and t.dim() == 1 and t.shape == q.shape for t in (q, e, u2))
        assert m["rank"] == int(n * keep[l])
        assert 0.0 < m["relative_error"] < 1.0 and m["error"] <= m["energy"]
        assert 0 <= m["worst_channel"] < q.numel() and m["worst_channel_relative_error"] >= m["relative_error"]
    assert ad.report_output_errors() == {}                          # read once
    single = {l: dict(report[l]) for l in layers}

    monkeypatch.setenv("MODEGPT_RANK_CURVE", "1")
    ad.config = conf("both")
    compress_nystrom(ad, cov_mlp, keep, layers)
    curves = ad.report_rank_curves()                                # the curves first: excess_over_optimum needs them
    report = ad.report_output_errors()
    assert sorted(curves) == layers and sorted(report) == layers
    for l in layers:
        m, curve = report[l], ad.rank_curves[l]
        assert {k: m[k] for k in single[l]} == single[l]            # the same numbers as without the curve
        assert m["predicted_objective"] == float(curve[m["rank"]])
        slack = RC_RATIO * 64 * n * U
        print("E2E %s layer %d: rank %d of %d, relative_error %.3e, worst channel %d at %.3e, excess_over_optimum %.3e" % (
            kind, l, m["rank"], n, m["relative_error"], m["worst_channel"], m["worst_channel_relative_error"], m["excess_over_optimum"]))
        assert m["excess_over_optimum"] >= -slack

    for l in layers:
        off = torch.load(os.path.join(str(tmp_path / "off"), f"layer_{l}_mlp"), map_location="cpu")
        for name in ("on", "both"):
            on = torch.load(os.path.join(str(tmp_path / name), f"layer_{l}_mlp"), map_location="cpu")
            assert sorted(off) == sorted(on)
            for k in off:
                assert torch.equal(off[k].contiguous().view(torch.int16), on[k].contiguous().view(torch.int16)), (l, name, k)
