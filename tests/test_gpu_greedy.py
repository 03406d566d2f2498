"""mdg_nystrom_greedy_select (ops.nystrom_greedy_select) -- MLP columns by block-greedy descent on the objective the Nystrom refit
minimises -- against the long-double model tests/greedy_model.py, and MODEGPT_MLP_GREEDY end to end.

`order` is compared entry for entry: tests/test_greedy_model_host.py asserts that every round's cut of every case here is at least
1e-6 wide relative to the picked gain in long double (the narrowest is 1.2e-5), far above what fp64 rounding moves a gain by.

Tolerance of `objective` and `cut` (a criterion measured against the reference; no bound c(n, r) 2^-53 A was derived).  Errors are absolute and
compared on the scale A = sum_i (|W| |M| |W|^T)_ii, not on the value's own: a small J_t has lost its leading digits.  With
e_dev = max |device - long double| and e_cpu = max |plain fp64 numpy model - long double| over all entries of the output:
    e_dev <= 8 e_cpu + n 2^-53 A.
The 8 covers the different summation orders and the hybrid (Yt, diag(R), right-looking B) against the model's right-looking R.

MEASURED on an MI355X (every test prints its figures before it asserts: lines TOL, ROUTE, RIDGE, E2E under pytest -s).  Largest
observed per shape over all (r, T) and both weight types, objective / cut:
    n = 48  (d = 8):    e_dev / bound 0.031 / 0.003    e_dev / e_cpu 3.9 / 1.0    e_dev / A 1.8e-16 / 2.0e-17
    n = 130 (d = 40):   e_dev / bound 0.013 / 0.015    e_dev / e_cpu 8.1 / 5.7    e_dev / A 2.3e-16 / 2.6e-16
    n = 300 (d = 136):  e_dev / bound 0.001 / 0.001    e_dev / e_cpu 11  / 3.6    e_dev / A 2.5e-17 / 3.6e-17
    (bound = 8 e_cpu + n 2^-53 A; where e_dev / e_cpu exceeds 8 both errors are 1e-17 A, two orders under the floor, which decides)
Independent route: |objective[T] - curve[r]| <= 4.4e-17 A in every case.  Ridge comparison, (130, 40), J / J0 in long double: ridge rule
9.945e-8, T = 8 7.499e-8 (1.33 x smaller), T = r 7.067e-8 (1.41 x).
"""
import os

import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests import greedy_model as G

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
EPS = G.EPS
WDTS = [torch.bfloat16, torch.float64]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int64)


def device_case(n, d, wdt, dev):
    C, W = G.shared_case(n, d)
    return torch.from_numpy(C).to(dev), W.to(wdt).to(dev)


def run(ops, Cd, Wd, r, rounds, eps=EPS):
    order, objective, cut, n_dead = ops.nystrom_greedy_select(Cd, Wd, r, rounds, eps=eps)
    torch.cuda.synchronize()
    return order.cpu().numpy(), objective.cpu().numpy(), cut.cpu().numpy(), int(n_dead.cpu())


def max_err(got, ref):
    """max |got - ref| over the entries where the reference is a number; the NaN patterns must agree."""
    got, ref = R.ld(np.asarray(got, dtype=np.float64)), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    ok = ~np.isnan(ref)
    return float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0


def check_tolerance(what, n, A, got, ref, cpu):
    e_dev, e_cpu = max_err(got, ref), max_err(cpu, ref)
    bound = 8 * e_cpu + n * U * A
    print("TOL %-44s e_dev/A %.3e e_cpu/A %.3e e_dev/bound %.3f e_dev/e_cpu %.3g" % (
        what, e_dev / A, e_cpu / A, e_dev / bound, e_dev / e_cpu if e_cpu > 0 else float("inf")))
    assert e_dev <= bound, "%s: e_dev %.3e > 8 e_cpu + n u A = %.3e (e_cpu %.3e)" % (what, e_dev, bound, e_cpu)


# ---------------------------------------------------------------- against the long-double model
@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f64"])
@pytest.mark.parametrize("n,d,r,rounds", G.gpu_cases(), ids=["n%d-d%d-r%d-T%d" % c for c in G.gpu_cases()])
def test_against_long_double_model(ops, dev, n, d, r, rounds, wdt):
    Cd, Wd = device_case(n, d, wdt, dev)
    order, objective, cut, n_dead = run(ops, Cd, Wd, r, rounds)
    ref_order, ref_obj, ref_cut, ref_dead, _ = G.reference(n, d, r, rounds)
    _, cpu_obj, cpu_cut, _, _ = G.reference_fp64(n, d, r, rounds)
    assert order.dtype == np.int64 and order.shape == (r,) and objective.shape == (rounds + 1,) and cut.shape == (rounds, 2)
    assert order.tolist() == ref_order.tolist()
    assert n_dead == ref_dead == 0
    A = G.scale_A(*G.shared_case(n, d))
    what = "n=%d d=%d r=%d T=%d %s" % (n, d, r, rounds, str(wdt)[6:])
    check_tolerance("objective " + what, n, A, objective, ref_obj, cpu_obj)
    check_tolerance("cut       " + what, n, A, cut, ref_cut, cpu_cut)


# ---------------------------------------------------------------- an independent route: the rank curve along order ++ rest
@pytest.mark.parametrize("n,d", G.SHAPES)
def test_objective_meets_the_rank_curve(ops, dev, n, d):
    Cd, Wd = device_case(n, d, torch.bfloat16, dev)
    A = G.scale_A(*G.shared_case(n, d))
    scores = ops.ridge_scores(Cd, G.RIDGE).cpu().numpy()
    for r in (int(0.7 * n), n - 1):
        for rounds in (8, r):
            order, objective, _, _ = run(ops, Cd, Wd, r, rounds)
            perm = torch.from_numpy(G.order_with_rest(order, scores)).to(dev)
            curve = ops.nystrom_rank_curve(Cd, perm, Wd, eps=EPS).cpu().numpy()
            ref = G.reference(n, d, r, rounds)[1]
            e_cpu = max_err(G.reference_fp64(n, d, r, rounds)[1], ref)
            bound = 8 * e_cpu + n * U * A
            diff = abs(float(objective[rounds]) - float(curve[r]))
            print("ROUTE n=%d r=%d T=%d: |objective[T] - curve[r]| / A %.3e, bound / A %.3e" % (n, r, rounds, diff / A, bound / A))
            assert diff <= bound
            assert abs(float(objective[0]) - float(curve[0])) <= bound


# ---------------------------------------------------------------- it beats the rule it replaces
@pytest.mark.parametrize("rounds", [8, "r"])
def test_beats_the_ridge_rule(ops, dev, rounds):
    """The correlated (130, 40) case: J of the device's selection is below J of the ridge rule's, both in long double."""
    n, d = 130, 40
    r = int(0.7 * n)
    rounds = r if rounds == "r" else rounds
    C, W = G.shared_case(n, d)
    Cd, Wd = device_case(n, d, torch.bfloat16, dev)
    order = run(ops, Cd, Wd, r, rounds)[0]
    ridge = ops.select_smallest_sorted(ops.ridge_scores(Cd, G.RIDGE), r).cpu().numpy()
    j_greedy, j_ridge, j0 = G.objective_of(C, W, order), G.objective_of(C, W, ridge), G.objective_of(C, W, [])
    print("RIDGE T=%d: greedy %.3e, ridge rule %.3e of J0: ridge / greedy %.3f" % (rounds, j_greedy / j0, j_ridge / j0, j_ridge / j_greedy))
    assert j_greedy < j_ridge


# ---------------------------------------------------------------- layout and edges
def padded(A, fill, dev, rows, cols, col0):
    buf = torch.full((A.shape[0] + rows, A.shape[1] + cols), fill, dtype=A.dtype, device=dev)
    view = buf[:A.shape[0], col0:col0 + A.shape[1]]
    view.copy_(A)
    return buf, view


@pytest.mark.parametrize("wdt", WDTS, ids=["bf16", "f64"])
def test_leading_dimensions_and_upper_triangle(ops, dev, wdt):
    """ldc > n and ld_wd > n (column slices of wider NaN-filled buffers, data pointers off the 16-byte boundary), NaN above the
    diagonal of C: the outputs of the contiguous call bit for bit, the inputs and their surroundings unchanged."""
    n, d, r, rounds = 130, 40, 91, 8
    Cd, Wd = device_case(n, d, wdt, dev)
    want = ops.nystrom_greedy_select(Cd, Wd, r, rounds)
    Cl = torch.tril(Cd)
    Cl[torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev), 1)] = float("nan")
    cbuf, Cv = padded(Cl, float("nan"), dev, 3, 37, 5)
    wbuf, Wv = padded(Wd, float("nan"), dev, 2, 11, 3)
    assert Cv.stride(0) == n + 37 and Wv.stride(0) == n + 11
    before = (cbuf.clone(), wbuf.clone())
    got = ops.nystrom_greedy_select(Cv, Wv, r, rounds)
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b))
    assert bool(torch.isfinite(got[1]).all())
    assert torch.equal(bits(cbuf), bits(before[0])) and torch.equal(bits(wbuf), bits(before[1]))


def test_rank_zero_rank_n_and_more_rounds_than_columns(ops, dev):
    n, d = 48, 8
    Cd, Wd = device_case(n, d, torch.bfloat16, dev)
    A = G.scale_A(*G.shared_case(n, d))
    order, objective, cut, n_dead = run(ops, Cd, Wd, 0, 5)
    ref = G.reference(n, d, 0, 5)
    assert order.shape == (0,) and n_dead == 0 and np.isnan(cut).all()
    assert (objective == objective[0]).all() and abs(objective[0] - float(ref[1][0])) <= n * U * A
    order, objective, cut, n_dead = run(ops, Cd, Wd, n, 3)
    assert sorted(order.tolist()) == list(range(n)) and n_dead == 0
    check_tolerance("objective n=48 r=n T=3", n, A, objective, G.reference(n, d, n, 3)[1], G.reference_fp64(n, d, n, 3)[1])   # (J(all) = 0)
    a = run(ops, Cd, Wd, 5, 5)
    b = run(ops, Cd, Wd, 5, 9)                                        # T > r counts as r; the rounds beyond repeat
    assert a[0].tolist() == b[0].tolist() == G.reference(n, d, 5, 9)[0].tolist()
    assert np.array_equal(a[1], b[1][:6]) and (b[1][6:] == a[1][5]).all()
    assert np.array_equal(a[2], b[2][:5], equal_nan=True) and np.isnan(b[2][5:]).all()


# ---------------------------------------------------------------- dead picks
def test_duplicate_columns_are_dead_picks(ops, dev):
    """eps = 0 and exact duplicate columns of integer data: once an original is in S its copy's R_jj is a rounding of zero, below
    the floor n 2^-52 M_jj.  The copies are picked only when the eligible columns run out, then by index; they are counted, and no
    pivot fails."""
    C, W, dup = G.duplicate_case()
    n, live = C.shape[0], C.shape[0] - len(dup)
    Cd, Wd = torch.from_numpy(C).to(dev), W.to(dev)
    order, objective, cut, n_dead = run(ops, Cd, Wd, live, live, eps=0.0)            # (run raises on MDG_ERR_NOT_PD)
    ref = G.greedy(C, W, live, live, eps=0.0)
    assert n_dead == 0 and not set(dup) & set(order.tolist()) and order.tolist() == ref[0].tolist()
    order, objective, cut, n_dead = run(ops, Cd, Wd, n, n, eps=0.0)
    assert n_dead == len(dup) and order[live:].tolist() == sorted(dup) and order[:live].tolist() == ref[0].tolist()
    assert np.isnan(cut[live:]).all() and (objective[live:] == objective[live]).all()
    with ops.DeferredStatus(dev) as st:
        ops.nystrom_greedy_select(Cd, Wd, n, n, eps=0.0)
    st.check()                                                        # no NOT_PD in the deferred status either


# ---------------------------------------------------------------- non-finite input, with guards around every output
GUARD = 64


def guarded(count, dtype, dev, fill):
    buf = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + count]


@pytest.mark.parametrize("what", ["W column", "C entry", "C diagonal"])
def test_non_finite_input_stays_in_bounds(dev, what):
    from modegpt_amd import _lib
    lib = _lib.load()
    n, d, r, rounds = 130, 40, 91, 8
    Cd, Wd = device_case(n, d, torch.bfloat16, dev)
    Cd, Wd = Cd.clone(), Wd.clone()
    if what == "W column":
        Wd[:, 17] = float("nan")
    elif what == "C entry":
        Cd[77, 20] = float("nan")
    else:
        Cd[60, 60] = float("nan")
    inputs = (Cd.clone(), Wd.clone())
    obuf, order = guarded(r, torch.int64, dev, -7)
    jbuf, objective = guarded(rounds + 1, F64, dev, -7.0)
    cbuf, cut = guarded(2 * rounds, F64, dev, -7.0)
    dbuf, n_dead = guarded(1, torch.int64, dev, -7)
    nbytes = lib.mdg_nystrom_greedy_ws_bytes(n, d, r, rounds)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.mdg_nystrom_greedy_select(Cd.data_ptr(), n, n, Wd.data_ptr(), d, n, _lib.MDG_BF16, EPS, r, rounds, order.data_ptr(),
                                       objective.data_ptr(), cut.data_ptr(), n_dead.data_ptr(), ws.data_ptr(), nbytes, None)
    torch.cuda.synchronize()
    assert rc in (_lib.MDG_OK, _lib.MDG_ERR_NOT_PD), lib.mdg_last_error()
    o = order.cpu().tolist()
    assert len(set(o)) == r and min(o) >= 0 and max(o) < n
    assert 0 <= int(n_dead.cpu()) <= r
    for buf, count, fill in ((obuf, r, -7), (jbuf, rounds + 1, -7.0), (cbuf, 2 * rounds, -7.0), (dbuf, 1, -7)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + count:] == fill).all())
    assert torch.equal(bits(Cd), bits(inputs[0])) and torch.equal(bits(Wd), bits(inputs[1]))


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("n,d,r,rounds,wdt", [(130, 40, 91, 8, torch.bfloat16), (300, 136, 210, 3, torch.float64)])
def test_two_runs_agree_bit_for_bit(ops, dev, n, d, r, rounds, wdt):
    Cd, Wd = device_case(n, d, wdt, dev)
    a = ops.nystrom_greedy_select(Cd, Wd, r, rounds)
    b = ops.nystrom_greedy_select(Cd, Wd, r, rounds)
    with ops.DeferredStatus(dev) as st:
        c = ops.nystrom_greedy_select(Cd, Wd, r, rounds)
    st.check()
    for x, y, z in zip(a, b, c):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))


# ---------------------------------------------------------------- refusals
def test_bad_arguments(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    n, d, r, rounds = 48, 8, 10, 3
    Cd, Wd = device_case(n, d, torch.bfloat16, dev)
    order = torch.full((r,), -1, dtype=torch.int64, device=dev)
    objective = torch.full((rounds + 1,), -1.0, dtype=F64, device=dev)
    nbytes = lib.mdg_nystrom_greedy_ws_bytes(n, d, r, rounds)
    assert nbytes >= 8 * (d * n + r * n)
    assert lib.mdg_nystrom_greedy_ws_bytes(n, d, n + 1, rounds) == 0 and lib.mdg_nystrom_greedy_ws_bytes(n, d, r, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(n_=n, d_=d, ldc=n, ldw=n, wdt=_lib.MDG_BF16, r_=r, T=rounds, nb=nbytes, c=Cd.data_ptr(), w=Wd.data_ptr(), o=order.data_ptr(),
             j=objective.data_ptr(), wsp=ws.data_ptr()):
        return lib.mdg_nystrom_greedy_select(c, n_, ldc, w, d_, ldw, wdt, EPS, r_, T, o, j, None, None, wsp, nb, None)

    def refused(needle, **kw):
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        assert needle in lib.mdg_last_error(), (kw, lib.mdg_last_error())

    refused(b"null", c=None)
    refused(b"null", w=None)
    refused(b"null", j=None)
    refused(b"null order", o=None)
    refused(b"bad sizes", n_=0)
    refused(b"bad sizes", d_=0)
    refused(b"bad sizes", ldc=n - 1)
    refused(b"bad sizes", ldw=n - 1)
    refused(b"rank", r_=-1)
    refused(b"rank", r_=n + 1)
    refused(b"rounds", T=0)
    refused(b"bf16 or f64", wdt=_lib.MDG_F32)
    refused(b"workspace", nb=nbytes - 1)
    refused(b"workspace", wsp=None)
    torch.cuda.synchronize()
    assert bool((order == -1).all()) and bool((objective == -1.0).all())             # nothing was enqueued
    assert call() == _lib.MDG_OK
    assert call(r_=0, o=None) == _lib.MDG_OK                          # r == 0: order may be NULL
    torch.cuda.synchronize()
    assert float(objective[0]) > 0


# ---------------------------------------------------------------- end to end: MODEGPT_MLP_GREEDY
@pytest.mark.parametrize("kind", ["llama_gqa", "opt"])
def test_model_end_to_end(dev, kind, tmp_path, monkeypatch):
    """A random-init 2-layer model.  Switch unset: ops.nystrom_greedy_select is never called, nothing of the feature is recorded, and
    the artefacts are, bit for bit, what the ridge rule's own chain of ops gives (ridge_scores -> select_smallest_sorted ->
    gather_rows / nystrom_down).  MODEGPT_MLP_GREEDY=4 with MODEGPT_RANK_CURVE=1: the artefacts sit on the greedy idx, the report
    and the "no certificate" entry are there, the rank curve's independent value meets the descent's last objective, the saved
    checkpoint loads through the shipped modeling file, and the same run from saved statistics gives the same bits."""
    transformers = pytest.importorskip("transformers")
    from modegpt_amd import ops
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression.compress_mlp import compress_nystrom
    from modegpt_amd.compression.compress_qk import compress_qk
    from modegpt_amd.compression.compress_vo import compress_vo
    from modegpt_amd.compression_utils import allocate_global_sparsity
    from modegpt_amd.model_utils import save_compressed_model
    from tests.test_gpu_e2e import _tiny_model

    for var in ("MODEGPT_MLP_GREEDY", "MODEGPT_RANK_CURVE", "MODEGPT_CALIBS_SAVE", "MODEGPT_CALIBS_LOAD"):
        monkeypatch.delenv(var, raising=False)
    model = _tiny_model(kind, dev)
    conf = lambda name: CompressionConfig(temp_storage_dir=str(tmp_path / name), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5,
                                          dataset="synthetic", calib_size=6, calibs_batch_size=4, compression_ratio=0.3,
                                          order="mlp,qk,vo")

    def adapter(name):
        ad = ModelAdapter.from_model(model, None)
        ad.config = conf(name)
        return ad

    ad, stats = adapter("off"), str(tmp_path / "stats")
    cov_mlp, cov_q, cov_k, cov_x, bi = load_calibs(ad, n_samples=6, batch_size=4, dataset="synthetic", target_layers=[],
                                                   calibs_save_path=stats)
    keep = allocate_global_sparsity(bi, 0.3, smoothing=0.15, max_sparsity=0.8, adapter=ad)
    layers, n = list(range(ad.n_layers)), ad.get_n_inner()
    calls, real = [], ops.nystrom_greedy_select
    monkeypatch.setattr(ops, "nystrom_greedy_select", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    load = lambda ad_, l: torch.load(os.path.join(ad_.config.temp_storage_dir, f"layer_{l}_mlp"), map_location="cpu")
    same = lambda a, b: a.shape == b.shape and torch.equal(bits(a), bits(b))

    # ---- unset: the reference's rule, nothing of the feature
    compress_nystrom(ad, [c.clone() for c in cov_mlp], keep, layers)
    ad.report_selection_margins()
    assert ad.report_mlp_greedy() == {} and calls == []
    assert "mlp_greedy" not in ad.metrics and "_mlp_greedy" not in ad.__dict__
    assert all("margin" in ad.metrics["mlp_selection"][str(l)] for l in layers)
    ridge = float(torch.tensor(1e-4, dtype=torch.float32).double())
    for l in layers:
        comps, off = ad.get_mlp_components(l), load(ad, l)
        rank = int(n * keep[l])
        idx = ops.select_smallest_sorted(ops.ridge_scores(cov_mlp[l].to(dev), ridge), rank)
        assert same(off["up"], ops.gather_rows(comps.up_proj.weight.detach().to(torch.bfloat16), idx).cpu())
        assert same(off["down"], ops.nystrom_down(cov_mlp[l].to(dev), idx, comps.down_proj.weight.detach(), eps=EPS).cpu())

    # ---- MODEGPT_MLP_GREEDY=4 MODEGPT_RANK_CURVE=1
    monkeypatch.setenv("MODEGPT_MLP_GREEDY", "4")
    monkeypatch.setenv("MODEGPT_RANK_CURVE", "1")

    def compress(ad_, covs):
        compress_nystrom(ad_, [c.clone() for c in covs[0]], keep, layers)
        masks = compress_qk(ad_, ([c.clone() for c in covs[1]], [c.clone() for c in covs[2]]), keep, target_layers=layers)
        compress_vo(ad_, [c.clone() for c in covs[3]], keep, target_layers=layers)
        ad_.report_selection_margins()
        report = ad_.report_mlp_greedy()
        ad_.report_rank_curves()
        return masks, report

    on = adapter("on")
    masks, report = compress(on, (cov_mlp, cov_q, cov_k, cov_x))
    assert len(calls) == len(layers) and sorted(report) == layers
    differs = 0
    for l in layers:
        comps, art = on.get_mlp_components(l), load(on, l)
        rank = int(n * keep[l])
        W_d = comps.down_proj.weight.detach()
        order, objective, cut, n_dead = real(cov_mlp[l].to(dev), W_d, rank, 4)
        idx = torch.sort(order).values
        assert same(art["up"], ops.gather_rows(comps.up_proj.weight.detach().to(torch.bfloat16), idx).cpu())
        assert same(art["down"], ops.nystrom_down(cov_mlp[l].to(dev), idx, W_d, eps=EPS).cpu())
        differs += not same(art["up"], load(ad, l)["up"])
        m = on.metrics["mlp_greedy"][str(l)]
        assert m == report[l] and m["rounds"] == 4 and m["rank"] == rank and m["dead_picks"] == int(n_dead.cpu()) == 0
        assert m["objective"] == objective.cpu().tolist() and len(m["objective"]) == 5
        assert m["objective_over_total"] == m["objective"][-1] / m["objective"][0] and 0 < m["min_cut_gap"] < 1
        # the rank curve along order ++ rest, an independent route to the same number (the tolerance of the kernel tests, with
        # e_cpu of this layer's own statistic)
        C, W = cov_mlp[l].cpu().numpy(), W_d.cpu()
        A = G.scale_A(C, W)
        e_cpu = max_err(G.greedy(C, W, rank, 4, dt=np.float64)[1], G.greedy(C, W, rank, 4)[1])
        assert abs(m["greedy_at_rank"] - m["objective"][-1]) <= 8 * e_cpu + n * U * A
        assert m["greedy_at_rank"] == float(on.rank_curves[l][rank]) and m["ridge_at_rank"] > 0
        assert m["greedy_over_ridge"] == m["greedy_at_rank"] / m["ridge_at_rank"]
        print("E2E %s layer %d: rank %d of %d, objective_over_total %.3e, greedy_over_ridge %.3f, min_cut_gap %.3e" % (
            kind, l, rank, n, m["objective_over_total"], m["greedy_over_ridge"], m["min_cut_gap"]))
        sel = on.metrics["mlp_selection"][str(l)]
        assert sel["statistic"] == "greedy" and sel["certificate"] is None and sel["certified"] is None and "margin" not in sel
    assert differs > 0, "the greedy selection took the ridge rule's columns in every layer"

    # ---- the same run from the saved statistics: the same bits
    again = adapter("again")
    loaded = load_calibs(again, n_samples=6, batch_size=4, dataset="synthetic", target_layers=[], load_calibs_from=stats)
    compress(again, loaded[:4])
    for l in layers:
        a, b = load(on, l), load(again, l)
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        assert on.metrics["mlp_greedy"][str(l)] == again.metrics["mlp_greedy"][str(l)]

    # ---- the checkpoint through the shipped modeling file
    on.convert_model(saved_layers_dir=on.config.temp_storage_dir)
    on.patch_config()
    out = str(tmp_path / "ckpt")
    save_compressed_model(on, rotary_masks=masks, save_dir=out, source_model_name="none")
    reloaded = transformers.AutoModelForCausalLM.from_pretrained(out, trust_remote_code=True, dtype=torch.bfloat16).to(dev).eval()
    assert "Rebuild" in type(reloaded).__module__
    ids = torch.randint(0, 211, (2, 20), generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        assert bool(torch.isfinite(reloaded(ids).logits.float()).all())
