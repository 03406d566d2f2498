"""mdg_qk_rank_curve (ops.qk_rank_curve) -- what the Q/K pair selection costs the attention logits on the calibration statistic, per
query head and at every rank -- against the long-double model tests/qk_error_model.py, and MODEGPT_QK_ERROR=1 end to end.

Criterion (a priori, include/modegpt_hip.h; nothing here is fitted to what the kernel gives): entry by entry
    |curve_h - ref| <= (hd^2 + 2) 2^-53 A_h ,    |curve - ref|, |greedy_curve - objective(greedy_order)| <= (g hd^2 + 2) 2^-53 sum_h A_h ,
    |terms - ref| <= (2 g |cols| + 2) 2^-53 terms ,
A_h[m] = sum over cols(D_m) x cols(D_m) of |P_h|: one rounding per ridge addition, product and addition, in any order.  Every test
prints its largest error / bound before it asserts (lines MODEL, ORDER, GREEDY, E2E under pytest -s).

MEASURED on an MI355X, largest error / bound per line kind:
    MODEL  curve_h, curve and greedy_curve: 1.5e-1 at hd = 2 (three terms per value), 1.0e-1 at hd = 5, 9.2e-2 / 2.8e-2 at hd = 6,
           1.3e-2 / 5.7e-3 at hd = 16, 1.2e-3 at hd = 64, 3.6e-4 at hd = 128, 8.6e-5 / 3.6e-5 at hd = 256 (curve_h / group) -- the range of
           the plain fp64 numpy route of tests/test_qk_error_host.py (4.9e-2 at hd = 8 .. 4.5e-4 at hd = 128); scale 1.5e-1 .. 4.2e-5;
           terms 0.18 .. 0.45 of (2 g |cols| + 2) u (a bound of a few roundings is nearly met by a few roundings)
    ORDER  8/2 heads of 128, random permutation / reversed score order: curve_h 3.0e-4 / 3.4e-4, curve 3.8e-5 / 4.7e-5
    GREEDY the chosen unit's increment above the smallest one: 0 at every step of all 8 cases (the bound was never needed)
    TIED   f(terms) against mdg_qk_select_margin's out[0] / out[1]: 0 ulp in 17 of 18 figures, 1 ulp in one (OPT, r = 14)
    NONMONOTONE  [1.1399999999999997, 3.0, 0.0] for 3 x [0.38, 1, 0]
    E2E    llama_gqa (4/2 heads of 32, ranks 22 / 32): relative_error 2.7e-1 / 0, diagonal_ratio 8.0, greedy 2.6e-1;
           opt (4 heads of 32): 2.3e-1 / 0, diagonal_ratio 1.16, greedy 2.3e-1, layer 1's curve not monotone; error against the model
           4.3e-4 .. 1.7e-3 of the bound; the run from saved statistics gives the same report
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import qk_error_model as QK

pytestmark = pytest.mark.gpu
F64 = torch.float64
LD, U = QK.LD, QK.U
GROUPED, MHA, OPT = QK.ROPE_GROUPED, QK.ROPE_MHA, QK.OPT
RIDGES = [(0.0, 0.0), (1e-4, 1e-2)]
# (mode, n_heads, n_kv, hd)
SHAPES = [(GROUPED, 4, 2, 16), (GROUPED, 3, 1, 6), (GROUPED, 8, 2, 128), (GROUPED, 2, 1, 256),
          (MHA, 2, 2, 64), (MHA, 1, 1, 2),
          (OPT, 3, 3, 64), (OPT, 1, 1, 128), (OPT, 2, 2, 5)]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def problem(builder, n_heads, n_kv, hd):
    """(cov_q, cov_k) on the host, fp64 numpy, computed once, never modified."""
    build = QK.BUILDERS[builder]
    cq, ck = build(n_heads, hd, seed=1000 + hd), build(n_kv, hd, seed=2000 + hd)
    return cq, ck


def score_order(ops, dev, cq, ck, mode, rq, rk):
    """The units of every kv head in mdg_qk_select's order: the first ns mask entries at rank = hd.  int64 [n_kv, ns] on the device."""
    hd = cq.shape[-1]
    ns, _ = QK.units(mode, hd)
    mask = ops.qk_select(torch.from_numpy(cq).to(dev), torch.from_numpy(ck).to(dev), hd, mode, rq, rk)[0]
    return mask[:, :ns].contiguous()


def run(ops, dev, cq, ck, mode, rq, rk, order, **kw):
    """ops.qk_rank_curve on host arrays -> numpy (curve_h, curve, terms, scale, greedy_curve, greedy_order)."""
    out = ops.qk_rank_curve(torch.from_numpy(np.ascontiguousarray(cq)).to(dev), torch.from_numpy(np.ascontiguousarray(ck)).to(dev), mode,
                            rq, rk, order, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def within(what, got, ref, bound):
    """|got - ref| <= bound entry by entry (where the bound is 0 the value is exact); prints the largest error / bound first."""
    err = np.abs(got.astype(LD) - ref)
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print("%-90s largest error / bound %.3e" % (what, worst))
    assert bool(np.isfinite(got).all()), what
    assert bool((err <= bound).all()), "%s: largest error / bound %.3g" % (what, worst)
    return worst


def check_against_model(what, out, cq, ck, mode, rq, rk, order_np):
    n_heads, n_kv, hd = cq.shape[0], ck.shape[0], cq.shape[-1]
    g = n_heads // n_kv
    ns, w = QK.units(mode, hd)
    curve_h, curve, terms, scale, g_curve, g_order = out
    ref = QK.model(cq, ck, mode, rq, rk, order_np)
    within("MODEL %s curve_h" % what, curve_h, ref["curve_h"], (hd * hd + 2) * U * ref["A_h"])
    within("MODEL %s curve" % what, curve, ref["curve"], (g * hd * hd + 2) * U * ref["A"])
    t_ref = QK.terms(cq, ck, mode, rq, rk, order_np)
    within("MODEL %s terms" % what, terms, t_ref, (2 * g * w + 2) * U * t_ref)
    within("MODEL %s scale" % what, scale, ref["A"][:, 0], (g * hd * hd + 2) * U * ref["A"][:, 0])
    assert bool((bits(torch.from_numpy(curve_h[:, ns].copy())) == 0).all()) and bool((bits(torch.from_numpy(curve[:, ns].copy())) == 0).all())
    if g_curve is not None:
        assert all(sorted(row) == list(range(ns)) for row in g_order.tolist()), "greedy_order is not a permutation"
        o_ref, o_A = QK.objective(cq, ck, mode, rq, rk, g_order)
        within("MODEL %s greedy_curve" % what, g_curve, o_ref, (g * hd * hd + 2) * U * o_A)
        assert bool((bits(torch.from_numpy(g_curve[:, ns].copy())) == 0).all())
    return ref


# ---------------------------------------------------------------- 1. against long double
@pytest.mark.parametrize("ridges", RIDGES, ids=lambda r: "rho%g_%g" % r)
@pytest.mark.parametrize("builder", sorted(QK.BUILDERS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "mode%d-%d_%d-hd%d" % s)
def test_against_long_double(ops, dev, shape, builder, ridges):
    mode, n_heads, n_kv, hd = shape
    cq, ck = problem(builder, n_heads, n_kv, hd)
    order = score_order(ops, dev, cq, ck, mode, *ridges)
    out = run(ops, dev, cq, ck, mode, *ridges, order)
    check_against_model("mode %d %d/%d hd %d %s rho %g %g" % (mode, n_heads, n_kv, hd, builder, *ridges), out, cq, ck, mode, *ridges,
                        order.cpu().numpy())


# ---------------------------------------------------------------- 2. exact
def test_integer_statistics_are_exact(ops, dev):
    mode, n_heads, n_kv, hd = GROUPED, 8, 2, 128
    g, ns = n_heads // n_kv, hd // 2
    rng = np.random.default_rng(7)

    def ints(n):
        M = rng.integers(-1024, 1025, (n, hd, hd))
        return np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1))
    iq, ik = ints(n_heads), ints(n_kv)
    cq, ck = iq.astype(np.float64), ik.astype(np.float64)
    for name, order in (("score", score_order(ops, dev, cq, ck, mode, 0.0, 0.0)),
                        ("random", torch.stack([torch.from_numpy(rng.permutation(ns)) for _ in range(n_kv)]).to(dev))):
        curve_h, curve, terms, scale, g_curve, g_order = run(ops, dev, cq, ck, mode, 0.0, 0.0, order)
        ref = QK.model(iq, ik, mode, 0, 0, order.cpu().numpy(), dtype=np.int64)          # every partial sum is an integer below 2^53
        assert int(ref["A"].max()) < 2 ** 53
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                      # noqa: E731
        assert torch.equal(t(curve_h), t(ref["curve_h"].astype(np.float64))), name
        assert torch.equal(t(curve), t(ref["curve"].astype(np.float64))), name
        assert torch.equal(t(scale), t(ref["A"][:, 0].astype(np.float64))), name
        o_ref = QK.model(iq, ik, mode, 0, 0, g_order, dtype=np.int64)["curve"]
        assert torch.equal(t(g_curve), t(o_ref.astype(np.float64))), name
        for arr in (curve_h, curve, g_curve):
            assert bool((bits(t(arr[:, ns])) == 0).all()), "[ns] must be +0.0 to the bit"
        # the group's curve is the ascending-h sum of its heads', to the bit (here on floats that happen to be integers; below on real data)
        acc = t(curve_h).view(n_kv, g, ns + 1)
        s = acc[:, 0].clone()
        for q in range(1, g):
            s = s + acc[:, q]
        assert same(s, t(curve)), name


def test_group_curve_is_the_ascending_sum_of_its_heads_to_the_bit(ops, dev):
    for mode, n_heads, n_kv, hd in ((GROUPED, 8, 2, 128), (GROUPED, 3, 1, 6)):
        cq, ck = problem("full", n_heads, n_kv, hd)
        g, ns = n_heads // n_kv, hd // 2
        curve_h, curve = run(ops, dev, cq, ck, mode, 1e-4, 1e-2, score_order(ops, dev, cq, ck, mode, 1e-4, 1e-2), want_greedy=False)[:2]
        acc = torch.from_numpy(curve_h).view(n_kv, g, ns + 1)
        s = acc[:, 0].clone()
        for q in range(1, g):
            s = s + acc[:, q]
        assert same(s, torch.from_numpy(curve))


# ---------------------------------------------------------------- 3. the order is honoured
def test_any_order_is_honoured(ops, dev):
    mode, n_heads, n_kv, hd = GROUPED, 8, 2, 128
    cq, ck = problem("full", n_heads, n_kv, hd)
    ns = hd // 2
    rng = np.random.default_rng(11)
    score = score_order(ops, dev, cq, ck, mode, 1e-4, 1e-2)
    orders = {"random": torch.stack([torch.from_numpy(rng.permutation(ns)) for _ in range(n_kv)]).to(dev),
              "reversed": torch.flip(score, dims=[1]).contiguous()}
    base = run(ops, dev, cq, ck, mode, 1e-4, 1e-2, score)
    for name, order in orders.items():
        out = run(ops, dev, cq, ck, mode, 1e-4, 1e-2, order)
        check_against_model("ORDER " + name, out, cq, ck, mode, 1e-4, 1e-2, order.cpu().numpy())
        assert not np.array_equal(out[1][:, 1:ns], base[1][:, 1:ns])                 # (another order: another curve between the ends)
        assert np.array_equal(out[5], base[5]) and np.array_equal(out[4], base[4])   # the greedy outputs do not depend on `order`


def test_out_of_range_order_entries_touch_nothing_else(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    mode, n_heads, n_kv, hd = GROUPED, 4, 2, 16
    cq, ck = (torch.from_numpy(a).to(dev) for a in problem("full", n_heads, n_kv, hd))
    ns, G, SENT = hd // 2, 64, -7.25
    sizes = [n_heads * (ns + 1), n_kv * (ns + 1), n_kv * ns, n_kv, n_kv * (ns + 1)]
    offs, at = [], G
    for n in sizes:
        offs.append(at)
        at += n + G
    buf = torch.full((at,), SENT, dtype=F64, device=dev)
    ibuf = torch.full((2 * G + n_kv * ns,), -77, dtype=torch.int64, device=dev)
    order = score_order(ops, dev, cq.cpu().numpy(), ck.cpu().numpy(), mode, 0.0, 0.0)
    bad = order.clone()
    bad[0, 0], bad[0, 3], bad[1, ns - 1] = -5, 2 ** 40, ns + 7
    ptr = lambda i: buf.data_ptr() + 8 * offs[i]                                       # noqa: E731
    for o in (order, bad):
        rc = lib.mdg_qk_rank_curve(cq.data_ptr(), ck.data_ptr(), n_heads, n_kv, hd, 0.0, 0.0, mode, o.data_ptr(), 0.0, 0.0, ptr(0), ptr(1),
                                   ptr(2), ptr(3), ptr(4), ibuf.data_ptr() + 8 * G, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.MDG_OK
        torch.cuda.synchronize()
        guard = torch.ones(at, dtype=torch.bool, device=dev)
        for off, n in zip(offs, sizes):
            guard[off:off + n] = False
            assert bool((buf[off:off + n] != SENT).all())                              # every output entry was written
        assert bool((buf[guard] == SENT).all()), "a guard region was written"
        assert bool((ibuf[:G] == -77).all()) and bool((ibuf[G + n_kv * ns:] == -77).all())
        assert all(sorted(row) == list(range(ns)) for row in ibuf[G:G + n_kv * ns].view(n_kv, ns).tolist())


# ---------------------------------------------------------------- 4. non-monotone
def test_non_monotone_curve_is_returned_raw(ops, dev):
    s = 3.0
    cq = np.array([[[1.0, -0.9], [-0.9, 1.0]]]) * s
    ck = np.array([[[1.0, 0.9], [0.9, 1.0]]])
    order = torch.tensor([[0, 1]], dtype=torch.int64, device=dev)
    curve_h, curve, terms, scale, g_curve, g_order = run(ops, dev, cq, ck, OPT, 0.0, 0.0, order)
    P = QK.product(cq[0], ck[0], 0.0, 0.0)
    bound = (4 + 2) * U * float(np.abs(P).sum())
    want = np.array([0.38, 1.0, 0.0]) * s
    print("NONMONOTONE curve", curve[0].tolist(), "wanted", want.tolist())
    assert bool((np.abs(curve[0] - want) <= bound + 4 * U * s).all()) and np.array_equal(curve, curve_h)      # (0.81 and 0.38 are not fp64 numbers)
    assert curve[0][1] > curve[0][0] > 0.0 and curve[0][2] == 0.0                      # one column dropped costs MORE than both: unclamped
    assert np.array_equal(terms, np.array([[s, s]]))
    # the greedy order: dropping either unit first costs 1; ties go to the lower index, which is then LAST in keep-first order
    assert g_order.tolist() == [[1, 0]] and abs(g_curve[0][1] - s) <= bound


# ---------------------------------------------------------------- 5. greedy semantics
@pytest.mark.parametrize("shape", [(GROUPED, 4, 2, 16), (OPT, 3, 3, 64), (GROUPED, 8, 2, 128), (OPT, 2, 2, 5)], ids=lambda s: "mode%d-%d_%d-hd%d" % s)
def test_greedy_takes_the_smallest_increment_at_every_step(ops, dev, shape):
    mode, n_heads, n_kv, hd = shape
    g = n_heads // n_kv
    ns, _ = QK.units(mode, hd)
    for builder in sorted(QK.BUILDERS):
        cq, ck = problem(builder, n_heads, n_kv, hd)
        g_order = run(ops, dev, cq, ck, mode, 1e-4, 1e-2, score_order(ops, dev, cq, ck, mode, 1e-4, 1e-2))[5]
        worst = 0.0
        for kv in range(n_kv):
            assert sorted(g_order[kv].tolist()) == list(range(ns))
            B, Babs = QK.group_blocks(cq, ck, mode, 1e-4, 1e-2, kv)
            dropped = []
            for step in range(ns):
                chosen = int(g_order[kv][ns - 1 - step])
                inc, scale = QK.greedy_increments(B, dropped), QK.greedy_increments(Babs, dropped)
                left = [u for u in range(ns) if u not in dropped]
                best = min(left, key=lambda u: (inc[u], u))
                bound = (g * hd * hd + 2) * U * (scale[chosen] + scale[best])
                excess = float(inc[chosen] - inc[best])
                worst = max(worst, excess / float(bound) if bound > 0 else 0.0)
                assert chosen in left and excess <= bound, (kv, step, chosen, best, excess, float(bound))
                dropped.append(chosen)
        print("GREEDY mode %d %d/%d hd %d %s: largest (chosen - smallest increment) / bound %.3e" % (mode, n_heads, n_kv, hd, builder, worst))


def test_greedy_ties_go_to_the_lower_unit(ops, dev):
    hd, i, j = 12, 3, 8
    cq, ck = (a.copy() for a in problem("full", 1, 1, hd))
    for S in (cq[0], ck[0]):                                                          # unit j becomes a bit copy of unit i
        S[j, :] = S[i, :]
        S[:, j] = S[:, i]
    order = torch.arange(hd, dtype=torch.int64, device=dev)[None].contiguous()
    g_order = run(ops, dev, cq, ck, OPT, 0.0, 0.0, order)[5][0].tolist()
    assert sorted(g_order) == list(range(hd))
    assert g_order.index(i) > g_order.index(j), g_order                              # i (lower) was dropped first: it sits later, keep-first


# ---------------------------------------------------------------- 6. tied to the existing selection
@pytest.mark.parametrize("mode,n_heads,n_kv", [(GROUPED, 4, 2), (MHA, 2, 2), (OPT, 2, 2)])
def test_tied_to_qk_select_and_its_margin(ops, dev, mode, n_heads, n_kv):
    hd, (rq, rk) = 16, (1e-4, 1e-2)
    cq, ck = problem("full", n_heads, n_kv, hd)
    cqd, ckd = torch.from_numpy(cq).to(dev), torch.from_numpy(ck).to(dev)
    ns, w = QK.units(mode, hd)
    order = score_order(ops, dev, cq, ck, mode, rq, rk)
    terms = ops.qk_rank_curve(cqd, ckd, mode, 0.0, 0.0, order, want_greedy=False, terms_ridges=(rq, rk))[2]
    assert same(terms, ops.qk_rank_curve(cqd, ckd, mode, rq, rk, order, want_greedy=False)[2])      # the terms' ridges are their own
    assert bool((terms[:, 1:] <= terms[:, :-1]).all()), "terms must not increase along the score order"
    f = (lambda t: t) if mode == MHA else torch.sqrt
    for r in (2, hd // 2, hd - 2):
        take = r // w
        mask = ops.qk_select(cqd, ckd, r, mode, rq, rk)[0]
        assert torch.equal(mask[:, :take], order[:, :take])                             # rank r is a prefix of the rank-hd order
        if w == 2:
            assert torch.equal(mask[:, take:], order[:, :take] + hd // 2)
        margin = ops.qk_select_margin(cqd, ckd, r, mode, rq, rk, mask, 0.0, 0.0)
        for col, idx in ((0, take - 1), (1, take)):
            got, want = f(terms[:, idx]), margin[:, col]
            ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
            print("TIED mode %d r %d out[%d]: largest difference %.2f ulp" % (mode, r, col, float((torch.abs(got - want) / ulp).max())))
            assert bool((torch.abs(got - want) <= 4 * ulp).all()), (mode, r, col)


# ---------------------------------------------------------------- 7. non-finite isolation
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["q_offdiag", "q_diag", "k_offdiag"])
def test_non_finite_entries_stay_where_the_header_says(ops, dev, where, value):
    mode, n_heads, n_kv, hd = GROUPED, 4, 2, 16
    g, ns = 2, 8
    cq, ck = (a.copy() for a in problem("full", n_heads, n_kv, hd))
    order = score_order(ops, dev, cq, ck, mode, 1e-4, 1e-2)                          # one order for every run: from the clean statistic
    clean = run(ops, dev, cq, ck, mode, 0.0, 0.0, order, terms_ridges=(1e-4, 1e-2))
    a, b = (3, 9) if "offdiag" in where else (3, 3)                                  # columns 3 and 9: units 3 and 1
    if where.startswith("q"):
        cq[1, a, b] = value                                                           # query head 1 of kv group 0
        hit_heads = [1]
    else:
        ck[0, a, b] = value                                                           # kv head 0: both of its query heads
        hit_heads = [0, 1]
    out = run(ops, dev, cq, ck, mode, 0.0, 0.0, order, terms_ridges=(1e-4, 1e-2))
    curve_h, curve, terms, scale, g_curve, g_order = out
    pos = order[0].cpu().tolist()
    last = min(pos.index(a % ns), pos.index(b % ns))                                  # D_m holds both units for m <= last
    bad = np.arange(ns + 1) <= last
    for h in range(g):
        if h in hit_heads:
            assert np.array_equal(~np.isfinite(curve_h[h]), bad), (h, curve_h[h])
            assert np.array_equal(curve_h[h][~bad].view(np.int64), clean[0][h][~bad].view(np.int64))
        else:
            assert np.array_equal(curve_h[h].view(np.int64), clean[0][h].view(np.int64))                  # the group's other head: to the bit
    assert np.array_equal(~np.isfinite(curve[0]), bad) and not np.isfinite(scale[0])
    assert not np.isfinite(g_curve[0][0]) and g_curve[0][ns] == 0.0 and sorted(g_order[0].tolist()) == list(range(ns))
    if where == "q_diag" and value == float("inf"):
        assert np.array_equal(~np.isfinite(terms[0]), np.arange(ns) == pos.index(a))   # that unit's term alone
    elif where == "q_diag":
        assert bool(np.isfinite(terms[0]).all()) and terms[0][pos.index(a)] < clean[2][0][pos.index(a)]   # fmax drops the NaN: counted as 0
    else:
        assert np.array_equal(terms[0].view(np.int64), clean[2][0].view(np.int64))   # the terms read diagonals only
    for got, ref in zip(out, clean):                                                 # the other kv head: every output to the bit
        lo = g if got.shape[0] == n_heads else 1
        assert np.array_equal(np.ascontiguousarray(got[lo:]).view(np.int64), np.ascontiguousarray(ref[lo:]).view(np.int64))


# ---------------------------------------------------------------- 8. alignment and determinism
def test_unaligned_views_and_two_runs_give_the_same_bits(ops, dev):
    mode, n_heads, n_kv, hd = GROUPED, 8, 2, 128
    cq, ck = problem("deficient", n_heads, n_kv, hd)
    order = score_order(ops, dev, cq, ck, mode, 1e-4, 1e-2)

    def shifted(a):
        flat = torch.empty(a.size + 1, dtype=F64, device=dev)
        view = flat[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view
    aligned = ops.qk_rank_curve(torch.from_numpy(cq).to(dev), torch.from_numpy(ck).to(dev), mode, 1e-4, 1e-2, order)
    q8, k8 = shifted(cq), shifted(ck)
    first = ops.qk_rank_curve(q8, k8, mode, 1e-4, 1e-2, order)
    second = ops.qk_rank_curve(q8, k8, mode, 1e-4, 1e-2, order)
    torch.cuda.synchronize()
    for x, y, z in zip(aligned, first, second):
        assert same(x, y) and same(y, z)


# ---------------------------------------------------------------- 9. argument errors
def test_bad_arguments(ops, dev):
    from modegpt_amd import _lib
    lib = _lib.load()
    n_heads, n_kv, hd = 4, 2, 16
    cq, ck = (torch.from_numpy(a).to(dev) for a in problem("full", n_heads, n_kv, hd))
    ns = hd // 2
    order = torch.arange(ns, dtype=torch.int64, device=dev).repeat(n_kv, 1).contiguous()
    big = torch.full((4096,), -1.0, dtype=F64, device=dev)
    ibig = torch.full((4096,), -1, dtype=torch.int64, device=dev)
    p = [big.data_ptr() + 8 * 512 * i for i in range(5)]

    def call(q=cq.data_ptr(), k=ck.data_ptr(), nh=n_heads, nkv=n_kv, hd_=hd, mode=GROUPED, o=order.data_ptr(), ch=p[0], c=p[1], t=p[2], s=p[3],
             gc=p[4], go=ibig.data_ptr()):
        return lib.mdg_qk_rank_curve(q, k, nh, nkv, hd_, 1e-4, 1e-2, mode, o, 1e-4, 1e-2, ch, c, t, s, gc, go, None)

    bad = [dict(q=None), dict(k=None), dict(o=None), dict(ch=None), dict(c=None),      # a null required pointer
           dict(hd_=15), dict(hd_=15, mode=MHA, nh=2),                                  # odd hd in a RoPE mode
           dict(hd_=258), dict(hd_=260),                                                # hd / 2 > 128
           dict(mode=OPT), dict(mode=OPT, hd_=130, nh=2), dict(mode=MHA),               # OPT / MHA with n_heads != n_kv, OPT hd > 128
           dict(gc=None), dict(go=None),                                                # one of the greedy pair
           dict(nkv=3), dict(nkv=0), dict(hd_=0), dict(mode=3), dict(mode=-1)]
    for kw in bad:
        assert call(**kw) == _lib.MDG_ERR_BAD_ARG, kw
        with pytest.raises(RuntimeError):
            _lib.check(call(**kw), "mdg_qk_rank_curve")
    torch.cuda.synchronize()
    assert bool((big == -1.0).all()) and bool((ibig == -1).all())                      # nothing was enqueued
    assert call() == _lib.MDG_OK and call(t=None, s=None, gc=None, go=None) == _lib.MDG_OK      # every optional output absent
    torch.cuda.synchronize()
    assert bool(torch.isfinite(big[:n_heads * (ns + 1)]).all())
    with pytest.raises(RuntimeError):
        ops.qk_rank_curve(cq.cpu(), ck.cpu(), GROUPED, 0.0, 0.0, order.cpu())         # no CPU fallback
    for kw in (dict(order=order[:, :-1]), dict(order=order.to(torch.int32)), dict(cov_k=ck[:, :-1]), dict(cov_q=cq[0]), dict(mode=7)):
        args = dict(cov_q=cq, cov_k=ck, mode=GROUPED, ridge_q=0.0, ridge_k=0.0, order=order)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.qk_rank_curve(**args)


# ---------------------------------------------------------------- 10. end to end: MODEGPT_QK_ERROR=1
@pytest.mark.parametrize("kind", ["llama_gqa", "opt"])
def test_model_end_to_end(dev, kind, tmp_path, monkeypatch):
    from modegpt_amd import ops
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig
    from modegpt_amd.adapters.model_adapter import ModelAdapter
    from modegpt_amd.calibration import load_calibs
    from modegpt_amd.compression import compress_qk as CQ
    from tests.test_gpu_e2e import _tiny_model

    model_ = _tiny_model(kind, dev)
    conf = lambda name: CompressionConfig(temp_storage_dir=str(tmp_path / name), nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5,       # noqa: E731
                                          dataset="synthetic", calib_size=6, calibs_batch_size=4, compression_ratio=0.3,
                                          order="mlp,qk,vo")
    ad = ModelAdapter.from_model(model_, None)
    ad.config = conf("off")
    stats = str(tmp_path / "stats")
    calibs = load_calibs(ad, n_samples=6, batch_size=4, dataset="synthetic", calibs_save_path=stats, target_layers=[])
    layers = list(range(ad.n_layers))
    keep = [0.7, 1.0][:ad.n_layers] + [0.6] * max(0, ad.n_layers - 2)
    hd, g = ad.head_dim, ad.n_heads // ad.n_kv_heads
    mode, rq, rk = CQ.qk_mode_and_ridges(ad.arch, ad.n_kv_heads != ad.n_heads, ad.config.ridge_qk)
    ns, w = QK.units(mode, hd)

    def compress(adapter, cov):
        """Layer by layer, as compress_qk does, keeping the mask every layer's selection returned."""
        return [CQ.compress_layer(adapter, l, CQ.qk_rank_rule(hd, keep[l], adapter.arch), cov_q_list=cov[1][l], cov_k_list=cov[2][l],
                                  rotary_masks=[]).cpu() for l in layers]

    # the switch unset: nothing is launched, no key appears
    calls = []
    real = ops.qk_rank_curve
    monkeypatch.setattr(ops, "qk_rank_curve", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    monkeypatch.delenv("MODEGPT_QK_ERROR", raising=False)
    CQ.compress_qk(ad, (calibs[1], calibs[2]), keep, target_layers=layers)
    assert not calls and ad.report_qk_errors() == {}
    assert "qk_logit_error" not in ad.metrics and not getattr(ad, "qk_errors", None)

    def check_on(adapter, cov, masks, name):
        report = adapter.report_qk_errors()
        assert sorted(report) == layers and sorted(adapter.metrics["qk_logit_error"]) == [str(l) for l in layers]
        json.dumps(adapter.metrics["qk_logit_error"], allow_nan=False)
        for l in layers:
            m = adapter.metrics["qk_logit_error"][str(l)]
            host = adapter.qk_errors[l]
            assert m == report[l] and len(host) == 7 and all(not t.is_cuda for t in host)
            order = host[6].numpy()
            rank = CQ.qk_rank_rule(hd, keep[l], adapter.arch)
            take = rank // w
            assert m["rank"] == rank and m["units_kept"] == take and m["n_kv"] == adapter.n_kv_heads == len(m["heads"])
            assert np.array_equal(masks[l][:, :take].numpy(), order[:, :take])           # the selection is a prefix of the order
            cq, ck = (c[l].detach().cpu().to(F64).numpy() for c in (cov[1], cov[2]))
            ref = QK.model(cq, ck, mode, 0.0, 0.0, order)                               # the raw statistics: ridges 0
            t_ref = QK.terms(cq, ck, mode, rq, rk, order)                               # the terms of the real scores
            unit = (g * hd * hd + 2) * U
            worst = 0.0
            for kv, hm in enumerate(m["heads"]):
                for key, at in (("energy", 0), ("error", take)):
                    err, bound = abs(LD(hm[key]) - ref["curve"][kv][at]), unit * ref["A"][kv][at]
                    assert err <= bound, (l, kv, key)
                    worst = max(worst, float(err / bound) if bound > 0 else 0.0)
                want_diag = t_ref[kv][take:].sum()
                assert abs(LD(hm["diagonal_estimate"]) - want_diag) <= (2 * g * w + 2 + ns) * U * want_diag
                assert len(hm["head_relative_error"]) == g and hm["noise_floor"] is not None and hm["noise_floor"] < 1e-6
            total_err, total_bound = abs(LD(m["error"]) - ref["curve"][:, take].sum()), unit * ref["A"][:, take].sum() + 4 * U * ref["curve"][:, take].sum()
            assert total_err <= total_bound
            if keep[l] == 1.0:
                assert m["error"] == 0.0 and m["relative_error"] == 0.0 and all(hm["error"] == 0.0 for hm in m["heads"])
            else:
                assert 0.0 < m["relative_error"] < 1.0 and 0.0 <= m["greedy_relative_error"] < 1.0
            print("E2E %s %s layer %d: rank %d of %d, relative_error %.3e, diagonal_ratio %s, greedy %.3e, non_monotone %s, error vs model %.2e "
                  "of the bound" % (kind, name, l, rank, hd, m["relative_error"], m["diagonal_ratio"], m["greedy_relative_error"],
                                    m["non_monotone"], worst))
        assert adapter.report_qk_errors() == {}                                          # read once
        return report

    off_masks = compress(ad, calibs)
    assert not calls
    monkeypatch.setenv("MODEGPT_QK_ERROR", "1")
    ad.config = conf("on")
    masks = compress(ad, calibs)
    assert len(calls) == len(layers)
    assert all(torch.equal(a, b) for a, b in zip(off_masks, masks))                      # the report changes no selection
    report = check_on(ad, calibs, masks, "on")

    # once through saved statistics: a fresh adapter, no forward pass
    ad2 = ModelAdapter.from_model(model_, None)
    ad2.config = conf("loaded")
    fired = []
    hook = model_.register_forward_pre_hook(lambda *a: fired.append(1))
    try:
        calibs2 = load_calibs(ad2, n_samples=6, batch_size=4, dataset="synthetic", load_calibs_from=stats, target_layers=[])
    finally:
        hook.remove()
    assert not fired, "the model ran"
    assert check_on(ad2, calibs2, compress(ad2, calibs2), "loaded") == report

    for l in layers:                                                                     # ... and no artefact
        off = torch.load(os.path.join(str(tmp_path / "off"), f"layer_{l}_qk"), map_location="cpu")
        for name in ("on", "loaded"):
            on = torch.load(os.path.join(str(tmp_path / name), f"layer_{l}_qk"), map_location="cpu")
            assert sorted(off) == sorted(on)
            for k in off:
                assert torch.equal(off[k].contiguous().view(torch.int16), on[k].contiguous().view(torch.int16)), (l, name, k)


def test_run_modegpt_writes_the_report_beside_qk_selection(dev, tmp_path, monkeypatch):
    """The driver with MODEGPT_QK_ERROR=1 (the local-checkpoint set-up of tests/test_gpu_e2e.py): metrics.json holds a qk_logit_error
    entry per layer beside qk_selection."""
    transformers = pytest.importorskip("transformers")
    tokenizers = pytest.importorskip("tokenizers")
    from modegpt_amd import run_modegpt
    from modegpt_amd.adapters.CompressionConfig import CompressionConfig

    vocab = {f"w{i}": i for i in range(208)}
    vocab.update({"<unk>": 208, "<s>": 209, "</s>": 210})
    tok = tokenizers.Tokenizer(tokenizers.models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.Whitespace()
    fast = transformers.PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", bos_token="<s>", eos_token="</s>")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(hidden_size=128, intermediate_size=320, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, head_dim=32, vocab_size=211, max_position_embeddings=64, initializer_range=0.15)
    src = tmp_path / "src_model"
    transformers.LlamaForCausalLM(cfg).to(torch.bfloat16).save_pretrained(src)
    fast.save_pretrained(src)
    monkeypatch.chdir(tmp_path)                                                          # logs/, metrics/ land in the temp dir
    monkeypatch.setenv("MODEGPT_QK_ERROR", "1")
    conf = CompressionConfig(model=str(src), output_dir=str(tmp_path / "out"), temp_storage_dir=str(tmp_path / "out" / "layers"),
                             dataset="synthetic", order="mlp,qk,vo", calib_size=8, calibs_batch_size=4, compression_ratio=0.3,
                             nystrom_ridge=1e-4, ridge_qk=1e-2, ridge_vo=1e-5, note="pytest-qk-error")
    ppl = run_modegpt.main(config=conf)
    assert ppl is not None and ppl == ppl
    runs = json.load(open(tmp_path / "metrics" / "metrics.json"))
    # (metrics.json holds every run of this process; the driver's is the one with a perplexity)
    mine = [r for r in runs.values() if "qk_logit_error" in r and "ppl-synthetic" in r]
    assert len(mine) == 1, sorted(runs)
    m = mine[0]
    assert sorted(m["qk_logit_error"]) == sorted(m["qk_selection"]) == ["0", "1"]
    for l, entry in m["qk_logit_error"].items():
        assert entry["n_kv"] == 2 == len(entry["heads"]) and entry["head_dim"] == 32 and entry["rank"] % 2 == 0
        assert entry["energy"] > 0 and 0.0 <= entry["relative_error"] < 1.0 and entry["noise_floor"] < 1e-6
        print("DRIVER layer %s: rank %d, relative_error %.3e, diagonal_ratio %s, greedy %.3e" % (
            l, entry["rank"], entry["relative_error"], entry["diagonal_ratio"], entry["greedy_relative_error"]))
