"""Host (no GPU): the long-double model of the MLP error-versus-rank curve (tests/rank_curve_model.py) -- that the suffix sums of
the column norms of W[:, pi] L ARE the Nystrom residual traces, the sandwich that ties the curve to the refit the engine stores,
the prefix property of the ridge-score order -- and ops.decode_rank_curve, which is pure host code."""
import functools
import math

import numpy as np
import pytest
import torch

from modegpt_amd import ops
from tests import chol_ref as R
from tests import rank_curve_model as RC

EPS = 1e-6
RIDGE = float(torch.tensor(1e-4, dtype=torch.float32).double())


@functools.lru_cache(maxsize=None)
def case(n, d, tokens):
    """(C, W, order): a gated-activation covariance, a bf16-valued down projection, the ridge-score order."""
    C = RC.covariance(RC.gated_acts(tokens, n, seed=n + d))
    gen = torch.Generator().manual_seed(17 * n + d)
    W = (torch.randn(d, n, generator=gen) * 0.05).to(torch.bfloat16).double().numpy()
    return C, W, RC.argsort_stable(RC.ridge_scores_fp64(C, RIDGE))


def test_curve_is_the_schur_complement_trace_at_every_rank():
    """n = 48: curve[r] against tr(W (M - M[:, S] M_SS^-1 M[S, :]) W^T) computed directly with a solve, for r = 0 .. n.  Both sides
    are long double; they differ by the rounding of two different routes, of order n 2^-64 cond(M_SS) -- cond <= ~1e5 here (the
    column scales span three decades of variance): 1e-12 of curve[0] is three decades above that and four below fp64 noise."""
    n, d = 48, 7
    C, W, order = case(n, d, 200)
    cv = RC.curve(C, order, W, EPS)
    assert cv.shape == (n + 1,)
    direct = np.array([RC.schur_trace(C, order, W, EPS, r) for r in range(n + 1)])
    worst = float((np.abs(cv - direct) / cv[0]).max())
    print("SCHUR n=48 max |curve - direct| / curve[0] = %.3e" % worst)
    assert worst <= 1e-12
    # curve[0] = tr(W M W^T), the energy of the uncompressed output
    M = R.ld(RC.gathered(C, np.arange(n), EPS))
    assert abs(cv[0] - ((R.ld(W) @ M) * R.ld(W)).sum()) <= 1e-15 * cv[0]


@pytest.mark.parametrize("n,d,tokens", [(48, 7, 200), (385, 70, 300)])
def test_curve_is_non_increasing_and_ends_at_zero(n, d, tokens):
    C, W, order = case(n, d, tokens)
    for cv in (RC.curve(C, order, W, EPS), RC.curve_fp64(C, order, W, EPS)):
        assert cv[n] == 0
        assert bool((cv[:-1] >= cv[1:]).all())
        assert cv[0] > 0


# (385, 70, 300): fewer tokens than features -- C has rank 300 and only eps makes M factorable
@pytest.mark.parametrize("keep", [0.5, 0.7, 0.9])
@pytest.mark.parametrize("n,d,tokens", [(385, 70, 300), (384, 96, 1024)])
def test_sandwich_around_the_stored_refit(n, d, tokens, keep):
    """E_D + eps ||U||^2 - eps ||W_S||^2 <= curve[r] <= E_D + eps ||U||^2 with D the refit mdg_nystrom_down computes
    (chol_ref.nystrom: solved with C[S, :]), everything in long double.  The slack allowed is the rounding of the long-double
    routes themselves, as in the Schur test: 1e-12 of curve[0] (the sandwich is ~1e-5 of it wide)."""
    C, W, order = case(n, d, tokens)
    r = int(n * keep)
    idx = np.sort(order[:r])
    D = R.nystrom(torch.from_numpy(C), idx, W, EPS)
    lo, hi = RC.sandwich(C, W, idx, D, EPS)
    cv = RC.curve(C, order, W, EPS)
    q = cv[0]
    print("SANDWICH n=%d keep=%.1f width/q %.3e  (hi - curve)/q %.3e  (curve - lo)/q %.3e" % (
        n, keep, float((hi - lo) / q), float((hi - cv[r]) / q), float((cv[r] - lo) / q)))
    assert lo - 1e-12 * q <= cv[r] <= hi + 1e-12 * q
    assert lo < hi


def test_prefix_property_of_the_order():
    """sorted(argsort_stable(scores)[:r]) is the selection mdg_select_smallest_sorted states ("ties: lower index first, NaN
    largest"), for every r -- scores with ties, a NaN, an inf and a signed zero."""
    s = np.array([0.5, 0.25, 0.5, np.nan, 0.125, 0.25, 0.0, -0.0, np.inf, 0.5, 0.25, 3.0, np.nan, 0.125])
    order = RC.argsort_stable(s)
    assert sorted(order.tolist()) == list(range(len(s)))
    for r in range(len(s) + 1):
        assert sorted(order[:r].tolist()) == RC.smallest_sorted(s, r).tolist(), r
    # and torch's stable argsort is that order
    assert torch.argsort(torch.from_numpy(s), stable=True).tolist() == order.tolist()


# ---------------------------------------------------------------- ops.decode_rank_curve
def test_decode_keep_grid_and_rounding():
    n = 37
    curve = [float(n - r) for r in range(n + 1)]                 # rel(r) = 1 - r / n
    m = ops.decode_rank_curve(curve, 25)
    assert m["n"] == n and m["rank"] == 25 and m["energy"] == float(n)
    assert m["rel_error"] == curve[25] / curve[0]
    assert len(m["keep"]) == 20 and m["keep"][0] == 0.05 and m["keep"][-1] == 1.0
    assert all(abs(k - 0.05 * (i + 1)) < 1e-12 for i, k in enumerate(m["keep"]))
    assert m["rel_error_at_keep"] == [curve[int(n * k)] / curve[0] for k in m["keep"]]      # int(n * keep), as compress_weights
    assert m["rel_error_at_keep"][-1] == 0.0
    assert int(n * m["keep"][13]) == 25                           # 0.7 * 37 = 25.9 -> 25
    # accepts a CPU tensor as well
    assert ops.decode_rank_curve(torch.tensor(curve, dtype=torch.float64), 25) == m


def test_decode_smallest_rank_search():
    n = 1000
    curve = [10.0 ** (-4.0 * r / n) for r in range(n)] + [0.0]    # rel(r) = 10^(-4 r / n), then 0
    m = ops.decode_rank_curve(curve, 700)
    for target, key in ((1e-1, "0.1"), (1e-2, "0.01"), (1e-3, "0.001")):
        want = next(r for r in range(n + 1) if curve[r] / curve[0] <= target)
        assert m["rank_for_rel_error"][key] == want
        assert want > 0 and curve[want - 1] / curve[0] > target
    assert set(m["rank_for_rel_error"]) == {"0.1", "0.01", "0.001"}
    # a curve that never reaches a target before the end: only the full rank (error 0) does
    m = ops.decode_rank_curve([1.0] * 50 + [0.05, 0.0], 10)
    assert m["rank_for_rel_error"] == {"0.1": 50, "0.01": 51, "0.001": 51}
    # a flat curve: nothing but the full rank
    m = ops.decode_rank_curve([2.0] * 8 + [0.0], 3)
    assert m["rank_for_rel_error"] == {"0.1": 8, "0.01": 8, "0.001": 8} and m["rel_error"] == 1.0
    # rank 0 and rank n
    assert ops.decode_rank_curve([2.0, 1.0, 0.0], 0)["rel_error"] == 1.0
    assert ops.decode_rank_curve([2.0, 1.0, 0.0], 2)["rel_error"] == 0.0
    with pytest.raises(ValueError):
        ops.decode_rank_curve([2.0, 1.0, 0.0], 3)


@pytest.mark.parametrize("energy", [0.0, float("nan"), float("inf")])
def test_decode_zero_and_non_finite_energy(energy):
    m = ops.decode_rank_curve([energy, energy, 0.0], 1)
    assert m["n"] == 2 and m["rank"] == 1
    assert (math.isnan(m["energy"]) if energy != energy else m["energy"] == energy)
    assert m["rel_error"] is None
    assert m["rel_error_at_keep"] == [None] * 20
    assert m["rank_for_rel_error"] == {"0.1": None, "0.01": None, "0.001": None}
