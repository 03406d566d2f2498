"""CPU: the host model of the greedy MLP selection (tests/greedy_model.py) against what it claims to be, and the conditions the
GPU cases of tests/test_gpu_greedy.py rest on."""
import numpy as np
import pytest

from tests import chol_ref as R
from tests import greedy_model as G
from tests import rank_curve_model as RC

LD = R.LD


def test_partition():
    for r in (0, 1, 5, 33, 91, 300):
        for rounds in (1, 3, 8, 32, max(r, 1), r + 7):
            m = G.partition(r, rounds)
            T = min(rounds, r)
            assert len(m) == rounds and sum(m) == r
            assert all(x >= 1 for x in m[:T]) and all(x == 0 for x in m[T:])
            assert max(m[:T], default=0) - min(m[:T], default=0) <= 1
            assert m[:T] == [r * (t + 1) // T - r * t // T for t in range(T)]
    assert G.partition(10, 3) == [3, 3, 4] and G.partition(2, 5) == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("n,d,r,kind", [(12, 4, 8, "mixed"), (24, 6, 10, "iid")])
def test_exact_greedy_is_brute_force(n, d, r, kind):
    """T = r: at every step the picked column is the one whose J(S + {j}), recomputed from scratch, is smallest."""
    C, W = G.case(n, d, kind, seed=3)
    order, objective, cut, n_dead, _ = G.greedy(C, W, r, r)
    assert n_dead == 0 and len(set(order.tolist())) == r
    A = G.scale_A(C, W)
    for step in range(r):
        S = order[:step].tolist()
        rest = [j for j in range(n) if j not in S]
        J = np.array([G.objective_of(C, W, S + [j]) for j in rest])
        best = rest[int(np.argmin(J))]
        assert best == order[step], (step, best, order[step])
        assert abs(J.min() - objective[step + 1]) <= 1e-15 * A
        # the gain IS the drop, and the cut holds the picked gain and the runner-up's
        assert abs((objective[step] - objective[step + 1]) - cut[step, 0]) <= 1e-15 * A
        if len(rest) > 1:
            assert abs((objective[step] - np.sort(J)[1]) - cut[step, 1]) <= 1e-15 * A
        else:
            assert np.isnan(cut[step, 1])


@pytest.mark.parametrize("n,d", G.SHAPES[:2])
def test_objective_properties(n, d):
    C, W = G.shared_case(n, d)
    A = G.scale_A(C, W)
    scores = RC.ridge_scores_fp64(C, G.RIDGE)
    for r in (int(0.7 * n), n):
        for rounds in (1, 3, r):
            order, objective, cut, n_dead, _ = G.reference(n, d, r, rounds)
            assert sorted(set(order.tolist())) == sorted(order.tolist()) and len(order) == r
            assert all(objective[t + 1] <= objective[t] for t in range(rounds))
            assert abs(objective[rounds] - G.objective_of(C, W, order)) <= 1e-15 * A
            perm = G.order_with_rest(order, scores)
            assert sorted(perm.tolist()) == list(range(n))
            assert abs(objective[rounds] - RC.curve(C, perm, W, G.EPS)[r]) <= 1e-15 * A
            assert abs(objective[0] - RC.curve(C, perm, W, G.EPS)[0]) <= 1e-15 * A
            m = G.partition(r, rounds)
            at = 0
            for t in range(rounds):                      # ascending index within a round
                assert list(order[at:at + m[t]]) == sorted(order[at:at + m[t]])
                at += m[t]


def test_rounds_beyond_the_rank_repeat():
    C, W = G.shared_case(48, 8)
    a = G.greedy(C, W, 3, 3)
    b = G.greedy(C, W, 3, 8)
    assert list(a[0]) == list(b[0])
    assert np.array_equal(a[1], b[1][:4]) and all(b[1][4:] == a[1][3])
    assert np.array_equal(a[2], b[2][:3], equal_nan=True) and np.isnan(b[2][3:]).all()
    z = G.greedy(C, W, 0, 5)
    assert len(z[0]) == 0 and len(z[1]) == 6 and all(z[1] == z[1][0]) and np.isnan(z[2]).all()


@pytest.mark.parametrize("n,d", G.SHAPES)
def test_gpu_cases_are_well_separated(n, d):
    """The condition the GPU comparison of `order` rests on: in every shared case every round's cut is at least 1e-6 wide relative
    to the picked gain, in long double, and nothing is dead; the plain fp64 model then takes the same columns in the same order."""
    narrowest = np.inf
    for n_, d_, r, rounds in G.gpu_cases():
        if (n_, d_) != (n, d):
            continue
        order, objective, cut, n_dead, gaps = G.reference(n, d, r, rounds)
        assert n_dead == 0, (r, rounds)
        assert min(gaps, default=np.inf) >= 1e-6, (r, rounds, min(gaps))
        narrowest = min(narrowest, min(gaps, default=np.inf))
        assert list(G.reference_fp64(n, d, r, rounds)[0]) == list(order), (r, rounds)
    print("GAP n=%d d=%d: narrowest cut over all (r, T): %.3e" % (n, d, narrowest))


def test_greedy_beats_the_ridge_rule_on_the_correlated_case():
    n, d = 130, 40
    r = int(0.7 * n)
    C, W = G.shared_case(n, d)
    ridge = RC.smallest_sorted(RC.ridge_scores_fp64(C, G.RIDGE), r)
    j_ridge, j0 = G.objective_of(C, W, ridge), G.objective_of(C, W, [])
    for rounds in (8, r):
        j = G.reference(n, d, r, rounds)[1][-1]
        print("RIDGE %.3e  T=%d %.3e  (of J0)" % (j_ridge / j0, rounds, j / j0))
        assert j < j_ridge


def test_duplicates_are_dead_picks():
    C, W, dup = G.duplicate_case()
    n = C.shape[0]
    live = n - len(dup)
    for dt in (LD, np.float64):
        order, objective, cut, n_dead, _ = G.greedy(C, W, live, live, eps=0.0, dt=dt)
        assert n_dead == 0 and not set(dup) & set(order.tolist())
        order, objective, cut, n_dead, _ = G.greedy(C, W, n, n, eps=0.0, dt=dt)
        assert n_dead == len(dup) and list(order[live:]) == sorted(dup)
        assert np.isnan(cut[live:]).all() and all(objective[live:] == objective[live])
