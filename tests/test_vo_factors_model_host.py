"""Host (no GPU, no package): the metrics tests/vo_error_model.py adds for tests/test_gpu_vo_factors.py -- W (whitening), P (per-head
map), F (signed factors), L (MHA Gram) -- on the model's own factors.  In long double they vanish to 1e-17 times a size factor; on
the fp64 model they stay under the criterion's floor 64 (d + hd + r) 2^-53 for the GPU test's cases (the reference alone stays within
the criterion); and a deliberately wrong factor pushes each of them above that floor by many orders."""
import numpy as np
import pytest

from tests import vo_error_model as VO
from tests.output_error_model import LD
from tests.test_gpu_vo_factors import CASES, RIDGE, U, case_id, case_key, gaps_hold, metric_values, model_factors, problem, spectra


def metrics_of(case):
    return "WPFL" if case[3][0] == case[3][1] else "WPF"


@pytest.mark.parametrize("case", CASES, ids=case_id)    # (the ranks of one problem share its decomposition)
def test_model_factors_meet_their_own_metrics(case):
    hd, r, d = case[:3]
    key = case_key(*case)
    tv, to = model_factors(key, r, RIDGE, LD)
    cv, co = model_factors(key, r, RIDGE, np.float64)
    cond = max(float(s[0][0] / s[0][r - 1]) for s in spectra(key, RIDGE, LD))
    for m in metrics_of(case):
        if m in "PF":
            assert gaps_hold(key, r, RIDGE, m)
        exact = metric_values(key, r, RIDGE, tv, to, m)
        fp64 = metric_values(key, r, RIDGE, cv, co, m)
        floor = 64 * (d + hd + r) * U
        print("MODEL %s %s: long double %.3e, fp64 %.3e, floor %.3e (lam_1 / lam_r %.2e)" % (case_id(case), m, exact, fp64, floor, cond))
        # long double: P and F compare the factors with themselves (0); W and L carry the decomposition's own rounding, 2^-64 per
        # operation over sums of length d + hd -- 1e-17 times the size
        assert exact <= 1e-17 * (d + hd + r)
        assert fp64 <= floor


def wrong_factors(key, r, how):
    """The long-double factors of rank r with one deliberate defect."""
    kind, d, n_heads, n_kv, hd = key[:5]
    C, Wv, Wo = problem(*key)
    spec = spectra(key, RIDGE, LD)
    if how == "swapped component":                      # components 0 and 1 of kv head 0 exchanged, in v alone
        v, o = (t.copy() for t in model_factors(key, r, RIDGE, LD))
        v[[0, 1]] = v[[1, 0]]
        return v, o
    if how == "transposed V":
        bad = [(lam, V.T.copy(), lam2, Up) for lam, V, lam2, Up in spec]
        return VO.factors(bad, Wv, Wo, n_heads, n_kv, hd, r, LD)
    assert how == "S for 1 / S"                         # v' = S_r V_r^T W_v,g (MHA: Up_r^T S V^T W_v); o' as it should be
    rows = []
    for g, (lam, V, lam2, Up) in enumerate(spec):
        S = np.sqrt(lam)
        P = (V[:, :r] * S[:r]).T if lam2 is None else Up[:, :r].T @ (V * S).T
        rows.append(P @ VO.wide(Wv, LD)[g * hd:(g + 1) * hd])
    return np.concatenate(rows), model_factors(key, r, RIDGE, LD)[1]


# what each defect must move: a permutation of whitened components is still whitened, and L reads o alone
SEEN_BY = {"swapped component": "PF", "transposed V": "WPFL", "S for 1 / S": "WPF"}
assert set("".join(SEEN_BY.values())) == set("WPFL")


@pytest.mark.parametrize("how", list(SEEN_BY))
@pytest.mark.parametrize("case", [CASES[4], CASES[6]], ids=case_id)
def test_a_wrong_factor_is_seen_by_every_metric(case, how):
    hd, r, d = case[:3]
    key = case_key(*case)
    v, o = wrong_factors(key, r, how)
    floor = 64 * (d + hd + r) * U
    for m in metrics_of(case):
        err = metric_values(key, r, RIDGE, v, o, m)
        print("WRONG %s %s %s: %.3e (floor %.3e)" % (case_id(case), how, m, err, floor))
        if m in SEEN_BY[how]:
            assert err > 1e6 * floor, (how, m, err)


def test_the_safe_division_changes_nothing_where_s_is_positive():
    """VO.factors drops a component whose eigenvalue is 0 (as vo.hip does) and is otherwise V / S entry by entry."""
    case = CASES[4]
    key = case_key(*case)
    kind, d, n_heads, n_kv, hd = key[:5]
    for lam, V, _, _ in spectra(key, RIDGE, LD):
        S = np.sqrt(np.maximum(lam, 0))
        assert bool((S > 0).all())
    C, Wv, Wo = problem(*key)
    v, _ = model_factors(key, hd, RIDGE, LD)
    lam, V, _, _ = spectra(key, RIDGE, LD)[0]
    want = (V / np.sqrt(lam)).T @ VO.wide(Wv, LD)[:hd]
    assert np.array_equal(v[:hd], want)
    dead = case_key(*case, dead=(1, 5))
    tv, to = model_factors(dead, hd, RIDGE, LD)
    assert bool(np.isfinite(tv).all()) and bool(np.isfinite(to).all())
    assert bool((tv[2 * hd - 1] == 0).all()) and spectra(dead, RIDGE, LD)[1][0][-1] == 0
