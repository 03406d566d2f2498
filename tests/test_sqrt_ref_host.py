"""tests/sqrt_ref.py checks itself (no GPU): the long-double truths square back to the input, the fp64 Newton-Schulz model reaches
"ok" where tests/test_gpu_sqrt_large.py expects the Newton route to answer and gives up on the indefinite spectrum, and the
yardstick e_ref of every accuracy case is finite (printed under pytest -s)."""
import numpy as np
import pytest

from tests import eig_ref as R
from tests import sqrt_ref as S

EXACT_CASES = [((R.exact_spectrum, 256, kind), S.EXACT_RIDGE) for kind in S.EXACT_KINDS]


def _name(case, ridge):
    return f"{S.case_name(case)} ridge={ridge:g}"


def _truth(case, ridge, scaled=False):
    if case[0] is R.exact_spectrum:
        return S.exact_truth(case[1], case[2], ridge, scaled)
    return S.truth(case, ridge, scaled)


@pytest.mark.parametrize("case,ridge", S.TRUTH_CASES + EXACT_CASES, ids=lambda v: S.case_name(v) if isinstance(v, tuple) else None)
def test_truth_squares_back_and_yardsticks_are_finite(case, ridge):
    A = S.case_matrix(case)
    n = A.shape[0]
    root, inv, lam = _truth(case, ridge)
    clamped = bool((lam + ridge < 0).any())
    if not clamped:                                        # (with a clamp the root is that of the PSD part, not of A + ridge I)
        r = float(S.res_root(root, A, ridge))
        print(f"{_name(case, ridge)}: truth res_root {r:.3e} against n 2^-60 = {n * 2.0 ** -60:.3e}")
        assert r <= n * 2.0 ** -60
    else:
        H, f = R.ld(R.exact_spectrum(case[1], case[2])[2]), np.sqrt(np.maximum(lam + ridge, 0))
        assert float(S.frob_err(root @ root, (H * f * f) @ H.T)) <= n * 2.0 ** -60
    for route, scaled, rdg in (("newton", False, ridge), ("eigen", False, ridge), ("eigen", True, 1e-3)):
        t = _truth(case, rdg, scaled)
        refs = S.references(case, rdg, scaled, route)
        assert len(refs) == 2
        for slot, what in ((1, "root"), (2, "inverse root")):
            e = S.e_ref(refs, lambda X: S.frob_err(X, t[slot - 1]), slot)
            print(f"e_ref {_name(case, rdg)} scaled={scaled} {route} {what}: {e:.3e}  ({' / '.join(r[0] for r in refs)})")
            assert np.isfinite(e)
        if route == "eigen":
            e = S.e_ref(refs, lambda l: S.eval_err(l, t[2]), 3)
            print(f"e_ref {_name(case, rdg)} scaled={scaled} eigenvalues: {e:.3e}")
            assert np.isfinite(e)


@pytest.mark.parametrize("case,ridge", S.TRUTH_CASES + EXACT_CASES + [(S.GATE_CASE, S.GATE_RIDGES[0])],
                         ids=lambda v: S.case_name(v) if isinstance(v, tuple) else None)
def test_newton_model_status(case, ridge):
    """"ok" on every input the Newton route is expected to answer; the indefinite spectrum is given up on, not iterated to the end."""
    root, inv, steps, status = S.newton_yardstick(case, ridge)
    print(f"Newton-Schulz model {_name(case, ridge)}: {status} after {steps} steps")
    if case[0] is R.exact_spectrum and case[2] == "indefinite":
        assert status in ("diverged", "stuck") and root is None
        return
    assert status == "ok"
    assert float(S.asym(root)) == 0.0 and float(S.asym(inv)) == 0.0
    # a sanity bound only (the accepted residual 1e-7 squared per step): the model's root does square back to A + ridge I
    assert float(S.res_root(root, S.case_matrix(case), ridge)) < 1e-9


def test_newton_model_step_counts():
    """The counts the iteration needs: ~log_2.25(||A||_F / lambda_min) + a few, growing with the condition number."""
    s5 = S.newton_yardstick(S.GATE_CASE, 1e-5)[2]
    s12 = S.newton_yardstick(S.GATE_CASE, 1e-12)[2]
    sw = S.newton_yardstick((R.wishart, 130), 1e-5)[2]
    print(f"Newton-Schulz model steps: wishart(130) {sw}, rank_deficient(130) ridge 1e-5 {s5}, ridge 1e-12 {s12}")
    assert sw < s5 < s12 < S.NS_MAX_STEPS


@pytest.mark.parametrize("n", S.RESIDUAL_SIZES)
def test_residual_yardsticks(n):
    case = (R.wishart, n)
    A = S.case_matrix(case)
    assert S.newton_yardstick(case, 1e-5)[3] == "ok"       # (else references() would hand a Newton call the Jacobi yardstick)
    for route, second in (("newton", "Newton-Schulz model"), ("eigen", "fp64 Jacobi")):
        refs = S.references(case, 1e-5, False, route)
        assert [r[0] for r in refs] == ["LAPACK formula", second]
        e1 = S.e_ref(refs, lambda X: S.res_root(X, A, 1e-5), 1)
        e2 = max(float(S.res_inv(r[2], r[1])) for r in refs)
        print(f"e_ref wishart n={n} {route}: res_root {e1:.3e} res_inv {e2:.3e}")
        assert np.isfinite(e1) and np.isfinite(e2) and e1 < 1e-12 and e2 < 1e-9


def test_gate_yardsticks():
    for ridge in S.GATE_RIDGES:
        route = "newton" if ridge >= 1e-12 else "eigen"
        t = S.truth(S.GATE_CASE, ridge)
        refs = S.references(S.GATE_CASE, ridge, False, route)
        e = S.e_ref(refs, lambda X: S.frob_err(X, t[0]), 1)
        print(f"e_ref rank_deficient(130) ridge={ridge:g} {route} root: {e:.3e}  ({' / '.join(r[0] for r in refs)})")
        assert np.isfinite(e) and len(refs) == 2
        ei = S.e_ref(refs, lambda X: S.frob_err(X, t[1]), 2)
        print(f"e_ref rank_deficient(130) ridge={ridge:g} {route} inverse root: {ei:.3e}")
        assert np.isfinite(ei)
        # the gate of test_gpu_sqrt_large.py::test_ridge_gate holds the inverse root at the two positive ridges, not at 0
        assert (float(t[2].min()) + ridge > 130 * 2.0 ** -52 * float(np.abs(t[2]).max())) == (ridge > 0)


def test_metrics_on_known_matrices():
    D = np.diag([4.0, 9.0])
    Rt = np.diag([2.0, 3.0])
    assert S.res_root(Rt, D, 0.0) == 0 and S.res_inv(np.diag([0.5, 1 / 3]), Rt) < 2.0 ** -53 and S.asym(Rt) == 0
    X = np.array([[2.0, 1.0], [0.0, 3.0]])
    assert abs(float(S.asym(X)) - np.sqrt(2.0 / 14.0)) < 1e-15
    assert abs(float(S.frob_err(X, Rt)) - 1.0 / np.sqrt(13.0)) < 1e-15
    P = S.pad_even(np.ones((3, 3)))
    assert P.shape == (4, 4) and P[3].sum() == 0 and P[:, 3].sum() == 0 and S.pad_even(D) is D
