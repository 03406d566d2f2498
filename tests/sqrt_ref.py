"""Host reference of the large square root (mdg_sqrt_psd_large), on top of tests/eig_ref.py.

truth       (root, inv_root, evals) in np.longdouble: eig_ref.reference's long-double Jacobi eigenpairs through eig_ref.sqrt_psd (the
            reference's clamps).  A case is (builder, *args) as eig_ref.reference takes it; cached per process.  One to four seconds at
            n = 130 and about four times that at n = 200, by the CPU: used at those sizes only.
exact_truth the same without an eigensolve at n = 256: A = H diag(lam) H^T of eig_ref.exact_spectrum is exact in fp64, so the truth
            is H f(lam) H^T formed in long double (one long-double product, 0.14 s).
newton_schulz  a plain numpy model of the Newton-Schulz route (eigh.hip sqrt_psd_newton), the iteration and the three stopping
            rules as the source states them, the dtype as a parameter.  In fp64 it is that route's yardstick -- what the iteration
            achieves in working precision on the CPU -- as eig_ref's fp64 Jacobi is the yardstick of the eigen route.
metrics     frob_err, res_root, res_inv, asym: all evaluated in long double.  The residuals need no truth and serve the sizes where a
            long-double Jacobi is too slow, and odd n, which eig_ref.round_robin refuses.

Nothing here is fitted to what the device returns."""
import functools

import numpy as np

from tests import eig_ref as R

LD = R.LD
_J64 = {}                  # case -> (lam, V) of the fp64 host Jacobi


# ---------------------------------------------------------------- truths
@functools.lru_cache(maxsize=None)
def truth(case, ridge, scaled=False):
    """(root, inv_root, evals descending) in long double of A = case[0](*case[1:]); read-only."""
    _, (lam, V, sweeps), (lam64, V64, sweeps64) = R.reference(*case)
    assert sweeps <= R.MAX_SWEEPS and sweeps64 <= R.MAX_SWEEPS, "truth: a host Jacobi run did not converge"
    _J64.setdefault(case, (lam64, V64))                    # (eigen_yardstick need not run the fp64 Jacobi again)
    root, inv = R.sqrt_psd(lam, V, ridge, scaled)
    for x in (root, inv):
        x.setflags(write=False)
    return root, inv, lam


@functools.lru_cache(maxsize=None)
def exact_truth(n, kind, ridge, scaled=False):
    """(root, inv_root, evals descending) in long double of eig_ref.exact_spectrum(n, kind), no eigensolve."""
    _, lam, H = R.exact_spectrum(n, kind)
    root, inv = R.sqrt_psd(R.ld(lam), R.ld(H), ridge, scaled)
    for x in (root, inv):
        x.setflags(write=False)
    return root, inv, R.ld(lam)


def pad_even(A):
    """A with one zero row and column appended when n is odd: the pair of the added index never rotates (a_pq = 0 exactly), which
    is how the device pads to a multiple of 128."""
    n = A.shape[0]
    if n % 2 == 0:
        return A
    P = np.zeros((n + 1, n + 1), dtype=A.dtype)
    P[:n, :n] = A
    return P


def _jacobi64(case):
    """(lam, V) of eig_ref's fp64 Jacobi with the device's arithmetic, once per case and process: the pairs eig_ref.reference
    computed beside a truth where there is one, else a run of its own (odd n padded).  The run must have converged: the
    rebuild from an unconverged one would raise e_ref unnoticed."""
    if case not in _J64:
        A = case_matrix(case)
        n = A.shape[0]
        lam, V, sweeps = R.jacobi_eigh(pad_even(A), np.float64, "device", sort=False)
        assert sweeps <= R.MAX_SWEEPS, f"the fp64 host Jacobi did not converge on {case_name(case)}"
        if n % 2:                                          # the added index never rotates: its pair is (0, e_n), in place
            assert lam[n] == 0.0 and V[n, n] == 1.0 and not V[:n, n].any() and not V[n, :n].any()
        _J64[case] = (lam[:n].copy(), V[:n, :n].copy())
    return _J64[case]


def eigen_yardstick(case, ridge, scaled=False):
    """(root, inv_root, evals) of the eigen route's fp64 host yardstick: eig_ref.sqrt_psd on eig_ref's fp64 Jacobi pairs (the device's
    arithmetic on the CPU).  Odd n: padded with a zero row and column, whose eigenpair (0, e_n) is dropped again."""
    lam, V = _jacobi64(case)
    root, inv = R.sqrt_psd(lam, V, ridge, scaled)
    return root, inv, lam


# ---------------------------------------------------------------- the Newton-Schulz route in numpy
NS_MAX_STEPS = 64


def newton_schulz(A, ridge, dtype=np.float64):
    """(root, inv_root, steps, status) of the coupled Newton-Schulz iteration for sqrt(sym_lower(A) + ridge I) as eigh.hip states it:
        Y0 = A / c, Z0 = I, c = ||A||_F;  T = 3 I - Z Y;  res = ||I - Z Y||_F;  Y <- Y T / 2, Z <- T Z / 2
    stopping rules, read at step k = 0, 1, .. after res is formed:
        res is NaN or > 1e6                                        -> "diverged"  (not positive definite)
        res < 1e-7 and res > 0.25 prev, or res < 1e-14 n           -> "ok"        (the round-off floor)
        k > 8 and res > 0.999 prev and res > 0.9 sqrt(n)           -> "stuck"     (singular / indefinite: at ||I||)
        64 steps                                                   -> "max_steps"
    root = sqrt(c) (Y + Y^T) / 2, inv_root = (Z + Z^T) / (2 sqrt(c)).  steps = the number of updates of (Y, Z) made.  root and inv_root are
    None unless status is "ok"."""
    dt = dtype
    a = R.sym_lower(np.asarray(A).astype(dt))
    n = a.shape[0]
    eye = np.eye(n, dtype=dt)
    a = a + dt(ridge) * eye
    c2 = (a * a).sum()
    with np.errstate(all="ignore"):
        Y = a * (dt(1) / np.sqrt(c2))
        Z = eye.copy()
        prev, status, steps = dt(1e300), "max_steps", 0
        for k in range(NS_MAX_STEPS):
            T = -(Z @ Y) + dt(3) * eye
            res = np.sqrt(((T - dt(2) * eye) ** 2).sum())
            steps = k
            if not (res == res) or res > 1e6:
                status = "diverged"
                break
            if (res < 1e-7 and res > 0.25 * prev) or res < 1e-14 * n:
                status = "ok"
                break
            if k > 8 and res > 0.999 * prev and res > 0.9 * np.sqrt(dt(n)):
                status = "stuck"
                break
            prev = res
            Y, Z = dt(0.5) * (Y @ T), dt(0.5) * (T @ Z)
    if status != "ok":
        return None, None, steps, status
    c = np.sqrt(np.sqrt(c2))
    return dt(0.5) * c * (Y + Y.T), dt(0.5) / c * (Z + Z.T), steps, status


@functools.lru_cache(maxsize=None)
def newton_yardstick(case, ridge):
    A = case[0](*case[1:])
    return newton_schulz(A[0] if isinstance(A, tuple) else A, ridge, np.float64)


def lapack_formula(A, ridge, scaled=False):
    """(root, inv_root, evals ascending) of the reference formula oracle.modegpt_oracle.sqrt_M in fp64 on the CPU (LAPACK eigh)."""
    import torch
    from oracle import modegpt_oracle as O
    M = torch.from_numpy(np.ascontiguousarray(A))
    root, inv = O.sqrt_M(M, ridge, scaled=scaled, inverse_sqrt=True)
    return root.numpy(), inv.numpy(), torch.linalg.eigvalsh(M).numpy()


# ---------------------------------------------------------------- metrics, all evaluated in long double
def _fro(X):
    return np.sqrt((X * X).sum())


def frob_err(X, T):
    """||X - T||_F / ||T||_F"""
    T = R.ld(T)
    return _fro(R.ld(X) - T) / _fro(T)


def res_root(root, A, ridge):
    """||R R - (sym_lower(A) + ridge I)||_F / ||A + ridge I||_F"""
    Rl = R.ld(root)
    Ar = R.sym_lower(R.ld(A)) + LD(ridge) * np.eye(Rl.shape[0], dtype=LD)
    return _fro(Rl @ Rl - Ar) / _fro(Ar)


def res_inv(inv_root, root):
    """||Rinv R - I||_F / sqrt(n)"""
    Rl = R.ld(root)
    n = Rl.shape[0]
    return _fro(R.ld(inv_root) @ Rl - np.eye(n, dtype=LD)) / np.sqrt(LD(n))


def asym(root):
    """||R - R^T||_F / ||R||_F"""
    Rl = R.ld(root)
    return _fro(Rl - Rl.T) / _fro(Rl)


def eval_err(lam, truth_lam):
    """max |sorted lam - sorted truth| / max |truth|"""
    t = np.sort(R.ld(truth_lam))
    return np.abs(np.sort(R.ld(lam)) - t).max() / np.abs(t).max()


# ---------------------------------------------------------------- the cases tests/test_gpu_sqrt_large.py runs
def references(case, ridge, scaled, route):
    """[(name, root, inv_root, evals or None)]: the fp64 CPU results whose LARGER error is e_ref of a call on `route` ("newton": no
    eigenvalues wanted, not scaled, ridge >= 1e-12; "eigen": anything else).
      the reference formula through LAPACK eigh, always;
      the route's own host yardstick: the Newton-Schulz model where it reaches "ok", else (the call falls back) and on the eigen
      route the rebuild from eig_ref's fp64 Jacobi pairs (seconds at n = 256, the slowest case n = 384 several times that)."""
    A = case_matrix(case)
    refs = [("LAPACK formula",) + lapack_formula(A, ridge, scaled)]
    ns = newton_yardstick(case, ridge) if route == "newton" else None
    if ns is not None and ns[3] == "ok":
        refs.append(("Newton-Schulz model", ns[0], ns[1], None))
    else:
        refs.append(("fp64 Jacobi",) + eigen_yardstick(case, ridge, scaled))
    return refs


def e_ref(refs, metric, slot):
    """The larger error of the references: metric(X) over X = entry `slot` (1 root, 2 inv_root, 3 evals) of every reference that has it."""
    return max(float(metric(r[slot])) for r in refs if r[slot] is not None)


TRUTH_CASES = [((R.wishart, 130), 1e-5), ((R.rank_deficient, 130), 1e-5), ((R.rank_deficient, 200), 1e-5), ((R.graded, 130, 2), 1e-5)]
EXACT_KINDS = ("distinct", "indefinite", "rank_one")
EXACT_RIDGE = 1e-4
RESIDUAL_SIZES = (1, 2, 127, 128, 129, 257, 384)
GATE_CASE = (R.rank_deficient, 130)
GATE_RIDGES = (1e-12, 5e-13, 0.0)


def case_matrix(case):
    A = case[0](*case[1:])
    return A[0] if isinstance(A, tuple) else A


def case_name(case):
    return "-".join([case[0].__name__] + [str(a) for a in case[1:]])
