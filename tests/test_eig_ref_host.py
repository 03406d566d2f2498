"""tests/eig_ref.py against what is known exactly (no GPU): the long-double Jacobi reproduces the Hadamard spectra, the fp64 run of
the device's arithmetic converges on every matrix the GPU tests use within the device's 40 sweeps, and the model of the
device's final ranking is a permutation for every input.

Eigenvalues are held to 2^-60 relative to max |lambda|.  An eigenvector is determined by the matrix only up to
(backward error) x max |lambda| / gap, so its entries are held to 2^-60 max |lambda| / (smallest gap of the spectrum): 64 x 2^-60 for
the spectrum 64 .. 1 (measured 1.4 x 2^-60), and a cluster's projector, whose gap to the other clusters is 1 of lambda_max = 3, to
3 x 2^-60."""
import numpy as np
import pytest

from tests import eig_ref as R

TRUTH = 2.0 ** -60
SIZES = (16, 64)


@pytest.mark.parametrize("kind", R.EXACT_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_long_double_reproduces_exact_spectra(n, kind):
    A, lam, H = R.exact_spectrum(n, kind)
    _, (got, V, sweeps), _ = R.reference(R.exact_spectrum, n, kind)
    assert sweeps <= R.MAX_SWEEPS
    lmax = np.abs(lam).max()
    e_val = float(np.abs(got - R.ld(lam)).max() / lmax)
    print(f"n={n} {kind}: sweeps {sweeps}, eigenvalues {e_val / TRUTH:.2f} x 2^-60")
    assert e_val <= TRUTH
    Hl = R.ld(H)
    for value, sl in R.clusters_of(lam):
        others = np.abs(lam[lam != value] - value)
        gap = others.min() if others.size else lmax
        if sl.stop - sl.start == 1:
            e = float(np.abs(R.fix_signs(V[:, sl], Hl[:, sl]) - Hl[:, sl]).max())
        else:                                           # only the invariant subspace is determined
            e = float(np.abs(V[:, sl] @ V[:, sl].T - Hl[:, sl] @ Hl[:, sl].T).max())
        assert e <= TRUTH * lmax / gap, f"eigenvalue {value}: vectors off by {e / TRUTH:.2f} x 2^-60, gap {gap}"


BUILDERS = [(R.wishart, (n,)) for n in (2, 6, 16, 62, 64, 96, 126, 128)] + \
           [(R.rank_deficient, (n,)) for n in (2, 6, 16, 62, 64, 96, 126, 128)] + \
           [(R.zero_diagonal, (n,)) for n in (2, 6, 16, 62, 64)] + \
           [(R.graded, (64, g)) for g in (8, 16, 30)] + [(R.graded, (128, 12))] + \
           [(R.exact_spectrum, (n, kind)) for n in SIZES for kind in R.EXACT_KINDS]


@pytest.mark.parametrize("builder,args", BUILDERS, ids=lambda v: v.__name__ if callable(v) else "-".join(map(str, v)))
def test_fp64_run_converges_within_the_device_limit(builder, args):
    """The device's arithmetic in fp64 on the CPU: convergence inside 40 sweeps on every builder (the GPU tests share these
    references through the cache), and the long-double run agrees with it to fp64 accuracy."""
    A, (lam, V, sw), (lam64, V64, sw64) = R.reference(builder, *args)
    n = A.shape[0]
    print(f"{builder.__name__}{args}: sweeps {sw64} (fp64) / {sw} (long double)")
    assert sw64 <= R.MAX_SWEEPS and sw <= R.MAX_SWEEPS
    scale = max(float(np.abs(lam).max()), np.finfo(np.float64).tiny)
    assert float(np.abs(R.ld(lam64) - lam).max()) <= 64 * n * 2.0 ** -52 * scale
    assert float(np.abs(R.ld(V64).T @ R.ld(V64) - np.eye(n)).max()) <= 64 * n * 2.0 ** -52
    assert float(np.abs(V.T @ V - np.eye(n)).max()) <= 64 * n * 2.0 ** -63


def test_scaled_input_converges_without_overflow():
    """A 2^520: the product a_pp a_qq overflows, sqrt|a_pp| sqrt|a_qq| does not; same sweeps, eigenvalues scaled exactly."""
    A = R.wishart(16)
    lam, V, sw = R.jacobi_eigh(A, np.float64)
    for k in (520, -520):
        lam_k, V_k, sw_k = R.jacobi_eigh(np.ldexp(A, k), np.float64)
        assert sw_k == sw and (lam_k == np.ldexp(lam, k)).all() and (V_k == V).all()


NAN, INF = float("nan"), float("inf")
RANK_CASES = [
    [3.0, 1.0, 2.0],
    [1.0, NAN, -0.0, 0.0, INF, -INF, 1.0, NAN],
    [NAN] * 6,
    [0.0, -0.0, 0.0, -0.0],
    [INF, INF, -INF, NAN, -INF],
    [2.0] * 5,
    [NAN, 1.0],
    [1.0, NAN],
]


@pytest.mark.parametrize("diag", RANK_CASES)
def test_rank_descending_is_a_permutation(diag):
    order = R.rank_descending(diag)
    assert sorted(order.tolist()) == list(range(len(diag)))
    d = np.asarray(diag)[order]
    nan = np.isnan(d)
    k = int(nan.sum())
    assert nan[:k].all() and not nan[k:].any()                          # NaN first
    assert (d[k:-1] >= d[k + 1:]).all()                                 # then descending
    for a, b in zip(range(len(d) - 1), range(1, len(d))):               # ties (NaN with NaN, -0 with 0) keep index order
        if (nan[a] and nan[b]) or d[a] == d[b]:
            assert order[a] < order[b]


def test_rank_descending_known_order_and_random_mixes():
    assert R.rank_descending([1.0, NAN, -0.0, 0.0, INF, -INF, 1.0, NAN]).tolist() == [1, 7, 4, 0, 6, 2, 3, 5]
    rng = np.random.default_rng(5)
    pool = np.array([NAN, INF, -INF, 0.0, -0.0, 1.0, 1.0, -2.5, 7.0])
    for _ in range(200):
        d = rng.choice(pool, size=int(rng.integers(1, 33)))
        assert sorted(R.rank_descending(d).tolist()) == list(range(d.shape[0]))
