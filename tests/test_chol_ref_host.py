"""The extended-precision Cholesky reference (tests/chol_ref.py) checked on the host: against LAPACK on a well-conditioned matrix,
and against its own backward-error bound on an ill-conditioned one.  No GPU."""
import numpy as np
import pytest
import torch

from tests import chol_ref as R

U = 2.0 ** -53


@pytest.fixture(scope="module")
def well():
    n = 150
    A = R.spd_matrix(n, 1.0, seed=1)                           # condition 10
    L = R.cholesky(A)
    return n, A, L


def test_long_double_is_extended():
    assert np.finfo(R.LD).eps <= 2.0 ** -63


def test_factor_against_lapack(well):
    n, A, L = well
    Lt = torch.linalg.cholesky(A).numpy()
    assert np.array_equal(np.triu(L, 1), np.zeros((n, n)))
    # forward error of LAPACK's factor: cond * n u at the most; a few ulp of the entries' scale sqrt(a_ii) here
    err = np.abs(L - R.ld(Lt)) / np.sqrt(R.ld(A).diagonal())[:, None]
    assert float(err.max()) < 16 * U, float(err.max() / U)


def test_solve_against_lapack(well):
    n, A, L = well
    B = torch.randn(n, 7, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    X = R.cholesky_solve(L, B)
    Xt = torch.cholesky_solve(B, torch.linalg.cholesky(A)).numpy()
    err = np.abs(X - R.ld(Xt)).max(axis=0) / np.abs(X).max(axis=0)
    assert float(err.max()) < 10 * 16 * U, float(err.max() / U)             # cond(A) = 10
    # the reference's own residual, in long double: B - A X at the level of 2^-64, far under what fp64 can hold
    res = np.abs(R.ld(B) - R.ld(A) @ X).max() / (np.abs(R.ld(A)).sum(axis=1).max() * np.abs(X).max())
    assert float(res) < n * 2.0 ** -62
    # and the two substitutions separately
    Y = R.solve_lower(L, B)
    assert float(np.abs(L @ Y - R.ld(B)).max()) < n * 2.0 ** -62 * float(np.abs(Y).max())
    Z = R.solve_lower_t(L, Y)
    assert float(np.abs(L.T @ Z - Y).max()) < n * 2.0 ** -62 * float(np.abs(Z).max())


def test_inverse_against_lapack(well):
    n, A, L = well
    X = R.tri_inverse(L)
    assert float(np.abs(X @ L - np.eye(n, dtype=R.LD)).max()) < n * 2.0 ** -62
    s = R.inverse_diag(X)
    st = torch.linalg.inv(A).diagonal().numpy()
    assert float((np.abs(s - R.ld(st)) / s).max()) < 10 * 16 * U
    Lt = torch.linalg.cholesky(A)
    Xt = torch.linalg.inv(Lt).numpy()
    assert float(np.abs(X - R.ld(Xt)).max() / np.abs(X).max()) < 10 * 16 * U


def test_nystrom_against_lapack():
    gen = torch.Generator().manual_seed(3)
    n, r, d = 90, 31, 5
    H = torch.randn(4 * n, n, generator=gen, dtype=torch.float64)
    C = H.T @ H / (4 * n)
    W = torch.randn(d, n, generator=gen, dtype=torch.float64)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values
    got = R.nystrom(C, idx.numpy(), W, 1e-6)
    Ckk = C[idx][:, idx] + 1e-6 * torch.eye(r, dtype=torch.float64)
    want = torch.cholesky_solve(C[idx, :] @ W.T, torch.linalg.cholesky(Ckk)).numpy()
    assert got.shape == (r, d)
    assert float((np.abs(got - R.ld(want)).max(axis=0) / np.abs(got).max(axis=0)).max()) < 1e-12


@pytest.mark.parametrize("n,p,g", [(200, 10.0, 0.0), (200, 10.0, 2.0)])
def test_own_residual_on_condition_1e10(n, p, g):
    """|A - L L^T|_ij <= n 2^-64 sqrt(a_ii a_jj) for the reference's own factor (Higham Thm 10.3 at u = 2^-64), evaluated by
    the residual helper -- full, and through the sampled-pairs path, which must agree with it."""
    A = R.spd_matrix(n, p, g, seed=4)
    L = R.cholesky(A)
    res = R.residual(A, L)
    dg = np.sqrt(R.ld(A).diagonal())
    assert float((np.abs(res) / (dg[:, None] * dg[None, :])).max()) <= n * 2.0 ** -64
    rng = np.random.default_rng(5)
    i = rng.integers(0, n, 500)
    j = rng.integers(0, n, 500)
    i, j = np.maximum(i, j), np.minimum(i, j)
    sampled = R.residual(A, L, (i, j), chunk=64)
    assert bool((np.abs(sampled - res[i, j]) <= n * 2.0 ** -64 * dg[i] * dg[j]).all())   # two summation orders of n terms
    # an fp64 factor shows up at the fp64 level: the helper resolves what it is for
    res64 = R.residual(A, torch.linalg.cholesky(A).numpy())
    worst = float((np.abs(res64) / (dg[:, None] * dg[None, :])).max())
    assert 2.0 ** -58 < worst <= (n + 1) * U


def test_not_positive_definite_names_the_order():
    A = torch.eye(40, dtype=torch.float64)
    A[17, 17] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="order 18 "):
        R.cholesky(A)


def test_refine_solve_reaches_the_long_double_solution(well):
    n, A, L = well
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    X = R.cholesky_solve(L, B)
    Xr = R.refine_solve(A.numpy(), B.numpy())
    assert float(np.abs(X - Xr).max() / np.abs(X).max()) < 10 * n * 2.0 ** -63
