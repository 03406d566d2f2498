"""Extended-precision host reference of the Cholesky family (potrf / potrs / diag of the inverse / Nystrom solve), plain and slow:
every routine is a row or column loop of a few vectorised lines in np.longdouble (x87 80-bit: 64-bit mantissa), not a blocked
algorithm.  About 0.05 s for a factorisation and 0.1 s for a triangular inverse at n = 385, 1.2 s and 3.7 s at n = 1100 (cubic), so
full references are for n <= ~700; larger matrices are checked through `residual` on sampled entries and `refine_solve`.

The lower triangle of a symmetric input is authoritative everywhere; nothing above the diagonal is read."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, \
    "tests/chol_ref.py needs an extended-precision np.longdouble (eps <= 2^-63); this platform's is %r" % np.finfo(LD).eps


def spd_matrix(n, p, g=0.0, seed=0):
    """Q diag(logspace(0, -p)) Q^T (Q from the QR of a seeded Gaussian matrix), symmetrised, optionally graded: entry (i, j)
    times d_i d_j with d = logspace(0, -g) in random order.  fp64 torch tensor; condition ~10^p before the grading, whose
    diagonal then spans 10^(2g) -- a check relative to the largest entry sees nothing of the small rows."""
    import torch
    gen = torch.Generator().manual_seed(1000003 * seed + n)
    Q, _ = torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=torch.float64))
    A = (Q * torch.logspace(0, -p, n, dtype=torch.float64)) @ Q.T
    if g:
        d = torch.logspace(0, -g, n, dtype=torch.float64)[torch.randperm(n, generator=gen)]
        A = A * d[:, None] * d[None, :]
    A = torch.tril(A)
    return A + torch.tril(A, -1).T


def ld(a):
    """Exact widening of a torch / numpy fp64 (or narrower) array to long double."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(LD)


def cholesky(A):
    """Lower factor of the SPD matrix whose lower triangle is A's, column by column.  Raises LinAlgError naming the order of the
    first leading minor that is not positive definite."""
    L = np.tril(ld(A))
    n = L.shape[0]
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        d = L[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError("the leading minor of order %d is not positive-definite" % (j + 1))
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] /= L[j, j]
    return L


def solve_lower(L, B):
    """Y with L Y = B (forward substitution), B [n, nrhs]."""
    Y = ld(B).copy()
    for i in range(L.shape[0]):
        if i:
            Y[i] -= L[i, :i] @ Y[:i]
        Y[i] /= L[i, i]
    return Y


def solve_lower_t(L, Y):
    """X with L^T X = Y (backward substitution)."""
    X = ld(Y).copy()
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        if i + 1 < n:
            X[i] -= L[i + 1:, i] @ X[i + 1:]
        X[i] /= L[i, i]
    return X


def cholesky_solve(L, B):
    """(L L^T)^-1 B."""
    return solve_lower_t(L, solve_lower(L, B))


def tri_inverse(L):
    """inv(L), lower triangular, row by row: X[i, :i] = -(L[i, :i] X[:i, :i]) / l_ii."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = 1 / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) * X[i, i]
    return X


def inverse_diag(X):
    """diag((L L^T)^-1) from X = inv(L): the squared column norms of X."""
    return (X * X).sum(axis=0)


def nystrom(C, idx, W_d, eps):
    """(C[idx, idx] + eps I)^-1 C[idx, :] W_d^T -> [r, d].  The ridge is added in fp64, as the kernel adds it (one rounding of
    c_ii + eps), so both factorise the same matrix."""
    C64 = np.asarray(C.detach().cpu().numpy() if hasattr(C, "detach") else C, dtype=np.float64)
    idx = np.asarray(idx)
    Ckk = C64[np.ix_(idx, idx)].copy()
    Ckk[np.diag_indices_from(Ckk)] += np.float64(eps)
    cross = ld(C64[idx, :]) @ ld(W_d).T
    return cholesky_solve(cholesky(Ckk), cross)


def residual(A, L, pairs=None, chunk=2048):
    """A_ij - sum_k L_ik L_jk in long double (L: the factor under test, widened exactly; only its lower triangle is read).
    pairs=None: the full lower triangle as an [n, n] array (zeros above the diagonal).  pairs=(i, j) index arrays with
    j <= i: those entries only, as gathered dot products in chunks of `chunk` pairs (sorted by column so that a chunk's
    products stop at its largest column)."""
    A, L = ld(A), np.tril(ld(L))
    n = L.shape[0]
    if pairs is None:
        R = np.zeros((n, n), dtype=LD)
        for i in range(n):
            R[i, :i + 1] = A[i, :i + 1] - L[:i + 1, :i + 1] @ L[i, :i + 1]
        return R
    i, j = (np.asarray(p, dtype=np.int64) for p in pairs)
    assert (j <= i).all()
    out = np.empty(i.shape[0], dtype=LD)
    order = np.argsort(j, kind="stable")
    for s in range(0, order.shape[0], chunk):
        sel = order[s:s + chunk]
        k = int(j[sel].max()) + 1                     # l_jk = 0 for k > j
        out[sel] = A[i[sel], j[sel]] - (L[i[sel], :k] * L[j[sel], :k]).sum(axis=1)
    return out


def refine_solve(A, B, steps=2):
    """A^-1 B for a symmetric positive definite fp64 A too large for `cholesky`: the fp64 LAPACK solve, then `steps` of
    iterative refinement with the residual B - A x taken in long double and the solution kept in long double.  Each step
    multiplies the error by ~cond(A) n 2^-53; the result is good to ~cond(A) 2^-64."""
    import torch
    A64 = np.asarray(A, dtype=np.float64)
    A64 = np.tril(A64) + np.tril(A64, -1).T
    Lt = torch.linalg.cholesky(torch.from_numpy(A64))
    solve = lambda R: torch.cholesky_solve(torch.from_numpy(np.ascontiguousarray(R.astype(np.float64))), Lt).numpy()
    Al, Bl = ld(A64), ld(B)
    X = ld(solve(Bl))
    for _ in range(steps):
        X = X + ld(solve(Bl - Al @ X))
    return X
