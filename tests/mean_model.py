"""Long double host model of the mean-aware MLP refit ("The MLP intercept"): column sums, the centred
statistic S = C - mu mu^T, the refit D = W_d S[:,k] (S_kk + eps I)^-1, the intercept b' = b_d + W_d mu - D^ mu_k of a STORED tensor
D^, the two norms the kernel reports, and the a priori bounds the GPU tests hold the kernels to.  Plain numpy in np.longdouble
(64-bit mantissa) on top of tests/chol_ref.py; nothing here touches a GPU."""
import numpy as np

from tests import chol_ref as R

LD = R.LD
U = 2.0 ** -53


def ld(a):
    return R.ld(a)


def bf16_round(a):
    """fp64 -> fp32 -> bf16 (round to nearest even twice, as torch's .to(bfloat16) does), returned as fp64."""
    f = np.asarray(a, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(f.shape)


def col_sums(x, relu=False):
    """sum_t f(x[t, :]) in long double; f = max(., 0) with relu."""
    x = ld(x)
    if relu:
        x = np.where(x > 0, x, np.where(np.isnan(x), x, LD(0)))
    return x.sum(axis=0)


def center(C, mu):
    """S = C - mu mu^T in long double."""
    mu = ld(mu)
    return ld(C) - np.outer(mu, mu)


def refit(S, idx, W_d, eps):
    """D [d, r] = W_d S[:, k] (S_kk + eps I)^-1 with the ridge added in fp64 to the fp64 S the kernel factorises (chol_ref.nystrom)."""
    return R.nystrom(np.asarray(S, dtype=np.float64), idx, W_d, eps).T


def delta(W_d, D_hat, idx, mu):
    """(delta, W_d mu): delta = W_d mu - D^ mu_k."""
    mu = ld(mu)
    wmu = ld(W_d) @ mu
    return wmu - ld(D_hat) @ mu[np.asarray(idx)], wmu


def intercept(W_d, D_hat, idx, mu, b_d=None):
    """(b', ||delta||^2, ||W_d mu||^2): b' = b_d + delta for the tensor D^ that is stored."""
    dl, wmu = delta(W_d, D_hat, idx, mu)
    b = dl if b_d is None else ld(b_d) + dl
    return b, (dl * dl).sum(), (wmu * wmu).sum()


def bias_bound(W_d, D_hat, idx, mu, b_d=None):
    """Entry-wise bound of bias_f64: (n + r + 2) 2^-53 (|b_i| + sum_j |W_ij mu_j| + sum_p |D^_ip mu_k(p)|) -- n + r exact products
    added in any order, one subtraction, one addition of b_d."""
    mu = np.abs(ld(mu))
    n, r = np.shape(W_d)[1], np.shape(D_hat)[1]
    mag = np.abs(ld(W_d)) @ mu + np.abs(ld(D_hat)) @ mu[np.asarray(idx)]
    if b_d is not None:
        mag = mag + np.abs(ld(b_d))
    return (n + r + 2) * LD(U) * mag


def norm_terms(W_d, D_hat, idx, mu):
    """The sums of absolute terms the two norms are accurate against: sum_i (sum |terms of delta_i|)^2 and sum_i (sum_j |W_ij mu_j|)^2."""
    mu = np.abs(ld(mu))
    a = np.abs(ld(W_d)) @ mu
    b = np.abs(ld(D_hat)) @ mu[np.asarray(idx)]
    return ((a + b) ** 2).sum(), (a ** 2).sum()


def augmented_fit(C, mu, idx, W_d, eps, b_d=None):
    """The least-squares fit of W_d h + b_d on the augmented feature [h_k; 1] from the moments, ridge eps on D only:
        [ C_kk + eps I   mu_k ] [ D^T  ]   [ C[k, :] W_d^T + mu_k b_d^T ]
        [ mu_k^T          1   ] [ b'^T ] = [ mu^T W_d^T + b_d^T         ]
    solved in long double.  Returns (D [d, r], b' [d])."""
    idx = np.asarray(idx)
    C, mu, W = ld(C), ld(mu), ld(W_d)
    d = W.shape[0]
    b = np.zeros(d, dtype=LD) if b_d is None else ld(b_d)
    r = len(idx)
    A = np.zeros((r + 1, r + 1), dtype=LD)
    A[:r, :r] = C[np.ix_(idx, idx)] + LD(eps) * np.eye(r, dtype=LD)
    A[r, :r] = mu[idx]
    A[:r, r] = mu[idx]
    A[r, r] = 1
    rhs = np.zeros((r + 1, d), dtype=LD)
    rhs[:r] = C[idx, :] @ W.T + np.outer(mu[idx], b)
    rhs[r] = W @ mu + b
    # A is symmetric indefinite-looking but positive definite exactly when S_kk + eps I is (its Schur complement); eliminate the last
    # row by hand so that the Cholesky factor is that of the Schur complement
    Skk = A[:r, :r] - np.outer(mu[idx], mu[idx])
    L = _chol_ld(Skk)
    D_T = R.cholesky_solve(L, rhs[:r] - np.outer(mu[idx], rhs[r]))
    bp = rhs[r] - mu[idx] @ D_T
    return D_T.T, bp


def _chol_ld(A):
    """chol_ref.cholesky keeps long double input as it is (ld() of a long double array is the array)."""
    return R.cholesky(A)


def centred_fit(C, mu, idx, W_d, eps, b_d=None):
    """The issue's two lines in long double, nothing rounded: D = W_d S[:,k] (S_kk + eps I)^-1, b' = b_d + W_d mu - D mu_k."""
    idx = np.asarray(idx)
    S, W, m = center(C, mu), ld(W_d), ld(mu)
    Skk = S[np.ix_(idx, idx)] + LD(eps) * np.eye(len(idx), dtype=LD)
    D = R.cholesky_solve(_chol_ld(Skk), S[idx, :] @ W.T).T
    bp = W @ m - D @ m[idx]
    return D, bp if b_d is None else bp + ld(b_d)


def residual(W_d, idx, D):
    """u [d, n]: row i = row i of W_d minus row i of D scattered to the columns idx."""
    u = ld(W_d).copy()
    u[:, np.asarray(idx)] -= ld(D)
    return u


def quad(u, M):
    """u_i M u_i^T per row."""
    u = ld(u)
    return ((u @ ld(M)) * u).sum(axis=1)


def token_errors(H, W_d, idx, D, bias=None, b_d=None):
    """From the token matrix itself, in long double: y = W_d h + b_d, y' = D h_k + bias per token.  Returns (mean_t (y - y') [d],
    sum_t ||y - y'||^2)."""
    H = ld(H)
    e = H @ ld(W_d).T - H[:, np.asarray(idx)] @ ld(D).T
    if b_d is not None:
        e = e + ld(b_d)
    if bias is not None:
        e = e - ld(bias)
    return e.mean(axis=0), (e * e).sum()


def cond(A):
    """2-norm condition number of a symmetric positive definite matrix (fp64 eigenvalues are plenty for an assertion)."""
    w = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    return float(w[-1] / w[0])


def lattice_case(d, n, r, seed, repeat=False):
    """Integer data for mdg_nystrom_intercept: W [d, n] and D^ [d, r] in [-8, 8] (exact in bf16), mu [n] in [-16, 16], b_d [d] in
    [-64, 64], idx the first r entries of a random permutation (shuffled: any order must do), with `repeat` five of them (fewer where
    r < 10) overwritten by copies of five others.  Every product and partial sum is a small integer, so any fp64 summation order
    gives the long double model's bits (lattice_is_exact states the conditions)."""
    rng = np.random.default_rng(104729 * seed + 31 * n + r)
    W = rng.integers(-8, 9, size=(d, n)).astype(np.float64)
    D = rng.integers(-8, 9, size=(d, r)).astype(np.float64)
    mu = rng.integers(-16, 17, size=n).astype(np.float64)
    idx = rng.permutation(n)[:r].astype(np.int64)
    if repeat:
        k = min(5, r // 2)
        pos = rng.permutation(r)[:2 * k]
        idx[pos[:k]] = idx[pos[k:]]
    b_d = rng.integers(-64, 65, size=d).astype(np.float64)
    return {"W": W, "D": D, "mu": mu, "idx": idx, "b_d": b_d}


def lattice_is_exact(c):
    """The magnitude conditions under which fp64 evaluates a lattice case without a rounding, in any order: the absolute terms of
    each of a row's two sums add up to less than 2^20 (so every partial sum, delta and b_d + delta are integers below 2^22, their
    squares below 2^44 < 2^53), and each of the two sums of squares -- of the rows' absolute-term sums, which dominate the rows --
    stays below 2^48."""
    mu = np.abs(c["mu"])
    a = np.abs(c["W"]) @ mu
    b = np.abs(c["D"]) @ mu[c["idx"]]
    t_delta, t_wmu = norm_terms(c["W"], c["D"], c["idx"], c["mu"])
    return bool(a.max() < 2 ** 20 and b.max() < 2 ** 20 and np.abs(c["b_d"]).max() <= 64 and t_delta < 2 ** 48 and t_wmu < 2 ** 48)


def intercept_fp64(W_d, D_hat, idx, mu, b_d=None, order="ascending", chunk=2048):
    """The intercept in PLAIN fp64, one addition at a time: `ascending` adds the columns left to right, `chunks_reversed` takes the
    chunks of `chunk` columns last to first (ascending within a chunk, the chunk's sum added to the total).  Returns what
    intercept() returns, as fp64."""
    def dots(A, v):
        A, v = np.asarray(A, dtype=np.float64), np.asarray(v, dtype=np.float64)
        P = A * v[None, :]
        if order == "ascending":
            return np.cumsum(P, axis=1)[:, -1]                 # (cumsum is sequential; np.sum would add pairwise)
        tot = np.zeros(A.shape[0])
        for a0 in reversed(range(0, A.shape[1], chunk)):
            tot = tot + np.cumsum(P[:, a0:a0 + chunk], axis=1)[:, -1]
        return tot
    mu = np.asarray(mu, dtype=np.float64)
    wmu = dots(W_d, mu)
    dl = wmu - dots(D_hat, mu[np.asarray(idx)])
    b = dl if b_d is None else np.asarray(b_d, dtype=np.float64) + dl
    sq = (lambda v: np.cumsum(v * v)[-1]) if order == "ascending" else (lambda v: np.cumsum((v * v)[::-1])[-1])
    return b, sq(dl), sq(wmu)


def generic_case(d, n, r, seed):
    """Generic data for mdg_nystrom_intercept: W and D^ bf16-rounded Gaussians, mu = |Gaussian| times a per-column power of two in
    2^-3 .. 2^3, b_d a bf16-rounded Gaussian, idx shuffled.  The reference is intercept(), the tolerance bias_bound()."""
    rng = np.random.default_rng(15485863 * seed + 31 * n + r)
    W = bf16_round(rng.standard_normal((d, n)))
    D = bf16_round(rng.standard_normal((d, r)))
    mu = np.abs(rng.standard_normal(n)) * 2.0 ** rng.integers(-3, 4, size=n)
    idx = rng.permutation(n)[:r].astype(np.int64)
    b_d = bf16_round(rng.standard_normal(d))
    return {"W": W, "D": D, "mu": mu, "idx": idx, "b_d": b_d}


# the shapes (d, n, r) of tests/test_gpu_intercept_kernel.py: the smallest at which each piece of the kernel's structure can go wrong
# (2048-column LDS chunks, 16-byte vectors of eight, 16 rows per workgroup, 4 per wave, 256 rows per trip of the norms loop)
INTERCEPT_SHAPES = {
    "A": (1, 1, 1),               # one row of a 16-row workgroup, no vector
    "B": (3, 9, 7),               # fewer rows than a wave owns; one vector + tail, tail only
    "C": (17, 2048, 2048),        # exactly one full chunk; r == n; one row into a second workgroup
    "D": (16, 2049, 2047),        # a second chunk of length 1; a chunk one short of full
    "E": (257, 2053, 2049),       # a last chunk of 5 (no vector), of 1; the norms loop's second trip with one row
    "F": (531, 4105, 3891),       # two full chunks + 9; r = 2048 + 1843; ragged workgroup, ragged wave, third norms trip
    "G": (40, 6144, 4096),        # three / two full chunks, nothing ragged
}


def make_case(n, r, d, tokens=512, seed=0):
    """h = |Gaussian| * column scale (every mean of the order of its standard deviation), bf16-valued, [tokens, n]; W_d [d, n]
    bf16-valued; C = H^T H / tokens and mu = mean_t h (exact in fp64 for tokens = 512); a selection idx of r sorted columns.  numpy fp64 arrays."""
    rng = np.random.default_rng(7919 * seed + n)
    scale = 2.0 ** rng.integers(-2, 3, size=n)
    # ... on the grid 2^-12 * scale: at most 2^15 grid units per entry, so the column sums (2^24 units) and the second moments
    # (2^39 units of 2^-24 s_i s_j) of up to 512 tokens are exact in fp64, and with a power-of-two token count so are C and mu
    H = bf16_round(np.abs(rng.standard_normal((tokens, n))) * scale)
    H = bf16_round(np.round(H / scale * 4096.0) / 4096.0 * scale)
    W = bf16_round(rng.standard_normal((d, n)) / np.sqrt(n))
    Hl = ld(H)
    C = (Hl.T @ Hl / LD(tokens)).astype(np.float64)
    C = np.tril(C) + np.tril(C, -1).T
    mu = (Hl.sum(axis=0) / LD(tokens)).astype(np.float64)
    idx = np.sort(rng.permutation(n)[:r]).astype(np.int64)
    b_d = bf16_round(rng.standard_normal(d) * 0.1)
    return {"H": H, "W": W, "C": C, "mu": mu, "idx": idx, "b_d": b_d}
