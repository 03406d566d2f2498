"""Host reference of the batched Jacobi eigensolver (mdg_syevj_batched): a plain two-sided cyclic Jacobi in numpy, written once
with the dtype as a parameter.  Run in np.longdouble (x87 80-bit: 64-bit mantissa) it is the truth the device is measured against;
run in np.float64 it is the yardstick -- what this algorithm achieves in working precision on the CPU -- from which every
tolerance of tests/test_gpu_eigh.py is taken.  Also the Python model of the kernel's final ranking (`rank_descending`) and the
seeded matrices the tests share.

The rotation test is the kernel's, |a_pq| > eps sqrt|a_pp| sqrt|a_qq| with eps the dtype's, relative to the pair's own diagonal:
what gives a graded positive definite matrix every eigenvalue to high relative accuracy (Demmel & Veselic, Jacobi's method is
more accurate than QR, SIAM J. Matrix Anal. Appl. 13, 1992).  The pair order is the round-robin tournament: n - 1 rounds of n / 2
disjoint pairs, one round's rotations applied together (they commute: disjoint index pairs).

The routine is written once; its parameters are the dtype and how a rotation is applied (`update`): the device's expression, for
the fp64 yardstick, or Rutishauser's, whose error is small enough in long double to serve as the truth (jacobi_eigh).

About 0.1 s for a long-double decomposition at n = 64 and 1 - 3 s at n = 128: tests at n = 128 use a handful of matrices.
Only the lower triangle of an input is read, as on the device."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, \
    "tests/eig_ref.py needs an extended-precision np.longdouble (eps <= 2^-63); this platform's is %r" % np.finfo(LD).eps
MAX_SWEEPS = 40          # the device's limit (eigh.hip syevj_batched)


def ld(a):
    """Exact widening of a torch / numpy fp64 (or narrower) array to long double."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(LD)


def sym_lower(A):
    """The symmetric matrix whose lower triangle is A's."""
    S = np.array(A)
    upper = np.triu_indices(S.shape[0], 1)
    S[upper] = S.T[upper]                                             # (copied, not added: a -0.0 on the diagonal stays -0.0)
    return S


# ---------------------------------------------------------------- the ranking rule
def rank_descending(diag):
    """order with order[pos] = index of the entry at descending position pos, by the device's rule: NaN before everything else,
    then by value, ties by index; -0.0 == 0.0 is a tie.  A total order for every bit pattern, so `order` is a permutation."""
    d = np.asarray(diag, dtype=np.float64)
    n = d.shape[0]
    k, i = np.arange(n)[:, None], np.arange(n)[None, :]
    on, mn = np.isnan(d)[:, None], np.isnan(d)[None, :]
    with np.errstate(invalid="ignore"):
        finite_rule = (d[:, None] > d[None, :]) | ((d[:, None] == d[None, :]) & (k < i))
    ahead = np.where(on | mn, on & (~mn | (k < i)), finite_rule)      # ahead[k, i]: entry k stands before entry i
    pos = ahead.sum(axis=0)
    order = np.full(n, -1, dtype=np.int64)
    order[pos] = np.arange(n)
    return order


# ---------------------------------------------------------------- Jacobi
def round_robin(n):
    """The n - 1 rounds of the tournament on n (even) players as (P, Q) index arrays of n / 2 disjoint pairs each; every pair
    meets once per sweep.  Player n - 1 stays, the others move round a circle of n - 1 seats."""
    assert n >= 2 and n % 2 == 0, "round_robin: n must be even"
    t = np.arange(1, n // 2)
    rounds = []
    for r in range(n - 1):
        P = np.concatenate(([n - 1], (r + t) % (n - 1)))
        Q = np.concatenate(([r], (r - t) % (n - 1)))
        rounds.append((P, Q))
    return rounds


def jacobi_eigh(A, dtype=LD, update="device", max_sweeps=MAX_SWEEPS, sort=True):
    """(evals descending [n], evecs [n, n] with eigenvector j in column j, sweeps) of the symmetric matrix whose lower triangle is
    A's (n even), every operation in `dtype`.  sweeps counts the last, rotation-free sweep too, as the device does; it is
    max_sweeps + 1 when that many sweeps did not converge.
    update: how a rotation (c, s) = (cos, sin) is applied to a pair of rows / columns (x, y) -- the same rotation either way:
      "device"       x' = c x - s y, y' = s x + c y, the diagonal like every other entry: the kernel's arithmetic.
      "rutishauser"  x' = x - s (y + h x), y' = y + s (x - h y), h = s / (1 + c), a_pp -= t a_pq, a_qq += t a_pq (Rutishauser 1966,
                     Handbook for Automatic Computation II/1): the rounding error of a rotation is proportional to s, not to 1,
                     so the many small rotations of the late sweeps cost nothing.  Measured on the exact Hadamard spectra at
                     n = 64 in long double: eigenvalues 0.4 - 0.6 x 2^-60 of lambda_max, against 3.5 - 11 x 2^-60 for "device"."""
    assert update in ("device", "rutishauser")
    eps = dtype(np.finfo(dtype).eps)
    a = sym_lower(np.asarray(A).astype(dtype))
    n = a.shape[0]
    V = np.eye(n, dtype=dtype)
    rounds = round_robin(n)
    zero, one, two = dtype(0), dtype(1), dtype(2)
    sweeps, converged = 0, False
    while sweeps < max_sweeps and not converged:
        sweeps += 1
        rotated = False
        for P, Q in rounds:
            app, aqq, apq = a[P, P], a[Q, Q], a[P, Q]
            rot = np.abs(apq) > eps * np.sqrt(np.abs(app)) * np.sqrt(np.abs(aqq))
            if not rot.any():
                continue
            rotated = True
            with np.errstate(over="ignore", invalid="ignore"):        # (the lanes of pairs that do not rotate are discarded)
                tau = (aqq - app) / (two * np.where(rot, apq, one))
                t = np.where(rot, np.where(tau >= 0, one, -one) / (np.abs(tau) + np.sqrt(one + tau * tau)), zero)
            c = one / np.sqrt(one + t * t)
            s = t * c
            cc, sc = c[:, None], s[:, None]
            if update == "device":
                x, y = a[:, P], a[:, Q]                               # A <- A J (columns)
                a[:, P], a[:, Q] = c * x - s * y, s * x + c * y
                x, y = a[P, :], a[Q, :]                               # A <- J^T A (rows)
                a[P, :], a[Q, :] = cc * x - sc * y, sc * x + cc * y
                x, y = V[:, P], V[:, Q]                               # V <- V J
                V[:, P], V[:, Q] = c * x - s * y, s * x + c * y
            else:
                h = s / (one + c)
                hc = h[:, None]
                x, y = a[:, P], a[:, Q]
                a[:, P], a[:, Q] = x - s * (y + h * x), y + s * (x - h * y)
                x, y = a[P, :], a[Q, :]
                a[P, :], a[Q, :] = x - sc * (y + hc * x), y + sc * (x - hc * y)
                x, y = V[:, P], V[:, Q]
                V[:, P], V[:, Q] = x - s * (y + h * x), y + s * (x - h * y)
                a[P, P], a[Q, Q] = app - t * apq, aqq + t * apq
            a[P[rot], Q[rot]] = 0
            a[Q[rot], P[rot]] = 0
        converged = not rotated
    if not converged:
        sweeps = max_sweeps + 1
    lam = np.diagonal(a).copy()
    if sort:
        order = np.argsort(-lam, kind="stable")                       # (finite: descending, ties by index)
        lam, V = lam[order], V[:, order]
    return lam, V, sweeps


@functools.lru_cache(maxsize=None)
def reference(builder, *args):
    """(A, truth, yardstick) of A = builder(*args) (its first element when the builder returns a tuple), each (lam, V, sweeps):
    truth = long double with Rutishauser's update, yardstick = fp64 with the device's arithmetic -- what the kernel's algorithm
    achieves in working precision on the CPU.  Computed once per process, read-only."""
    A = builder(*args)
    A = A[0] if isinstance(A, tuple) else A
    lam, V, sw = jacobi_eigh(A, LD, "rutishauser")
    lam64, V64, sw64 = jacobi_eigh(A, np.float64, "device")
    for x in (A, lam, V, lam64, V64):
        x.setflags(write=False)
    return A, (lam, V, sw), (lam64, V64, sw64)


def fix_signs(V, V_ref):
    """V with every column's sign chosen so that it agrees with V_ref's column (by the sign of their inner product)."""
    V = ld(V)
    sgn = np.sign((V * V_ref).sum(axis=0))
    sgn[sgn == 0] = 1
    return V * sgn


# ---------------------------------------------------------------- matrices (all seeded, fp64 numpy, symmetric)
def _gen(seed, n):
    return np.random.default_rng(1000003 * seed + n)


def wishart(n, seed=0):
    """X^T X / t with t = 3 n Gaussian tokens: well conditioned, full rank."""
    X = _gen(seed, n).standard_normal((3 * n, n))
    return sym_lower(X.T @ X / (3 * n))


def rank_deficient(n, seed=1):
    """A Gram matrix with tokens = n / 2: half the spectrum is zero up to rounding."""
    t = max(n // 2, 1)
    X = _gen(seed, n).standard_normal((t, n))
    return sym_lower(X.T @ X / t)


def zero_diagonal(n, seed=2):
    """(P + P^T) / 2 of a random permutation matrix with the diagonal removed: every a_pp is 0, so the rotation threshold is 0 and
    the first rotations are by 45 degrees (tau = 0); indefinite, with repeated eigenvalues."""
    P = np.eye(n)[_gen(seed, n).permutation(n)]
    A = (P + P.T) / 2
    np.fill_diagonal(A, 0.0)
    if not A.any():                                                   # (the identity permutation: nothing left)
        A = np.eye(n)[::-1].copy() / 2
        np.fill_diagonal(A, 0.0)
    return A


def well_conditioned(n, cond=4.0, seed=3):
    """B = Q diag(linspace(1, cond)) Q^T with Q from the QR of a Gaussian matrix: cond(B) = cond."""
    Q, _ = np.linalg.qr(_gen(seed, n).standard_normal((n, n)))
    return sym_lower((Q * np.linspace(1.0, cond, n)) @ Q.T)


GRADED_COND = 4.0


def graded(n, g, seed=3):
    """D B D with D = diag(logspace(0, -g)) and cond(B) = 4: cond(A) ~ 10^(2 g), yet every eigenvalue and eigenvector is determined
    to a relative accuracy of order cond(B) by the entries (Demmel & Veselic)."""
    d = np.logspace(0.0, -float(g), n)
    return sym_lower(well_conditioned(n, GRADED_COND, seed) * d[:, None] * d[None, :])


def hadamard(n):
    """The Sylvester Hadamard matrix over sqrt(n), n a power of 4: orthogonal, entries +-1/sqrt(n) exactly representable."""
    r = int(round(np.sqrt(n)))
    assert r * r == n and n & (n - 1) == 0, "hadamard: n must be a power of 4"
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H / r


EXACT_KINDS = ("distinct", "clusters", "indefinite", "rank_one")


def exact_spectrum(n, kind, seed=4):
    """(A, lam, H): A = H diag(lam) H^T EXACTLY in fp64 (lam: small integers or half-integers, H's entries +-1/sqrt(n), every partial
    sum a small multiple of 1/(2n)), lam descending, H's columns permuted (seeded) so that column j belongs to lam[j].
      distinct    n, n-1, .., 1
      clusters    3, 2, 1 in 20 / 22 / 22 copies at n = 64 (5 / 5 / 6 at n = 16): only each cluster's projector is determined
      indefinite  n/2 - 1/2, .., -n/2 + 1/2  (distinct half-integers, none zero)
      rank_one    3, 0, .., 0"""
    if kind == "distinct":
        lam = np.arange(n, 0, -1, dtype=np.float64)
    elif kind == "clusters":
        sizes = {64: (20, 22, 22), 16: (5, 5, 6)}[n]
        lam = np.repeat([3.0, 2.0, 1.0], sizes)
    elif kind == "indefinite":
        lam = np.arange(n - 1, -1, -1, dtype=np.float64) - n / 2 + 0.5
    elif kind == "rank_one":
        lam = np.zeros(n)
        lam[0] = 3.0
    else:
        raise ValueError(kind)
    H = hadamard(n)[:, _gen(seed, n).permutation(n)]
    A = (H * lam) @ H.T
    A_exact = (ld(H) * ld(lam)) @ ld(H).T
    assert (ld(A) == A_exact).all() and (A == A.T).all(), "exact_spectrum: A is not exact in fp64"
    return A, lam, H


def clusters_of(lam):
    """[(value, slice)] of the runs of equal entries of a descending spectrum."""
    out, start = [], 0
    for j in range(1, len(lam) + 1):
        if j == len(lam) or lam[j] != lam[start]:
            out.append((lam[start], slice(start, j)))
            start = j
    return out


def sqrt_psd(lam, V, ridge, scaled):
    """(root, inv_root) = V f(lam) V^T with the reference's clamps (compression_utils.py sqrt_M): f = sqrt(max(lam + ridge * scale,
    0)), g = 1 / max(f, 1e-12), scale = lam_max if scaled else 1; in the dtype of lam / V."""
    dt = lam.dtype.type
    scale = lam.max() if scaled else dt(1)
    f = np.sqrt(np.maximum(lam + dt(ridge) * scale, dt(0)))
    g = dt(1) / np.maximum(f, dt(1e-12))
    return (V * f) @ V.T, (V * g) @ V.T
