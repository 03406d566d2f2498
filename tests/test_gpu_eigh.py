"""The batched Jacobi eigensolver (mdg_syevj_batched, and mdg_sqrt_psd_small on top of it) against the extended-precision host
reference tests/eig_ref.py: every size class of the kernel, exact / clustered / indefinite / rank-one spectra, graded matrices,
diagonal input, scaling by 2^k, batch independence, non-finite input and the argument checks.

THE RULE of every accuracy assertion.  truth = eig_ref's long-double run, e64 = the error of eig_ref's fp64 run (the device's
arithmetic on the CPU) against the truth, on the same matrix and in the same metric.  The kernel must stay within

    max(4 e64, n 2^-52 scale)

4 = two bits for FMA contraction and the different association on the device; the floor keeps a lucky small e64 from becoming the
bar (scale: 1 for a metric that is already relative; cond(B) = 4 for the graded matrices D B D, whose eigenvalues and eigenvectors
are determined to n 2^-52 cond(B) at best -- Demmel & Veselic 1992).  Nothing is measured against the kernel itself; every test
prints e64, the kernel's error and their ratio (lines RULE under pytest -s) before it asserts.  DESIGN.md "Eigensolver accuracy"
holds the ratios measured on an MI355X.

MEASURED on an MI355X, kernel error / e64, smallest - largest per family (largest share of the bound):
    sizes and paths   eigenvalues 0.48 - 3.67 (0.69; the 3.67 is the zero-diagonal n = 6 matrix, both errors under the floor, <= 1.49
                      elsewhere)   |V^T V - I| 0.81 - 1.73 (0.43)   |A V - V L| 0.58 - 1.76 (0.44)
    exact spectra     eigenvalues 0.50 - 1.16 (0.29)   eigenvectors 0.74 - 1.56 (0.30)   cluster projectors 0.49 - 1.36 (0.22)
                      rank one: other |lambda| 1.7e-16 (n = 16), 7.1e-16 (n = 64) against floors 1.1e-14, 4.3e-14
    graded            eigenvalues 0.95 - 0.96 (0.24)   eigenvectors 0.97 - 1.01 (0.14)
                      largest relative eigenvalue error, kernel / LAPACK eigvalsh: g = 8: 1.6e-14 / 7.3e-14, g = 16: 1.4e-14 / 1.2e-13,
                      g = 30: 7.2e-15 / 9.7e-13, n = 128 g = 12: 2.7e-14 / 1.6e-13
    sqrt_psd_small    root 0.95 - 1.11 (0.28)   inverse root 0.67 - 1.00 (0.25; 1.1e-11 on the rank-deficient matrix, e64 1.6e-11)
"""
import functools

import numpy as np
import pytest
import torch

from tests import eig_ref as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
U52 = 2.0 ** -52


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def solve(ops, dev, mats):
    """ops.syevj on the batch of numpy matrices -> (evals [b, n], evecs [b, n, n]) as CPU tensors."""
    lam, V = ops.syevj(torch.from_numpy(np.stack(mats)).to(dev))
    return lam.cpu(), V.cpu()


def held(what, err, e64, floor):
    err, e64 = float(err), float(e64)
    bound = max(4 * e64, floor)
    print(f"RULE {what}: e64 {e64:.3e} kernel {err:.3e} ratio {err / e64 if e64 else float('inf'):.2f} "
          f"floor {floor:.3e} -> {err / bound:.3f} of the bound")
    assert err <= bound, f"{what}: kernel error {err:.3e} above max(4 x {e64:.3e}, {floor:.3e})"


# ---------------------------------------------------------------- metrics, all evaluated in long double
def eval_err(lam, truth):
    return np.abs(R.ld(lam) - truth).max() / np.abs(truth).max()


def orth_err(V):
    V = R.ld(V)
    return np.abs(V.T @ V - np.eye(V.shape[0])).max()


def resid_err(A, lam, V, lmax):
    A, lam, V = R.ld(A), R.ld(lam), R.ld(V)
    return np.abs(A @ V - V * lam).max() / lmax


def vec_err(V, truth):
    return np.abs(R.fix_signs(V, truth) - truth).max()


# ---------------------------------------------------------------- 1. sizes and paths
@pytest.mark.parametrize("n", [2, 6, 16, 62, 64, 96, 126, 128])
def test_sizes_and_paths(ops, dev, n):
    """The run-time-n instantiation (2, 6, 16, 62, 96, 126) and the two compile-time ones (64, 128): a Wishart and a rank-deficient
    matrix each, at n <= 64 a zero-diagonal one as the third of the batch.  ops.syevj raises if a matrix hits the sweep limit."""
    builders = [R.wishart, R.rank_deficient] + ([R.zero_diagonal] if n <= 64 else [])
    refs = [R.reference(b, n) for b in builders]
    lam, V = solve(ops, dev, [r[0] for r in refs])
    for k, (b, (A, (tl, tV, _), (l64, V64, _))) in enumerate(zip(builders, refs)):
        lmax = np.abs(tl).max()
        tag = f"{b.__name__} n={n}"
        held(f"{tag} eigenvalues / lambda_max", eval_err(lam[k].numpy(), tl), eval_err(l64, tl), n * U52)
        held(f"{tag} |V^T V - I|", orth_err(V[k].numpy()), orth_err(V64), n * U52)
        held(f"{tag} |A V - V L| / lambda_max", resid_err(A, lam[k].numpy(), V[k].numpy(), lmax), resid_err(A, l64, V64, lmax),
             n * U52)


# ---------------------------------------------------------------- 2. exact spectra
@pytest.mark.parametrize("kind", R.EXACT_KINDS)
@pytest.mark.parametrize("n", [16, 64])
def test_exact_spectra(ops, dev, n, kind):
    A, lam_exact, H = R.exact_spectrum(n, kind)
    _, _, (l64, V64, _) = R.reference(R.exact_spectrum, n, kind)
    lam, V = solve(ops, dev, [A])
    lam, V = lam[0].numpy(), V[0].numpy()
    tl, Hl = R.ld(lam_exact), R.ld(H)
    tag = f"exact {kind} n={n}"
    floor = n * U52
    if kind == "rank_one":
        held(f"{tag} lambda_1", abs(R.ld(lam[:1]) - tl[:1]).max() / tl[0], abs(R.ld(l64[:1]) - tl[:1]).max() / tl[0], floor)
        rest = np.abs(lam[1:]).max()
        print(f"RULE {tag} other |lambda|: kernel {rest:.3e} floor {floor * lam_exact[0]:.3e}")
        assert rest <= floor * lam_exact[0]
        return
    held(f"{tag} eigenvalues / max|lambda|", eval_err(lam, tl), eval_err(l64, tl), floor)
    if kind == "clusters":                                 # inside a cluster only the projector is determined
        for value, sl in R.clusters_of(lam_exact):
            P = Hl[:, sl] @ Hl[:, sl].T
            proj = lambda W: np.abs(R.ld(W[:, sl]) @ R.ld(W[:, sl]).T - P).max()
            held(f"{tag} projector of lambda = {value:g}", proj(V), proj(V64), floor)
    else:
        held(f"{tag} eigenvectors entry-wise", vec_err(V, Hl), vec_err(V64, Hl), floor)


# ---------------------------------------------------------------- 3. graded matrices: what Jacobi is chosen for
@pytest.mark.parametrize("n,g", [(64, 8), (64, 16), (64, 30), (128, 12)])
def test_graded_relative_accuracy(ops, dev, n, g):
    """D B D, D = logspace(0, -g), cond(B) = 4: EVERY eigenvalue to high relative accuracy (its own size is the scale), the
    eigenvectors entry-wise.  An absolute rotation threshold, or LAPACK's tridiagonal route, loses the small ones."""
    A, (tl, tV, _), (l64, V64, _) = R.reference(R.graded, n, g)
    lam, V = solve(ops, dev, [A])
    lam, V = lam[0].numpy(), V[0].numpy()
    rel = lambda l: np.abs((R.ld(l) - tl) / tl).max()
    floor = n * U52 * R.GRADED_COND
    e_lapack = float(rel(torch.linalg.eigvalsh(torch.from_numpy(A.copy())).flip(-1).numpy()))
    held(f"graded n={n} g={g} eigenvalues, each relative to itself", rel(lam), rel(l64), floor)
    held(f"graded n={n} g={g} eigenvectors entry-wise", vec_err(V, tV), vec_err(V64, tV), floor)
    print(f"RULE graded n={n} g={g} largest relative eigenvalue error: kernel {float(rel(lam)):.3e} LAPACK eigvalsh {e_lapack:.3e}")
    assert float(rel(lam)) <= e_lapack


# ---------------------------------------------------------------- 4. already diagonal input
def _diagonals(n):
    rng = np.random.default_rng(40 + n)
    mixed = rng.choice(np.array([3.0, -1.0, 0.0, -0.0, 7.5, -2.25, 1e-300, 3.0]), size=n)
    mixed[1], mixed[n // 2], mixed[n - 1] = -0.0, 0.0, -0.0
    return {"identity": np.ones(n), "zero": np.zeros(n), "mixed": mixed}


@pytest.mark.parametrize("case", ["identity", "zero", "mixed"])
@pytest.mark.parametrize("n", [16, 64])
def test_diagonal_input_is_only_ranked(ops, dev, n, case):
    """No pair rotates: evals are the diagonal's own bits in the order of the ranking rule (NaN-free here: descending, ties and
    -0.0 / 0.0 by index), evecs the permutation matrix of that order."""
    d = _diagonals(n)[case]
    lam, V = solve(ops, dev, [np.diag(d)])
    order = R.rank_descending(d)
    assert same_bits(lam[0], torch.from_numpy(d[order]))
    perm = np.zeros((n, n))
    perm[order, np.arange(n)] = 1.0
    assert torch.equal(V[0], torch.from_numpy(perm))


# ---------------------------------------------------------------- 5. scale invariance
@functools.lru_cache(maxsize=None)
def _solo(ops, dev, builder, *args):
    """ops.syevj of one matrix alone (CPU tensors), once per process."""
    A = builder(*args)
    lam, V = solve(ops, dev, [A[0] if isinstance(A, tuple) else A])
    return lam[0], V[0]


@pytest.mark.parametrize("k", [100, -100, 520, -520])
def test_scaling_by_a_power_of_two_changes_nothing(ops, dev, k):
    """The rotation test sqrt|a_pp| sqrt|a_qq| scales exactly; at k = +-520 the product a_pp a_qq overflows / underflows."""
    A = R.wishart(64)
    lam0, V0 = _solo(ops, dev, R.wishart, 64)
    lam, V = solve(ops, dev, [np.ldexp(A, k)])
    assert same_bits(lam[0], torch.from_numpy(np.ldexp(lam0.numpy(), k)))
    assert same_bits(V[0], V0)


# ---------------------------------------------------------------- 6. batch independence
def test_batch_members_do_not_see_each_other(ops, dev):
    diag = lambda n: np.diag(_diagonals(n)["mixed"])
    items = [(R.wishart, 64), (diag, 64), (R.graded, 64, 16), (R.rank_deficient, 64)]
    lam, V = solve(ops, dev, [b(*a) for b, *a in items])
    for k, (b, *a) in enumerate(items):
        lam1, V1 = solve(ops, dev, [b(*a)])
        assert same_bits(lam[k], lam1[0]) and same_bits(V[k], V1[0]), f"matrix {k} of the batch"


# ---------------------------------------------------------------- 7. non-finite input
NAN, INF = float("nan"), float("inf")


def poisoned(n, how):
    A = R.wishart(n, 7).copy()
    i, j = n // 2 + 1, 3                                   # i > j: the lower triangle
    if how == "nan_diag":
        A[i, i] = NAN
    elif how == "nan_lower":
        A[i, j] = NAN                                      # (A[j, i] stays finite: only the lower triangle is read)
    elif how == "nan_row_col":
        A[i, :] = NAN
        A[:, i] = NAN
    elif how == "all_nan":
        A[:] = NAN
    elif how == "inf":
        A[i, j] = A[j, i] = INF
    else:
        raise ValueError(how)
    return A


POISONS = ["nan_diag", "nan_lower", "nan_row_col", "all_nan", "inf"]


@pytest.mark.parametrize("how", POISONS)
@pytest.mark.parametrize("n", [16, 64])
def test_non_finite_matrix_is_reported_and_isolated(ops, dev, n, how):
    from modegpt_amd import _lib
    first, last = R.wishart(n), R.rank_deficient(n)
    batch = torch.from_numpy(np.stack([first, poisoned(n, how), last])).to(dev)
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.syevj(batch)
    # the raw entry point in deferred-status mode: same error from check(), the neighbours untouched by the bad matrix
    work = batch.clone()
    evals = torch.full((3, n), 7.0, dtype=F64, device=dev)
    evecs = torch.full((3, n, n), 7.0, dtype=F64, device=dev)
    with ops.DeferredStatus(dev) as st:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mdg_syevj_batched(work.data_ptr(), n, 3, evals.data_ptr(), evecs.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "mdg_syevj_batched")
    with pytest.raises(RuntimeError, match="non-finite"):
        st.check()
    evals, evecs = evals.cpu(), evecs.cpu()
    for k, (b, a) in ((0, (R.wishart, n)), (2, (R.rank_deficient, n))):
        lam1, V1 = _solo(ops, dev, b, a)
        assert same_bits(evals[k], lam1) and same_bits(evecs[k], V1), f"matrix {k} beside a non-finite one"
    assert torch.isnan(evals[1]).all() and torch.isnan(evecs[1]).all()


def test_nan_above_the_diagonal_is_not_read(ops, dev):
    A = R.wishart(64)
    B = A.copy()
    B[3, 40] = NAN
    B[0, 63] = INF
    lam, V = solve(ops, dev, [B])
    lam0, V0 = _solo(ops, dev, R.wishart, 64)
    assert same_bits(lam[0], lam0) and same_bits(V[0], V0)


def test_sqrt_psd_small_reports_non_finite_input(ops, dev):
    M = torch.from_numpy(np.stack([R.wishart(64), poisoned(64, "nan_row_col")])).to(dev)
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.sqrt_psd_small(M, 1e-5, False, True)


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("n_heads,n_kv", [(4, 2), (2, 2)])
def test_vo_compress_reports_a_poisoned_statistic(ops, dev, n_heads, n_kv, deferred):
    """sigma_x with one NaN row and column (what a NaN activation column leaves behind) through the grouped and the two-SVD MHA
    variant: the error names the non-finite input, at once or from the deferred status."""
    d, hd, rank = 64, 16, 8
    gen = torch.Generator().manual_seed(11)
    Wv = torch.randn(n_kv * hd, d, generator=gen).to(torch.bfloat16).to(dev)
    Wo = torch.randn(d, n_heads * hd, generator=gen).to(torch.bfloat16).to(dev)
    sigma = torch.from_numpy(poisoned(d, "nan_row_col")).to(dev)
    if deferred:
        with ops.DeferredStatus(dev) as st:
            ops.vo_compress(sigma, Wv, Wo, n_heads, n_kv, hd, rank, 1e-4)
        with pytest.raises(RuntimeError, match="non-finite"):
            st.check()
    else:
        with pytest.raises(RuntimeError, match="non-finite"):
            ops.vo_compress(sigma, Wv, Wo, n_heads, n_kv, hd, rank, 1e-4)


@pytest.mark.parametrize("want_evals", [True, False])
def test_sqrt_psd_large_rejects_nan(ops, dev, want_evals):
    M = R.wishart(130).copy()
    M[70, 3] = M[3, 70] = NAN
    with pytest.raises(RuntimeError, match="non-finite"):          # (return code and NaN-filled outputs: test_gpu_sqrt_large.py)
        ops.sqrt_psd_large(torch.from_numpy(M).to(dev), 1e-5, False, True, want_evals=want_evals)


# ---------------------------------------------------------------- 8. mdg_sqrt_psd_small against long double
@pytest.mark.parametrize("ridge,scaled,inverse", [(1e-5, False, True), (1e-3, True, False)])
def test_sqrt_psd_small_against_long_double(ops, dev, ridge, scaled, inverse):
    """Root and inverse root rebuilt from the long-double eigenpairs with the reference's clamps, errors relative to the largest
    entry; e64: the same rebuild in fp64 from eig_ref's fp64 eigenpairs."""
    n = 64
    refs = [R.reference(R.rank_deficient, n), R.reference(R.graded, n, 8)]
    M = torch.from_numpy(np.stack([r[0] for r in refs])).to(dev)
    root, inv, evals = ops.sqrt_psd_small(M, ridge, scaled, inverse)
    lam, _ = ops.syevj(M)
    assert same_bits(evals.cpu(), lam.cpu())
    for k, (name, (A, (tl, tV, _), (l64, V64, _))) in enumerate(zip(("rank_deficient", "graded g=8"), refs)):
        truth = R.sqrt_psd(tl, tV, ridge, scaled)
        yard = R.sqrt_psd(l64, V64, ridge, scaled)
        err = lambda X, T: np.abs(R.ld(X) - T).max() / np.abs(T).max()
        tag = f"sqrt_psd_small {name} ridge={ridge:g} scaled={scaled}"
        held(f"{tag} root", err(root[k].cpu().numpy(), truth[0]), err(yard[0], truth[0]), n * U52)
        if inverse:
            held(f"{tag} inverse root", err(inv[k].cpu().numpy(), truth[1]), err(yard[1], truth[1]), n * U52)


# ---------------------------------------------------------------- 9. argument checks
@pytest.mark.parametrize("n", [7, 130, 0])
def test_unsupported_sizes_are_rejected_before_any_launch(ops, dev, n):
    from modegpt_amd import _lib
    cap = 130 * 130
    A = torch.full((cap,), 5.0, dtype=F64, device=dev)
    evals = torch.full((cap,), 5.0, dtype=F64, device=dev)
    evecs = torch.full((cap,), 5.0, dtype=F64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().mdg_syevj_batched(A.data_ptr(), n, 1, evals.data_ptr(), evecs.data_ptr(),
                                           torch.cuda.current_stream(dev).cuda_stream)
    with pytest.raises(RuntimeError, match=r"syevj: n=%d must be even and in \[2, 128\]" % n):
        _lib.check(rc, "mdg_syevj_batched")
    torch.cuda.synchronize(dev)
    for t in (A, evals, evecs):                            # nothing ran: every buffer still holds its fill
        assert bool((t == 5.0).all())
    if n == 7:
        with pytest.raises(RuntimeError, match="must be even"):
            ops.syevj(torch.eye(7, dtype=F64, device=dev)[None])
