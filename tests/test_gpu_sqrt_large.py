"""mdg_sqrt_psd_large on both routes (Newton-Schulz GEMMs; block Jacobi) against the extended-precision host reference
tests/sqrt_ref.py: long-double truths, the residual metrics at the structural sizes, the ridge gate between the routes, run-to-run
bits, leading dimension / upper triangle / workspace, non-finite input, the fall-back, the argument checks and the sqrt_M surface.

The product build cannot say which route ran; the tests choose it by the documented arguments: want_evals=False, scaled=False,
ridge >= 1e-12 ATTEMPTS Newton-Schulz ("newton" below); want_evals=True or scaled=True forces the eigen route ("eigen").

THE RULE of every accuracy assertion (as tests/test_gpu_eigh.py).  On the same input and in the same metric the kernel must stay within

    max(4 e_ref, n 2^-52 scale)

e_ref = the LARGER of two fp64 CPU errors: the reference formula oracle.modegpt_oracle.sqrt_M (LAPACK eigh), and the route's own
host yardstick -- sqrt_ref.newton_schulz in fp64 for a Newton call (where that model gives up, as the call then falls back, and for
every eigen call: eig_ref.sqrt_psd on eig_ref's fp64 Jacobi pairs).
4 = two bits for FMA contraction and the different association on the device; the floor keeps a lucky small e_ref from becoming the
bar (scale 1: every metric is relative).  The metric is sqrt_ref.frob_err against the long-double truth, or the residuals res_root /
res_inv where there is none -- Frobenius norms, in which the perturbation bound of the square root is stated
(||A^1/2 - B^1/2||_F <= ||A - B||_F / (lambda_min(A)^1/2 + lambda_min(B)^1/2)).  Nothing is measured against the kernel itself; every
test prints e_ref, the kernel's error and their ratio (lines RULE under pytest -s) before it asserts.

MEASURED on an MI355X, kernel error / e_ref, smallest - largest per route and metric (largest share of the bound):
    Newton-Schulz   root 0.04 - 1.07 (0.27)   inverse root 0.04 - 1.00 (0.25)   res_root 0.12 - 1.00 (0.25)   res_inv 0.21 - 1.00 (0.10)
                    steps: 10 (wishart 130; 127 - 129), 11 (257, 384), 24 (rank-deficient 130 and 200), 18 (graded; rank one), 15 (distinct),
                    43 (rank-deficient, ridge 1e-12), 6 then the fall-back (indefinite) -- each the host model's own count
    eigen route     root 0.03 - 1.74 (0.31)   inverse root 0.02 - 1.72 (0.43)   eigenvalues 0.00 - 0.06 (0.02)
                    res_root 0.02 - 1.00 (0.25)   res_inv 0.02 - 1.00 (0.15); 2 - 8 sweeps, 14 on rank_deficient(200)
    ridge gate      inverse root 0.98 at ridge 1e-12 (Newton-Schulz, 43 steps; 3.3e-4 against e_ref 3.4e-4), 0.26 at 5e-13 (eigen route)
    eigen contract  ||root - truth||_F at most 0.0057 of 4 tau ||A||_F / (2 sqrt(max(lambda_min, 0) + ridge))
    Before the eigen route orthogonalised V and formed V^T A V afresh ahead of its last sweep it missed THE RULE four times: res_root at
    n = 257 (1.63 of the bound) and 384 (1.80; 9.7e-13 and 1.7e-12), the root of the 160 x 160 fall-back case (1.25) and of
    rank_deficient(200) scaled (1.03), with six more between 0.92 and 0.99.  Before the three double-precision atomicAdds were
    replaced by fixed-order sums, the reproducibility, layout and sqrt_M-slice tests failed on the Newton route (bits differed between
    calls); the non-finite tests failed with "block Jacobi did not converge in 30 sweeps" and unwritten outputs.
"""
import functools

import numpy as np
import pytest
import torch

from tests import eig_ref as R
from tests import sqrt_ref as S

pytestmark = pytest.mark.gpu
F64 = torch.float64
U52 = 2.0 ** -52
NAN, INF = float("nan"), float("inf")
SENT = 7.0
EIGEN_TAU = 1e-13          # the eigen route's stopping threshold ||off||_F <= tau ||A||_F, read from eigh.hip


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_result(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y))


def held(what, err, e_ref, floor):
    err, e_ref = float(err), float(e_ref)
    bound = max(4 * e_ref, floor)
    print(f"RULE {what}: e_ref {e_ref:.3e} kernel {err:.3e} ratio {err / e_ref if e_ref else float('inf'):.2f} "
          f"floor {floor:.3e} -> {err / bound:.3f} of the bound")
    assert err <= bound, f"{what}: kernel error {err:.3e} above max(4 x {e_ref:.3e}, {floor:.3e})"


def call(ops, dev, A, ridge, route, scaled=False, inverse=True):
    """ops.sqrt_psd_large on the numpy / torch matrix A -> (root, inv_root, evals) as CPU tensors (None where not asked for)."""
    M = A if torch.is_tensor(A) else torch.from_numpy(np.ascontiguousarray(A))
    out = ops.sqrt_psd_large(M.to(dev), ridge, scaled, inverse, want_evals=(route == "eigen"))
    torch.cuda.synchronize(dev)
    return tuple(None if t is None else t.cpu() for t in out)


@functools.lru_cache(maxsize=None)
def plain(ops, dev, case, ridge, route, scaled=False):
    """The plain call's result on a case (CPU tensors), once per process, read-only."""
    return call(ops, dev, S.case_matrix(case), ridge, route, scaled)


def direct(dev, M, n, ld, ridge, route, scaled=False, inverse=True, fill=0xFF, ws_short=0, null=(), n_arg=None, stream=None):
    """The library entry itself, outputs pre-filled with SENT and a workspace of the test's own with every byte `fill`.
    -> (rc, message, root, inv_root, evals) as CPU tensors.  null: names of pointer arguments passed as NULL."""
    from modegpt_amd import _lib
    lib = _lib.load()
    root = torch.full((n, n), SENT, dtype=F64, device=dev)
    inv = torch.full((n, n), SENT, dtype=F64, device=dev) if inverse else None
    ev = torch.full((n,), SENT, dtype=F64, device=dev) if route == "eigen" else None
    nbytes = lib.mdg_sqrt_psd_large_ws_bytes(n)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    ptr = lambda name, t: None if (t is None or name in null) else t.data_ptr()
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
        rc = lib.mdg_sqrt_psd_large(ptr("M", M), n if n_arg is None else n_arg, ld, float(ridge), int(scaled), ptr("root", root),
                                    ptr("inv", inv), ptr("ev", ev), ptr("ws", ws), nbytes - ws_short, st)
    msg = _lib.last_error() if rc != 0 else ""
    torch.cuda.synchronize(dev)
    return (rc, msg) + tuple(None if t is None else t.cpu() for t in (root, inv, ev))


def truth_of(case, ridge, scaled=False):
    if case[0] is R.exact_spectrum:
        return S.exact_truth(case[1], case[2], ridge, scaled)
    return S.truth(case, ridge, scaled)


# ---------------------------------------------------------------- 1. against the long-double truth
EXACT_CASES = [((R.exact_spectrum, 256, kind), S.EXACT_RIDGE) for kind in S.EXACT_KINDS]
VARIANTS = [("newton", False), ("eigen", False), ("eigen", True)]


@pytest.mark.parametrize("route,scaled", VARIANTS, ids=["newton", "eigen", "eigen-scaled"])
@pytest.mark.parametrize("case,ridge", S.TRUTH_CASES + EXACT_CASES, ids=lambda v: S.case_name(v) if isinstance(v, tuple) else None)
def test_against_truth(ops, dev, case, ridge, route, scaled):
    """Root, inverse root and (eigen route) the eigenvalues, sorted, against the truth; scaled: ridge 1e-3 times lambda_max.  On the
    indefinite spectrum the truth carries the reference's clamps and the Newton call answers through its fall-back; on rank one
    (A + ridge I is positive definite) the Newton route itself answers, held to the same truth."""
    ridge = 1e-3 if scaled else ridge
    n = S.case_matrix(case).shape[0]
    t_root, t_inv, t_lam = truth_of(case, ridge, scaled)
    refs = S.references(case, ridge, scaled, route)
    root, inv, ev = plain(ops, dev, case, ridge, route, scaled)
    tag = f"{S.case_name(case)} ridge={ridge:g} {route}{' scaled' if scaled else ''}"
    held(f"{tag} root", S.frob_err(root.numpy(), t_root), S.e_ref(refs, lambda X: S.frob_err(X, t_root), 1), n * U52)
    held(f"{tag} inverse root", S.frob_err(inv.numpy(), t_inv), S.e_ref(refs, lambda X: S.frob_err(X, t_inv), 2), n * U52)
    if route == "eigen":
        held(f"{tag} eigenvalues / |lambda|max", S.eval_err(ev.numpy(), t_lam), S.e_ref(refs, lambda l: S.eval_err(l, t_lam), 3),
             n * U52)
        # the header's a-priori contract of the eigen route, from its stopping rule off <= tau ||A||_F, tau = 1e-13 (eigh.hip), and
        # ||A^1/2 - B^1/2||_F <= ||A - B||_F / (lambda_min(A)^1/2 + lambda_min(B)^1/2)
        rho = ridge * (float(t_lam.max()) if scaled else 1.0)
        normA = float(np.sqrt((R.ld(S.case_matrix(case)) ** 2).sum()))
        contract = 4 * EIGEN_TAU * normA / (2 * np.sqrt(max(float(t_lam.min()), 0.0) + rho))
        err_abs = float(np.sqrt(((R.ld(root.numpy()) - t_root) ** 2).sum()))
        print(f"RULE {tag} root, absolute, against the stopping rule's bound: kernel {err_abs:.3e} bound {contract:.3e} -> "
              f"{err_abs / contract:.4f} of it")
        assert err_abs <= contract
    else:
        assert ev is None


# ---------------------------------------------------------------- 2. residuals at the structural sizes
@pytest.mark.parametrize("route", ["newton", "eigen"])
@pytest.mark.parametrize("n", S.RESIDUAL_SIZES)
def test_residuals_at_structural_sizes(ops, dev, n, route):
    """Gram matrices of 3 n tokens.  n <= 128: one 128-block pair (m = 1, one round, no permutation); 129: m = 2; 257: odd m = 3; 128
    and 384: exact multiples of the tile; 1, 127, 129, 257: odd n, the padding of the eigen route and the GEMMs' edge tiles."""
    case = (R.wishart, n)
    A = S.case_matrix(case)
    refs = S.references(case, 1e-5, False, route)
    assert refs[1][0] == ("Newton-Schulz model" if route == "newton" else "fp64 Jacobi")
    root, inv, ev = plain(ops, dev, case, 1e-5, route)
    tag = f"wishart n={n} {route}"
    held(f"{tag} res_root", S.res_root(root.numpy(), A, 1e-5), S.e_ref(refs, lambda X: S.res_root(X, A, 1e-5), 1), n * U52)
    held(f"{tag} res_inv", S.res_inv(inv.numpy(), root.numpy()), max(float(S.res_inv(r[2], r[1])) for r in refs), n * U52)
    if route == "newton":                                  # the finish kernel averages S and S^T: symmetric to the bit
        assert float(S.asym(root.numpy())) == 0.0 and float(S.asym(inv.numpy())) == 0.0
    else:
        assert ev.shape == (n,) and bool(torch.isfinite(ev).all())


# ---------------------------------------------------------------- 3. the ridge gate
@pytest.mark.parametrize("ridge", S.GATE_RIDGES)
def test_ridge_gate(ops, dev, ridge):
    """The same call (no eigenvalues, not scaled) on the rank-deficient matrix: ridge 1e-12 attempts Newton-Schulz (the host model
    reaches "ok"), 5e-13 and 0 go to the eigen route.  The inverse root is held by THE RULE wherever the input determines it:
    lambda_min + ridge > n 2^-52 lambda_max, the eigenvalue noise of any fp64 solver.  That holds at 1e-12 and 5e-13 (f ~ 1e-6, far
    above the 1e-12 clamp on f; 1.6e-13 is the noise); at ridge 0 rounding decides the sign of lambda + ridge and with it whether
    g is 1e12 or not, so there it is only reported."""
    case = S.GATE_CASE
    n = S.case_matrix(case).shape[0]
    route = "newton" if ridge >= 1e-12 else "eigen"
    if route == "newton":
        assert S.newton_yardstick(case, ridge)[3] == "ok"
    t_root, t_inv, t_lam = S.truth(case, ridge)
    refs = S.references(case, ridge, False, route)
    root, inv, ev = plain(ops, dev, case, ridge, "newton")
    assert ev is None
    tag = f"rank_deficient-130 ridge={ridge:g} ({route} expected)"
    held(f"{tag} root", S.frob_err(root.numpy(), t_root), S.e_ref(refs, lambda X: S.frob_err(X, t_root), 1), n * U52)
    noise = n * U52 * float(np.abs(t_lam).max())
    if float(t_lam.min()) + ridge > noise:
        held(f"{tag} inverse root", S.frob_err(inv.numpy(), t_inv), S.e_ref(refs, lambda X: S.frob_err(X, t_inv), 2), n * U52)
    else:
        assert ridge == 0.0                                # (the one ridge of the three at which nothing determines it)
        print(f"RULE {tag} inverse root: not held (lambda_min + ridge = {float(t_lam.min()) + ridge:.3e} within the eigenvalue "
              f"noise {noise:.3e})")
        assert bool(torch.isfinite(inv).all())


# ---------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("route", ["newton", "eigen"])
@pytest.mark.parametrize("n", [130, 257])
def test_three_calls_give_the_same_bits(ops, dev, n, route):
    """No floating-point atomics: ||A||_F^2, the Newton-Schulz residual and the off-norm are summed in a fixed order, so the scale of
    Y0, the step / sweep count and every bit of the result are the same on every call -- and on another stream."""
    case = (R.rank_deficient, n) if n == 130 else (R.wishart, n)
    A = S.case_matrix(case)
    first = plain(ops, dev, case, 1e-5, route)
    for k in range(2):
        assert same_result(call(ops, dev, A, 1e-5, route), first), f"call {k + 2} differs from the first"
    side = torch.cuda.Stream(dev)
    M = torch.from_numpy(A).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        out = ops.sqrt_psd_large(M, 1e-5, False, True, want_evals=(route == "eigen"))
    side.synchronize()
    assert same_result(tuple(None if t is None else t.cpu() for t in out), first), "the call on a second stream differs"


# ---------------------------------------------------------------- 5. layout
@pytest.mark.parametrize("route", ["newton", "eigen"])
@pytest.mark.parametrize("n", [130, 257])
def test_layout_changes_nothing(ops, dev, n, route):
    """ld > n with the data pointer off the 16-byte boundary, NaN / Inf strictly above the diagonal (the lower triangle is
    authoritative on both routes), a workspace of exactly the queried size with every byte 0xFF: the plain call's bits, and the
    input buffer is not written."""
    case = (R.rank_deficient, n) if n == 130 else (R.wishart, n)
    A = S.case_matrix(case)
    want = plain(ops, dev, case, 1e-5, route)
    # a window of a larger NaN-filled buffer
    buf = torch.full((n + 3, n + 37), NAN, dtype=F64)
    buf[:n, 5:5 + n] = torch.from_numpy(A)
    buf_d = buf.to(dev)
    view = buf_d[:n, 5:5 + n]
    assert view.stride(0) == n + 37 and view.data_ptr() % 16 == 8
    out = ops.sqrt_psd_large(view, 1e-5, False, True, want_evals=(route == "eigen"))
    torch.cuda.synchronize(dev)
    assert same_result(tuple(None if t is None else t.cpu() for t in out), want), "ld > n changes the result"
    assert same_bits(buf_d.cpu(), buf), "the input buffer was written"
    # a poisoned upper triangle
    P = A.copy()
    iu = np.triu_indices(n, 1)
    P[iu] = np.where(np.arange(iu[0].size) % 2 == 0, NAN, INF)
    assert same_result(call(ops, dev, P, 1e-5, route), want), "the upper triangle is read"
    # a poisoned workspace, through the entry itself
    M = torch.from_numpy(A).to(dev)
    rc, msg, root, inv, ev = direct(dev, M, n, n, 1e-5, route)
    assert rc == 0, msg
    assert same_result((root, inv, ev), want), "the workspace's old contents are read"
    assert same_bits(M.cpu(), torch.from_numpy(A))


# ---------------------------------------------------------------- 6. non-finite input
@pytest.mark.parametrize("route", ["newton", "eigen"])
@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "inf", "-inf"])
def test_non_finite_input_is_named_and_outputs_are_nan(ops, dev, value, route):
    """A NaN or Inf anywhere in the lower triangle: MDG_ERR_NO_CONVERGE, the non-finite-input message (found by the load pass, not
    after 30 sweeps), root, inv_root and evals_out all NaN."""
    from modegpt_amd import _lib
    n = 130
    for i, j in ((0, 0), (n - 1, 0), (n - 1, n - 1), (70, 3)):
        A = R.wishart(n).copy()
        A[i, j] = value                                    # (A[j, i] stays finite: only the lower triangle is read)
        rc, msg, root, inv, ev = direct(dev, torch.from_numpy(A).to(dev), n, n, 1e-5, route)
        assert rc == _lib.MDG_ERR_NO_CONVERGE, f"({i}, {j}): rc {rc} {msg!r}"
        assert msg.startswith("mdg_sqrt_psd_large:") and "non-finite" in msg, msg
        assert bool(torch.isnan(root).all()) and bool(torch.isnan(inv).all()), f"({i}, {j}): outputs not NaN-filled"
        assert ev is None or bool(torch.isnan(ev).all())
    with pytest.raises(RuntimeError, match="non-finite"):
        ops.sqrt_psd_large(torch.from_numpy(A).to(dev), 1e-5, False, True, want_evals=(route == "eigen"))


# ---------------------------------------------------------------- 7. the fall-back
def indefinite160():
    """The 160 x 160 matrix of test_gpu_kernels.py's fall-back test: one eigenvalue -0.5 below -ridge."""
    gen = torch.Generator().manual_seed(2)
    Q, _ = torch.linalg.qr(torch.randn(160, 160, generator=gen, dtype=F64))
    lam = torch.linspace(0.01, 3.0, 160, dtype=F64)
    lam[0] = -0.5
    M = (Q * lam) @ Q.T
    return R.sym_lower(((M + M.T) / 2).numpy())


@pytest.mark.parametrize("case", [(R.exact_spectrum, 256, "indefinite"), (indefinite160,)], ids=["exact256", "qr160"])
def test_indefinite_input_falls_back_to_the_eigen_route(ops, dev, case):
    """No real root of A + ridge I exists; the Newton call must notice and return the eigen route's answer -- to the bit -- which
    is held to the clamped truth."""
    ridge = 1e-4
    n = S.case_matrix(case).shape[0]
    assert S.newton_yardstick(case, ridge)[3] in ("diverged", "stuck")
    newton = plain(ops, dev, case, ridge, "newton")
    eigen = plain(ops, dev, case, ridge, "eigen")
    assert same_bits(newton[0], eigen[0]) and same_bits(newton[1], eigen[1])
    t_root, t_inv, _ = truth_of(case, ridge)
    refs = S.references(case, ridge, False, "newton")
    held(f"{S.case_name(case)} fall-back root", S.frob_err(newton[0].numpy(), t_root), S.e_ref(refs, lambda X: S.frob_err(X, t_root), 1),
         n * U52)


def test_newton_route_answers_on_a_definite_input(ops, dev):
    """The other side of the fall-back test: on wishart(130) the two calls' bits differ, so the Newton route did answer."""
    newton = plain(ops, dev, (R.wishart, 130), 1e-5, "newton")
    eigen = plain(ops, dev, (R.wishart, 130), 1e-5, "eigen")
    assert not same_bits(newton[0], eigen[0])


# ---------------------------------------------------------------- 8. argument checks
BAD_ARGS = {"null M": dict(null=("M",)), "null root": dict(null=("root",)), "n = 0": dict(n_arg=0), "n = -1": dict(n_arg=-1),
            "ld = n - 1": dict(ld=129), "null ws": dict(null=("ws",)), "ws one byte short": dict(ws_short=1)}


@pytest.mark.parametrize("route", ["newton", "eigen"])
@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_arguments_are_rejected_before_any_launch(ops, dev, what, route):
    from modegpt_amd import _lib
    n = 130
    M = torch.from_numpy(R.wishart(n)).to(dev)
    kw = dict(ld=n)
    kw.update(BAD_ARGS[what])
    ld = kw.pop("ld")
    rc, msg, root, inv, ev = direct(dev, M, n, ld, 1e-5, route, **kw)
    assert rc == _lib.MDG_ERR_BAD_ARG, f"{what}: rc {rc}"
    assert msg.startswith("mdg_sqrt_psd_large:"), msg
    for t in (root, inv, ev):                              # nothing ran: every output still holds its fill
        assert t is None or bool((t == SENT).all()), f"{what}: an output was written"


def test_ops_rejects_what_is_not_one_square_matrix(ops, dev):
    with pytest.raises(ValueError, match="one square matrix"):
        ops.sqrt_psd_large(torch.zeros(130, 131, dtype=F64, device=dev), 1e-5, False, True)
    with pytest.raises(ValueError, match="one square matrix"):
        ops.sqrt_psd_large(torch.zeros(2, 130, 130, dtype=F64, device=dev), 1e-5, False, True)


# ---------------------------------------------------------------- 9. the sqrt_M surface
@pytest.mark.parametrize("inverse", [False, True])
def test_sqrt_M_batch_slices_are_the_single_calls(ops, dev, inverse):
    from modegpt_amd.compression_utils import sqrt_M
    cases = [(R.wishart, 130), (R.rank_deficient, 130)]
    M = torch.from_numpy(np.stack([S.case_matrix(c) for c in cases])).to(dev)
    out = sqrt_M(M, ridge_lambda=1e-5, inverse_sqrt=inverse)
    roots, invs = (out if inverse else (out, None))
    for k, c in enumerate(cases):
        want = plain(ops, dev, c, 1e-5, "newton")
        assert same_bits(roots[k].cpu(), want[0]), f"root of slice {k}"
        if inverse:
            assert same_bits(invs[k].cpu(), want[1]), f"inverse root of slice {k}"
