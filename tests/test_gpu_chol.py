"""The Cholesky family (mdg_potrf_lower, mdg_potrs_lower, mdg_ridge_scores, mdg_nystrom_down / _overlapped) against the
extended-precision host reference tests/chol_ref.py: entry-wise, strided, at the block edges and at every kind of pivot failure.

Backward error of potrf (section "potrf").  For any summation order |A - L L^T|_ij <= gamma_{n+1} (|L||L^T|)_ij <=
gamma_{n+1} / (1 - gamma_{n+1}) sqrt(a_ii a_jj) (Higham, Accuracy and Stability, Thm 10.3 and eq. 10.7); asserted entry by entry,
with the residual in long double, as  |A - L L^T|_ij <= (n + 16) 2^-53 sqrt(a_ii a_jj).  The +16 pays for the device's
l_jj = d * rsqrt(d), l_ij = a_ij * rsqrt(d) (rsqrt: 1 ulp, plus one multiply) in place of a correctly rounded square root and a
divide.

Forward accuracy (section "forward").  e_kernel <= R * max(e_torch, 64 n 2^-53), both errors against the long-double
reference in the same entry-wise metric, e_torch from the plain fp64 CPU routine.  R was fixed once from the GPU run as 4 x the
largest observed ratio rounded up to a power of two and may never exceed 32; a ratio above 32 is a finding, not a tolerance.

What potrf writes above the diagonal (section "strides").  The contract asserted is the one of include/modegpt_hip.h: outside the
128 x 128 diagonal blocks nothing above the diagonal is read or written, inside them entries may be overwritten.

MEASURED on an MI355X (every test prints its figure before it asserts: lines BACKWARD, FORWARD, UPPER under pytest -s)
Backward residual maxima as fractions of (n + 16) u sqrt(a_ii a_jj), matrices p3 / p8 / p6g3 / acts:
    n = 16: 0.051 0.050 0.037 0.111    n = 129: 0.040 0.124 0.078 0.079    n = 385: 0.018 0.023 0.026 0.023
    n = 640: 0.017 0.013 0.013 0.018   sampled: 2049 p3 0.0064, 2049 p6g3 0.0055, 2304 p8 0.018, 2304 p6g3 0.025, 4224 p6g3 0.013
    (largest 0.124; LAPACK's factor of the same matrices: 0.003 - 0.011)
Forward ratios e_kernel / max(e_torch, 64 n u), largest per group:
    potrf factor    p3 0.009   p8 0.52 (n = 385)   p6g3 0.33   acts 0.002
    ridge scores    p3 0.017   p6g3 0.59 / 0.95 / 0.71 / 0.55 at n = 129 / 385 / 640 / 704   acts 0.002
    potrs n = 385   p3 0.013   p6g3 1.58 / 1.39 / 1.37 / 1.59 / 1.53 at nrhs = 1 / 70 / 127 / 129 / 257;   n = 2049: 0.001
    nystrom_down    0.006 at the most (the floor 64 n u decides: e_kernel and e_torch are both 1e-15 .. 4e-14)
    largest 1.59 -> 4 x 1.59 = 6.4 -> R = 8.
    Where e_torch is under the floor 64 n u (p3, acts, nystrom_down: ratios 0.001 - 0.02) the criterion admits errors two to three
    decades above what the kernels deliver; it bites on p8 and p6g3, where LAPACK's own error is above the floor.
Above the diagonal, finite sentinel: every entry (8128 of 8128) of every 128 x 128 diagonal block but the first is overwritten, none
in the first block, none outside the diagonal blocks (n = 385: blocks 1 and 2; n = 2304: blocks 1 .. 17, the one behind the
2048-wide outer panel included).
"""
import functools
import re

import numpy as np
import pytest
import torch

from tests import chol_ref as R
from tests.test_gpu_kernels import acts

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
NB = 128                                   # diagonal block of the factorisation
RATIO = 8.0                                # R of the forward-accuracy criterion (module docstring: 4 x 1.59 rounded up)
RIDGE = float(torch.tensor(1e-4, dtype=torch.float32).double())
KINDS = {"p3": (3.0, 0.0), "p8": (8.0, 0.0), "p6g3": (6.0, 3.0)}


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- matrices and their references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def acts_cov(n):
    gen = torch.Generator().manual_seed(7000 + n)
    H = acts(gen, 3 * n, n).double()
    C = H.T @ H / (3 * n)
    C = torch.tril(C)
    return C + torch.tril(C, -1).T


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """(C, ridge, A): the call's input, the ridge it is given and A = C + ridge I as the kernel forms it (one fp64 addition per
    diagonal entry), which is what every reference factorises."""
    if kind == "acts":
        C = acts_cov(n)
        return C, RIDGE, C + torch.diag(torch.full((n,), RIDGE, dtype=F64))
    p, g = KINDS[kind]
    A = R.spd_matrix(n, p, g, seed=list(KINDS).index(kind))
    return A, 0.0, A


@functools.lru_cache(maxsize=None)
def ref_factor(kind, n):
    return R.cholesky(matrix(kind, n)[2])


@functools.lru_cache(maxsize=None)
def ref_inverse(kind, n):
    return R.tri_inverse(ref_factor(kind, n))


@functools.lru_cache(maxsize=None)
def torch_factor(kind, n):
    return torch.linalg.cholesky(matrix(kind, n)[2])


def check_forward(what, e_kernel, e_torch, n):
    """e_kernel <= RATIO * max(e_torch, 64 n u); prints the ratio before it asserts."""
    base = max(float(e_torch), 64 * n * U)
    ratio = float(e_kernel) / base
    print("FORWARD %-44s e_kernel %.3e e_torch %.3e ratio %.3f" % (what, float(e_kernel), float(e_torch), ratio))
    assert ratio <= RATIO, "%s: e_kernel %.3e, e_torch %.3e, ratio %.2f > %g" % (what, e_kernel, e_torch, ratio, RATIO)


def blocks(inv, n):
    """The inverted diagonal blocks of potrf's second output (behind them the buffer holds the call's status word)."""
    return inv[:(n + NB - 1) // NB * NB * NB]


def device_factor(ops, dev, A):
    Ad = A.to(dev).clone()
    inv = ops.potrf_lower(Ad)
    return Ad, inv


# ---------------------------------------------------------------- potrf: entry-wise backward error
def check_backward(what, A, L, pairs=None):
    n = A.shape[0]
    dg = np.sqrt(R.ld(A).diagonal())
    res = np.abs(R.residual(A, L, pairs))
    scale = dg[:, None] * dg[None, :] if pairs is None else dg[pairs[0]] * dg[pairs[1]]
    frac = res / ((n + 16) * U * scale)
    worst = float(frac.max())
    print("BACKWARD %-30s max |A - L L^T|_ij / ((n + 16) u sqrt(a_ii a_jj)) = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: entry-wise residual is %.3f of the bound at %s" % (
        what, worst, np.unravel_index(int(frac.argmax()), frac.shape) if pairs is None else
        (int(pairs[0][frac.argmax()]), int(pairs[1][frac.argmax()])))


@pytest.mark.parametrize("n", [16, 129, 385, 640])
@pytest.mark.parametrize("kind", ["p3", "p8", "p6g3", "acts"])
def test_potrf_backward_error_and_factor(ops, dev, kind, n):
    """Full residual in long double, every entry under the derived bound; and the factor itself against the long-double one,
    entry-wise relative to sqrt(a_ii) (every entry of row i of L is at most that), under the forward criterion."""
    A = matrix(kind, n)[2]
    Ad, _ = device_factor(ops, dev, A)
    L = torch.tril(Ad).cpu()
    check_backward("%s n=%d" % (kind, n), A, L)
    Lref = ref_factor(kind, n)
    dg = np.sqrt(R.ld(A).diagonal())[:, None]
    e_kernel = (np.abs(R.ld(L) - Lref) / dg).max()
    e_torch = (np.abs(R.ld(torch_factor(kind, n)) - Lref) / dg).max()
    check_forward("potrf factor %s n=%d" % (kind, n), e_kernel, e_torch, n)


def sampled_pairs(n, per_tile=64, seed=0):
    """Every diagonal entry, and `per_tile` seeded random entries of every 128 x 128 tile of the lower triangle."""
    rng = np.random.default_rng(seed + n)
    I, J = [np.arange(n)], [np.arange(n)]
    for bi in range(0, n, NB):
        for bj in range(0, bi + 1, NB):
            i = rng.integers(bi, min(n, bi + NB), per_tile)
            j = rng.integers(bj, min(n, bj + NB), per_tile)
            I.append(np.maximum(i, j))
            J.append(np.minimum(i, j))
    return np.concatenate(I), np.concatenate(J)


# 2049: one outer panel and one row; 2304: the panel and two blocks behind the lower-only update; 4224: three outer panels (that
# case takes 1.7 s on the GPU host -- the QR and the product that build the matrix, 40 128 long-double dot products -- the others 0.4 s)
@pytest.mark.parametrize("kind,n", [("p3", 2049), ("p6g3", 2049), ("p8", 2304), ("p6g3", 2304), ("p6g3", 4224)])
def test_potrf_backward_error_sampled(ops, dev, kind, n):
    A = matrix(kind, n)[2]
    Ad, _ = device_factor(ops, dev, A)
    check_backward("%s n=%d sampled" % (kind, n), A, torch.tril(Ad).cpu(), sampled_pairs(n))


# ---------------------------------------------------------------- leading dimensions, and what may be touched
SENTINELS = [pytest.param(-7.25, id="finite"), pytest.param(float("nan"), id="nan")]


def padded(A, fill, dev, rows=5, cols=37, col0=0):
    """A inside a (rows more) x (cols more) buffer filled with `fill`, starting at column col0 -> (buffer, view)."""
    n, m = A.shape
    buf = torch.full((n + rows, m + cols), fill, dtype=A.dtype, device=dev)
    view = buf[:n, col0:col0 + m]
    view.copy_(A)
    return buf, view


def outside_unchanged(buf, before, n, m, col0=0):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:n, col0:col0 + m] = False
    return torch.equal(bits(buf)[mask], bits(before)[mask])


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("n", [385, 2304])
def test_potrf_leading_dimension(ops, dev, n, fill):
    """buf[:n, :n] of an (n + 5) x (n + 37) buffer: the factor and the inverted diagonal blocks are those of the contiguous call bit
    for bit, and nothing outside the logical matrix changes."""
    A = torch.tril(matrix("p3", n)[2])
    Ad, inv = device_factor(ops, dev, A)
    buf, view = padded(A, fill, dev)
    before = buf.clone()
    inv_s = ops.potrf_lower(view)
    assert view.stride(0) == n + 37
    assert same_bits(torch.tril(view), torch.tril(Ad))
    assert same_bits(blocks(inv_s, n), blocks(inv, n))
    assert outside_unchanged(buf, before, n, n)


@pytest.mark.parametrize("n", [385, 2304])
def test_potrf_above_the_diagonal(ops, dev, n):
    """The contract of include/modegpt_hip.h.  Strictly above the diagonal, entries outside the 128 x 128 diagonal blocks are
    neither read nor written: NaN there reaches nothing, a sentinel there survives bit for bit.  Entries inside the diagonal blocks
    may be overwritten with unspecified values, and are not read for the result either: with NaN everywhere above the diagonal the
    lower triangle and the inverted blocks are those of the call with zeros there, bit for bit."""
    A = torch.tril(matrix("p3", n)[2])
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    Ad, inv = device_factor(ops, dev, A)
    blk = torch.arange(n) // NB
    in_diag_block = (blk[:, None] == blk[None, :]) & upper
    for fill in (float("nan"), -7.25):
        Af = A.clone()
        Af[upper] = fill
        Afd, inv_f = device_factor(ops, dev, Af)
        assert same_bits(torch.tril(Afd), torch.tril(Ad)), fill
        assert same_bits(blocks(inv_f, n), blocks(inv, n)), fill
        changed = (bits(Afd.cpu()) != bits(Af)) & upper
        assert not bool((changed & ~in_diag_block).any()), "written above the diagonal outside the diagonal blocks"
        if fill == fill:    # the finite sentinel shows what is overwritten (NaN + x stays the same NaN)
            per_block = [int(changed[b * NB:(b + 1) * NB, b * NB:(b + 1) * NB].sum()) for b in range((n + NB - 1) // NB)]
            full = [int(in_diag_block[b * NB:(b + 1) * NB, b * NB:(b + 1) * NB].sum()) for b in range(len(per_block))]
            print("UPPER n=%d entries overwritten above the diagonal, per diagonal block: %s of %s" % (n, per_block, full))


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("n,nrhs", [(385, 70), (385, 129), (2304, 5)])
def test_potrs_leading_dimensions(ops, dev, n, nrhs, fill):
    """X = big[:, 3:3 + nrhs] and L inside a wider buffer: the solution of the contiguous call bit for bit, nothing outside X
    changes, and L and inv_diag are left as they were."""
    A = torch.tril(matrix("p3", n)[2])
    Ad, inv = device_factor(ops, dev, A)
    B = torch.randn(n, nrhs, generator=torch.Generator().manual_seed(n + nrhs), dtype=F64)
    Xc = B.to(dev).clone()
    ops.potrs_lower(Ad, inv, Xc)
    lbuf, lview = padded(torch.tril(Ad), fill, dev)
    xbuf, xview = padded(B, fill, dev, rows=2, cols=9, col0=3)
    l_before, x_before, inv_before = lbuf.clone(), xbuf.clone(), inv.clone()
    ops.potrs_lower(lview, inv, xview)
    assert xview.stride(0) == nrhs + 9 and xview.data_ptr() == xbuf.data_ptr() + 3 * 8
    assert same_bits(xview, Xc)
    assert outside_unchanged(xbuf, x_before, n, nrhs, col0=3)
    assert same_bits(lbuf, l_before) and same_bits(inv, inv_before)


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("n", [385, 704])
def test_ridge_scores_leading_dimension(ops, dev, n, fill):
    C, ridge, _ = matrix("acts", n)
    want, want_sens = ops.ridge_scores(C.to(dev), ridge, want_sens=True)
    buf, view = padded(C, fill, dev)
    before = buf.clone()
    got, sens = ops.ridge_scores(view, ridge, want_sens=True)
    assert same_bits(got, want) and same_bits(sens, want_sens)
    assert same_bits(buf, before)                       # C is not modified, nor anything around it


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("wdt", [torch.bfloat16, torch.float64], ids=["bf16", "f64"])
def test_nystrom_leading_dimensions(ops, dev, wdt, fill):
    """C and W_down as column slices of wider buffers (their data pointers then sit off the 16-byte boundary the vector loads
    want): both outputs bit for bit those of the contiguous call, inputs and their surroundings unchanged."""
    n, r, d = 640, 449, 130
    gen = torch.Generator().manual_seed(11)
    C = acts_cov(n)
    W = (torch.randn(d, n, generator=gen) * 0.05).to(wdt)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values.to(dev)
    want, want64 = ops.nystrom_down(C.to(dev), idx, W.to(dev), want_f64=True)
    cbuf, cview = padded(C, fill, dev, rows=3, cols=37, col0=5)
    wbuf, wview = padded(W, fill, dev, rows=2, cols=11, col0=3)
    c_before, w_before = cbuf.clone(), wbuf.clone()
    got, got64 = ops.nystrom_down(cview, idx, wview, want_f64=True)
    torch.cuda.synchronize()
    assert same_bits(got64, want64)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert same_bits(cbuf, c_before)
    assert torch.equal(wbuf.view(torch.int16 if wdt == torch.bfloat16 else torch.int64),
                       w_before.view(torch.int16 if wdt == torch.bfloat16 else torch.int64))


# ---------------------------------------------------------------- forward accuracy against the extended reference
@pytest.mark.parametrize("n", [129, 385, 640, 704])   # 385: m = 1 at s = 128, and 129 rows behind zero full pairs at s = 256;
@pytest.mark.parametrize("kind", ["p3", "p6g3", "acts"])                                 # 640: a level whose only pair is ragged
def test_ridge_scores_entrywise(ops, dev, kind, n):
    """max_j |s_j - ref_j| / ref_j against LAPACK's diag(inv(A)) in the same metric; the same bits with and without the
    sensitivities; and the certificate sens_j >= (sum_a sqrt(c_aa) |z_aj|)^2 with z = A^-1 from the reference inverse (Z = X^T X is
    formed in fp64 from the long-double X: its error n u (|X|^T |X|)_aj moves the right-hand side by n u sqrt(sens_j) at the most,
    four decades under the 1e-9 allowed)."""
    C, ridge, A = matrix(kind, n)
    plain = ops.ridge_scores(C.to(dev), ridge)
    scores, sens = ops.ridge_scores(C.to(dev), ridge, want_sens=True)
    assert same_bits(plain, scores)
    X = ref_inverse(kind, n)
    want = R.inverse_diag(X)
    e_kernel = (np.abs(R.ld(scores) - want) / want).max()
    e_torch = (np.abs(R.ld(torch.linalg.inv(A).diagonal()) - want) / want).max()
    check_forward("ridge scores %s n=%d" % (kind, n), e_kernel, e_torch, n)
    X64 = torch.from_numpy(X.astype(np.float64))
    first_order = ((X64.T @ X64).abs().T @ torch.sqrt(torch.diagonal(C))) ** 2
    assert bool((sens.cpu() * (1 + 1e-9) >= first_order).all()), (first_order / sens.cpu()).max().item()


def column_error(X, ref):
    return (np.abs(R.ld(X) - ref).max(axis=0) / np.abs(ref).max(axis=0)).max()


@pytest.mark.parametrize("nrhs", [1, 70, 127, 129, 257])
@pytest.mark.parametrize("kind", ["p3", "p6g3"])
def test_potrs_entrywise(ops, dev, kind, nrhs):
    """Per column of the right-hand side ||x - ref||_inf / ||ref||_inf at n = 385, the device's own factor behind it, against
    torch.cholesky_solve with LAPACK's factor."""
    n = 385
    A = matrix(kind, n)[2]
    B = torch.randn(n, nrhs, generator=torch.Generator().manual_seed(nrhs), dtype=F64)
    ref = R.cholesky_solve(ref_factor(kind, n), B)
    Ad, inv = device_factor(ops, dev, A)
    X = B.to(dev).clone()
    ops.potrs_lower(Ad, inv, X)
    e_torch = column_error(torch.cholesky_solve(B, torch_factor(kind, n)), ref)
    check_forward("potrs %s n=%d nrhs=%d" % (kind, n, nrhs), column_error(X, ref), e_torch, n)


@pytest.mark.parametrize("nrhs", [1, 129])
def test_potrs_entrywise_one_row_behind_the_block(ops, dev, nrhs):
    """n = 2049: one full 2048 block and one row, so the forward and the backward carry have a single row.  The long-double factor
    costs ~8 s at this size, so the reference is fp64 cholesky_solve plus two steps of iterative refinement with long-double
    residuals (chol_ref.refine_solve; cond(A) = 1e3, good to ~1e-16), and of the 129 columns the reference is taken for eight --
    the first and last two, and both sides of the 16- and 64-wide sub-tile edges and of the 128-wide tile edge -- a long-double
    product with all of them would take 5 s; the columns of a solve are independent and n = 385 checks every one of 257.
    Every column is then compared with fp64 cholesky_solve: both lie within their errors of the solution, so they differ by at
    most (R + 1) max(e_torch, 64 n u) of the column's norm, e_torch the largest of the columns that have a reference."""
    n, kind = 2049, "p3"
    A = matrix(kind, n)[2]
    B = torch.randn(n, nrhs, generator=torch.Generator().manual_seed(nrhs), dtype=F64)
    cols = [0] if nrhs == 1 else [0, 1, 15, 16, 63, 64, 127, 128]
    ref = R.refine_solve(A.numpy(), B[:, cols].numpy())
    Ad, inv = device_factor(ops, dev, A)
    X = B.to(dev).clone()
    ops.potrs_lower(Ad, inv, X)
    Xt = torch.cholesky_solve(B, torch_factor(kind, n))
    e_torch = column_error(Xt[:, cols], ref)
    check_forward("potrs %s n=%d nrhs=%d" % (kind, n, nrhs), column_error(X.cpu()[:, cols], ref), e_torch, n)
    assert bool(torch.isfinite(X).all())
    apart = ((X.cpu() - Xt).abs().amax(dim=0) / Xt.abs().amax(dim=0)).max().item()
    print("FORWARD potrs %s n=%d nrhs=%d all columns against fp64 LAPACK: %.3e" % (kind, n, nrhs, apart))
    assert apart <= (RATIO + 1) * max(float(e_torch), 64 * n * U)


@pytest.mark.parametrize("wdt", [torch.bfloat16, torch.float32], ids=["bf16", "f64"])   # (fp32 is widened to fp64 by _as_weight)
@pytest.mark.parametrize("d", [1, 130])
@pytest.mark.parametrize("r", [1, 128, 129, 449])
def test_nystrom_down_entrywise(ops, dev, r, d, wdt):
    """down_f64 per entry relative to its column's largest entry, against the oracle's fp64 chain (O.nystrom_down); the floor of the
    criterion takes n = 640, the length of the sums of the cross product.  The bf16 output is the fp64 one transposed and rounded."""
    from oracle import modegpt_oracle as O
    n = 640
    gen = torch.Generator().manual_seed(100 * r + d)
    C = acts_cov(n)
    W = (torch.randn(d, n, generator=gen) * 0.05).to(wdt)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values
    out, f64 = ops.nystrom_down(C.to(dev), idx.to(dev), W.to(dev), eps=1e-6, want_f64=True)
    torch.cuda.synchronize()
    assert out.shape == (d, r) and f64.shape == (r, d)
    assert torch.equal(out.view(torch.int16), f64.T.to(torch.bfloat16).contiguous().view(torch.int16))
    ref = R.nystrom(C, idx.numpy(), W.double(), 1e-6)
    e_torch = column_error(O.nystrom_down(C, W, idx), ref)
    check_forward("nystrom_down r=%d d=%d %s" % (r, d, str(wdt)[6:]), column_error(f64, ref), e_torch, n)


# ---------------------------------------------------------------- overlapped against plain Nystrom
@pytest.mark.parametrize("n,r,d", [(640, 449, 130), (2304, 1613, 256)])
def test_nystrom_overlapped_is_bit_identical(ops, dev, monkeypatch, n, r, d):
    gen = torch.Generator().manual_seed(n + r)
    H = acts(gen, 2 * n, n).double().to(dev)
    C = H.T @ H / (2 * n)
    C = torch.tril(C) + torch.tril(C, -1).T
    W = (torch.randn(d, n, generator=gen) * 0.05).to(torch.bfloat16).to(dev)
    idx = torch.sort(torch.randperm(n, generator=gen)[:r]).values.to(dev)
    res = {}
    for overlap in (False, True, False, True):
        monkeypatch.setattr(ops, "NYSTROM_OVERLAP", overlap)
        out, f64 = ops.nystrom_down(C, idx, W, want_f64=True)
        torch.cuda.synchronize()
        if overlap in res:
            assert torch.equal(out, res[overlap][0]) and torch.equal(f64, res[overlap][1])    # each path repeats itself
        res[overlap] = (out, f64)
    assert bool(torch.isfinite(res[True][1]).all())
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])


# ---------------------------------------------------------------- pivot failures
N_PIVOT = 2100                           # 16 full blocks and a last one of 52 rows, identity-padded to 128 inside the kernel


@functools.lru_cache(maxsize=None)
def near_identity():
    noise = torch.randn(N_PIVOT, N_PIVOT, generator=torch.Generator().manual_seed(5), dtype=F64)
    return torch.eye(N_PIVOT, dtype=F64) + 0.01 * (noise + noise.T) / 2


def order_of(exc):
    m = re.search(r"leading minor of order (\d+) is not positive-definite", str(exc.value))
    assert m, str(exc.value)
    return int(m.group(1))


# 16-lane sub-block edges (15 | 16), 128 edges (127 | 128), the last pivot of the outer panel and the first one behind it (2048: the
# stand-alone diagonal kernel behind the lower-only update, never reached by look-ahead), the last row of the ragged last block
@pytest.mark.parametrize("p", [0, 15, 16, 127, 128, 2047, 2048, 2099])
def test_negative_pivot_is_reported_where_lapack_reports_it(ops, dev, p):
    A = near_identity().clone()
    A[p, p] = -1.0
    with pytest.raises(torch.linalg.LinAlgError) as cpu:
        torch.linalg.cholesky(A)
    with pytest.raises(torch.linalg.LinAlgError) as gpu:
        ops.potrf_lower(A.to(dev))
    assert order_of(gpu) == p + 1 == order_of(cpu)


@pytest.mark.parametrize("p", [2064])    # inside the ragged last block, on a 16-lane edge
def test_exact_zero_pivot(ops, dev, p):
    A = torch.diag(torch.linspace(1.0, 3.0, N_PIVOT, dtype=F64))
    A[p, :] = 0.0
    A[:, p] = 0.0
    with pytest.raises(torch.linalg.LinAlgError) as gpu:
        ops.potrf_lower(A.to(dev))
    assert order_of(gpu) == p + 1


@pytest.mark.parametrize("p", [300, 2050])    # a look-ahead block; the stand-alone kernel's ragged block
def test_nan_pivot(ops, dev, p):
    A = near_identity().clone()
    A[p, p] = float("nan")
    with pytest.raises(torch.linalg.LinAlgError) as gpu:
        ops.potrf_lower(A.to(dev))
    assert order_of(gpu) == p + 1


def test_first_of_two_failures_is_reported_also_deferred(ops, dev):
    A = near_identity().clone()
    A[2048, 2048] = -1.0
    A[300, 300] = -1.0
    with pytest.raises(torch.linalg.LinAlgError) as gpu:
        ops.potrf_lower(A.to(dev))
    assert order_of(gpu) == 301
    with ops.DeferredStatus(dev) as st:
        ops.potrf_lower(A.to(dev))                     # does not raise here
    with pytest.raises(torch.linalg.LinAlgError) as deferred:
        st.check()
    assert order_of(deferred) == 301
    good = near_identity().clone().to(dev)
    ops.potrf_lower(good)                              # and a good factorisation passes afterwards
    L = torch.linalg.cholesky(near_identity())
    assert float((torch.tril(good).cpu() - L).abs().max()) < 1e-13


def test_tiny_positive_pivot_is_not_a_failure(ops, dev):
    """Positive definite with smallest pivot 1e-300 (diagonal, so the pivot is the entry): no report, and l_pp = sqrt(1e-300)."""
    for p in (0, 130, 2099):
        d = torch.linspace(1.0, 3.0, N_PIVOT, dtype=F64)
        d[p] = 1e-300
        Ad = torch.diag(d).to(dev)
        ops.potrf_lower(Ad)
        got = torch.diagonal(Ad).cpu()
        # d * rsqrt(d): rsqrt within 1 ulp (2 u), the multiply and the reference's sqrt half an ulp each (u): 4 u, doubled
        assert float(((got - d.sqrt()).abs() / d.sqrt()).max()) <= 8 * U
