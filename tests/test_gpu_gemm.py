"""mdg_gemm_f64 mode by mode, through the C ABI directly (batch, batch strides, row gather, flags).

Two kinds of reference:
- exact operands: small integers (exact in bf16 too) with alpha in {1, 0.5, -2} and beta in {0, 1, -2}, so that every product
  and every partial sum is exact in fp64 whatever the accumulation order.  The result must then EQUAL the CPU product -- one
  wrong element, a missing or doubled k-slice, a misplaced tile or a clip one off fails.  (Values are compared with ==, so the
  sign of an exact zero is not asserted; everything outside the written region is compared bit for bit.)
- real operands: full 53-bit mantissas, mixed signs, column scales over several binades, checked entry by entry against a
  long-double reference: |C - C_ref|_ij <= 2 (K + 2) 2^-53 (|alpha| (|A| |B|)_ij + |beta| |C0|_ij).  A sum carried in
  reduced precision fails that where integer data cannot tell.

Every case runs on both staging paths: the vector path (16-byte aligned operands, leading dimensions a multiple of 8 elements,
k-ranges a multiple of 16) and the element-wise path (A's base one element off, an odd leading dimension).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F64, BF16 = torch.float64, torch.bfloat16
LOWER_ONLY, A_LOWER_TRI, B_LOWER_TRI, A_UPPER_TRI = 1, 2, 4, 8
TILE = 128
SENT = -12345.5          # what C holds outside the region a call may write (compared bit for bit afterwards)
ALPHA_BETA = [(1.0, 0.0), (0.5, 1.0), (-2.0, -2.0), (1.0, -2.0), (-2.0, 0.0), (0.5, 0.0)]


@pytest.fixture(scope="module")
def lib(dev):
    from modegpt_amd import _lib
    return _lib.load()


def _code(dt):
    from modegpt_amd import _lib
    return _lib.MDG_F64 if dt == F64 else _lib.MDG_BF16


def _bits(t):
    return t.view(torch.int64) if t.dtype == F64 else t.view(torch.int16)


def _ints(gen, n):
    return torch.randint(-8, 9, (n,), generator=gen).to(F64)


def gemm_call(lib, M, N, K, alpha, A, a_off, sa_i, sa_k, B, b_off, sb_k, sb_j, beta, Cbuf, c_off, ldc, rows=None,
              batch=1, a_bs=0, b_bs=0, c_bs=0, flags=0):
    """One mdg_gemm_f64 call on flat device buffers; *_off are element offsets of the operands' origins."""
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.mdg_gemm_f64(M, N, K, float(alpha), A.data_ptr() + a_off * A.element_size(), _code(A.dtype), sa_i, sa_k,
                          None if rows is None else rows.data_ptr(), B.data_ptr() + b_off * B.element_size(), _code(B.dtype),
                          sb_k, sb_j, float(beta), Cbuf.data_ptr() + c_off * Cbuf.element_size(), _code(Cbuf.dtype), ldc,
                          batch, a_bs, b_bs, c_bs, flags, C.c_void_p(stream))
    assert rc == 0, lib.mdg_last_error()
    torch.cuda.synchronize()


def strided(flat, off, bs, batch, rows, cols, s_r, s_c):
    """[batch, len(rows), len(cols)] view-by-index of a flat CPU tensor: element (b, i, j) at off + b bs + rows[i] s_r + cols[j] s_c."""
    b = torch.arange(batch).view(-1, 1, 1)
    idx = off + b * bs + rows.view(1, -1, 1) * s_r + cols.view(1, 1, -1) * s_c
    return flat[idx]


def c_index(c_off, c_bs, batch, M, N, ldc):
    return strided(torch.arange(c_off + (batch - 1) * c_bs + M * ldc + 1), c_off, c_bs, batch, torch.arange(M), torch.arange(N),
                   ldc, 1)


def written_mask(M, N, flags):
    """Which entries of C [M, N] the call writes: all of them, or with LOWER_ONLY the whole tiles on and below the diagonal."""
    ti, tj = torch.arange(M).view(-1, 1) // TILE, torch.arange(N).view(1, -1) // TILE
    return (ti >= tj) if flags & LOWER_ONLY else torch.ones(M, N, dtype=torch.bool)


class Operand:
    """op(X) of shape [rows, K] in one of the two layouts: k-contiguous (X[i * ld + k]) or x-contiguous (X[k * ld + i])."""

    def __init__(self, gen, n_x, K, kc, dtype, aligned, batch=1, bs=None, real=False, scale=None):
        ext = K if kc else n_x
        ld = (ext + 15) // 16 * 16 + 16 if aligned else (ext | 1) + 2
        self.ld = ld
        self.off = 0 if aligned else 1
        self.s_x, self.s_k = (ld, 1) if kc else (1, ld)
        span = (n_x if kc else K) * ld
        self.bs = span + (16 if aligned else 3) if bs is None else bs
        size = self.off + (batch - 1) * self.bs + span + 8
        if real:
            v = torch.randn(size, generator=gen, dtype=F64)
            v = v * torch.exp2(torch.randint(-6, 7, (size,), generator=gen).to(F64))   # spread over binades, mixed signs
            if scale is not None:                                                        # + a scale per row / column x
                xs = (torch.arange(size) - self.off) % max(self.bs, 1)
                x = (xs // ld) if kc else (xs % ld)
                v = v * scale[x.clamp(0, scale.numel() - 1)]
        else:
            v = _ints(gen, size)
        self.host = v.to(dtype).to(F64) if dtype == BF16 else v
        self.dtype, self.batch, self.n_x, self.K = dtype, batch, n_x, K

    def dev(self, device):
        return self.host.to(self.dtype).to(device)

    def op(self, rows=None):
        r = torch.arange(self.n_x) if rows is None else rows.cpu()
        return strided(self.host, self.off, self.bs, self.batch, r, torch.arange(self.K), self.s_x, self.s_k)


def run_exact(lib, dev, gen, M, N, K, adt, bdt, cdt, akc, bkc, aligned, alpha, beta, rows=None, n_rows_a=None, batch=1,
              b_bs=None, a_bs=None, flags=0, tweak=None, c_nan=None):
    """Build the operands, run the kernel, compare with the exact reference: the written region equal, the rest bit for bit."""
    A = Operand(gen, n_rows_a or M, K, akc, adt, aligned, batch, a_bs)
    B = Operand(gen, N, K, bkc, bdt, aligned, batch, b_bs)          # described as [j, k]: op(B) = its transpose
    if tweak is not None:
        tweak(A, B)                                               # place the NaNs of a triangle contract
    ldc = N + (4 if aligned else 3)
    c_bs = M * ldc + 5
    csize = (batch - 1) * c_bs + M * ldc + 2 * ldc
    c0 = torch.full((csize,), SENT, dtype=F64)
    ci = c_index(0, c_bs, batch, M, N, ldc)
    c0[ci] = _ints(gen, ci.numel()).view(ci.shape)
    if c_nan is not None:
        c0[ci] = float("nan")
    c0 = c0.to(cdt)
    Cd = c0.clone().to(dev)
    rows_d = None if rows is None else rows.to(dev)
    gemm_call(lib, M, N, K, alpha, A.dev(dev), A.off, A.s_x, A.s_k, B.dev(dev), B.off, B.s_k, B.s_x, beta, Cd, 0, ldc,
              rows_d, batch, A.bs, B.bs, c_bs, flags)
    opA = torch.nan_to_num(A.op(rows), nan=0.0)                    # (NaN marks an entry of the zero triangle the call never reads)
    opB = torch.nan_to_num(B.op(), nan=0.0).transpose(1, 2)
    prod = alpha * (opA @ opB)
    old = c0.to(F64)[ci]
    want = prod + beta * old if beta != 0 else prod
    wmask = written_mask(M, N, flags).expand(batch, M, N)
    got = Cd.cpu()
    exp = c0.clone()
    exp[ci[wmask]] = want[wmask].to(cdt)
    outside = torch.ones(csize, dtype=torch.bool)
    outside[ci[wmask]] = False
    assert torch.equal(_bits(got)[outside], _bits(exp)[outside]), "entries outside the written region changed"
    g, e = got[ci[wmask]].to(F64), exp[ci[wmask]].to(F64)
    bad = (g != e).nonzero()
    assert bad.numel() == 0, f"{bad.numel()} wrong of {g.numel()}: first at {bad[:4].flatten().tolist()} got {g[bad[:4]].flatten().tolist()} want {e[bad[:4]].flatten().tolist()}"


PAIRS = [(F64, F64), (F64, BF16), (BF16, F64), (BF16, BF16)]
SHAPES = [(1, 1, 1), (127, 129, 16), (128, 128, 128), (129, 257, 17), (257, 127, 129), (130, 200, 48), (256, 256, 15)]


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("akc,bkc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("adt,bdt", PAIRS, ids=["f64f64", "f64bf16", "bf16f64", "bf16bf16"])
@pytest.mark.parametrize("cdt", [F64, BF16], ids=["cf64", "cbf16"])
def test_exact_dtypes_layouts_shapes(lib, dev, adt, bdt, cdt, akc, bkc, aligned):
    gen = torch.Generator().manual_seed(PAIRS.index((adt, bdt)) * 8 + 4 * (cdt == F64) + 2 * akc + bkc + 100 * aligned)
    for s, (M, N, K) in enumerate(SHAPES):
        alpha, beta = ALPHA_BETA[s % len(ALPHA_BETA)]
        if cdt == BF16:
            beta = 0.0
        run_exact(lib, dev, gen, M, N, K, adt, bdt, cdt, akc, bkc, aligned, alpha, beta)


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("cdt", [F64, BF16], ids=["cf64", "cbf16"])
def test_beta_zero_ignores_garbage_in_c(lib, dev, cdt, aligned):
    """BLAS semantics: beta = 0 never reads C (the ops front ends write into torch.empty buffers) -- a NaN-filled C comes out exact."""
    gen = torch.Generator().manual_seed(3)
    for M, N, K in [(256, 256, 64), (129, 130, 33)]:
        run_exact(lib, dev, gen, M, N, K, F64, BF16, cdt, True, True, aligned, -2.0, 0.0, c_nan=True)
        run_exact(lib, dev, gen, M, N, K, BF16, F64, cdt, False, False, aligned, 0.5, 0.0, c_nan=True)


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("adt", [F64, BF16], ids=["af64", "abf16"])
@pytest.mark.parametrize("kind", ["sorted", "unsorted", "repeated"])
def test_row_gather(lib, dev, adt, kind, aligned):
    gen = torch.Generator().manual_seed(17)
    n_a = 700
    for M, N, K in [(300, 200, 64), (128, 130, 48), (1, 5, 16), (257, 64, 17)]:
        if kind == "sorted":
            rows = torch.randperm(n_a, generator=gen)[:M].sort().values
        elif kind == "unsorted":
            rows = torch.randperm(n_a, generator=gen)[:M]
        else:
            rows = torch.randint(0, n_a, (M,), generator=gen)
            rows[: M // 3] = rows[0]
        for bdt, bkc in [(BF16, True), (F64, False)]:
            run_exact(lib, dev, gen, M, N, K, adt, bdt, F64, True, bkc, aligned, 1.0, -2.0, rows=rows, n_rows_a=n_a)
        run_exact(lib, dev, gen, M, N, K, adt, BF16, BF16, True, True, aligned, -2.0, 0.0, rows=rows, n_rows_a=n_a)
        # an x-contiguous gathered A (always element-wise)
        run_exact(lib, dev, gen, M, N, K, adt, F64, F64, False, True, aligned, 0.5, 1.0, rows=rows, n_rows_a=n_a)


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("akc,bkc", [(True, True), (False, False), (True, False)])
def test_batched(lib, dev, akc, bkc, aligned):
    """batch = 3 with batch strides of their own, a broadcast B (b_bs = 0, as the VO products use it) and an odd A batch stride
    (which turns the vector path off for the whole call)."""
    gen = torch.Generator().manual_seed(23)
    for M, N, K in [(130, 257, 64), (256, 128, 48)]:
        run_exact(lib, dev, gen, M, N, K, F64, F64, F64, akc, bkc, aligned, 0.5, -2.0, batch=3)
        run_exact(lib, dev, gen, M, N, K, BF16, BF16, F64, akc, bkc, aligned, 1.0, 0.0, batch=3, b_bs=0)
        run_exact(lib, dev, gen, M, N, K, F64, BF16, BF16, akc, bkc, aligned, -2.0, 0.0, batch=3, b_bs=0)
        A_odd = Operand(gen, M, K, akc, F64, aligned, 1).bs + 1
        run_exact(lib, dev, gen, M, N, K, F64, F64, F64, akc, bkc, aligned, 1.0, 1.0, batch=3, a_bs=A_odd | 1)


# ---------------------------------------------------------------- triangle flags
def _nan_a(upper):
    """op(A)[i, k] for a triangle flag: the zero triangle is 0 inside the row tile's diagonal 128-block (those entries ARE read),
    NaN beyond it (never read: k >= i0 + 128 for A_LOWER_TRI, k < i0 for A_UPPER_TRI)."""
    def tweak(A, B):
        for b in range(A.batch):
            for i in range(A.n_x):
                i0 = i // TILE * TILE
                for k in range(A.K):
                    zero = (k < i) if upper else (k > i)
                    if not zero:
                        continue
                    never = (k < i0) if upper else (k >= i0 + TILE)
                    A.host[A.off + b * A.bs + i * A.s_x + k * A.s_k] = float("nan") if never else 0.0
    return tweak


def _nan_b(A, B):
    """op(B)[k, j] = 0 for k < j: 0 inside the column tile's diagonal block, NaN for k < j0."""
    for b in range(B.batch):
        for j in range(B.n_x):
            j0 = j // TILE * TILE
            for k in range(min(j, B.K)):
                B.host[B.off + b * B.bs + j * B.s_x + k * B.s_k] = float("nan") if k < j0 else 0.0


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
def test_lower_only(lib, dev, aligned):
    """LOWER_ONLY (M == N, the Cholesky trailing update at beta = 1): tiles strictly above the diagonal keep C bit for bit,
    tiles on the diagonal are written whole."""
    gen = torch.Generator().manual_seed(31)
    for n, K in [(300, 64), (256, 128), (129, 17), (1, 16)]:
        run_exact(lib, dev, gen, n, n, K, F64, F64, F64, True, True, aligned, -1.0, 1.0, flags=LOWER_ONLY)
        run_exact(lib, dev, gen, n, n, K, F64, F64, F64, True, False, aligned, 0.5, -2.0, flags=LOWER_ONLY)


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("flag", [A_LOWER_TRI, A_UPPER_TRI, B_LOWER_TRI], ids=["A_LOWER", "A_UPPER", "B_LOWER"])
def test_triangle_flags_clip_the_k_range(lib, dev, flag, aligned):
    """The unread part of the zero triangle holds NaN: the result is still exact only if the k-range is really clipped."""
    gen = torch.Generator().manual_seed(37)
    tweak = _nan_b if flag == B_LOWER_TRI else _nan_a(flag == A_UPPER_TRI)
    for M, N, K in [(300, 130, 300), (256, 256, 256), (130, 300, 300)]:
        if flag == B_LOWER_TRI:
            M, N = N, min(N, K)
        run_exact(lib, dev, gen, M, N, K, F64, F64, F64, True, True, aligned, 1.0, 1.0, flags=flag, tweak=tweak)
        run_exact(lib, dev, gen, M, N, K, F64, F64, F64, True, False, aligned, -1.0, 0.0, flags=flag, tweak=tweak)


@pytest.mark.parametrize("n", [450, 640])
def test_doubling_level_batched_triangular_pair(lib, dev, n):
    """The two batched calls of one level of the triangular inverse by doubling (chol.hip, tri_inverse_doubling), s = 128, with
    the ragged trailing pair of n = 450 (rows 384..449): T_p = L[R, Cb] X[Cb, Cb] (B_LOWER_TRI), X[R, Cb] = -X[R, R] T_p
    (A_LOWER_TRI), NaN in the upper triangles beyond the diagonal tiles."""
    gen = torch.Generator().manual_seed(n)
    s, ld = 128, n + 8
    L = torch.tril(_ints(gen, n * ld).view(n, ld)[:, :n])
    X = torch.tril(_ints(gen, n * ld).view(n, ld)[:, :n])
    for M_ in (L, X):
        for i in range(n):
            M_[i, (i // TILE + 1) * TILE:] = float("nan")   # beyond the diagonal tile: never read
    Lf = torch.zeros(n, ld, dtype=F64)
    Xf = torch.zeros(n, ld, dtype=F64)
    Lf[:, :n], Xf[:, :n] = L, X
    Ld, Xd = Lf.flatten().to(dev), Xf.flatten().to(dev)
    T = torch.full((s * s * 4 + 16,), float("nan"), dtype=F64, device=dev)
    full = n // (2 * s)
    r0_last = full * 2 * s + s
    Xw = Xf.clone()
    for p0, cnt, m in [(0, full, s), (full, 1 if r0_last < n else 0, n - r0_last)]:
        if cnt <= 0:
            continue
        c0 = p0 * 2 * s
        r0 = c0 + s
        psL, psX = 2 * s * ld + 2 * s, 2 * s * ld + 2 * s
        gemm_call(lib, m, s, s, 1.0, Ld, r0 * ld + c0, ld, 1, Xd, c0 * ld + c0, ld, 1, 0.0, T, 0, s, batch=cnt, a_bs=psL,
                  b_bs=psX, c_bs=s * s, flags=B_LOWER_TRI)
        gemm_call(lib, m, s, m, -1.0, Xd, r0 * ld + r0, ld, 1, T, 0, s, 1, 0.0, Xd, r0 * ld + c0, ld, batch=cnt, a_bs=psX,
                  b_bs=s * s, c_bs=psX, flags=A_LOWER_TRI)
        for p in range(cnt):
            cb, rb = c0 + p * 2 * s, r0 + p * 2 * s
            Tp = torch.nan_to_num(Lf[rb:rb + m, cb:cb + s]) @ torch.nan_to_num(Xf[cb:cb + s, cb:cb + s])
            Xw[rb:rb + m, cb:cb + s] = -(torch.nan_to_num(Xf[rb:rb + m, rb:rb + m]) @ Tp)
    got = Xd.cpu().view(n, ld)
    assert torch.equal(torch.nan_to_num(got, nan=7.5), torch.nan_to_num(Xw, nan=7.5)), "doubling level differs from the exact product"


# ---------------------------------------------------------------- real operands
@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "elementwise"])
@pytest.mark.parametrize("akc,bkc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("bdt", [F64, BF16], ids=["bf64", "bbf16"])
def test_real_operands_entrywise_bound(lib, dev, bdt, akc, bkc, aligned):
    """|C - C_ref|_ij <= c (K + 2) 2^-53 (|alpha| (|A||B|)_ij + |beta| |C0|_ij) with c = 2, C_ref in long double."""
    gen = torch.Generator().manual_seed(41 + akc + 2 * bkc)
    c = 2.0
    for M, N, K, alpha, beta in [(257, 129, 512, 0.7, -1.3), (128, 256, 1024, -1.0, 0.0), (130, 131, 129, 1.0, 1.0)]:
        scale = torch.exp2(torch.randint(-8, 9, (max(N, K) + 64,), generator=gen).to(F64))
        A = Operand(gen, M, K, akc, F64, aligned, real=True)
        B = Operand(gen, N, K, bkc, bdt, aligned, real=True, scale=scale)
        ldc = N + (4 if aligned else 3)
        c0 = torch.randn(M * ldc, generator=gen, dtype=F64) * 100.0
        Cd = c0.clone().to(dev)
        gemm_call(lib, M, N, K, alpha, A.dev(dev), A.off, A.s_x, A.s_k, B.dev(dev), B.off, B.s_k, B.s_x, beta, Cd, 0, ldc)
        a, b = A.op()[0].numpy(), B.op()[0].numpy().T
        old = c0.view(M, ldc)[:, :N].numpy()
        ref = np.longdouble(alpha) * (a.astype(np.longdouble) @ b.astype(np.longdouble)) + np.longdouble(beta) * old.astype(np.longdouble)
        got = Cd.cpu().view(M, ldc)[:, :N].numpy().astype(np.longdouble)
        bound = c * (K + 2) * 2.0 ** -53 * (abs(alpha) * (np.abs(a) @ np.abs(b)) + abs(beta) * np.abs(old))
        err = np.abs(got - ref).astype(np.float64)
        worst = (err / bound).max()
        assert worst <= 1.0, f"M={M} N={N} K={K}: error {worst:.3g} x the bound"


# ---------------------------------------------------------------- fp64 -> bf16 rounding of the shipped tensors
def _rounding_cases():
    """fp64 values at the edges of torch's double -> float -> bf16 rounding (common.hpp, f64_to_bf16)."""
    u = 2.0 ** -8                          # half a bf16 ulp at 1
    v = [1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 3 + 2 * u, 0.75 + u / 2,     # exact ties: to even below, to even above
         1 + u + 2 ** -40, 1 + 3 * u - 2 ** -40, -(1 + u + 2 ** -40),          # ties only after the rounding to fp32 ...
         1 + u + 2 ** -22, 1 + 3 * u - 2 ** -22,                               # ... and off the tie in fp32 too
         1 + u - 2 ** -52, 1 + u + 2 ** -52,
         3.3895313892515355e38, 3.39e38, 3.396e38, 3.3961e38, 3.4e38, -3.4e38,  # bf16 max .. fp32 max: max or inf
         3.4028234663852886e38, 3.4028235e38, 3.402823669209385e38, 1e39, -1e300, 1e308,   # fp32 max and beyond: inf
         1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -151, 2.0 ** -126, 2.0 ** -127 * 1.5,  # fp32 subnormals
         2.0 ** -130, 1e-39, 2.0 ** -133 + 2.0 ** -141, 9.18e-41, 1e-300, -1e-320,  # bf16 subnormals, below fp32's range
         0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan"), 1.0, -2.5]
    return torch.tensor(v, dtype=F64)


def _bf16_bits_equal(got, want):
    """Bit for bit, except that a NaN must come out as the kernel's one NaN, 0x7FC0 (torch's own CPU conversion gives 0x7FC0 or,
    on its vectorised path, 0xFFFF for a negative NaN)."""
    g, w = got.view(torch.int16), want.view(torch.int16)
    nan = torch.isnan(want.float())
    return torch.equal(g[~nan], w[~nan]) and bool((g[nan] == 0x7FC0).all())


def test_bf16_rounding_of_cast_transpose(dev):
    """ops.cast_transpose (writes every down_proj) bit for bit against torch's CPU .to(bfloat16): crafted edge values in a ragged
    matrix (rows, cols not multiples of 32) read through a leading dimension larger than its width."""
    from modegpt_amd import ops
    gen = torch.Generator().manual_seed(53)
    cases = _rounding_cases()
    for rows, cols, pad in [(37, 45, 3), (129, 70, 8), (1, 200, 1), (300, 1, 5)]:
        rnd = torch.randn(rows * cols, generator=gen, dtype=F64) * torch.exp2(torch.randint(-140, 128, (rows * cols,), generator=gen).to(F64))
        vals = rnd.clone()
        pos = torch.randperm(rows * cols, generator=gen)[:min(rows * cols, cases.numel())]
        vals[pos] = cases[:pos.numel()]
        buf = torch.full((rows, cols + pad), float("nan"), dtype=F64)
        buf[:, :cols] = vals.view(rows, cols)
        got = ops.cast_transpose(buf.to(dev)[:, :cols]).cpu()
        want = buf[:, :cols].T.contiguous().to(BF16)
        assert _bf16_bits_equal(got, want), (rows, cols, (got.view(torch.int16) != want.view(torch.int16)).nonzero()[:8].tolist())
    x = cases.view(-1, 1).repeat(1, 3)                 # every case through the kernel, in each of three columns
    assert _bf16_bits_equal(ops.cast_transpose(x.to(dev)).cpu(), x.T.contiguous().to(BF16))


def test_bf16_rounding_of_gemm_output(lib, dev):
    """The GEMM's bf16 epilogue: an [M, 1] column of the crafted values times a [1, 1] one, bit for bit against torch's rounding
    of the same fp64 products.  (Zeros are left out: the sum behind each element starts from +0, so a -0 product comes out +0
    as in any fp64 GEMM.)"""
    cases = _rounding_cases()
    cases = cases[(cases.abs() >= 2.0 ** -1022) | torch.isnan(cases)]     # (no zeros, no fp64 subnormals)
    for scale, alpha in [(1.0, 1.0), (0.5, 2.0), (-1.0, 1.0)]:
        a = cases.repeat(3)                            # two tile rows, the second ragged
        Ad, Bd = a.to(dev), torch.tensor([scale], dtype=F64, device=dev)
        Cd = torch.full((a.numel(), 2), float("nan"), dtype=BF16, device=dev)
        gemm_call(lib, a.numel(), 1, 1, alpha, Ad, 0, 1, 1, Bd, 0, 1, 1, 0.0, Cd, 0, 2)
        want = (alpha * (a * scale)).to(BF16)
        assert _bf16_bits_equal(Cd[:, 0].cpu().contiguous(), want), (scale, alpha)
        assert bool(torch.isnan(Cd[:, 1].float()).all().item())
