"""GPU: the index kernels of modegpt_amd/csrc/select.hip -- mdg_select_smallest_sorted, mdg_select_margin, mdg_gather_rows_16,
mdg_cast_transpose_f64_bf16, mdg_qk_select -- against the plain references of tests/select_ref.py, through ops and through the raw
ABI.  Every assertion is equality of indices or of bits: the inputs are chosen so that no product or sum of a kernel rounds
differently under FMA contraction (stated where they are built).  Sizes sit on the kernels' block, tile and loop edges; buffers
carry guard entries; every index handed to a kernel is in range."""
import numpy as np
import pytest
import torch

from modegpt_amd import _lib
from tests import select_ref as S

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
GUARD = 64
ROPE_GROUPED, ROPE_MHA, OPT = _lib.MDG_QK_ROPE_GROUPED, _lib.MDG_QK_ROPE_MHA, _lib.MDG_QK_OPT


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(dev):
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def refused(lib, rc, name):
    return rc == _lib.MDG_ERR_BAD_ARG and name.encode() in lib.mdg_last_error()


# ---------------------------------------------------------------- mdg_select_smallest_sorted
SELECT_N = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097]
SELECT_KINDS = ["distinct", "equal", "four_values", "ascending", "descending", "special"]


def select_scores(kind, n):
    rng = np.random.default_rng(1000 * SELECT_KINDS.index(kind) + n)
    if kind == "distinct":
        s = rng.permutation(n) * 0.25 - 3.0 + rng.random() * 2.0 ** -10
    elif kind == "equal":
        s = np.full(n, 0.75)
    elif kind == "four_values":
        s = np.array([-1.5, 0.0, 2.0 ** -30, 7.0])[rng.integers(0, 4, n)]
    elif kind == "ascending":
        s = np.sort(rng.standard_normal(n))
    elif kind == "descending":
        s = np.sort(rng.standard_normal(n))[::-1].copy()
    else:
        pool = np.array([-0.0, 0.0, INF, -INF, 5e-324, -5e-324, 2.0 ** -1040, -2.0 ** -1040, 1.0, -1.0, 1e300])
        s = np.where(rng.random(n) < 0.5, pool[rng.integers(0, pool.size, n)], rng.standard_normal(n))
        s[rng.random(n) < 0.25] = NAN
    return np.ascontiguousarray(s, dtype=np.float64)


def select_ks(s):
    n = s.size
    ks = {1, n // 2, n - 1, n}
    live = int((~np.isnan(s)).sum())
    if live < n:                                  # the threshold element the last finite score, and a NaN itself
        ks |= {live, live + 1}
    return sorted(k for k in ks if 1 <= k <= n)


@pytest.mark.parametrize("kind", SELECT_KINDS)
@pytest.mark.parametrize("n", SELECT_N)
def test_select_smallest_sorted(ops, lib, dev, n, kind):
    """n on and around rank_threshold_kernel's blocks of 256 and LDS tiles of 1024 and compact_kernel's 1024 threads (per = 1, 2, 3, 5);
    k at both ends, in the middle and -- with NaN present -- at the last finite score and at the first NaN."""
    s = select_scores(kind, n)
    sd = torch.from_numpy(s).to(dev)
    for k in select_ks(s):
        want = torch.from_numpy(S.smallest_sorted(s, k))
        if kind == "equal":
            assert want.tolist() == list(range(k))
        got = ops.select_smallest_sorted(sd, k)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (n, k, kind)
        # raw ABI into a guarded buffer, twice
        runs = []
        for _ in range(2):
            buf = torch.full((k + GUARD,), -1, dtype=torch.int64, device=dev)
            assert lib.mdg_select_smallest_sorted(sd.data_ptr(), n, k, buf.data_ptr(), stream()) == _lib.MDG_OK
            runs.append(buf.cpu())
        assert torch.equal(runs[0][:k], want), (n, k, kind)
        assert bool((runs[0][k:] == -1).all()), (n, k, kind)
        assert torch.equal(runs[0], runs[1]), (n, k, kind)


def test_select_nothing(ops, lib, dev):
    """k == 0 is inside the header's contract (k >= 0): an empty selection, also when the index buffer of no entries is a null pointer
    (what torch hands out for an empty tensor)."""
    s = torch.rand(300, dtype=F64, device=dev)
    got = ops.select_smallest_sorted(s, 0)
    assert got.dtype == torch.int64 and got.numel() == 0
    buf = torch.full((GUARD,), -1, dtype=torch.int64, device=dev)
    assert lib.mdg_select_smallest_sorted(s.data_ptr(), 300, 0, buf.data_ptr(), stream()) == _lib.MDG_OK
    assert lib.mdg_select_smallest_sorted(s.data_ptr(), 300, 0, None, stream()) == _lib.MDG_OK
    assert bool((buf.cpu() == -1).all())
    # a null index buffer with something to write stays refused
    assert refused(lib, lib.mdg_select_smallest_sorted(s.data_ptr(), 300, 1, None, stream()), "mdg_select_smallest_sorted")


# ---------------------------------------------------------------- mdg_select_margin
MARGIN_EPS = 2.0 ** -20      # with integer sens in [0, 64], eps * sens is exact: s +- eps sens rounds once, contracted into an FMA or not


def margin_case(case, n, k):
    """(scores, sens, idx, certified or None): what the case is built to give whenever there is something to separate."""
    rng = np.random.default_rng(97 * n + 7 * k + len(case))
    s = rng.random(n)
    sens = rng.integers(0, 64, n).astype(np.float64)
    between = 0 < k < n
    if case == "certified":                         # unselected scores a whole unit above the selected: 1 >> 2 * 64 eps
        idx = S.smallest_sorted(s, k)
        rest = np.ones(n, dtype=bool)
        rest[idx] = False
        s[rest] += 1.0
        return s, sens, idx, 1.0
    if case == "flagged":                           # every score inside [0, 2^-16); the threshold pair carries 64 eps = 2^-14
        s *= 2.0 ** -16
        idx = S.smallest_sorted(s, k)
        if between:
            order = np.argsort(s, kind="stable")
            sens[order[k - 1]] = sens[order[k]] = 64.0
        return s, sens, idx, 0.0 if between else 1.0
    if case == "not_the_smallest":                  # ascending, but the k LARGEST
        idx = np.sort(np.argsort(s, kind="stable")[n - k:])
        return s, sens, idx, 0.0 if between else 1.0
    if case == "nan":                               # NaN on both sides, each carrying the largest sens there is
        nan = rng.random(n) < 0.2
        live = np.flatnonzero(~nan)
        take = min(k, live.size)
        chosen = live[np.argsort(s[live], kind="stable")[:take]]
        extra = np.flatnonzero(nan)[:k - take] if k > take else np.zeros(0, dtype=np.int64)
        swap = np.flatnonzero(nan)[-2:]             # and up to two NaN in place of finite selected scores
        swap = swap[~np.isin(swap, extra)][:max(0, min(2, take - 1))]
        chosen = chosen[:take - swap.size]
        idx = np.sort(np.concatenate((chosen, extra, swap))).astype(np.int64)
        s[nan] = NAN
        sens[nan] = 64.0
        assert idx.size == k and np.unique(idx).size == k
        return s, sens, idx, None
    assert case == "zero_sens"                      # distinct scores, no uncertainty: certified
    return s, np.zeros(n), S.smallest_sorted(s, k), 1.0


@pytest.mark.parametrize("case", ["certified", "flagged", "not_the_smallest", "nan", "zero_sens"])
@pytest.mark.parametrize("n", [1, 50, 1023, 1025, 3000])
def test_select_margin(ops, dev, n, case):
    """The raw eight numbers, bit for bit: n below, across and at three times the kernel's 1024 threads; k == 0 and k == n leave the
    sentinels of the empty side."""
    for k in sorted({0, 1, n // 2, n}):
        s, sens, idx, certified = margin_case(case, n, k)
        want = S.margin8(s, sens, idx, n, k, MARGIN_EPS)
        if certified is not None:
            assert want[7] == certified, (n, k, case)
        got = ops.select_margin(torch.from_numpy(s).to(dev), torch.from_numpy(sens).to(dev), torch.from_numpy(idx).to(dev), MARGIN_EPS)
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n, k, case, got.tolist(), want.tolist())


# ---------------------------------------------------------------- mdg_gather_rows_16
def random_bits16(shape, seed):
    """Every 16-bit pattern is fair: NaN payloads, infinities and subnormals of both 2-byte float types among them."""
    return torch.from_numpy(np.random.default_rng(seed).integers(-32768, 32768, shape, dtype=np.int16))


GATHER_SRC_ROWS = 37
GATHER_ROWS = [36, 36, 20, 5, 5, 0, 36, 1, 19, 20, 35, 0]      # duplicates, descending runs, the last row of the source


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n_cols", [1, 7, 8, 264, 2056, 2049])
def test_gather_rows(ops, dev, n_cols, dtype):
    bits = random_bits16((GATHER_SRC_ROWS, n_cols + 8), seed=n_cols)
    rows = torch.tensor(GATHER_ROWS, dtype=torch.int64)
    W = bits.to(dev).view(dtype)
    for lo in (0, 8):                                           # the whole matrix; a column slice: ld_src > n_cols
        src = W[:, lo:lo + n_cols] if lo else W[:, :n_cols].contiguous()
        got = ops.gather_rows(src, rows.to(dev))
        assert got.dtype == dtype and tuple(got.shape) == (rows.numel(), n_cols)
        assert torch.equal(got.view(torch.int16).cpu(), bits[:, lo:lo + n_cols][rows]), (n_cols, lo)
    empty = ops.gather_rows(W[:, :n_cols], rows[:0].to(dev))
    assert tuple(empty.shape) == (0, n_cols)


@pytest.mark.parametrize("n_cols,ld_src,ld_out,off_src,off_out", [
    (264, 272, 280, 0, 0),         # vector path, padded on both sides
    (264, 272, 280, 1, 0),         # source base off by one element: scalar path
    (264, 272, 280, 0, 1),         # destination base off by one element
    (264, 272, 280, 1, 1),
    (264, 267, 280, 0, 0),         # a leading dimension that is no multiple of 8
    (2056, 2064, 2072, 0, 0),      # the vector loop goes round twice
    (2056, 2064, 2072, 0, 1),      # ... and the scalar loop nine times
    (7, 9, 11, 0, 0),
    (1, 1, 3, 1, 0)])
def test_gather_rows_raw(lib, dev, n_cols, ld_src, ld_out, off_src, off_out):
    rows = torch.tensor(GATHER_ROWS, dtype=torch.int64)
    n_rows = rows.numel()
    src = random_bits16((off_src + GATHER_SRC_ROWS * ld_src,), seed=ld_src + off_src)
    sentinel = 0x5a5a
    want = torch.full((off_out + n_rows * ld_out + GUARD,), sentinel, dtype=torch.int16)
    src2d = src[off_src:].view(GATHER_SRC_ROWS, ld_src)
    want[off_out:off_out + n_rows * ld_out].view(n_rows, ld_out)[:, :n_cols] = src2d[rows, :n_cols]
    sd, rd = src.to(dev), rows.to(dev)
    out = torch.full_like(want, sentinel).to(dev)
    rc = lib.mdg_gather_rows_16(sd.data_ptr() + 2 * off_src, ld_src, rd.data_ptr(), n_rows, n_cols, out.data_ptr() + 2 * off_out, ld_out,
                                stream())
    assert rc == _lib.MDG_OK
    assert torch.equal(out.cpu(), want)            # the rows, and the pad columns and guard entries unchanged
    # no rows: OK and nothing written
    out = torch.full_like(want, sentinel).to(dev)
    rc = lib.mdg_gather_rows_16(sd.data_ptr() + 2 * off_src, ld_src, rd.data_ptr(), 0, n_cols, out.data_ptr() + 2 * off_out, ld_out,
                                stream())
    assert rc == _lib.MDG_OK and bool((out.cpu() == sentinel).all())


# ---------------------------------------------------------------- mdg_cast_transpose_f64_bf16
def cast_values(rows, cols, seed):
    """[rows, cols] fp64: random values over 60 binades with the special ones scattered among them (the first ones wherever the matrix
    is smaller than their number)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows * cols, generator=gen, dtype=F64) * 2.0 ** torch.randint(-30, 30, (rows * cols,), generator=gen).double()
    dr = S.double_rounding_set()
    ties = dr / (1.0 + 2.0 ** -40)
    assert torch.equal(ties.float().double(), ties)            # (the exact bf16 ties themselves, even and odd)
    special = torch.cat((dr, ties, torch.tensor([
        0.0, -0.0, INF, -INF, NAN, 1e39, -1e39, 3.5e38, -3.5e38, 3.4e38, -3.4e38, 3.3895313892515355e38,
        2.0 ** -133, -2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * (1 + 2.0 ** -30), 3 * 2.0 ** -134, 2.0 ** -135, 2.0 ** -150,
        2.0 ** -149, 1e-320, -1e-320, 2.0 ** -126, 2.0 ** -127], dtype=F64)))
    where = torch.randperm(rows * cols, generator=gen)[:special.numel()]
    x[where] = special[:where.numel()]
    return x.view(rows, cols)


def assert_bf16_bits(got_bits, want, what):
    want_bits = want.contiguous().view(torch.int16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got_bits.view(torch.bfloat16)), nan), what
    assert torch.equal(got_bits[~nan], want_bits[~nan]), what


@pytest.mark.parametrize("rows,cols", [(1, 1), (31, 33), (32, 32), (33, 31), (100, 257)])
def test_cast_transpose(ops, lib, dev, rows, cols):
    x = cast_values(rows, cols, seed=rows * cols)
    want = S.to_bf16_via_float(x).T.contiguous()
    big = torch.full((rows + 3, cols + 5), 7.0, dtype=F64)
    big[2:2 + rows, 3:3 + cols] = x
    xd = big.to(dev)[2:2 + rows, 3:3 + cols]                   # ld_in = cols + 5
    got = ops.cast_transpose(xd)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (cols, rows)
    assert_bf16_bits(got.cpu().view(torch.int16), want, (rows, cols))
    # raw ABI: ld_out > rows inside a sentinel-filled buffer
    ld_out, sentinel = rows + 5, 0x5a5a
    out = torch.full((cols * ld_out + GUARD,), sentinel, dtype=torch.int16, device=dev)
    rc = lib.mdg_cast_transpose_f64_bf16(xd.data_ptr(), rows, cols, xd.stride(0), out.data_ptr(), ld_out, stream())
    assert rc == _lib.MDG_OK
    out = out.cpu()
    body = out[:cols * ld_out].view(cols, ld_out)
    assert_bf16_bits(body[:, :rows].contiguous(), want, (rows, cols, "raw"))
    assert bool((body[:, rows:] == sentinel).all()) and bool((out[cols * ld_out:] == sentinel).all())


# ---------------------------------------------------------------- mdg_qk_select
N_KV = 3
# Rotary modes: C_jj + rho is an integer multiple of 2^-3 (q side) / 2^-1 (k side), so every product is an integer times 2^-4 and
# the sums over at most 8 query heads stay far below 2^53 of those: exact, contracted or not.  Distinct sums differ by >= 2^-4,
# which a square root keeps apart by many ulp, and equal sums give equal roots.  OPT: C_jj + rho is (m / 2)^2 resp. (m / 4)^2 -- the
# square roots are the exact m / 2, m / 4 and so is their product.
RIDGES = {ROPE_GROUPED: (2.0 ** -3, 2.0 ** -1), ROPE_MHA: (2.0 ** -3, 2.0 ** -1), OPT: (2.0 ** -2, 2.0 ** -4)}


def qk_diagonals(mode, n, hd, rng, which):
    """[n, hd] diagonal entries on the exact grid of `which` side ('q' / 'k'); about one in six is at or under -rho (clamped)."""
    if mode == OPT:
        m = rng.integers(0, 7, (n, hd)).astype(np.float64)
        d = (m * m - 1.0) / (4.0 if which == "q" else 16.0)
        low = np.array([-1.0, -0.5, -3.0])
    else:
        step = 2.0 ** -3 if which == "q" else 2.0 ** -1
        d = rng.integers(-1, 12 if which == "q" else 7, (n, hd)) * step
        low = np.array([-1.0, -2.5, -16.0])
    clamp = rng.random((n, hd)) < 1.0 / 6.0
    return np.where(clamp, low[rng.integers(0, 3, (n, hd))], d)


def qk_matrices(diag, rng):
    n, hd = diag.shape
    Cm = rng.standard_normal((n, hd, hd)) * 100.0               # the off-diagonal entries are not read
    i = np.arange(hd)
    Cm[:, i, i] = diag
    return Cm


def qk_inputs(mode, n_heads, hd, case, seed):
    rng = np.random.default_rng(seed)
    dq, dk = qk_diagonals(mode, n_heads, hd, rng, "q"), qk_diagonals(mode, N_KV, hd, rng, "k")
    ns, width = (hd, 1) if mode == OPT else (hd // 2, 2)
    if case == "equal":                                         # every score the same: identity order
        dq[:], dk[:] = 1.0, 0.5
    elif case == "clamped":                                     # a third of the units of every kv head score exactly 0, from
        low = np.array([-0.5, -1.0, -7.0, -2.0 ** 40])          # diagonals at and under -rho_k (every one <= -2^-1)
        for h in range(N_KV):
            units = rng.permutation(ns)[:max(1, ns // 3)]
            for u in units:
                dk[h, [u + p * (hd // 2) for p in range(width)]] = low[rng.integers(0, 4, width)]
    return qk_matrices(dq, rng), qk_matrices(dk, rng)


QK_SHAPES = ([(ROPE_GROUPED, hd, g) for hd in (2, 64, 256) for g in (4, 8)] + [(ROPE_MHA, hd, 1) for hd in (2, 128, 256)]
             + [(OPT, hd, 1) for hd in (2, 128)])


def run_qk(ops, dev, cq, ck, rank, mode):
    rq, rk = RIDGES[mode]
    mask, q_rows, k_rows = ops.qk_select(torch.from_numpy(cq).to(dev), torch.from_numpy(ck).to(dev), rank, mode, rq, rk)
    return mask.cpu().numpy(), q_rows.cpu().numpy(), k_rows.cpu().numpy()


@pytest.mark.parametrize("mode,hd,g", QK_SHAPES)
def test_qk_select_at_its_limits(ops, dev, mode, hd, g):
    n_heads = N_KV * g
    rq, rk = RIDGES[mode]
    ns = hd if mode == OPT else hd // 2
    for case in ("general", "equal", "clamped"):
        cq, ck = qk_inputs(mode, n_heads, hd, case, seed=1000 * mode + hd + g)
        if case == "clamped":
            zero = (S.qk_scores(cq, ck, n_heads, N_KV, hd, rq, rk, mode) == 0).sum(axis=1)
            assert bool((zero >= max(1, ns // 3)).all())
        for rank in sorted({1 if mode == OPT else 2, hd}):
            want = S.qk_select_ref(cq, ck, n_heads, N_KV, hd, rq, rk, rank, mode)
            got = run_qk(ops, dev, cq, ck, rank, mode)
            for name, a, b in zip(("mask", "q_rows", "k_rows"), got, want):
                assert a.dtype == np.int64 and np.array_equal(a, b), (case, rank, name)
            if case == "equal":
                take = rank if mode == OPT else rank // 2
                first = list(range(take)) if mode == OPT else list(range(take)) + [hd // 2 + j for j in range(take)]
                assert got[0].tolist() == [first] * N_KV


@pytest.mark.parametrize("mode,hd,g", QK_SHAPES)
def test_qk_select_nan_diagonal(ops, dev, mode, hd, g):
    """One NaN diagonal entry of sigma_k, in one unit of kv head 1: the unit's score is NaN, it ranks first there, and the other heads
    select what they selected without it."""
    n_heads = N_KV * g
    rq, rk = RIDGES[mode]
    ns = hd if mode == OPT else hd // 2
    cq, ck = qk_inputs(mode, n_heads, hd, "general", seed=77 * mode + hd + g)
    unit = (2 * ns) // 3
    for j in sorted({unit, unit if mode == OPT else unit + hd // 2}):          # either partner of a rotary pair
        bad = ck.copy()
        bad[1, j, j] = NAN
        for rank in sorted({1 if mode == OPT else 2, hd}):
            clean = run_qk(ops, dev, cq, ck, rank, mode)
            got = run_qk(ops, dev, cq, bad, rank, mode)
            want = S.qk_select_ref(cq, bad, n_heads, N_KV, hd, rq, rk, rank, mode)
            assert int(want[0][1, 0]) == unit
            for name, a, b in zip(("mask", "q_rows", "k_rows"), got, want):
                assert np.array_equal(a, b), (j, rank, name)
            assert np.array_equal(got[0][[0, 2]], clean[0][[0, 2]])
            # the certificate of that selection sees the same NaN score: head 1 is not certified, the other heads' rows keep their bits
            cert = [ops.qk_select_margin(torch.from_numpy(cq).to(dev), torch.from_numpy(k_).to(dev), rank, mode, rq, rk,
                                         torch.from_numpy(m_).to(dev), 0.0, 0.0).cpu() for k_, m_ in ((ck, clean[0]), (bad, got[0]))]
            assert cert[1][1, 7].item() == 0.0
            assert torch.equal(cert[0][[0, 2]].view(torch.int64), cert[1][[0, 2]].view(torch.int64))


# ---------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_on_the_host(lib, dev):
    """Bad sizes and modes come back as MDG_ERR_BAD_ARG with the entry's name in the message, before anything is launched: the
    outputs keep their sentinels."""
    n = 100
    s = torch.rand(n, dtype=F64, device=dev)
    sens = torch.ones(n, dtype=F64, device=dev)
    idx = torch.full((n + GUARD,), -1, dtype=torch.int64, device=dev)
    out8 = torch.full((8,), 3.0, dtype=F64, device=dev)
    st = stream()
    for k in (n + 1, -1):
        assert refused(lib, lib.mdg_select_smallest_sorted(s.data_ptr(), n, k, idx.data_ptr(), st), "mdg_select_smallest_sorted"), k
        assert refused(lib, lib.mdg_select_margin(s.data_ptr(), sens.data_ptr(), idx.data_ptr(), n, k, 1e-3, out8.data_ptr(), st),
                       "mdg_select_margin"), k
    assert refused(lib, lib.mdg_select_smallest_sorted(s.data_ptr(), 0, 0, idx.data_ptr(), st), "mdg_select_smallest_sorted")
    assert refused(lib, lib.mdg_select_margin(s.data_ptr(), sens.data_ptr(), idx.data_ptr(), n, 5, -1e-3, out8.data_ptr(), st),
                   "mdg_select_margin")
    assert bool((idx.cpu() == -1).all()) and bool((out8.cpu() == 3.0).all())

    src = torch.zeros(8 * 16, dtype=torch.int16, device=dev)
    rows = torch.zeros(4, dtype=torch.int64, device=dev)
    dst = torch.full((4 * 16 + GUARD,), 0x5a5a, dtype=torch.int16, device=dev)
    for ld_src, ld_out, n_cols, n_rows in ((15, 16, 16, 4), (16, 15, 16, 4), (16, 16, 0, 4), (16, 16, 16, -1)):
        rc = lib.mdg_gather_rows_16(src.data_ptr(), ld_src, rows.data_ptr(), n_rows, n_cols, dst.data_ptr(), ld_out, st)
        assert refused(lib, rc, "mdg_gather_rows_16"), (ld_src, ld_out, n_cols, n_rows)
    assert bool((dst.cpu() == 0x5a5a).all())

    x = torch.ones(8, 16, dtype=F64, device=dev)
    t = torch.full((16 * 8 + GUARD,), 0x5a5a, dtype=torch.int16, device=dev)
    for rws, cls, ld_in, ld_out in ((8, 16, 15, 8), (8, 16, 16, 7), (0, 16, 16, 8), (8, 0, 16, 8)):
        rc = lib.mdg_cast_transpose_f64_bf16(x.data_ptr(), rws, cls, ld_in, t.data_ptr(), ld_out, st)
        assert refused(lib, rc, "mdg_cast_transpose_f64_bf16"), (rws, cls, ld_in, ld_out)
    assert bool((t.cpu() == 0x5a5a).all())

    hd = 256
    cq = torch.zeros(8, hd, hd, dtype=F64, device=dev)
    ck = torch.zeros(4, hd, hd, dtype=F64, device=dev)
    mask = torch.full((4 * hd,), -1, dtype=torch.int64, device=dev)
    q_rows = torch.full((8 * hd,), -1, dtype=torch.int64, device=dev)
    k_rows = torch.full((4 * hd,), -1, dtype=torch.int64, device=dev)

    def qk(n_heads, n_kv, hd_, rank, mode):
        return lib.mdg_qk_select(cq.data_ptr(), ck.data_ptr(), n_heads, n_kv, hd_, 1e-4, 1e-4, rank, mode, mask.data_ptr(),
                                 q_rows.data_ptr(), k_rows.data_ptr(), st)
    for what, args in [("odd rank, grouped", (8, 4, 64, 33, ROPE_GROUPED)), ("odd rank, MHA", (4, 4, 64, 33, ROPE_MHA)),
                       ("odd head_dim, rotary", (4, 4, 63, 32, ROPE_MHA)), ("hd = 256 in OPT mode", (4, 4, 256, 64, OPT)),
                       ("n_heads % n_kv", (7, 4, 64, 32, ROPE_GROUPED)), ("n_heads < n_kv", (2, 4, 64, 32, ROPE_GROUPED)),
                       ("grouped heads in MHA mode", (8, 4, 64, 32, ROPE_MHA)), ("grouped heads in OPT mode", (8, 4, 64, 32, OPT)),
                       ("rank > hd", (4, 4, 64, 66, ROPE_MHA)), ("rank 0", (4, 4, 64, 0, OPT)), ("hd > 256", (4, 4, 258, 64, ROPE_MHA)),
                       ("unknown mode", (4, 4, 64, 32, 3))]:
        assert refused(lib, qk(*args), "mdg_qk_select"), what
    for t_ in (mask, q_rows, k_rows):
        assert bool((t_.cpu() == -1).all())
    # and the same buffers with legal arguments are accepted
    assert qk(8, 4, 256, 256, ROPE_GROUPED) == _lib.MDG_OK
    torch.cuda.synchronize()
