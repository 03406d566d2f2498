"""GPU: mdg_sym_pack_lower / mdg_sym_unpack_lower -- the packed lower-triangle storage of a finalized statistic (csrc/sympack.hip).

Everything is compared as int64 bit patterns: the kernels move raw 64-bit words, so random words (NaNs of every payload, infinities,
subnormals among them) are the test data.  Sizes sit on both sides of the 64-wide tile edge; every matrix lives in a buffer of a
sentinel pattern with pad columns (ld = n + 3) and, for batch 3, a gap between the matrices, all of which must survive."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F64, I64 = torch.float64, torch.int64
SENTINEL = 0x7FF8DEADBEEF1234          # (a NaN with a payload: also shows that pad words are not rewritten through arithmetic)
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 320]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def random_words(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    hi = torch.randint(-2 ** 31, 2 ** 31, shape, dtype=I64, device=dev, generator=g)
    lo = torch.randint(0, 2 ** 32, shape, dtype=I64, device=dev, generator=g)
    return (hi << 32) | lo


def symmetric_words(batch, n, seed, dev):
    w = random_words((batch, n, n), seed, dev)
    return torch.tril(w) + torch.tril(w, -1).transpose(1, 2)


def framed(batch, n, ld, gap, dev):
    """(buffer of sentinels as int64, its [batch, n, n] fp64 view with row stride ld and batch stride n * ld + gap)."""
    bs = n * ld + gap
    buf = torch.full((batch * bs + 5,), SENTINEL, dtype=I64, device=dev)
    return buf, buf.view(F64).as_strided((batch, n, n), (bs, ld, 1))


def layouts(n):
    return [(1, n, 0), (1, n + 3, 0), (3, n, 7), (3, n + 3, 7)]


@pytest.mark.parametrize("n", SIZES)
def test_pack_and_round_trip_are_exact(ops, dev, n):
    rows, cols = np.tril_indices(n)
    rows, cols = torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)
    for batch, ld, gap in layouts(n):
        A = symmetric_words(batch, n, 100 * n + ld + batch, dev)
        src_buf, src = framed(batch, n, ld, gap, dev)
        src.view(I64).copy_(A)
        before = src_buf.clone()
        view = src[0] if batch == 1 else src
        packed = ops.sym_pack_lower(view)
        assert packed.shape == ((n * (n + 1) // 2,) if batch == 1 else (batch, n * (n + 1) // 2))
        want = A[:, rows, cols]
        assert torch.equal(packed.view(I64).reshape(batch, -1), want), (n, batch, ld)
        assert torch.equal(src_buf, before), "pack wrote to its source"

        dst_buf, dst = framed(batch, n, ld, gap, dev)
        ops.sym_unpack_lower(packed, dst[0] if batch == 1 else dst)
        assert torch.equal(dst.view(I64), A), (n, batch, ld)                 # both triangles
        assert torch.equal(dst_buf, before), "pad columns / the gap between the matrices / the tail were written"


def test_special_values_round_trip_bit_for_bit(ops, dev):
    n = 65
    specials = torch.tensor([0x7FF8000000000001, 0x7FF800000000BEEF, 0x7FF0000000000001, -0x0008000000000000 + 5,  # quiet / signalling NaNs, a negative NaN
                             0x7FF0000000000000, -0x0010000000000000,                                                # +Inf, -Inf (0xFFF0...)
                             -0x8000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, -0x8000000000000000 + 1],    # -0.0, subnormals
                            dtype=I64, device=dev)
    idx = torch.arange(n * n, device=dev).reshape(n, n)
    A = specials[(idx * 7 + idx // n) % specials.numel()]
    A = torch.tril(A) + torch.tril(A, -1).T
    assert torch.isnan(A.view(F64)).any() and torch.isinf(A.view(F64)).any()
    full = A.view(F64).clone()
    packed = ops.sym_pack_lower(full)
    r, c = np.tril_indices(n)
    assert torch.equal(packed.view(I64), A[torch.from_numpy(r).to(dev), torch.from_numpy(c).to(dev)])
    back = torch.zeros(n, n, dtype=F64, device=dev)
    ops.sym_unpack_lower(packed, back)
    assert torch.equal(back.view(I64), A)


@pytest.mark.parametrize("n", [65, 320])
def test_only_the_lower_triangle_is_read(ops, dev, n):
    A = symmetric_words(1, n, 7, dev)[0]
    other = torch.tril(A) + torch.triu(random_words((n, n), 8, dev), 1)      # (what a not-yet-mirrored buffer looks like)
    assert not torch.equal(A, other)
    assert torch.equal(ops.sym_pack_lower(A.view(F64)).view(I64), ops.sym_pack_lower(other.view(F64)).view(I64))


def test_bad_arguments_raise(ops, dev):
    with pytest.raises(RuntimeError):
        ops.sym_pack_lower(torch.zeros(4, 4, dtype=F64))                    # CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.sym_pack_lower(torch.zeros(4, 5, dtype=F64, device=dev))
    with pytest.raises(ValueError):
        ops.sym_unpack_lower(torch.zeros(9, dtype=F64, device=dev), torch.zeros(4, 4, dtype=F64, device=dev))


# n = 23 296 (182 x 128): the FULL matrix is 4.34 GB -- rows from 23 046 on start beyond byte 2^32 of it -- and its packed triangle
# 2.17 GB.  n = 32 896 (257 x 128): the PACKED triangle is 4.33 GB, rows from 32 768 on start beyond byte 2^32 of it (and the full
# matrix is 8.66 GB).  A 32-bit offset on either side reads or writes the wrong row.
@pytest.mark.parametrize("n", [23296, 32896])
def test_offsets_beyond_4gib(ops, dev, n):
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 16 * 2 ** 30:
        pytest.skip("needs 16 GB of free device memory")
    assert n * n * 8 > 2 ** 32
    full = torch.empty(n, n, dtype=F64, device=dev)
    cols = torch.arange(n, device=dev, dtype=F64)
    for r0 in range(0, n, 2048):                                              # full[i][j] = i * 65537 + j (exact in fp64)
        r = torch.arange(r0, min(n, r0 + 2048), device=dev, dtype=F64)
        torch.add(r[:, None] * 65537.0, cols[None, :], out=full[r0:r0 + 2048])
    edge_full = 2 ** 32 // (8 * n)                                            # the row of the full matrix that straddles byte 2^32
    rows = {0, 1, edge_full, edge_full + 1, n - 1}
    if n * (n + 1) // 2 * 8 > 2 ** 32:
        edge_packed = next(r for r in range(32700, n) if (r + 1) * (r + 2) // 2 * 8 > 2 ** 32)   # row r straddles byte 2^32 of the packed triangle
        rows |= {edge_packed, edge_packed + 1}
    packed = ops.sym_pack_lower(full)
    for i in sorted(rows):
        got = packed[i * (i + 1) // 2: i * (i + 1) // 2 + i + 1]
        assert torch.equal(got, i * 65537.0 + cols[:i + 1]), f"packed row {i}"
    assert packed[-1].item() == (n - 1) * 65537.0 + (n - 1)
    full.zero_()
    ops.sym_unpack_lower(packed, full)
    for i in sorted(rows):
        want = torch.cat([i * 65537.0 + cols[:i + 1], cols[i + 1:] * 65537.0 + i])   # lower part of row i, then the mirror of column i
        assert torch.equal(full[i], want), f"row {i}"
        assert torch.equal(full[:, i], want), f"column {i}"
    del full, packed
    gc.collect()
    torch.cuda.empty_cache()
