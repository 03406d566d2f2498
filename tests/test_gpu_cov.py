"""The fp64 covariance family of csrc/cov.hip (mdg_cov_accum, mdg_cov_accum_multi, mdg_cov_finalize, mdg_bi_accum) against the
references of tests/cov_ref.py (checked on the CPU by test_cov_ref_host.py, which also pins the split / no-split path of every shape
used here to the library's own workspace query).

EXACT comparisons.  Data of cov_ref.exact_inputs lies on a lattice on which no fp64 addition or fused multiply-add can round
(cov_ref.exact_cov's docstring), so the kernel's result is determined whatever its order of summation, its split over tokens or the
grouping inside a matrix instruction: every such test is torch.equal on values against exact_cov, entry by entry, no tolerance.  A
dropped, duplicated or misplaced token or column changes an integer and fails.

ROUNDING bounds (sections "rounding" and "bi: generic data") are a-priori, not measured.  A sum of `tokens` exact products in any
order is off by at most gamma_{tokens-1} sum_t |x_ti x_tj| <= tokens 2^-53 sqrt(sigma_ii sigma_jj) (Higham, Accuracy and Stability,
eq. 4.4, and Cauchy-Schwarz) -- the figure include/modegpt_hip.h quotes at mdg_ridge_scores.  bf16, fp16 and fp32 products are exact
in fp64; an fp64 product rounds once more, which makes it (tokens + 1) 2^-53 sum_t |x_ti x_tj|.  Every such test prints its largest
fraction of the bound before it asserts (pytest -s: lines ROUNDING, BI).

What the tests pin beyond the arithmetic (and include/modegpt_hip.h now states): mdg_cov_accum accumulates the 128 x 128 tiles on
the diagonal whole and neither reads nor writes the tiles strictly above it; its ReLU counts NaN, -Inf and -0.0 as 0; the problems of
one mdg_cov_accum_multi call may differ in their token counts.
"""
import functools

import numpy as np
import pytest
import torch

from modegpt_amd import _lib
from tests import cov_ref as R
from tests.test_gpu_chol import SENTINELS, bits, same_bits
from tests.test_gpu_kernels import acts

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -53
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16, F32, F64]
CODE = {BF16: _lib.MDG_BF16, F16: _lib.MDG_F16, F32: _lib.MDG_F32, F64: _lib.MDG_F64}
NAME = {BF16: "bf16", F16: "f16", F32: "f32", F64: "f64"}
JUNK = 77.0                                 # what lies beside a strided view: reading it would change an exact result
EDGE_TOKENS = list(range(1, 51)) + [63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128, 129, 254, 255]
FEW_TOKENS = [1, 17, 33, 65, 113]
SPLIT_TOKENS = [256, 257, 300, 1153, 1160, 4099]
RELU_TOKENS = [1, 16, 17, 48, 49, 255, 300]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def ws_bytes(tokens, n_feat, batch=1):
    return _lib.load().mdg_cov_accum_ws_bytes(tokens, n_feat, batch)


def plan(tokens, n_feat, batch=1):
    return R.split_plan(ws_bytes(tokens, n_feat, batch), tokens, n_feat, batch)


@functools.lru_cache(maxsize=None)
def exact_x(tokens, width, dtype, seed=0):
    return R.exact_inputs(tokens, width, dtype, seed)


def on_device(x, dev, path):
    """fast: a contiguous copy.  generic: the same data as columns [3, 3 + width) of a buffer 8 columns wider (a misaligned view:
    element-wise staging).  aligned<W>: columns [0, width) of a buffer W wide (16-byte aligned rows, vector staging allowed)."""
    if path == "fast":
        return x.to(dev)
    t, w = x.shape
    wide, c0 = (w + 8, 3) if path == "generic" else (int(path[7:]), 0)
    buf = torch.full((t, wide), JUNK, dtype=x.dtype, device=dev)
    buf[:, c0:c0 + w] = x.to(dev)
    return buf[:, c0:c0 + w]


def cov(ops, xd, heads=1, relu=False, sigma=None):
    feat = xd.shape[1] // heads
    if sigma is None:
        sigma = torch.zeros(heads, feat, feat, dtype=F64, device=xd.device)
    ops.cov_accum(sigma, xd, n_heads=heads, relu=relu)
    return sigma


def assert_lower_exact(got, want, what):
    g, w = torch.tril(got.cpu().reshape(want.shape)), torch.tril(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError("%s: %d entries of the lower triangle differ, first at %s: got %r, want %r" % (
            what, len(bad), at, g[at].item(), w[at].item()))


# ---------------------------------------------------------------- 1. pipeline edges, unsplit
@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("n_feat", [128, 256])
def test_pipeline_edges_unsplit(ops, dev, n_feat, path):
    """Every stage count at which cov_tile's prologue, steady loop (entered from 4 full stages) and two tails change, and every
    remainder of the 16-token stage next to them, in one workgroup per tile: each token count is a prefix of one data set."""
    for dtype in DTYPES:
        full = exact_x(255, n_feat, dtype)
        xd = on_device(full, dev, path)
        for t in (EDGE_TOKENS if dtype in (BF16, F32) else FEW_TOKENS):
            assert ws_bytes(t, n_feat) == 0
            assert_lower_exact(cov(ops, xd[:t]), R.exact_cov(full[:t]), "%s %d tokens" % (NAME[dtype], t))


# ---------------------------------------------------------------- 2. split edges
@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("n_feat", [128, 256])
def test_split_edges(ops, dev, n_feat, path):
    """Split over tokens, with a last part of 128, 1 (no full stage, one token), 8 and other lengths."""
    assert plan(1153, n_feat)[2] == 1 and plan(1160, n_feat)[2] == 8
    for dtype in (BF16, F32):
        full = exact_x(4099, n_feat, dtype)
        xd = on_device(full, dev, path)
        for t in SPLIT_TOKENS:
            ks, tps, last = plan(t, n_feat)
            assert ks > 1
            print("SPLIT n_feat=%d tokens=%d: %d splits of %d tokens, the last of %d" % (n_feat, t, ks, tps, last))
            assert_lower_exact(cov(ops, xd[:t]), R.exact_cov(full[:t]), "%s %d tokens" % (NAME[dtype], t))


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("tokens,feat,heads", [(515, 128, 3), (2048, 64, 4)])
def test_split_heads(ops, dev, dtype, tokens, feat, heads):
    assert plan(tokens, feat, heads)[0] > 1
    x = exact_x(tokens, feat * heads, dtype)
    assert_lower_exact(cov(ops, x.to(dev), heads), R.exact_cov(x, heads), "heads")


# ---------------------------------------------------------------- 3. ragged and unaligned staging
@pytest.mark.parametrize("tokens", [200, 333])
def test_ragged_widths(ops, dev, tokens):
    """Feature counts that are no multiple of the tile, of the 16-byte chunk, or of anything; 200 tokens in one part, 333 split."""
    for n_feat in (1, 2, 7, 16, 127, 129, 131, 200, 300):
        assert (plan(tokens, n_feat)[0] > 1) == (tokens == 333)
        for dtype in DTYPES:
            x = exact_x(tokens, n_feat, dtype)
            assert_lower_exact(cov(ops, x.to(dev)), R.exact_cov(x), "%s n_feat %d" % (NAME[dtype], n_feat))


@pytest.mark.parametrize("tokens", [200, 333])
@pytest.mark.parametrize("n_feat,wide", [(131, 320), (300, 512)])
def test_aligned_view_with_a_straddling_chunk(ops, dev, n_feat, wide, tokens):
    """x[:, 0:n_feat] of a wider buffer: rows are 16-byte aligned, so full chunks load as vectors, and the last chunk of every row
    crosses the end of the view (into JUNK) and must be staged element by element (131: every type; 300: the 2-byte types)."""
    for dtype in DTYPES:
        x = exact_x(tokens, n_feat, dtype)
        xd = on_device(x, dev, "aligned%d" % wide)
        assert xd.data_ptr() % 16 == 0 and (xd.stride(0) * xd.element_size()) % 16 == 0
        assert (n_feat * xd.element_size()) % 16 != 0 or (n_feat, dtype) in [(300, F32), (300, F64)]     # 300 = 75 x 4 elements
        assert_lower_exact(cov(ops, xd), R.exact_cov(x), NAME[dtype])


@pytest.mark.parametrize("tokens", [200, 333])
@pytest.mark.parametrize("heads,feat,dtypes", [(3, 20, [BF16]), (3, 200, [BF16, F64]), (2, 64, DTYPES)], ids=["3x20", "3x200", "2x64"])
def test_ragged_heads(ops, dev, heads, feat, dtypes, tokens):
    """Heads narrower than, and no multiple of, the tile: every head's tile ends inside its neighbour's columns, which hold other
    data.  3 x 20 in bf16 is 40 bytes a head: no head but the first starts on a 16-byte boundary, so no vector load is allowed."""
    assert (plan(tokens, feat, heads)[0] > 1) == (tokens == 333)
    for dtype in dtypes:
        x = exact_x(tokens, heads * feat, dtype)
        want = R.exact_cov(x, heads)
        assert not torch.equal(want[0], want[1])
        assert_lower_exact(cov(ops, x.to(dev), heads), want, NAME[dtype])


# ---------------------------------------------------------------- 4. ReLU
@pytest.mark.parametrize("path", ["fast", "generic"])
@pytest.mark.parametrize("n_feat", [128, 256])
def test_relu(ops, dev, n_feat, path):
    for dtype in DTYPES:
        full = exact_x(300, n_feat, dtype)
        assert bool((full < 0).any()) and bool(((full == 0) & torch.signbit(full)).any())
        xd = on_device(full, dev, path)
        for t in RELU_TOKENS:
            want = R.exact_cov(full[:t], relu=True)
            assert_lower_exact(cov(ops, xd[:t], relu=True), want, "%s %d tokens" % (NAME[dtype], t))
        assert not torch.equal(want, R.exact_cov(full, relu=False))


# ---------------------------------------------------------------- 5. accumulation and sigma's layout
def padded_sigma(batch, n, ld, bs, fill, dev, init=None):
    """`batch` n x n matrices with leading dimension ld, bs elements apart, inside a flat buffer of `fill` -> (buffer, view)."""
    buf = torch.full(((batch - 1) * bs + (n - 1) * ld + n + 11,), fill, dtype=F64, device=dev)
    view = buf.as_strided((batch, n, n), (bs, ld, 1))
    if init is None:
        view.zero_()
    else:
        view.copy_(init.to(dev))
    return buf, view


def outside_unchanged(buf, before, batch, n, ld, bs):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside.as_strided((batch, n, n), (bs, ld, 1)).fill_(True)
    return torch.equal(bits(buf)[~inside], bits(before)[~inside])


def direct_cov(xd, n_feat, batch, sigma_ptr, ld_sigma, bs, relu=0):
    lib = _lib.load()
    tokens = xd.shape[0]
    nbytes = lib.mdg_cov_accum_ws_bytes(tokens, n_feat, batch)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xd.device)
    _lib.check(lib.mdg_cov_accum(xd.data_ptr(), CODE[xd.dtype], tokens, n_feat, batch, xd.stride(0), relu, sigma_ptr, ld_sigma, bs,
                                 ws.data_ptr() if nbytes else None, nbytes, stream()), "mdg_cov_accum")
    return ws


@pytest.mark.parametrize("heads,feat", [(1, 256), (3, 200)])
def test_accumulates_onto_an_earlier_result(ops, dev, heads, feat):
    """Three calls (unsplit, split, one token) onto one sigma == the concatenated tokens."""
    x = exact_x(100 + 300 + 1, heads * feat, BF16)
    xd = x.to(dev)
    sigma = cov(ops, xd[:100], heads)
    first = R.exact_cov(x[:100], heads)
    assert_lower_exact(sigma, first, "first call")
    cov(ops, xd[100:400], heads, sigma=sigma)
    assert_lower_exact(sigma, R.exact_cov(x[100:400], heads, sigma0=first), "second call")
    cov(ops, xd[400:], heads, sigma=sigma)
    assert_lower_exact(sigma, R.exact_cov(x, heads), "all tokens")


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("tokens", [200, 333])
@pytest.mark.parametrize("feat", [128, 200])
def test_padded_sigma_layout(ops, dev, feat, tokens, fill):
    """ld_sigma = n_feat + 37, batch stride n_feat * ld_sigma + 5: the lower triangles of the contiguous call bit for bit, and
    nothing outside the matrices changes."""
    heads, ld = 3, feat + 37
    bs = feat * ld + 5
    x = exact_x(tokens, heads * feat, F32)
    xd = x.to(dev)
    contig = cov(ops, xd, heads)
    assert_lower_exact(contig, R.exact_cov(x, heads), "contiguous")
    buf, view = padded_sigma(heads, feat, ld, bs, fill, dev)
    before = buf.clone()
    ws = direct_cov(xd, feat, heads, buf.data_ptr(), ld, bs)
    assert same_bits(torch.tril(view), torch.tril(contig))
    assert outside_unchanged(buf, before, heads, feat, ld, bs)
    del ws


@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("tokens", [200, 333])
def test_above_the_diagonal(ops, dev, tokens, fill):
    """What mdg_cov_accum does above the diagonal (n_feat 384: three diagonal tiles, three below, three above).  The 128 x 128 tiles
    strictly above the diagonal are neither read nor written.  The diagonal tiles are accumulated whole: their entries above the
    diagonal receive the same sum as their mirror images (onto whatever they held).  The lower triangle never depends on any of it,
    and mdg_cov_finalize rebuilds everything above the diagonal from below."""
    n = 384
    x = exact_x(tokens, n, BF16)
    want = R.exact_cov(x)[0]
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    blk = torch.arange(n) // R.TILE
    above_tiles = blk[:, None] < blk[None, :]
    start = torch.zeros(n, n, dtype=F64)
    start[upper] = fill
    sigma = start.clone().to(dev)
    cov(ops, x.to(dev), sigma=sigma)
    got = sigma.cpu()
    assert_lower_exact(got, want, "lower triangle")
    assert torch.equal(bits(got)[above_tiles], bits(start)[above_tiles]), "a tile strictly above the diagonal was written"
    in_diag = upper & ~above_tiles
    assert same_bits(got[in_diag], (start + want)[in_diag]), "diagonal tiles are accumulated whole"
    ops.cov_finalize(sigma, 0.5)
    fin = sigma.cpu()
    assert bool(torch.isfinite(fin).all()) and torch.equal(fin, fin.T)
    assert torch.equal(fin, 0.5 * want)


# ---------------------------------------------------------------- 6. no tokens
@pytest.mark.parametrize("fill", SENTINELS)
def test_no_tokens(dev, fill):
    sigma = torch.full((2, 128, 128), fill, dtype=F64, device=dev)
    before = sigma.clone()
    rc = _lib.load().mdg_cov_accum(None, _lib.MDG_BF16, 0, 128, 2, 256, 0, sigma.data_ptr(), 128, 128 * 128, None, 0, stream())
    assert rc == _lib.MDG_OK
    assert same_bits(sigma, before)


# ---------------------------------------------------------------- 7. element conversion
LAYOUT = {BF16: (np.uint16, 16, 7), F16: (np.uint16, 16, 10), F32: (np.uint32, 32, 23), F64: (np.uint64, 64, 52)}


def pattern_row(dtype, width, seed):
    """One row of `dtype` from bit patterns: smallest / largest subnormal, smallest / largest normal, +-1, +-0, then random finite
    patterns of every exponent."""
    utype, nbits, mant = LAYOUT[dtype]
    sign, ones = 1 << (nbits - 1), (1 << (nbits - 1 - mant)) - 1
    full = (1 << mant) - 1
    one = (ones >> 1) << mant
    pats = [1, full, 1 << mant, ((ones - 1) << mant) | full, one, one | sign, 0, sign]
    rng = np.random.default_rng([seed, nbits, mant])
    while len(pats) < width:
        pats.append((int(rng.integers(0, 2)) * sign) | (int(rng.integers(0, ones)) << mant) | int(rng.integers(0, full + 1)))
    signed = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}[utype]
    raw = torch.from_numpy(np.array(pats, dtype=utype).view(signed))
    return raw.view(dtype).reshape(1, width)


@pytest.mark.parametrize("width", [128, 130], ids=["128-fast", "130-generic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_element_conversion(ops, dev, dtype, width):
    """One token: sigma_ij = 0 + x_i x_j, a single product -- exact in fp64 for bf16, fp16 and fp32 elements, rounded once for fp64
    ones (overflow to Inf and underflow through the subnormals included) -- so the widening of every kind of element shows bit for
    bit.  The reference is numpy's outer product added to +0, as the kernel adds it to a zeroed sigma (which turns a -0 product
    into +0)."""
    row = pattern_row(dtype, width, seed=7)
    v = row.double().numpy()[0]
    assert np.all(np.isfinite(v)) and np.count_nonzero(v == 0) == 2
    with np.errstate(over="ignore", under="ignore"):
        want = torch.from_numpy(0.0 + np.outer(v, v))
    got = cov(ops, row.to(dev))[0]
    assert same_bits(torch.tril(got.cpu()), torch.tril(want))


# ---------------------------------------------------------------- 8. non-finite input
def klass(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    return torch.isposinf(a) * 1 + torch.isneginf(a) * 2 + torch.isnan(a) * 3


def column_hit(n, j):
    hit = torch.zeros(n, n, dtype=torch.bool)
    hit[j, :] = True
    hit[:, j] = True
    return hit


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("tokens", [40, 300])
def test_nonfinite_stays_in_its_row_and_column(ops, dev, tokens, dtype):
    n, j = 256, 131
    low = torch.tril(torch.ones(n, n, dtype=torch.bool))
    hit = column_hit(n, j)
    base = exact_x(tokens, n, dtype)
    zeroed = base.clone()
    t1, t2 = tokens // 3, tokens - 2
    zeroed[t1, j] = 0
    zeroed[t2, j] = 0
    clean = R.exact_cov(zeroed)[0]
    for what, values in [("nan", (float("nan"), None)), ("+inf", (float("inf"), None)), ("+inf/-inf", (float("inf"), float("-inf")))]:
        x = zeroed.clone()
        x[t1, j] = values[0]
        if values[1] is not None:
            x[t2, j] = values[1]
        got = cov(ops, x.to(dev))[0].cpu()
        assert torch.equal(got[low & ~hit], clean[low & ~hit]), what + ": an entry outside row and column j changed"
        v = x.double()
        col = (v * v[:, j:j + 1]).sum(dim=0)                   # sigma[:, j] as an fp64 sum of products; its class has no order
        if what == "nan":
            assert bool(torch.isnan(got[low & hit]).all())
            assert bool(torch.isnan(col).all())
        else:
            assert bool((klass(col) != 0).all())
            assert torch.equal(klass(got[j, :j + 1]), klass(col[:j + 1])), what + ": row j"
            assert torch.equal(klass(got[j:, j]), klass(col[j:])), what + ": column j"
            assert len(set(klass(col).tolist())) >= 2


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
@pytest.mark.parametrize("tokens", [40, 300])
def test_relu_counts_nan_and_negative_infinity_as_zero(ops, dev, tokens, dtype):
    """relu != 0 is (v > 0 ? v : 0): NaN, -Inf and -0.0 become 0 (include/modegpt_hip.h says so at MDG_I8_RELU, whose fallback this
    route is), so the result is the exact one of the data with those elements zeroed."""
    n = 256
    base = exact_x(tokens, n, dtype)
    x, zeroed = base.clone(), base.clone()
    for k, (t, j) in enumerate([(0, 0), (tokens // 2, 131), (tokens - 1, 255), (tokens // 3, 64), (tokens - 3, 7), (1, 200)]):
        x[t, j] = [float("nan"), float("-inf"), -0.0][k % 3]
        zeroed[t, j] = 0
    want = R.exact_cov(zeroed, relu=True)
    got = cov(ops, x.to(dev), relu=True)
    assert bool(torch.isfinite(got).all())
    assert_lower_exact(got, want, "relu")


# ---------------------------------------------------------------- 9. rounding, non-integer data
@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("n_feat", [256, 200])
def test_rounding_bound(ops, dev, n_feat, dtype):
    tokens = 3000
    gen = torch.Generator().manual_seed(900 + n_feat)
    if dtype == F64:       # fp32 values would have exact products: give every element 53 significant bits
        x = acts(gen, tokens, n_feat, F32).double() * (1.0 + 2.0 ** -20 * torch.randn(tokens, n_feat, generator=gen, dtype=F64))
    else:
        x = acts(gen, tokens, n_feat, dtype)
    assert plan(tokens, n_feat)[0] > 1
    got = cov(ops, x.to(dev)).cpu().numpy().astype(R.LD)
    ref, scale = R.longdouble_cov(x)
    bound = tokens * U * scale * (1 + 1e-3) if dtype != F64 else (tokens + 1) * U * R.longdouble_abs_cov(x)
    il = np.tril_indices(n_feat)
    frac = (np.abs(got - ref) / bound)[0][il]
    print("ROUNDING %s n_feat=%d: max |got - long double| / bound = %.4f" % (NAME[dtype], n_feat, float(frac.max())))
    assert float(frac.max()) <= 1.0


# ---------------------------------------------------------------- 10. mdg_cov_accum_multi
MULTI = [(512, 1), (256, 1), (128, 4), (128, 2)]      # (n_feat, heads): sigma_mlp, sigma_x, sigma_q, sigma_k of one layer


def problem(xd, heads, sigma, ld_sigma=None, bs=None):
    feat = xd.shape[1] // heads
    ld_sigma = ld_sigma or feat
    return _lib.CovProblem(xd.data_ptr(), xd.shape[0], feat, heads, xd.stride(0), sigma.data_ptr(), ld_sigma, bs or feat * ld_sigma)


def multi_call(probs, dtype, dev, n=None, short=0, null_ws=False):
    """-> (status, workspace bytes the query asked for, the workspace)"""
    lib = _lib.load()
    n = len(probs) if n is None else n
    arr = (_lib.CovProblem * max(len(probs), 1))(*probs)
    nbytes = lib.mdg_cov_accum_multi_ws_bytes(n, arr, CODE[dtype])
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    rc = lib.mdg_cov_accum_multi(n, arr, CODE[dtype], None if null_ws else ws.data_ptr(), nbytes - short, stream())
    return rc, nbytes, ws


def multi_exact(dev, dtype, token_counts, calls):
    xs = [exact_x(t, f * h, dtype, seed=20 + i) for i, (t, (f, h)) in enumerate(zip(token_counts, MULTI))]
    xd = [x.to(dev) for x in xs]
    sig = [torch.zeros(h, f, f, dtype=F64, device=dev) for f, h in MULTI]
    for _ in range(calls):
        rc, nbytes, ws = multi_call([problem(a, h, s) for a, s, (f, h) in zip(xd, sig, MULTI)], dtype, dev)
        _lib.check(rc, "mdg_cov_accum_multi")
    for i, (x, s, (f, h)) in enumerate(zip(xs, sig, MULTI)):
        want = R.exact_cov(x, h)
        for _ in range(calls - 1):
            want = R.exact_cov(x, h, sigma0=want)
        assert_lower_exact(s, want, "problem %d" % i)
    return nbytes


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_multi_every_problem_split_and_accumulating(dev, dtype):
    """8200 tokens: every problem in two splits (offset-then-rebased partial pointers, one reduce launch per problem), twice."""
    nbytes = multi_exact(dev, dtype, [8200] * 4, calls=2)
    assert nbytes == 2 * sum(R.n_tri(f) * h for f, h in MULTI) * R.TILE * R.TILE * 8 > 0


@pytest.mark.parametrize("dtype", [BF16, F32], ids=NAME.get)
def test_multi_token_counts_may_differ(dev, dtype):
    """Split and unsplit problems, with a 17-token one, in one launch."""
    nbytes = multi_exact(dev, dtype, [8200, 300, 8193, 17], calls=1)
    assert nbytes == 2 * (R.n_tri(512) + 4) * R.TILE * R.TILE * 8 > 0


def test_multi_large_first_problem_stays_unsplit(dev):
    """768 heads of 128 features in front (768 tiles: the branch production's sigma_mlp takes) beside a 256-feature problem."""
    tokens, heads = 40, 768
    x0, x1 = exact_x(tokens, heads * 128, BF16, seed=30), exact_x(tokens, 256, BF16, seed=31)
    s0 = torch.zeros(heads, 128, 128, dtype=F64, device=dev)
    s1 = torch.zeros(1, 256, 256, dtype=F64, device=dev)
    a0, a1 = x0.to(dev), x1.to(dev)
    rc, nbytes, ws = multi_call([problem(a0, heads, s0), problem(a1, 1, s1)], BF16, dev)
    _lib.check(rc, "mdg_cov_accum_multi")
    assert nbytes == 0
    want = R.exact_cov(x0, heads).to(dev)
    assert torch.equal(torch.tril(s0), torch.tril(want))
    assert not torch.equal(want[0], want[767])
    assert_lower_exact(s1, R.exact_cov(x1), "second problem")


@pytest.mark.parametrize("fill", SENTINELS)
def test_multi_padded_sigma(dev, fill):
    tokens, pad = 8200, 2                     # the 4 x 128 problem in a padded layout
    xs = [exact_x(tokens, f * h, BF16, seed=20 + i) for i, (f, h) in enumerate(MULTI)]
    xd = [x.to(dev) for x in xs]
    sig = [torch.zeros(h, f, f, dtype=F64, device=dev) for f, h in MULTI]
    f, h = MULTI[pad]
    ld = f + 37
    bs = f * ld + 5
    buf, view = padded_sigma(h, f, ld, bs, fill, dev)
    before = buf.clone()
    probs = [problem(a, hh, s) for a, s, (ff, hh) in zip(xd, sig, MULTI)]
    probs[pad] = problem(xd[pad], h, buf, ld, bs)
    rc, nbytes, ws = multi_call(probs, BF16, dev)
    _lib.check(rc, "mdg_cov_accum_multi")
    assert nbytes > 0
    assert_lower_exact(view, R.exact_cov(xs[pad], h), "padded problem")
    assert outside_unchanged(buf, before, h, f, ld, bs)
    for i in (0, 1, 3):
        assert_lower_exact(sig[i], R.exact_cov(xs[i], MULTI[i][1]), "problem %d" % i)


def test_multi_bad_arguments(dev):
    lib = _lib.load()
    x = exact_x(8200, 256, BF16, seed=21).to(dev)
    x200 = exact_x(300, 200, BF16).to(dev)
    sigma = torch.full((256, 256), -7.25, dtype=F64, device=dev)
    before = sigma.clone()
    good = problem(x, 1, sigma)
    shifted = problem(x, 1, sigma)
    shifted.x = x.data_ptr() + 2
    assert lib.mdg_cov_accum_multi_ws_bytes(1, (_lib.CovProblem * 1)(good), CODE[BF16]) > 0
    cases = [("no problems", dict(probs=[good], n=0)), ("five problems", dict(probs=[good] * 5)),
             ("n_feat 200", dict(probs=[problem(x200, 1, sigma, 256)])), ("misaligned x", dict(probs=[shifted])),
             ("workspace one byte short", dict(probs=[good], short=1)), ("no workspace", dict(probs=[good], null_ws=True))]
    for what, kw in cases:
        rc, _, ws = multi_call(dev=dev, dtype=BF16, **kw)
        assert rc == _lib.MDG_ERR_BAD_ARG and "mdg_cov_accum_multi" in _lib.last_error(), what
        assert same_bits(sigma, before), what
    rc, _, ws = multi_call([good], BF16, dev)
    assert rc == _lib.MDG_OK and not same_bits(sigma, before)


# ---------------------------------------------------------------- 11. mdg_cov_finalize
@pytest.mark.parametrize("fill", SENTINELS)
@pytest.mark.parametrize("scale", [0.5, 1.0 / (5 * 2048)])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 200])
def test_finalize(dev, n, scale, fill):
    """Lower triangle <- fl(scale * lower), one fp64 rounding; the upper triangle its bit-exact mirror, NaN, +-Inf, -0.0 and subnormals
    included; what was above the diagonal is not read; the padding is not written."""
    batch, ld = 3, n + 5
    bs = n * ld + 7
    A = torch.randn(batch, n, n, generator=torch.Generator().manual_seed(n), dtype=F64)
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    A[0][upper] = float("nan")
    A[1, n - 1, 0] = float("nan")
    A[2, n // 2, n // 2] = -0.0
    if n >= 31:
        A[1, n - 2, 1] = float("inf")
        A[1, 5, 2] = float("-inf")
        A[2, 9, 3] = 1000 * 5e-324
        A[2, 30, 29] = -3 * 5e-324
        A[2, n - 1, n - 2] = 2.0 ** -1022
    buf, view = padded_sigma(batch, n, ld, bs, fill, dev, init=A)
    before = buf.clone()
    _lib.check(_lib.load().mdg_cov_finalize(buf.data_ptr(), n, batch, ld, bs, scale, stream()), "mdg_cov_finalize")
    got = view.cpu()
    assert same_bits(torch.tril(got), torch.tril(A * scale))
    assert same_bits(got, got.transpose(-1, -2).contiguous())
    assert outside_unchanged(buf, before, batch, n, ld, bs)
    assert bool(torch.isfinite(got[0]).all()), "NaN above the diagonal only must disappear"
    assert bool(torch.isnan(got[1, 0, n - 1])) and (n < 31 or (got[1, 1, n - 2] == float("inf") and got[1, 2, 5] == float("-inf")))


# ---------------------------------------------------------------- 12. mdg_bi_accum
BI_TOKENS = [1, 3, 4, 5, 8192, 8193, 20000]          # 4 tokens per workgroup, 2048 workgroups: a second pass from 8193
BI_D = [2, 63, 64, 65, 192]


@pytest.mark.parametrize("tokens", BI_TOKENS)
def test_bi_exact(ops, dev, tokens):
    """The integer total of bi_exact_inputs (same, opposite, perpendicular and zero rows) added to a start value of 3."""
    for k, d in enumerate(BI_D):
        dtype = DTYPES[(BI_TOKENS.index(tokens) + k) % 4]
        a, b, total = R.bi_exact_inputs(tokens, d, dtype, seed=5)
        out = torch.full((1,), 3.0, dtype=F64, device=dev)
        ops.bi_accum(out, a.to(dev), b.to(dev))
        assert out.item() == 3.0 + total, (d, NAME[dtype], out.item(), 3.0 + total)


def direct_bi(a, b, d, out, ws_short=0, ld=None):
    lib = _lib.load()
    nbytes = lib.mdg_bi_ws_bytes(a.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    rc = lib.mdg_bi_accum(a.data_ptr(), b.data_ptr(), CODE[a.dtype], a.shape[0], d, a.stride(0) if ld is None else ld, out.data_ptr(),
                          ws.data_ptr(), nbytes - ws_short, stream())
    return rc, ws


@pytest.mark.parametrize("fill", SENTINELS)
def test_bi_leading_dimension(dev, fill):
    tokens, d = 8193, 65
    a, b, total = R.bi_exact_inputs(tokens, d, F32, seed=6)
    bufs = [torch.full((tokens, d + 8), fill, dtype=F32, device=dev) for _ in range(2)]
    bufs[0][:, :d] = a.to(dev)
    bufs[1][:, :d] = b.to(dev)
    out = torch.full((1,), 3.0, dtype=F64, device=dev)
    rc, ws = direct_bi(bufs[0][:, :d], bufs[1][:, :d], d, out)
    _lib.check(rc, "mdg_bi_accum")
    assert out.item() == 3.0 + total


@pytest.mark.parametrize("dtype", DTYPES, ids=NAME.get)
def test_bi_generic_data(ops, dev, dtype):
    """|got - long double| <= 2^-53 (tokens (d + 8) + tokens S), S the sum itself: the first term pays each token's three dot products
    of d terms, two square roots, product, division and subtraction (a term is at most 2), the second the sum over tokens in any
    order.  Every term is at least 0.01, so one dropped or doubled token is four orders of magnitude above the bound."""
    tokens, d = 9000, 192
    gen = torch.Generator().manual_seed(12)
    a = acts(gen, tokens, d, F32)
    b = a + 0.3 * torch.randn(tokens, d, generator=gen)
    a, b = a.to(dtype), b.to(dtype)
    terms = 1.0 - torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)
    assert terms.min().item() >= 0.01
    want = R.longdouble_bi(a, b)
    out = torch.zeros(1, dtype=F64, device=dev)
    ops.bi_accum(out, a.to(dev), b.to(dev))
    bound = U * (tokens * (d + 8) + tokens * float(want))
    err = abs(float(R.LD(out.item()) - want))
    print("BI %s: S = %.6f, |got - long double| = %.3e = %.4f of the bound %.3e (smallest term %.4f)" % (
        NAME[dtype], float(want), err, err / bound, bound, terms.min().item()))
    assert err <= bound


# ---------------------------------------------------------------- 13. argument errors
def test_cov_accum_bad_arguments(dev):
    """Each returns MDG_ERR_BAD_ARG with a message before anything is launched: sigma and the workspace keep their bits."""
    lib = _lib.load()
    n, batch, tokens = 128, 2, 300
    x = exact_x(tokens, batch * n, BF16).to(dev)
    sigma = torch.full((batch, n, n), -7.25, dtype=F64, device=dev)
    before = sigma.clone()
    nbytes = lib.mdg_cov_accum_ws_bytes(tokens, n, batch)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    ws_before = ws.clone()
    ok = dict(dtype=_lib.MDG_BF16, ld=batch * n, ld_sigma=n, bs=n * n, ws=ws.data_ptr(), ws_bytes=nbytes)
    cases = [("ld < batch * n_feat", dict(ld=batch * n - 1), "ld"), ("ld_sigma < n_feat", dict(ld_sigma=n - 1), "ld_sigma"),
             ("overlapping matrices", dict(bs=n * n - 1), "stride"), ("dtype 7", dict(dtype=7), "dtype"),
             ("split without a workspace", dict(ws=None), "workspace"), ("workspace one byte short", dict(ws_bytes=nbytes - 1), "workspace")]
    for what, change, word in cases:
        a = dict(ok, **change)
        rc = lib.mdg_cov_accum(x.data_ptr(), a["dtype"], tokens, n, batch, a["ld"], 0, sigma.data_ptr(), a["ld_sigma"], a["bs"], a["ws"],
                               a["ws_bytes"], stream())
        assert rc == _lib.MDG_ERR_BAD_ARG, what
        assert "mdg_cov_accum" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
        assert same_bits(sigma, before) and torch.equal(ws, ws_before), what
    # the same call with nothing changed runs
    rc = lib.mdg_cov_accum(x.data_ptr(), ok["dtype"], tokens, n, batch, ok["ld"], 0, sigma.data_ptr(), n, n * n, ok["ws"], nbytes, stream())
    assert rc == _lib.MDG_OK and not same_bits(sigma, before)


def test_bi_accum_bad_arguments(dev):
    tokens, d = 100, 64
    a, b, _ = R.bi_exact_inputs(tokens, d, BF16, seed=8)
    a, b = a.to(dev), b.to(dev)
    out = torch.full((1,), 3.0, dtype=F64, device=dev)
    for what, kw in [("ld < d", dict(ld=d - 1)), ("workspace one byte short", dict(ws_short=1))]:
        rc, ws = direct_bi(a, b, d, out, **kw)
        assert rc == _lib.MDG_ERR_BAD_ARG and "mdg_bi_accum" in _lib.last_error(), what
        assert out.item() == 3.0, what
