"""The three-plane product of the exact route (i8_syrk_kernel<3>, cov_i8_product.hip) on either MFMA shape it can be built with
(MDG_I8_SHAPE3 = 16: v_mfma_i32_16x16x64_i8, one MFMA per stage of two k-steps; 32: v_mfma_i32_32x32x32_i8): the class sums are
exact int32 sums, so sigma must come out BIT FOR BIT what tests/i8_model.py's integer digits give, whichever shape is compiled in.

The inputs hold no remainder (every element's low 24 bits of its 46-bit integer are zero: planes 3 .. 5 empty, asserted), so
the whole statistic is the fold of the five class sums and the model exposes it exactly: M.product's expression.  A lane mapping
of the A / B / D registers that is transposed or permuted anywhere moves a product to another (row, column) and cannot pass:
every column has its own scale and its own sign pattern, nothing is symmetric, some tokens hold a value in one column only."""
import numpy as np
import pytest
import torch

from tests import i8_model as M

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def make_input(tokens, n, seed):
    """bf16 [tokens, n] whose elements lie 0 .. 15 binades under their column's maximum with low 24 bits of N zero, the digits of
    planes 1 and 2 driven to -128 and 127 and plane 0 to its own extremes (+-64: a bf16 significand has 8 bits and the column
    maximum's sits at bits 38 .. 45 of N, so |d_0| <= 64 whatever the data)."""
    g = np.random.default_rng(seed)
    sh = g.integers(0, 15, size=(tokens, n))                     # binades under the column maximum
    sig = g.integers(128, 256, size=(tokens, n))                 # 8-bit significands
    # digit extremes: N = sig << (38 - sh);  254 << 31 = 127 * 2^32 (plane 1 = 127), 128 << 32 (plane 1 = -128, carry into plane 0),
    # 254 << 23 = 127 * 2^24 (plane 2 = 127), 128 << 24 (plane 2 = -128, carry into plane 1); row 0 below: 255 << 38 (plane 0 = 64,
    # plane 1 = -64)
    special = np.array([(254, 7), (128, 6), (254, 15), (128, 14), (255, 8), (129, 14)])
    pick = g.integers(0, len(special), size=(tokens, n))
    use = g.random((tokens, n)) < 0.25
    sig = np.where(use, special[pick, 0], sig)
    sh = np.where(use, special[pick, 1], sh)
    sign = np.where(g.random((tokens, n)) < 0.5, -1.0, 1.0)
    sign[:, ::3] *= np.where(np.arange(tokens) % 2 == 0, 1.0, -1.0)[:, None]    # column-dependent sign patterns
    sign[:, 1::5] = 1.0
    x = sign * sig * np.exp2(-sh.astype(np.float64))
    x[0] = 255.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)    # every column's maximum, sh = 0
    if tokens > 8:
        for t, j in ((3, 1), (5, n - 1), (tokens - 1, n // 2 + 3)):   # tokens with a value in ONE column only
            v = x[t, j]
            x[t] = 0.0
            x[t, j] = v
    x *= np.exp2(g.integers(-6, 7, size=n).astype(np.float64))[None, :]   # every column its own scale
    X = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(X.double(), torch.from_numpy(x))          # (all of it is exact in bf16)
    return X


def folded_class_sums(d, E, device):
    """M.product(d, E, 5) for digits whose planes 3 .. 5 are empty -- the nine pairs of planes 0 .. 2 as exact integer sums (fp64
    products of integers, every partial sum < 2^53), folded high class to low, then the two column scales -- with the nine
    matrix products on `device` (the n = 2048 case is ~0.3 TFLOP)."""
    df = [torch.from_numpy(d[s].astype(np.float64)).to(device) for s in range(3)]
    n = d.shape[2]
    cls = [torch.zeros(n, n, dtype=F64, device=device) for _ in range(5)]
    for s in range(3):
        for t in range(3):
            cls[s + t] += df[s].T @ df[t]
    acc = torch.zeros(n, n, dtype=F64, device=device)
    for k in range(4, -1, -1):
        acc += cls[k] * 2.0 ** (80 - 8 * k)                      # (powers of two as exact Python floats: no pow() on the device)
    sc = torch.from_numpy(np.ldexp(1.0, (E - 172).astype(np.int64))).to(device)
    return acc * sc[:, None] * sc[None, :]


def check_digits(d, tokens):
    assert not d[3:].any(), "the inputs are built to leave no remainder"
    if tokens >= 64:
        for p in (1, 2):
            assert d[p].min() == -128 and d[p].max() == 127
        assert d[0].min() == -64 and d[0].max() == 64


# n = 128: one tile, one workgroup -- one k-step (half an MFMA's K: lane groups 2 and 3 multiply zeros), one full MFMA, an odd count,
# many stages plus an odd end.  n = 256: two diagonal tiles and the off-diagonal one.  n = 2048, 4096 + 32 tokens: the persistent
# launch; 136 tiles on 256 CUs, so every tile is cut into k-chunks (the k-split last round) and, the call being 129 k-steps --
# an odd number --, at least one chunk of every tile holds an odd number of k-steps however the schedule cuts it.
CASES = [(128, 32), (128, 64), (128, 96), (128, 2080), (256, 96), (256, 2080), (2048, 4096 + 32)]


@pytest.mark.parametrize("n,tokens", CASES)
def test_three_plane_product_is_the_exact_integer_result(ops, dev, monkeypatch, n, tokens):
    monkeypatch.setattr(ops, "I8_EXACT", True)                   # MDG_I8_EXACT_ALWAYS
    nk = (tokens + 31) // 32
    if n == 2048:
        assert nk % 2 == 1
    X = make_input(tokens, n, seed=1000 + n + tokens)
    d, E, _, rounded, _ = M.digits(X)
    assert int(rounded.sum()) == 0
    check_digits(d, tokens)
    if n <= 256:
        want = torch.from_numpy(M.product(d, E, 5)).to(dev)      # the model's own product
        if n == 128:                                             # ... which the device helper of the large case reproduces bit for bit
            helper = folded_class_sums(d, E, dev)
            assert torch.equal(helper, want), ((helper - want).abs().max() / want.abs().max()).item()
    else:
        want = folded_class_sums(d, E, dev)
    # Every folded sum is a multiple of 2^48 sc_i sc_j (the lowest class is 256^6); with the largest one, doubled, under 2^101 sc_i sc_j
    # (|s_ij| <= sqrt(s_ii s_jj), and so is every partial sum over tokens) each fp64 number the device forms on the way -- a tile's or
    # a k-chunk's fold, the combine pass's running sum, the second call's sum below -- is exact, however the schedule cuts the chunks.
    sc = np.ldexp(1.0, (E - 172).astype(np.int64))
    assert 2.0 * (torch.diagonal(want).cpu().numpy() / (sc * sc)).max() < 2.0 ** 101
    S = torch.zeros(n, n, dtype=F64, device=dev)
    info, st = {}, {}
    planes = ops.cov_accum_i8(S, X.to(dev), route_info=info, mfma_stats=st)
    assert planes in (5, 6) and info["exact"] and info["columns"] == [], info
    assert st["planes_run"] == 3 and st["executed"] == st["dense"], st      # the MFMA count keeps its unit: 32x32x32 pair-blocks
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=dev))
    diff = (S != want) & low
    if diff.any():
        i, j = [int(v) for v in diff.nonzero()[0]]
        pytest.fail(f"{int(diff.sum())} of {int(low.sum())} lower-triangle elements differ; first ({i}, {j}): got {S[i, j].item()!r}, "
                    f"exact {want[i, j].item()!r}")
    # a second call adds the same again: bit-identical doubling (the fold reads what is there)
    ops.cov_accum_i8(S, X.to(dev))
    assert torch.equal(torch.tril(S), torch.tril(want * 2.0))
