"""mdg_attn_decode (ops.attn_decode) -- split-key attention for T * G <= 32 -- against float64 torch on the CPU from the same bf16 /
f16 inputs: the cases, the reference and the bound of tests/attn_ref.py, the three layouts of tests/test_gpu_attn_fwd.py.

  exact    one admitted key per query has a scaled logit more than 120 above every other, so the output must be that key's v row BIT
           FOR BIT at every split count.  exact_case asserts the 120-nat gap when it builds the case; the chunk argument follows
           from that assertion: a chunk (and inside a chunk, a wave) that does not hold the winner has a maximum m_s at least
           120 nats = 173 binades under M, its weight 2^(m_s - M) underflows to exactly 0 in fp32, and the winner's chunk has
           weight 1, sum 1 and O_s = the winner's v row exactly.
  random   |out - reference| <= 4 u max_j |v[b, g, j, c]| entry-wise over the admitted keys, the bound of mdg_attn_fwd: the
           partials and the combine are fp32, so the only roundings to the element type are still the probabilities and the store.

Splits 1, 2, 3, 7, 256: 256 exceeds the key tiles of every shape (empty chunks), and at (6, 7, 32, 70, 1, 1) with 2 splits the
queries 0 .. 25 see nothing of the second chunk (a chunk wholly beyond the causal limit).

The column map (column c of the 32-column tile = query c / G, head of the group c % G) is internal: the workspace and out are
indexed by (batch, head, query).  What it must get right is that a column's q row, causal limit and output row belong to ONE
(query, head); the exact causal cases with G = 3, T = 3 (non-power-of-two map) and G = 8, T = 4 (tile exactly full) pin that: every
(query, head) there has its own winner and its own limit."""
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_attn_fwd import SENTINEL, layouts

pytestmark = pytest.mark.gpu

# (r_qk, r_vo, T, S, n_heads, n_kv)
SHAPES = [
    (2, 1, 1, 1, 1, 1),          # the minimum
    (90, 77, 1, 257, 8, 2),      # typical widths, one key past a tile boundary
    (128, 128, 1, 300, 8, 1),    # G = 8
    (130, 255, 1, 257, 8, 2),    # wide templates
    (256, 256, 2, 129, 2, 2),    # widest template, T = 2
    (64, 33, 4, 200, 8, 1),      # T * G = 32: the tile exactly full
    (6, 7, 32, 70, 1, 1),        # MHA, 32 queries, deep causal masking inside the last chunk
    (30, 64, 5, 70, 4, 1),       # T * G = 20
    (90, 77, 3, 64, 12, 4),      # G = 3: a non-power-of-two column map; S exactly one tile
    (64, 64, 1, 63, 4, 4),       # the neighbours of one tile
    (64, 64, 1, 65, 4, 4),
    (62, 65, 1, 65, 4, 4),       # the other six (NQ, NV) templates (attn_ref.template_of), at the bucket edges: (4, 4)
    (30, 129, 4, 130, 8, 2),     # (4, 8)
    (66, 33, 1, 130, 8, 1),      # (8, 2)
    (128, 255, 4, 65, 4, 2),     # (8, 8)
    (130, 64, 4, 130, 12, 4),    # (16, 2), G = 3
    (200, 128, 1, 65, 2, 2),     # (16, 4)
]
SPLITS = (1, 2, 3, 7, 256)


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def run_layouts(ops, dev, c, splits):
    Bq, H, T, _ = c.q.shape
    r_vo = c.v.shape[3]
    W = H * r_vo
    for name, q, k, v, out, where in layouts(c, dev):
        got = ops.attn_decode(q, k, v, c.scale, causal=c.causal, splits=splits, out=out)
        assert tuple(got.shape) == (Bq, T, H, r_vo) and got.dtype == q.dtype
        if out is not None:                                        # a caller-owned view: the bytes around it stay
            assert got is out
            big, off, pitch = where
            rows = big[off:].view(Bq * T, pitch)
            assert bool((rows[:, W:] == SENTINEL).all()), name + ": the padding of out was written"
            assert off == 0 or float(big[0]) == SENTINEL
        yield name, got.cpu()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_exact_selection_bit_for_bit_at_every_split_count(ops, dev, dt, shape, causal):
    c = R.exact_case(dt, shape, causal)
    for splits in SPLITS:
        for name, got in run_layouts(ops, dev, c, splits):
            same = R.bits(got) == R.bits(c.want)
            if not bool(same.all()):
                b, i, h, col = (~same).nonzero()[0].tolist()
                raise AssertionError(f"{name}, {splits} splits: out[{b}, {i}, {h}, {col}] = {float(got[b, i, h, col])!r}, want v row "
                                     f"of key {int(c.winners[b, h, i])} = {float(c.want[b, i, h, col])!r}; "
                                     f"{int((~same).sum())} entries differ")


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_random_data_within_the_derived_bound(ops, dev, dt, shape, causal):
    c = R.random_case(dt, shape, causal)
    bound = 4.0 * R.UNIT_ROUNDOFF[dt] * c.vmax
    fwd = ops.attn_fwd(c.q.to(dev), c.k.to(dev), c.v.to(dev), c.scale, causal=causal).cpu()
    for splits in SPLITS:
        for name, got in run_layouts(ops, dev, c, splits):
            err = (got.double() - c.want).abs()
            worst = float((err / bound.clamp(min=1e-300)).max())
            print(f"{dt} {R.shape_id(shape)} causal={causal} splits={splits} {name}: max err / bound = {worst:.3f}")
            assert bool((err <= bound).all()), f"{name}, {splits} splits: max err / bound = {worst:.3f}"
            if splits == 1:                                        # the same tensors through mdg_attn_fwd: the tile order differs, the bound holds
                diff = (got.double() - fwd.double()).abs()
                assert bool((diff <= bound).all()), f"{name}: 1 split vs attn_fwd: {float((diff / bound.clamp(min=1e-300)).max()):.3f}"
    # default split count: the rule, with this device's CU count
    got = ops.attn_decode(c.q.to(dev), c.k.to(dev), c.v.to(dev), c.scale, causal=causal).cpu()
    assert bool(((got.double() - c.want).abs() <= bound).all())


@pytest.mark.parametrize("shape", R.sweep_shapes(R.SWEEP_DECODE_TS), ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_trip_count_sweep_within_the_derived_bound(ops, dev, dt, shape):
    """Every k-step count nq = 1 .. 16 and every column-tile count nv = 1 .. 8 (attn_ref.SWEEP), causal, the bound unchanged.  T = 16
    with the sweep's group of 2: the kernel's domain ends at T * G = 32, the prefill sweep's T = 33 is outside it."""
    c = R.random_case(dt, shape, True)
    bound = 4.0 * R.UNIT_ROUNDOFF[dt] * c.vmax
    for splits in SPLITS:
        for name, got in run_layouts(ops, dev, c, splits):
            err = (got.double() - c.want).abs()
            worst = float((err / bound.clamp(min=1e-300)).max())
            print(f"{dt} {R.shape_id(shape)} splits={splits} {name}: max err / bound = {worst:.3f}")
            assert bool((err <= bound).all()), f"{name}, {splits} splits: max err / bound = {worst:.3f}"


@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_two_calls_give_the_same_bits(ops, dev, dt):
    for shape, splits in (((90, 77, 1, 257, 8, 2), 3), ((6, 7, 32, 70, 1, 1), 2), ((128, 128, 1, 300, 8, 1), 256)):
        c = R.random_case(dt, shape, True)
        q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
        first = ops.attn_decode(q, k, v, c.scale, causal=True, splits=splits)
        torch.empty(1 << 20, device=dev).fill_(float("nan"))       # whatever the next workspace lands on
        second = ops.attn_decode(q, k, v, c.scale, causal=True, splits=splits)
        assert torch.equal(R.bits(first), R.bits(second))


def _raw(lib, _lib, q, k, v, scale, causal, splits, ws, out):
    B, H, T, r_qk = q.shape
    KV, S, r_vo = k.shape[1], k.shape[2], v.shape[3]
    rc = lib.mdg_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16 if q.dtype == torch.bfloat16 else _lib.MDG_F16,
                             B, T, S, H, KV, r_qk, r_vo, k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                             scale, 1 if causal else 0, splits, ws.data_ptr(), ws.numel() * 4, out.data_ptr(), H * r_vo, None)
    _lib.check(rc, "mdg_attn_decode")
    torch.cuda.synchronize()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", [(90, 77, 3, 64, 12, 4), (6, 7, 32, 70, 1, 1), (130, 255, 1, 257, 8, 2)], ids=R.shape_id)
def test_a_poisoned_workspace_does_not_reach_out(ops, dev, shape, causal):
    """The workspace need not be initialised: every float the combine reads was written by this call, NaN everywhere else is never
    read (r_vo = 77, 7 and 255 leave pad columns; 256 splits leave empty chunks), and nothing beyond mdg_attn_decode_ws_bytes is
    written."""
    from modegpt_amd import _lib
    lib = _lib.load()
    c = R.random_case("bf16", shape, causal)
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    Bq, H, T, _ = q.shape
    r_vo = v.shape[3]
    bound = 4.0 * R.UNIT_ROUNDOFF["bf16"] * c.vmax
    for splits in (2, 256):
        need = lib.mdg_attn_decode_ws_bytes(Bq, T, H, r_vo, splits) // 4
        ws = torch.full((need + 64,), float("nan"), dtype=torch.float32, device=dev)
        out = torch.full((Bq, T, H, r_vo), SENTINEL, dtype=q.dtype, device=dev)
        _raw(lib, _lib, q, k, v, c.scale, causal, splits, ws, out)
        assert bool(torch.isnan(ws[need:]).all()), "the kernel wrote beyond mdg_attn_decode_ws_bytes"
        assert bool(torch.isfinite(out.float()).all())
        assert bool(((out.cpu().double() - c.want).abs() <= bound).all())
        assert torch.equal(R.bits(out.cpu()), R.bits(ops.attn_decode(q, k, v, c.scale, causal=causal, splits=splits).cpu()))


def test_no_key_at_all_stores_zeros_and_empty_calls_launch_nothing(ops, dev):
    q = torch.ones(2, 4, 1, 6, dtype=torch.bfloat16, device=dev)
    k = torch.ones(2, 2, 0, 6, dtype=torch.bfloat16, device=dev)
    v = torch.ones(2, 2, 0, 3, dtype=torch.bfloat16, device=dev)
    for splits in (1, 5):
        out = torch.full((2, 1, 4, 3), SENTINEL, dtype=torch.bfloat16, device=dev)
        ops.attn_decode(q, k, v, 1.0, causal=False, splits=splits, out=out)
        assert bool((out == 0).all())                              # S == 0, non-causal: zeros, as mdg_attn_fwd stores
    for Bq, T in ((0, 1), (2, 0)):
        got = ops.attn_decode(torch.zeros(Bq, 4, T, 6, dtype=torch.bfloat16, device=dev),
                              torch.zeros(Bq, 2, 9, 6, dtype=torch.bfloat16, device=dev),
                              torch.zeros(Bq, 2, 9, 3, dtype=torch.bfloat16, device=dev), 1.0, causal=False)
        assert tuple(got.shape) == (Bq, T, 4, 3)


def test_wrapper_refuses_what_it_cannot_pass_on(ops, dev):
    q = torch.zeros(2, 4, 5, 6, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(2, 2, 9, 6, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(2, 2, 9, 3, dtype=torch.bfloat16, device=dev)
    ops.attn_decode(q, k, v, 1.0)                                   # T * G = 10: served
    with pytest.raises(ValueError, match="32 columns"):            # T * G = 17 * 2
        ops.attn_decode(torch.zeros(2, 4, 17, 6, dtype=torch.bfloat16, device=dev), torch.zeros(2, 2, 20, 6, dtype=torch.bfloat16, device=dev),
                        torch.zeros(2, 2, 20, 3, dtype=torch.bfloat16, device=dev), 1.0)
    with pytest.raises(ValueError, match="32 columns"):            # MHA, T = 33
        ops.attn_decode(torch.zeros(1, 1, 33, 6, dtype=torch.bfloat16, device=dev), torch.zeros(1, 1, 40, 6, dtype=torch.bfloat16, device=dev),
                        torch.zeros(1, 1, 40, 3, dtype=torch.bfloat16, device=dev), 1.0)
    with pytest.raises(ValueError, match="bf16 or f16"):
        ops.attn_decode(q.float(), k.float(), v.float(), 1.0)
    with pytest.raises(ValueError, match="bf16 or f16"):
        ops.attn_decode(q, k.half(), v, 1.0)
    with pytest.raises(ValueError, match="contiguous last"):
        ops.attn_decode(q, k.transpose(2, 3).contiguous().transpose(2, 3), v, 1.0)
    with pytest.raises(ValueError, match="splits"):
        ops.attn_decode(q, k, v, 1.0, splits=0)
    with pytest.raises(ValueError, match="splits"):
        ops.attn_decode(q, k, v, 1.0, splits=257)
    with pytest.raises(ValueError):
        ops.attn_decode(q, k, v, 1.0, out=torch.empty(2, 5, 4, 4, dtype=torch.bfloat16, device=dev))
    with pytest.raises(RuntimeError, match="S=3"):
        ops.attn_decode(q, k[:, :, :3].contiguous(), v[:, :, :3].contiguous(), 1.0, causal=True)
