"""mdg_attn_fwd (ops.attn_fwd) -- fused attention forward for compressed heads of unequal q/k and v width -- against float64 torch
on the CPU from the same bf16 / f16 inputs (tests/attn_ref.py).

  exact    one admitted key per query has a scaled logit more than 120 above every other, so the output must be that key's v row
           BIT FOR BIT: pins the lane maps of both products, the permuted k order of the second, the GQA mapping, the causal
           mask (the key just beyond the limit carries the largest logit), the key-tile boundaries and the output layout.
  random   standard normal data, |scale * logit| <= 20, entry-wise |out - ref| <= 4 u max_j |v[b, g, j, c]| over the admitted
           keys, u = 2^-9 (bf16) / 2^-11 (f16): u max|v| from rounding the probabilities, u |out| from rounding the output, fp32
           accumulation and exp2 below u together; the 4 is twice the sum of the two rounding terms.  Derived, not tuned.

Every case runs in three layouts: contiguous operands; k and v as views of longer buffers with larger token, head and batch
strides (a static cache) and out with ld_out > n_heads * r_vo whose sentinel padding must stay; all bases offset by one element
with odd pitches, so the element-wise load and store paths run."""
import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def _cache_view(t, dev, extra_tokens, extra_heads, extra_width, offset):
    """t [B, KV, S, r] as a view of a longer buffer: more tokens, heads and columns than needed, base `offset` elements in."""
    Bt, KV, S, r = t.shape
    shape = (Bt, KV + extra_heads, S + extra_tokens, r + extra_width)
    n = shape[0] * shape[1] * shape[2] * shape[3]
    flat = torch.zeros(n + offset, dtype=t.dtype, device=dev)
    view = flat[offset:].view(shape)[:, :KV, :S, :r]
    view.copy_(t)
    return view


def layouts(c, dev):
    """(name, q, k, v, out view, (whole out buffer, base offset, row pitch)) for the three layouts."""
    Bq, H, T, r_qk = c.q.shape
    r_vo = c.v.shape[3]
    W = H * r_vo
    q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
    yield "contiguous", q, k, v, None, None
    for name, pad_t, pad_h, pad_w, off, pad_o in (("cache-views", 5, 1, 8, 0, 8), ("offset-odd", 3, 0, 3, 1, 3)):
        qf = torch.zeros(q.numel() + off, dtype=q.dtype, device=dev)
        qv = qf[off:].view(q.shape)
        qv.copy_(q)
        kv = _cache_view(k, dev, pad_t, pad_h, pad_w, off)
        vv = _cache_view(v, dev, pad_t, pad_h, pad_w, off)
        assert kv.stride(3) == 1 and (kv.shape[2] == 1 or kv.stride(2) == r_qk + pad_w)
        big = torch.full((Bq * T * (W + pad_o) + off,), SENTINEL, dtype=q.dtype, device=dev)
        out = big[off:].view(Bq, T, W + pad_o)[:, :, :W].unflatten(2, (H, r_vo))
        yield name, qv, kv, vv, out, (big, off, W + pad_o)


def run_layouts(ops, dev, c):
    Bq, H, T, _ = c.q.shape
    r_vo = c.v.shape[3]
    W = H * r_vo
    for name, q, k, v, out, where in layouts(c, dev):
        got = ops.attn_fwd(q, k, v, c.scale, causal=c.causal, out=out)
        assert tuple(got.shape) == (Bq, T, H, r_vo) and got.dtype == q.dtype
        if out is not None:
            assert got is out
            big, off, pitch = where
            rows = big[off:].view(Bq * T, pitch)
            assert bool((rows[:, W:] == SENTINEL).all()), name + ": the padding of out was written"
            assert off == 0 or float(big[0]) == SENTINEL
        yield name, got.cpu()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_exact_selection_bit_for_bit(ops, dev, dt, shape, causal):
    c = R.exact_case(dt, shape, causal)
    for name, got in run_layouts(ops, dev, c):
        same = R.bits(got) == R.bits(c.want)
        if not bool(same.all()):
            b, i, h, col = (~same).nonzero()[0].tolist()
            raise AssertionError(f"{name}: out[{b}, {i}, {h}, {col}] = {float(got[b, i, h, col])!r}, want v row of key "
                                 f"{int(c.winners[b, h, i])} = {float(c.want[b, i, h, col])!r}; {int((~same).sum())} entries differ")


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_random_data_within_the_derived_bound(ops, dev, dt, shape, causal):
    c = R.random_case(dt, shape, causal)
    bound = 4.0 * R.UNIT_ROUNDOFF[dt] * c.vmax
    for name, got in run_layouts(ops, dev, c):
        err = (got.double() - c.want).abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{dt} {R.shape_id(shape)} causal={causal} {name}: max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"{name}: max err / bound = {worst:.3f}"


@pytest.mark.parametrize("shape", R.sweep_shapes(R.SWEEP_FWD_TS), ids=R.shape_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_trip_count_sweep_within_the_derived_bound(ops, dev, dt, shape):
    """Every k-step count nq = 1 .. 16 and every column-tile count nv = 1 .. 8 (attn_ref.SWEEP), causal, the bound unchanged."""
    c = R.random_case(dt, shape, True)
    bound = 4.0 * R.UNIT_ROUNDOFF[dt] * c.vmax
    for name, got in run_layouts(ops, dev, c):
        err = (got.double() - c.want).abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{dt} {R.shape_id(shape)} {name}: max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"{name}: max err / bound = {worst:.3f}"


@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_a_non_trivial_scale(ops, dev, dt):
    shape = (90, 77, 200, 200, 8, 2)
    c = R.random_case(dt, shape, True, 0.37)
    bound = 4.0 * R.UNIT_ROUNDOFF[dt] * c.vmax
    got = ops.attn_fwd(c.q.to(dev), c.k.to(dev), c.v.to(dev), c.scale, causal=True).cpu()
    err = (got.double() - c.want).abs()
    print(f"{dt} scale {c.scale:.5f}: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # and the scale matters: the unscaled answer is outside the bound somewhere
    other = ops.attn_fwd(c.q.to(dev), c.k.to(dev), c.v.to(dev), c.scale / 0.37, causal=True).cpu()
    assert not bool(((other.double() - c.want).abs() <= bound).all())


def test_empty_calls_succeed_and_leave_out_untouched(ops, dev):
    for Bq, T in ((0, 5), (2, 0)):
        q = torch.zeros(Bq, 4, T, 6, dtype=torch.bfloat16, device=dev)
        k = torch.zeros(Bq, 2, 9, 6, dtype=torch.bfloat16, device=dev)
        v = torch.zeros(Bq, 2, 9, 3, dtype=torch.bfloat16, device=dev)
        got = ops.attn_fwd(q, k, v, 1.0)
        assert tuple(got.shape) == (Bq, T, 4, 3)
    # the C entry with live pointers and an empty extent: success, nothing written
    from modegpt_amd import _lib
    lib = _lib.load()
    q = torch.ones(2, 4, 5, 6, dtype=torch.bfloat16, device=dev)
    k = torch.ones(2, 2, 9, 6, dtype=torch.bfloat16, device=dev)
    v = torch.ones(2, 2, 9, 3, dtype=torch.bfloat16, device=dev)
    out = torch.full((2, 5, 4, 3), SENTINEL, dtype=torch.bfloat16, device=dev)
    for Bq, T in ((0, 5), (2, 0)):
        rc = lib.mdg_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _lib.MDG_BF16, Bq, T, 9, 4, 2, 6, 3, 2 * 9 * 6, 9 * 6, 6,
                              2 * 9 * 3, 9 * 3, 3, 1.0, 0, out.data_ptr(), 12, None)
        assert rc == _lib.MDG_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_wrapper_refuses_what_it_cannot_pass_on(ops, dev):
    q = torch.zeros(2, 4, 5, 6, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(2, 2, 9, 6, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(2, 2, 9, 3, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="contiguous last"):
        ops.attn_fwd(q, k.transpose(2, 3).contiguous().transpose(2, 3), v, 1.0)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k.float(), v, 1.0)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k[:, :, :8], v, 1.0)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k, v, 1.0, out=torch.empty(2, 5, 4, 4, dtype=torch.bfloat16, device=dev))
    with pytest.raises(RuntimeError, match="overlap"):
        buf = torch.zeros(q.numel() + 2 * 5 * 4 * 3, dtype=torch.bfloat16, device=dev)
        ops.attn_fwd(buf[:q.numel()].view(q.shape), k, v, 1.0, out=buf[8:8 + 120].view(2, 5, 4, 3))
    with pytest.raises(RuntimeError, match="S=3"):
        ops.attn_fwd(q, k[:, :, :3].contiguous(), v[:, :, :3].contiguous(), 1.0, causal=True)
