"""mdg_rope_rows (ops.rope_rows) -- the rotary embedding of a projection output in its own layout -- against the CPU expression of
tests/rope_rows_ref.py, which tests/test_rope_rows_host.py pins to transformers' apply_rotary_pos_emb: bit-identical, signs of zeros
included (NaN payloads excepted, rope_rows_ref.same_bits).  Shapes: head_dim 2 (one pair), 6 (odd half), 16, 64, 128, 256; 1, 3, 5
(one head per lane item), 6 (two) and 8 (four) heads; (B, T) = (1, 1), (1, 5), (2, 70) -- several workgroups, a partial last one,
a batch boundary inside a workgroup; freshly allocated operands take the 16-byte path where head_dim / 2 holds a pack, the views
below (odd pitch, element offset 1, odd padding) the element-wise one, and 5 heads of 256 make a lane loop more than once."""
import pytest
import torch

from tests import rope_rows_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def on(dev, c):
    return c.x.to(dev), c.cos.to(dev), c.sin.to(dev)


@pytest.mark.parametrize("hd", R.HEAD_DIMS)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_bit_identical_to_the_cpu_expression(ops, dev, dt, hd):
    for c in R.all_cases(dt, hd):
        x, cos, sin = on(dev, c)
        keep = x.clone()
        got = ops.rope_rows(x, cos, sin, c.n_heads, hd)
        assert got.shape == x.shape and got.dtype == x.dtype and got.data_ptr() != x.data_ptr()
        assert R.same_bits(got.cpu(), c.want), (dt, hd, c.n_heads, c.dims)
        assert torch.equal(R.bits(x), R.bits(keep)), "x was modified"
        again = ops.rope_rows(x, cos, sin, c.n_heads, hd, out=torch.empty_like(x))
        assert torch.equal(R.bits(again), R.bits(got))                     # deterministic, and `out` is honoured


LAYOUT_CASES = [(16, 3, 2, 70), (128, 8, 2, 70), (256, 5, 1, 5), (6, 6, 1, 5)]


@pytest.mark.parametrize("shape", LAYOUT_CASES, ids=lambda s: "hd%d-h%d-b%d-t%d" % s)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_views_odd_pitch_offset_out_and_padding(ops, dev, dt, shape):
    hd, n_heads, B, T = shape
    c = R.make_case(dt, hd, n_heads, B, T, "per_batch_halves_differ")
    x, cos, sin = on(dev, c)
    W = n_heads * hd
    nan = float("nan")
    # x a column slice of a wider buffer with an odd pitch
    wide = torch.zeros(B, T, W + 3, dtype=x.dtype, device=dev)
    wide[:, :, 1:1 + W] = x
    xs = wide[:, :, 1:1 + W]
    assert xs.stride(1) == W + 3 and not xs.is_contiguous()
    assert R.same_bits(ops.rope_rows(xs, cos, sin, n_heads, hd).cpu(), c.want), "column slice, odd pitch"
    # out at element offset 1 of a flat buffer, NaN before and behind it
    flat = torch.full((B * T * W + 2,), nan, dtype=x.dtype, device=dev)
    out = flat[1:1 + B * T * W].view(B, T, W)
    assert out.data_ptr() % 16 != 0
    assert ops.rope_rows(x, cos, sin, n_heads, hd, out=out) is out
    assert R.same_bits(out.cpu(), c.want), "out at element offset 1"
    assert bool(torch.isnan(flat[0])) and bool(torch.isnan(flat[-1]))
    # ld_out > width: the padding of out stays as it was, with a pitch that keeps the 16-byte path (+16 elements) and one that
    # does not (+3); cos / sin at element offset 1 with the second
    for pad, shift in ((16, 0), (3, 1)):
        big = torch.full((B, T, W + pad), nan, dtype=x.dtype, device=dev)
        before = R.bits(big).clone()
        if shift:
            cflat = torch.zeros(cos.numel() + 1, dtype=x.dtype, device=dev)
            sflat = torch.zeros(sin.numel() + 1, dtype=x.dtype, device=dev)
            cflat[1:] = cos.reshape(-1)
            sflat[1:] = sin.reshape(-1)
            cc, ss = cflat[1:].view(cos.shape), sflat[1:].view(sin.shape)
        else:
            cc, ss = cos, sin
        view = big[:, :, :W]
        ops.rope_rows(x, cc, ss, n_heads, hd, out=view)
        assert R.same_bits(view.cpu(), c.want), "ld_out = width + %d" % pad
        assert torch.equal(R.bits(big)[:, :, W:], before[:, :, W:]), "the padding of out was written (pad %d)" % pad


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_a_non_finite_element_changes_only_its_own_pair_of_its_own_row(ops, dev, dt, value):
    hd, n_heads, B, T = 16, 3, 2, 5
    c = R.make_case(dt, hd, n_heads, B, T, "shared")
    x, cos, sin = on(dev, c)
    clean = ops.rope_rows(x, cos, sin, n_heads, hd)
    b, t, h, col = 1, 3, 1, 11                                              # second half: its partner is column 3
    xp = x.clone()
    xp[b, t, h * hd + col] = value
    got = ops.rope_rows(xp, cos, sin, n_heads, hd)
    assert R.same_bits(got.cpu(), R.rope_rows(xp.cpu(), c.cos, c.sin, n_heads, hd))
    changed = (R.bits(got) != R.bits(clean)).nonzero().tolist()
    pair = [[b, t, h * hd + col - hd // 2], [b, t, h * hd + col]]
    assert changed and all(p in pair for p in changed), changed
    assert not bool(torch.isfinite(got[b, t, h * hd + col].float())) or not bool(torch.isfinite(got[b, t, h * hd + col - hd // 2].float()))


def test_in_place_and_overlapping_calls_are_refused(ops, dev):
    c = R.make_case("bf16", 16, 3, 2, 70, "shared")
    x, cos, sin = on(dev, c)
    keep = x.clone()
    with pytest.raises(RuntimeError, match="overlap"):
        ops.rope_rows(x, cos, sin, c.n_heads, c.hd, out=x)
    buf = torch.zeros(2 * x.numel(), dtype=x.dtype, device=dev)
    a = buf[:x.numel()].view(x.shape)
    a.copy_(x)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.rope_rows(a, cos, sin, c.n_heads, c.hd, out=buf[8:8 + x.numel()].view(x.shape))
    torch.cuda.synchronize()
    assert torch.equal(R.bits(x), R.bits(keep)) and torch.equal(R.bits(a), R.bits(keep))
    # right behind x is fine
    got = ops.rope_rows(a, cos, sin, c.n_heads, c.hd, out=buf[x.numel():].view(x.shape))
    assert R.same_bits(got.cpu(), c.want)
    for kw in (dict(out=torch.empty(2, 70, 49, dtype=x.dtype, device=dev)), dict(out=torch.empty_like(x, dtype=torch.float32))):
        with pytest.raises(ValueError):
            ops.rope_rows(x, cos, sin, c.n_heads, c.hd, **kw)
    with pytest.raises(ValueError):
        ops.rope_rows(x, cos[:, :5], sin[:, :5], c.n_heads, c.hd)
    with pytest.raises(ValueError):
        ops.rope_rows(x, cos, sin, c.n_heads + 1, c.hd)
