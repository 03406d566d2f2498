"""GPU: mdg_rope_gather at every dispatch variant of csrc/rope.hip, with and without the masked RMSNorm, in bf16 / f16 / f32.

The cases, their inputs and the reference are tests/rope_ref.py's (checked on the CPU by test_rope_ref_host.py, which also
proves that the cases' declared variants cover every template instantiation and run-time fork).  Per case here:

  * the plan of the REAL operands (ops.rope_gather_plan) is the variant the case declares;
  * without the norm the output equals the oracle bit for bit; with it every element lies inside the reference interval
    (a single number on all but a capped share of elements for the half types) and is finite -- the all-zero row, the row
    at RMS 1e-3 and the row containing 60000 included;
  * the output lives inside a buffer filled with a NaN pattern: every element is written, no byte around it is touched;
  * a NaN row changes its own outputs only (the per-unit inv select, the 16-lane and 4-lane sums stay in their rows).
"""
import pytest
import torch

from tests import rope_ref as R

pytestmark = pytest.mark.gpu

PAD = 256                                                   # elements of sentinel before and after the output (keeps 512-byte alignment)
SENTINEL = {2: (torch.int16, 0x7FC1), 4: (torch.int32, 0x7FC10001)}   # a NaN of every dtype: no finite result equals it


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def _bits(t):
    return t.view(SENTINEL[t.element_size()][0])


def _at_offset(t, off, dev):
    """t on the device as a contiguous view starting `off` elements into a fresh buffer."""
    flat = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run(ops, dev, name, dt, norm, x_bthr=None):
    """-> (out [B, H, T, r] on the CPU, its whole sentinel buffer as integers on the CPU, plan of the real operands)."""
    i = R.make_inputs(name, dt)
    layout, o = R.SHAPES[name][6], R.offsets(name)
    B, T, H, r = i.dims
    x = (i.x if x_bthr is None else x_bthr).reshape(B, T, H * r)
    if layout == "slice":
        wide = torch.zeros(B, T, o["ld_x"], dtype=x.dtype, device=dev)
        wide[:, :, 1:1 + H * r] = x.to(dev)
        xd = wide[:, :, 1:1 + H * r]
    else:
        xd = x.contiguous().to(dev)
    cos, sin = _at_offset(i.cos, o["cs"], dev), _at_offset(i.sin, o["cs"], dev)
    w = _at_offset(i.w, o["nw"], dev) if norm else None
    mask = None if i.rope_mask is None else i.mask.to(dev)
    n = B * H * T * r
    it, pattern = SENTINEL[x.element_size()]
    buf = torch.full((PAD + o["out"] + n + PAD,), pattern, dtype=it, device=dev).view(x.dtype)
    out = buf[PAD + o["out"]:PAD + o["out"] + n].view(B, H, T, r)
    plan = ops.rope_gather_plan(xd, cos, sin, mask, H, i.n_kv, i.hd, norm_weight=w, eps=R.EPS, out=out)
    got = ops.rope_gather(xd, cos, sin, mask, H, i.n_kv, i.hd, norm_weight=w, eps=R.EPS, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return got.cpu(), _bits(buf).cpu(), plan


def _check_containment(name, buf_bits, n):
    off = PAD + R.offsets(name)["out"]
    pattern = SENTINEL[buf_bits.element_size()][1]
    assert (buf_bits[:off] == pattern).all(), "bytes before the output were written"
    assert (buf_bits[off + n:] == pattern).all(), "bytes after the output were written"
    unwritten = (buf_bits[off:off + n] == pattern).sum().item()
    assert unwritten == 0, f"{unwritten} of {n} output elements were never written"


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_rope_variant(ops, dev, name, dt, norm):
    got, buf_bits, plan = _run(ops, dev, name, dt, norm)
    print(f"{name} {dt} norm={norm}: {R.variant_of(plan)} grid {plan['grid']} lds {plan['lds']}")
    assert R.variant_of(plan) == R.declared(name, dt, norm)
    _check_containment(name, buf_bits, got.numel())
    plain, (lo, hi) = R.reference(name, dt)
    if not norm:
        diff = (_bits(got) != _bits(plain)).nonzero()
        assert len(diff) == 0, f"{len(diff)} elements differ, [b, h, t, j] got want: " + "; ".join(
            f"{d.tolist()} {got[tuple(d)].item():.9g} {plain[tuple(d)].item():.9g}" for d in diff[:8])
        return
    ok = R.inside(got, lo, hi)
    share = R.nondegenerate_share(lo, hi)
    print(f"   inside {ok.double().mean().item():.6f}, non-degenerate {share:.4%}")
    assert torch.isfinite(got.float()).all()
    for what, (b, t, h) in R.SPECIAL.items():
        assert ok[b, h, t].all(), f"{what} row: {(~ok[b, h, t]).sum().item()} elements outside the interval"
    bad = (~ok).sum().item()
    assert bad == 0, f"{bad} of {ok.numel()} elements outside the interval"
    assert share <= R.NONDEGENERATE_CAP[dt]


# direct: HPT 4 (four heads of one token per thread group), HPT 1 (four tokens, dead ones in the last groups), the
# pre-pass; tile: CH 4 with several token tiles
@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("name", ["qwen_full_perm", "group5", "vec2_prepass", "tile_odd_ch4"])
def test_nan_row_stays_in_its_row(ops, dev, name, dt):
    i = R.make_inputs(name, dt)
    B, T, H, r = i.dims
    b, t, h = B - 1, T // 2, 1
    clean, _, plan = _run(ops, dev, name, dt, True)
    x = i.x.clone()
    x[b, t, h] = float("nan")
    dirty, buf_bits, plan2 = _run(ops, dev, name, dt, True, x_bthr=x)
    assert R.variant_of(plan) == R.variant_of(plan2) == R.declared(name, dt, True)
    _check_containment(name, buf_bits, dirty.numel())
    assert torch.isnan(dirty[b, h, t].float()).all()          # every output of the row depends on its own inv
    same = _bits(clean) == _bits(dirty)
    same[b, h, t] = True
    assert same.all(), f"{(~same).sum().item()} elements of OTHER rows changed: {(~same).nonzero()[:8].tolist()}"
