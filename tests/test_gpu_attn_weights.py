"""The softmax weight matrix of mdg_attn_fwd, mdg_attn_decode and their _masked entries, read back entry by entry on the GPU.

tests/attn_ref.py's probe: every key of a kv head is the same integer row, so every admitted key of a query has the same logit, and
v is a power of two w(b, g) on one diagonal per window -- out[b, i, h, c] of window j0 is then the weight of key j0 + c, exactly
w / n where the key is admitted (n = the query's admitted keys) and +0 where it is not.  A key that is wrongly admitted or dropped,
counted twice, or whose slot is swapped with another's -- in a mixed tile's bit map, in the permuted V order, at a decode chunk's
edge -- changes an entry from w / n to 0, to 2 w / n or the reverse: nothing hides under a bound.

Accepted per entry: the bits of +0 where the key is not admitted; elsewhere rn_E(x (1 -+ 2^-22)), x = w / n (attn_ref: derived from
the one fp32 reciprocal and the one rounding to the element type; for most n the two coincide and the check is bit equality).  Each
test prints the number of entries where the two differ.

One width per (NQ, NV) template, all nine, bf16 and f16; prefill (70, 200) and (33, 33); decode (1, 300) and (4, 130) at 1, 3, 7 and
256 splits; unmasked causal / full, and Bernoulli, left-padded causal (shallow and down to rows with one and no key), stripes and
whole-tile masks, each with `causal` on and off, in the five mask layouts (contiguous, batch stride 0, query stride 0, per head,
base one byte off 4-byte alignment).  The full mask x layout product runs on every width.  Through the raw C entries the Bernoulli
mask is also presented as uint8 with admitted bytes from {1, 2, 0x80, 0xFF}: same summary bytes, same output bits."""
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_attn_mask import _raw_decode, _raw_fwd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def device_mask(ad, H, T, S, dev):
    """The admission's mask as the kernel gets it: its own extents on the device, expanded to [B, Hm, T, S]."""
    base = ad.base
    if ad.layout == "off-by-one-byte":                      # base + 1: no row start is 4-byte aligned
        buf = torch.zeros(base.numel() + 1, dtype=base.dtype, device=dev)
        view = buf[1:].view(base.shape)
        view.copy_(base)
        assert view.data_ptr() % 4 == 1
    else:
        view = base.to(dev)
        assert view.data_ptr() % 4 == 0
    mask = view.expand(R.B, base.shape[1], T, S)
    assert S == 1 or mask.stride(3) == 1
    return mask


def read_back(run, vs):
    """run(v) -> out [B, T, H, r_vo] for every window, side by side: int16 bits [B, T, H, windows * r_vo] on the device."""
    return torch.cat([run(v) for v in vs], dim=3).contiguous().view(torch.int16)


def check(got, lo, hi, p, ad, width, ctx):
    ok = (got == lo) | (got == hi)
    if bool(ok.all()):
        return
    dtype = p.q.dtype
    b, i, h, key = (~ok).nonzero()[0].tolist()
    G = width[2] // width[3]
    val = lambda t: float(t[b, i, h, key].cpu().view(dtype))
    n = int(ad.adm[b, h, i].sum())
    S = ad.adm.shape[3]
    admitted = bool(ad.adm[b, h, i, key]) if key < S else False
    raise AssertionError(f"{ctx} {ad.name} layout={ad.layout} causal={ad.causal}: weight of key {key} for (b, i, h) = ({b}, {i}, {h}) "
                         f"is {val(got)!r}, want {val(lo)!r}" + (f" or {val(hi)!r}" if val(hi) != val(lo) else "")
                         + f" (w = {float(p.w[b, h // G])}, n = {n}, key admitted: {admitted}); {int((~ok).sum())} entries differ")


def plan(dt, width, T, S, dev):
    """The probe's operands on the device and, per admission, (admission, mask on the device or None, lo, hi) -- built once per (T, S)
    and shared by every run of it (the split counts of decode)."""
    H = width[2]
    p = R.probe_case(dt, width, T, S)
    q, k = p.q.to(dev), p.k.to(dev)
    vs = [R.probe_values(p, dt, j0).to(dev) for j0 in p.windows]
    differ, entries, items = 0, 0, []
    for ad in R.probe_admissions(T, S, H):
        lo, hi, d = R.probe_expected(p, dt, ad.adm, width)
        differ += d
        entries += int(ad.adm.sum())
        items.append((ad, None if ad.base is None else device_mask(ad, H, T, S, dev), lo.to(dev), hi.to(dev)))
    return p, q, k, vs, items, differ, entries


@pytest.mark.parametrize("width", R.PROBE_WIDTHS, ids=R.width_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_prefill_weight_of_every_key(ops, dev, dt, width):
    differ = entries = 0
    for T, S in R.PROBE_FWD_TS:
        p, q, k, vs, items, d, e = plan(dt, width, T, S, dev)
        differ, entries = differ + d, entries + e
        for ad, mask, lo, hi in items:
            got = read_back(lambda v: ops.attn_fwd(q, k, v, p.scale, causal=ad.causal, mask=mask), vs)
            check(got, lo, hi, p, ad, width, f"prefill T={T} S={S}")
    print(f"{dt} {R.width_id(width)} prefill: {differ} of {entries} admitted entries accept two roundings")


@pytest.mark.parametrize("width", R.PROBE_WIDTHS, ids=R.width_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_decode_weight_of_every_key(ops, dev, dt, width):
    differ = entries = 0
    for T, S in R.PROBE_DECODE_TS:
        assert T * (width[2] // width[3]) <= 32
        p, q, k, vs, items, d, e = plan(dt, width, T, S, dev)
        differ, entries = differ + d, entries + e
        for splits in R.PROBE_SPLITS:
            for ad, mask, lo, hi in items:
                got = read_back(lambda v: ops.attn_decode(q, k, v, p.scale, causal=ad.causal, splits=splits, mask=mask), vs)
                check(got, lo, hi, p, ad, width, f"decode T={T} S={S} splits={splits}")
    print(f"{dt} {R.width_id(width)} decode: {differ} of {entries} admitted entries accept two roundings")


# ---------------------------------------------------------------------------------------------------------------- mask bytes
def _raw_summary(mask, Bq, dev):
    """mdg_attn_mask_summary on a 0xff-filled buffer longer than needed: the reported bytes."""
    from modegpt_amd import _lib
    lib = _lib.load()
    Hm, T, S = mask.shape[1], mask.shape[2], mask.shape[3]
    st = [0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3)]
    need = int(lib.mdg_attn_mask_summary_bytes(Bq, Hm, T, S))
    summary = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)
    _lib.check(lib.mdg_attn_mask_summary(mask.data_ptr(), Bq, Hm, T, S, st[0], st[1], st[2], summary.data_ptr(), need, None),
               "mdg_attn_mask_summary")
    torch.cuda.synchronize()
    assert bool((summary[need:] == 0xFF).all()), "the summary kernel wrote beyond mdg_attn_mask_summary_bytes"
    return summary[:need].cpu()


def byte_masks(T, S, H, dev, seed):
    """A per-head Bernoulli mask twice: as 0 / 1 bytes and with every admitted byte drawn from {1, 2, 0x80, 0xFF} (uint8, on the
    device, contiguous: 4-byte loads where S allows them), and the admission on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    adm = torch.rand(R.B, H, T, S, generator=gen) < 0.5
    values = torch.tensor([1, 2, 0x80, 0xFF], dtype=torch.uint8)[torch.randint(0, 4, adm.shape, generator=gen)]
    assert set(values[adm].unique().tolist()) == {1, 2, 0x80, 0xFF}
    return adm.to(torch.uint8).to(dev), torch.where(adm, values, torch.zeros((), dtype=torch.uint8)).to(dev), adm


@pytest.mark.parametrize("width", R.PROBE_WIDTHS, ids=R.width_id)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_any_non_zero_mask_byte_admits(dev, dt, width):
    """The header's contract is one byte per element, non-zero admits: bytes other than 1 through the raw entries, on NaN / 0xff
    filled out, summary and workspace."""
    H = width[2]
    for kernel, T, S in [("fwd",) + ts for ts in R.PROBE_FWD_TS] + [("decode",) + ts for ts in R.PROBE_DECODE_TS]:
        p = R.probe_case(dt, width, T, S)
        q, k = p.q.to(dev), p.k.to(dev)
        vs = [R.probe_values(p, dt, j0).to(dev) for j0 in p.windows]
        ones, mixed, adm = byte_masks(T, S, H, dev, seed=T + 7 * S)
        if kernel == "fwd":
            assert torch.equal(_raw_summary(mixed, R.B, dev), _raw_summary(ones, R.B, dev))
        for causal in (False, True):
            full = adm & R.admitted(T, S, causal)
            lo, hi, _ = R.probe_expected(p, dt, full, width)
            ad = R.Admission("uint8-bernoulli", causal, "per-head", adm, full)
            for splits in ((None,) if kernel == "fwd" else R.PROBE_SPLITS):
                if kernel == "fwd":
                    run = lambda m: read_back(lambda v: _raw_fwd(q, k, v, p.scale, causal, m, dev), vs)
                else:
                    run = lambda m: read_back(lambda v: _raw_decode(q, k, v, p.scale, causal, m, splits, dev), vs)
                got_ones, got_mixed = run(ones), run(mixed)
                assert torch.equal(got_mixed, got_ones), (kernel, T, S, causal, splits, "bytes {1, 2, 0x80, 0xFF} against 0 / 1")
                check(got_mixed, lo.to(dev), hi.to(dev), p, ad, width, f"{kernel} T={T} S={S} splits={splits} uint8")
