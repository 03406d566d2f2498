"""The fp8 KV cache on the GPU: ops.kv8_append / ops.kv8_dequant bit for bit against a torch CPU reference of the layout in
include/modegpt_hip.h, and ops.attn_decode_kv8 against a float64 softmax on the DEQUANTISED cache within mdg_attn_decode's bound
4 u max_j |v_deq| (u = 2^-9 bf16, 2^-11 f16), which needs no new number: the kernel multiplies exactly the dequantised values.

The decode tests build their planes with the CPU reference, not with kv8_append, so each kernel is checked on its own."""
import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu
B, KV = 2, 2
NAN8 = 0x7F                      # e4m3fn's NaN


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


def quantise(x):
    """x [..., r] (values of a bf16 / f16 tensor) -> (e4m3 bytes uint8 [..., r], scale float32 [...]): the smallest power of two with
    amax / scale <= 448 from frexp of the row's amax, 1 for a zero row; torch's round-to-nearest-even conversion of x / scale."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    f, e = torch.frexp(amax)                                              # amax = f 2^e, 0.5 <= f < 1;  448 = 0.875 * 2^9
    ex = torch.where(f <= 0.875, e - 9, e - 8).clamp(-126, 127)
    scale = torch.where(amax == 0, torch.ones_like(amax), torch.ldexp(torch.ones_like(amax), ex))
    q = (xf / scale[..., None]).to(torch.float8_e4m3fn)
    assert float((xf / scale[..., None]).abs().max()) <= 448
    return q.view(torch.uint8), scale


def graded(shape, dtype, seed):
    """Standard normal rows [B, KV, n, r] whose magnitude runs over 2^-6 .. 2^5 across the tokens."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    mag = 2.0 ** ((torch.arange(shape[2]) * 5) % 12 - 6)
    return (x * mag[None, None, :, None]).to(dtype)


def planes(x, cap, dev, ops):
    """The cache that holds x [B, KV, S, r] in its first S rows, NaN-encoded beyond: (data, scale) on the GPU and the dequantised
    values as a CPU tensor of x's dtype."""
    S, r = x.shape[2], x.shape[3]
    q, s = quantise(x)
    data = torch.full((B, KV, cap, ops.kv8_pitch(r)), NAN8, dtype=torch.uint8)
    scale = torch.full((B, KV, cap), float("nan"))
    data[:, :, :S] = 0
    data[:, :, :S, :r] = q
    scale[:, :, :S] = s
    return data.to(dev), scale.to(dev), (q.view(torch.float8_e4m3fn).float() * s[..., None]).to(x.dtype)


@pytest.mark.parametrize("pos", [0, 3])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
@pytest.mark.parametrize("r", [2, 15, 16, 77, 90, 128, 256])
def test_append_matches_the_reference_bit_for_bit_and_dequant_inverts_it(ops, dev, r, dt, T, pos):
    dtype, cap, pitch = R.DTYPES[dt], 12, ops.kv8_pitch(r)
    rows = graded((B, T, KV, r), dtype, 100 * r + 10 * T + pos).clone()   # token-major, as a projection writes V
    rows[0, 0, 0] = 0                                                     # an all-zero row
    rows[1, T - 1, 1] = (rows[1, T - 1, 1].float().clamp(-1, 1) * 0.25).to(dtype)
    rows[1, T - 1, 1, r - 1] = 4.0                                        # amax an exact power of two
    for name, src in (("strided", rows.transpose(1, 2)), ("contiguous", rows.transpose(1, 2).contiguous())):
        data = torch.full((B, KV, cap, pitch), 0xAB, dtype=torch.uint8, device=dev)
        scale = torch.full((B, KV, cap), -7.0, device=dev)
        ops.kv8_append(src.to(dev) if name == "contiguous" else rows.to(dev).transpose(1, 2), data, scale, pos)
        want_q, want_s = quantise(src)
        got, got_s = data.cpu(), scale.cpu()
        assert torch.equal(got_s[:, :, pos:pos + T], want_s), name
        assert torch.equal(got[:, :, pos:pos + T, :r], want_q), name
        assert bool((got[:, :, pos:pos + T, r:] == 0).all()), name + ": padding bytes"
        keep = torch.ones(cap, dtype=torch.bool)
        keep[pos:pos + T] = False
        assert bool((got[:, :, keep] == 0xAB).all()) and bool((got_s[:, :, keep] == -7.0).all()), name + ": other rows were written"
        back = ops.kv8_dequant(data[:, :, pos:].contiguous(), scale[:, :, pos:].contiguous(), T, r, dtype).cpu()
        exact = want_q.view(torch.float8_e4m3fn).float() * want_s[..., None]
        normal = torch.ones_like(exact, dtype=torch.bool) if dt == "bf16" else (exact == 0) | (exact.abs() >= 2.0 ** -14)
        assert torch.equal(back.float()[normal], exact[normal]), name + ": dequant"


WIDTHS = [(6, 3), (90, 77), (128, 128), (130, 200)]
GROUPS = [(4, 1), (1, 3), (8, 4)]                                         # (G, T)
KEYS = (1, 63, 64, 65, 257)
SPLITS = (1, 3, 256)


def reference(q, k, v, scale, adm):
    """float64 softmax attention over the admitted keys (adm bool [B, H, T, S]); a query with none gets zeros: [B, T, H, r_vo]."""
    G = q.shape[1] // KV
    kk, vv = k.double().repeat_interleave(G, dim=1), v.double().repeat_interleave(G, dim=1)
    logits = (scale * (q.double() @ kk.transpose(2, 3))).masked_fill(~adm, float("-inf"))
    p = torch.softmax(logits, dim=-1).masked_fill(~adm.any(-1, keepdim=True), 0.0)
    vmax = (vv.abs()[:, :, None] * adm[..., None]).amax(3)                # [B, H, T, r_vo] over the admitted keys
    return (p @ vv).transpose(1, 2), vmax.transpose(1, 2), logits


def poisoned_out(shape, dtype, dev):
    torch.full((1 << 20,), float("nan"), device=dev)                      # what the call's workspace lands on
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "G%d-T%d" % g)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_decode_from_the_cache_within_the_bound_of_the_dequantised_values(ops, dev, dt, width, group, causal):
    (r_qk, r_vo), (G, T), dtype = width, group, R.DTYPES[dt]
    H = KV * G
    for S in KEYS:
        if causal and S < T:
            continue
        seed = 1000 * r_qk + 10 * S + G
        q = torch.randn(B, H, T, r_qk, generator=torch.Generator().manual_seed(seed)).to(dtype)
        kd, ks, k = planes(graded((B, KV, S, r_qk), dtype, seed + 1), S + 3, dev, ops)
        vd, vs, v = planes(graded((B, KV, S, r_vo), dtype, seed + 2), S + 3, dev, ops)
        raw = float((q.double() @ k.double().repeat_interleave(G, dim=1).transpose(2, 3)).abs().max())
        scale = min(r_qk ** -0.5, 20.0 / raw)
        adm = R.admitted(T, S, causal)[None, None].expand(B, H, T, S)
        want, vmax, _ = reference(q, k, v, scale, adm)
        bound = 4.0 * R.UNIT_ROUNDOFF[dt] * vmax
        for splits in SPLITS:
            out = poisoned_out((B, T, H, r_vo), dtype, dev)
            got = ops.attn_decode_kv8(q.to(dev), kd, ks, vd, vs, S, r_vo, scale, causal=causal, splits=splits, out=out).cpu()
            err = (got.double() - want).abs()
            worst = float((err / bound.clamp(min=1e-300)).max())
            print(f"{dt} qk{r_qk} vo{r_vo} G{G} T{T} S{S} causal={causal} splits={splits}: max err / bound = {worst:.3f}")
            assert bool((err <= bound).all()), f"S={S}, {splits} splits: max err / bound = {worst:.3f}"


@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_decode_under_a_left_padded_mask_and_a_fully_masked_query(ops, dev, dt):
    (r_qk, r_vo), (G, T), S, dtype = (90, 77), (4, 3), 130, R.DTYPES[dt]
    H = KV * G
    q = torch.randn(B, H, T, r_qk, generator=torch.Generator().manual_seed(5)).to(dtype)
    kd, ks, k = planes(graded((B, KV, S, r_qk), dtype, 6), S + 3, dev, ops)
    vd, vs, v = planes(graded((B, KV, S, r_vo), dtype, 7), S + 3, dev, ops)
    mask = R.admitted(T, S, True)[None, None].repeat(B, 1, 1, 1)          # the causal rule lives in the mask
    mask[1, :, :, :70] = False                                            # batch 1 is left-padded past the first tile
    mask[0, :, 1, :] = False                                              # a query that sees nothing
    raw = float((q.double() @ k.double().repeat_interleave(G, dim=1).transpose(2, 3)).abs().max())
    scale = min(r_qk ** -0.5, 20.0 / raw)
    want, vmax, _ = reference(q, k, v, scale, mask.expand(B, H, T, S))
    for splits in SPLITS:
        got = ops.attn_decode_kv8(q.to(dev), kd, ks, vd, vs, S, r_vo, scale, causal=False, splits=splits, mask=mask.to(dev),
                                  out=poisoned_out((B, T, H, r_vo), dtype, dev)).cpu()
        assert bool((got[0, 1] == 0).all()), "a fully masked query must give zeros"
        assert bool(((got.double() - want).abs() <= 4.0 * R.UNIT_ROUNDOFF[dt] * vmax).all()), splits


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "G%d-T%d" % g)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_one_key_wins_by_120_nats_and_its_dequantised_row_comes_back_bit_for_bit(ops, dev, dt, width, group, causal):
    """Column c = i * G + hg of kv head (b, g) owns contraction column p(c) and sign s(c); its winner key w(c) -- admitted for every
    query -- carries s 2^(4 + w % 3) in column p and the query 32 s there: the winner's scaled logit is >= 256 and every other admitted
    key's is <= 0, so the fp32 weights are exactly one-hot.  Wherever 2 r_qk >= T G every (query, head) has a (p, s) of its own;
    p runs over all k-steps of the first product, so a wrong column permutation selects another key or none."""
    (r_qk, r_vo), (G, T), dtype, S = width, group, R.DTYPES[dt], 257
    H, n = KV * G, 257 - T + 1
    k = torch.zeros(B, KV, S, r_qk)
    q = torch.zeros(B, H, T, r_qk)
    winners = torch.zeros(B, H, T, dtype=torch.int64)
    for b in range(B):
        for g in range(KV):
            for c in range(T * G):
                i, hg = divmod(c, G)
                p, s = (7 * c + 1) % r_qk, -1.0 if (c // r_qk + b + g) % 2 else 1.0
                w = (37 * (c % (2 * r_qk)) + 11 * b + 5 * g) % n          # columns that share (p, s) share the winner
                k[b, g, w, p] = s * 2.0 ** (4 + w % 3)
                q[b, g * G + hg, i, p] = 32.0 * s
                winners[b, g * G + hg, i] = w
    kd, ks, kq = planes(k.to(dtype), S + 3, dev, ops)
    vd, vs, v = planes(graded((B, KV, S, r_vo), dtype, 9 * r_vo + G), S + 3, dev, ops)
    assert torch.equal(kq.float(), k)                                     # powers of two: the cache holds k itself
    adm = R.admitted(T, S, causal)[None, None].expand(B, H, T, S)
    _, _, logits = reference(q, kq, v, 0.5, adm)
    top2 = logits.topk(2, dim=-1)
    assert torch.equal(top2.indices[..., 0], winners) and bool((top2.values[..., 0] - top2.values[..., 1] > 120).all())
    want = v.repeat_interleave(G, dim=1).gather(2, winners[..., None].expand(-1, -1, -1, r_vo)).transpose(1, 2)
    for splits in SPLITS:
        got = ops.attn_decode_kv8(q.to(dtype).to(dev), kd, ks, vd, vs, S, r_vo, 0.5, causal=causal, splits=splits).cpu()
        same = R.bits(got) == R.bits(want)
        assert bool(same.all()), f"{splits} splits: {int((~same).sum())} entries differ, first at {(~same).nonzero()[0].tolist()}"
