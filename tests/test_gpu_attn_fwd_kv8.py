"""ops.attn_fwd_kv8 (mdg_attn_fwd_kv8: any T straight from the fp8 KV cache) against a float64 softmax over the DEQUANTISED cache within
mdg_attn_fwd's bound 4 u max_j |v_deq| over the admitted keys (u = 2^-9 bf16, 2^-11 f16): the kernel multiplies exactly the
dequantised values, so no new number is needed.  Planes come from tests/test_gpu_kv8.py: B = KV = 2, cap = S + 3, NaN bytes and NaN
scales beyond S, so a row at or beyond S that is read at all shows."""
import pytest
import torch

from tests import attn_ref as R
from tests.test_gpu_kv8 import B, KV, WIDTHS, graded, ops, planes, poisoned_out, reference  # noqa: F401  (ops: a fixture)

pytestmark = pytest.mark.gpu
TS = [(33, 33), (33, 97), (70, 200), (5, 300)]     # partial query and key tiles, S - T no multiple of 32 or 64, several workgroups
GROUPS = [1, 4, 8]                                 # per kv head; T = 5 with G = 8: decode-sized T outside the decode kernel's 32 columns


def within_bound(ops, dev, dt, r_qk, r_vo, G, T, S, causal, mask=None):
    """One call on graded random planes against the float64 reference; returns (out, the operands for a second opinion)."""
    dtype, H, seed = R.DTYPES[dt], KV * G, 1000 * r_qk + 10 * S + G
    q = torch.randn(B, H, T, r_qk, generator=torch.Generator().manual_seed(seed)).to(dtype)
    kd, ks, k = planes(graded((B, KV, S, r_qk), dtype, seed + 1), S + 3, dev, ops)
    vd, vs, v = planes(graded((B, KV, S, r_vo), dtype, seed + 2), S + 3, dev, ops)
    raw = float((q.double() @ k.double().repeat_interleave(G, dim=1).transpose(2, 3)).abs().max())
    scale = min(r_qk ** -0.5, 20.0 / raw)
    adm = (R.admitted(T, S, causal)[None, None] if mask is None else mask).expand(B, H, T, S)
    want, vmax, _ = reference(q, k, v, scale, adm)
    got = ops.attn_fwd_kv8(q.to(dev), kd, ks, vd, vs, S, r_vo, scale, causal=causal, mask=None if mask is None else mask.to(dev),
                           out=poisoned_out((B, T, H, r_vo), dtype, dev)).cpu()
    err, bound = (got.double() - want).abs(), 4.0 * R.UNIT_ROUNDOFF[dt] * vmax
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{dt} qk{r_qk} vo{r_vo} G{G} T{T} S{S} causal={causal} masked={mask is not None}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"T={T}, S={S}: max err / bound = {worst:.3f}"
    return got, (q, kd, ks, vd, vs, scale)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("ts", TS, ids=lambda ts: "T%d-S%d" % ts)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_any_T_from_the_cache_within_the_bound_of_the_dequantised_values(ops, dev, dt, ts, width, G, causal):
    (T, S), dtype = ts, R.DTYPES[dt]
    got, (q, kd, ks, vd, vs, scale) = within_bound(ops, dev, dt, *width, G, T, S, causal)
    if dt == "bf16":       # the path this call replaces stages the same LDS images: equality is expected, printed, not asserted
        two = ops.attn_fwd(q.to(dev), ops.kv8_dequant(kd, ks, S, width[0], dtype), ops.kv8_dequant(vd, vs, S, width[1], dtype), scale,
                           causal=causal).cpu()
        print(f"    against attn_fwd on kv8_dequant: max |diff| = {float((got.float() - two.float()).abs().max()):.3e}")


@pytest.mark.parametrize("width", R.PROBE_WIDTHS, ids=R.width_id)
def test_every_width_template_once(ops, dev, width):
    assert sorted(R.template_of(*w[:2]) for w in R.PROBE_WIDTHS) == sorted(R.TEMPLATES)
    for dt in sorted(R.DTYPES):
        within_bound(ops, dev, dt, width[0], width[1], 2, 70, 200, True)


@pytest.mark.parametrize("Hm", ["one", "per-head"])
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_left_padded_mask_and_a_fully_masked_query(ops, dev, dt, Hm):
    G, T, S = 4, 40, 130
    mask = R.admitted(T, S, True)[None, None].repeat(B, 1 if Hm == "one" else KV * G, 1, 1)   # the causal rule lives in the mask
    mask[1, :, :, :70] = False                                            # batch 1 is left-padded past the first key tile
    mask[0, :, 1, :] = False                                              # a query that sees nothing
    got, _ = within_bound(ops, dev, dt, 90, 77, G, T, S, False, mask=mask)
    assert bool((got[0, 1] == 0).all()), "a fully masked query must give zeros"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: "qk%d-vo%d" % w)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_one_key_wins_by_120_nats_and_its_dequantised_row_comes_back_bit_for_bit(ops, dev, dt, width, G, causal):
    """test_gpu_kv8.py's construction at T = 70, S = 200: column c = i * G + hg of kv head (b, g) owns contraction column p(c) and sign
    s(c) and its winner key w(c) < S - T + 1, admitted for every query; columns that share (p, s) share the winner.  It pins the K
    column order through the converts, the V transposition and key permutation, the GQA map and the row scales (V is graded)."""
    (r_qk, r_vo), dtype, (T, S) = width, R.DTYPES[dt], (70, 200)
    H, n = KV * G, S - T + 1
    k, q = torch.zeros(B, KV, S, r_qk), torch.zeros(B, H, T, r_qk)
    winners = torch.zeros(B, H, T, dtype=torch.int64)
    for b in range(B):
        for g in range(KV):
            for c in range(T * G):
                i, hg = divmod(c, G)
                p, s = (7 * c + 1) % r_qk, -1.0 if (c // r_qk + b + g) % 2 else 1.0
                w = (37 * (c % (2 * r_qk)) + 11 * b + 5 * g) % n
                k[b, g, w, p] = s * 2.0 ** (4 + w % 3)
                q[b, g * G + hg, i, p] = 32.0 * s
                winners[b, g * G + hg, i] = w
    kd, ks, kq = planes(k.to(dtype), S + 3, dev, ops)
    vd, vs, v = planes(graded((B, KV, S, r_vo), dtype, 9 * r_vo + G), S + 3, dev, ops)
    assert torch.equal(kq.float(), k)                                     # powers of two: the cache holds k itself
    _, _, logits = reference(q, kq, v, 0.5, R.admitted(T, S, causal)[None, None].expand(B, H, T, S))
    top2 = logits.topk(2, dim=-1)
    assert torch.equal(top2.indices[..., 0], winners) and bool((top2.values[..., 0] - top2.values[..., 1] > 120).all())
    want = v.repeat_interleave(G, dim=1).gather(2, winners[..., None].expand(-1, -1, -1, r_vo)).transpose(1, 2)
    got = ops.attn_fwd_kv8(q.to(dtype).to(dev), kd, ks, vd, vs, S, r_vo, 0.5, causal=causal).cpu()
    same = R.bits(got) == R.bits(want)
    assert bool(same.all()), f"{int((~same).sum())} entries differ, first at {(~same).nonzero()[0].tolist()}"
