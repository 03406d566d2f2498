"""ops.rope_kv8_step / ops.rope_kv8_paged_step on the GPU: q_out and k_out against the CPU rotation of tests/rope_ref.py (bit for bit
without a norm, inside norm_rope_interval with one), the cache rows against tests/test_gpu_kv8.py's quantise of the call's own k_out
and of v byte for byte, every other byte of the planes / pools still the fill, and -- without a norm -- the planes / pools of
ops.rope_gather + ops.kv8_append / ops.kv8_paged_append."""
import functools

import pytest
import torch

from tests import attn_ref as R
from tests import rope_ref
from tests.test_gpu_kv8 import graded, quantise

pytestmark = pytest.mark.gpu
B, KV, EPS = 3, 2, 1e-6
HD = {6: 16, 90: 128, 256: 256}
CAP, POS = 70, 63                                                         # contiguous planes: rows 63 .. 63 + T - 1 of 70
TABLE = torch.tensor([[7, 2], [0, 8], [5, 1]], dtype=torch.int32)         # shuffled, non-monotone; pages 3, 4, 6 belong to nobody
CASES = [(w, m) for w in ((6, 3), (90, 77), (256, 256)) for m in (True,) + ((False,) if w[0] == 256 else ())]


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def case(dt, width, G, T, masked):
    """CPU inputs and references of one shape, computed once: q [B, T, H*r_qk], k [B, T, KV*r_qk], v token-major, cos / sin, mask, the
    two norm weights; per side (q, k) the plain rotation and the norm's interval, each [B, heads, T, r_qk]."""
    (r_qk, r_vo), dtype, hd, H = width, R.DTYPES[dt], HD[width[0]], KV * G
    seed = 1000 * r_qk + 10 * G + T
    gen = torch.Generator().manual_seed(seed)
    q = graded((B, H, T, r_qk), dtype, seed + 1).transpose(1, 2).contiguous()            # [B, T, heads, r]
    k = graded((B, KV, T, r_qk), dtype, seed + 2).transpose(1, 2).contiguous()
    k[0, 0, 0] = 0                                                                        # an all-zero K row
    v = graded((B, T, KV, r_vo), dtype, seed + 3)                                         # as a projection writes V
    ang = torch.rand(1 if masked else B, T, hd // 2, generator=gen) * 6.28
    emb = torch.cat((ang, ang), -1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    idx = torch.stack([torch.randperm(hd // 2, generator=gen)[:r_qk // 2] for _ in range(KV)])
    mask = torch.cat((idx, idx + hd // 2), dim=1) if masked else None
    nmask = mask if masked else torch.arange(hd).repeat(KV, 1)
    w = [torch.randn(hd, generator=gen).to(dtype) for _ in range(2)]
    ref = [(rope_ref.rotate(x.transpose(1, 2), cos, sin, mask, KV),
            rope_ref.norm_rope_interval(x, wt, EPS, nmask, KV, cos, sin, rope_mask=mask)) for x, wt in ((q, w[0]), (k, w[1]))]
    return q.reshape(B, T, -1), k.reshape(B, T, -1), v, cos, sin, mask, w, ref


def empty_pools(ops, width, page, dev):
    first, rows = (B, CAP) if page is None else (9, page)
    return [(torch.full((first, KV, rows, ops.kv8_pitch(r)), 0xAB, dtype=torch.uint8, device=dev),
             torch.full((first, KV, rows), -7.0, device=dev)) for r in width]


def run(ops, dev, dt, width, G, T, norm, masked, page):
    q, k, v, cos, sin, mask, w, ref = case(dt, width, G, T, masked)
    H, hd = KV * G, HD[width[0]]
    to = lambda t: None if t is None else t.to(dev)                       # noqa: E731
    qd, kd, vd, m = to(q), to(k), to(v).transpose(1, 2), to(mask)
    kw = dict(q_norm_weight=to(w[0]), k_norm_weight=to(w[1]), eps=EPS) if norm else {}
    pos = (0, page - 2, page) if page else (POS,) * B
    where = (TABLE.to(dev), torch.tensor(pos, dtype=torch.int32).to(dev)) if page else (POS,)
    step = ops.rope_kv8_paged_step if page else ops.rope_kv8_step

    pools = empty_pools(ops, width, page, dev)
    q_out, k_out = step(qd, kd, vd, to(cos), to(sin), m, H, KV, hd, pools[0], pools[1], *where, k_out=True, **kw)
    for name, got, (plain, (lo, hi)) in zip("qk", (q_out.cpu(), k_out.cpu()), ref):
        if norm:
            assert bool(rope_ref.inside(got, lo, hi).all()), f"{name}_out leaves the norm's interval"
        else:
            assert torch.equal(R.bits(got), R.bits(plain)), f"{name}_out differs from the rotation"
    for (data, scale), src, r in zip(pools, (k_out.cpu(), v.transpose(1, 2)), width):
        want_d, want_s = (t.cpu() for t in empty_pools(ops, (r,), page, "cpu")[0])
        q8, s = quantise(src)
        for b in range(B):
            for t in range(T):
                i, off = (int(TABLE[b, (pos[b] + t) // page]), (pos[b] + t) % page) if page else (b, POS + t)
                want_d[i, :, off] = 0                                     # the padding bytes
                want_d[i, :, off, :r] = q8[b, :, t]
                want_s[i, :, off] = s[b, :, t]
        assert torch.equal(data.cpu(), want_d) and torch.equal(scale.cpu(), want_s), f"r={r}: the cache differs from the reference"
    if not norm:                                                          # the chain this call replaces, on a second set
        chain = empty_pools(ops, width, page, dev)
        k_rot = ops.rope_gather(kd, to(cos), to(sin), m, KV, KV, hd)
        assert torch.equal(R.bits(ops.rope_gather(qd, to(cos), to(sin), m, H, KV, hd)), R.bits(q_out))
        if page:
            ops.kv8_paged_append(k_rot, vd, chain[0], chain[1], *where)
        else:
            ops.kv8_append(k_rot, *chain[0], POS)
            ops.kv8_append(vd, *chain[1], POS)
        assert all(torch.equal(a, b) for x, y in zip(pools, chain) for a, b in zip(x, y)), "not the chain's bytes"
    if (dt, width, G, T, norm) == ("bf16", (90, 77), 4, 5, True):          # a decode-style call: no bf16 k at all
        again = empty_pools(ops, width, page, dev)
        q2, none = step(qd, kd, vd, to(cos), to(sin), m, H, KV, hd, again[0], again[1], *where, **kw)
        assert none is None and torch.equal(R.bits(q2), R.bits(q_out))
        assert all(torch.equal(a, b) for x, y in zip(pools, again) for a, b in zip(x, y)), "k_out=None changed the cache"


PARAMS = [pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"]),
          pytest.mark.parametrize("T", [1, 5]),
          pytest.mark.parametrize("G", [1, 4]),
          pytest.mark.parametrize("width,masked", CASES, ids=lambda c: ("qk%d-vo%d" % c) if isinstance(c, tuple) else ("mask" if c else "nomask")),
          pytest.mark.parametrize("dt", sorted(R.DTYPES))]


def parametrised(fn):
    for p in PARAMS:
        fn = p(fn)
    return fn


@parametrised
def test_contiguous_step_gives_the_rotation_and_the_append_bytes(ops, dev, dt, width, masked, G, T, norm):
    run(ops, dev, dt, width, G, T, norm, masked, None)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
def test_a_group_of_16_takes_its_18_rows_in_two_chunks(ops, dev, norm):
    run(ops, dev, "bf16", (90, 77), 16, 5, norm, True, None)


@pytest.mark.parametrize("page", [64, 128])
@parametrised
def test_paged_step_gives_the_rotation_and_the_append_bytes(ops, dev, dt, width, masked, G, T, norm, page):
    run(ops, dev, dt, width, G, T, norm, masked, page)
