"""Bool masks on both attention kernels (mdg_attn_mask_summary, mdg_attn_fwd_masked, mdg_attn_decode_masked) on the GPU.

  summary     every byte of the tile summary against a torch reduction, over masks that put single elements at the corners of the
              partial edge tile, with expanded (stride 0) axes, per-head masks and rows off 4-byte alignment (the byte path)
  identities  no tolerance: an all-true mask changes nothing; causal=False with the causal rule in the mask equals causal=True
              without one (a skipped tile and a fully masked one both contribute alpha = 1, p = 0)
  one-hot     tests/attn_ref.exact_case with every query's winner masked out (and left padding): the output is the v row of the best
              ADMITTED key bit for bit, a row with nothing admitted is exactly zero; out, summary and workspace start as NaN / 0xff
  bound       random data, |scale * logit| <= 20: |out - fp64 masked softmax| <= 4 u max|v| over the admitted keys
  not read    k rows at masked keys hold +-Inf: same bits as with zeros there

Widths 90 / 77 (the 128 / 128 templates), 64 / 64 and 256 / 256 at every shape; the other six (NQ, NV) templates (EDGE_WIDTHS) at one
prefill and one decode shape each; groups of 4, 3 and 1; bf16 and f16."""
import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

# (r_qk, r_vo, n_heads, n_kv)
WIDTHS = [(90, 77, 8, 2), (64, 64, 4, 4), (256, 256, 2, 2)]
FWD_TS = [(100, 100), (37, 165)]
DECODE_TS = [(1, 63), (1, 64), (1, 65), (1, 300), (4, 63), (4, 64), (4, 65), (4, 300)]
SPLITS = (1, 3, 7)
# The other six (NQ, NV) templates (tests/attn_ref.template_of), at the bucket edges.  WIDTHS keep every (T, S) above; these run one
# prefill and one decode shape each (the fp64 CPU reference of the bound test is what takes the time).
EDGE_WIDTHS = [(62, 65, 4, 4), (30, 129, 6, 2), (66, 33, 8, 2), (128, 255, 4, 4), (130, 64, 8, 2), (200, 128, 2, 2)]
EDGE_FWD_TS = [(37, 165)]
EDGE_DECODE_TS = [(4, 130)]


def fwd_ts(w):
    return FWD_TS if w in WIDTHS else EDGE_FWD_TS


def decode_ts(w):
    return DECODE_TS if w in WIDTHS else EDGE_DECODE_TS


def wid(w):
    return "qk%d-vo%d-h%d-kv%d" % w


@pytest.fixture(scope="module")
def ops(dev):
    from modegpt_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------------------------------------------------------- summary
def summary_ref(mask):
    """[B, Hm, T, S] bool -> uint8 [B, Hm, ceil(T / 32), ceil(S / 64)]: 0 none, 1 all, 2 mixed; positions beyond T, S ignored."""
    Bm, Hm, T, S = mask.shape
    nT, nS = -(-T // 32), -(-S // 64)
    some = torch.zeros(Bm, Hm, nT * 32, nS * 64, dtype=torch.bool)
    every = torch.ones(Bm, Hm, nT * 32, nS * 64, dtype=torch.bool)
    some[:, :, :T, :S] = mask
    every[:, :, :T, :S] = mask
    some = some.view(Bm, Hm, nT, 32, nS, 64).any(dim=5).any(dim=3)
    every = every.view(Bm, Hm, nT, 32, nS, 64).all(dim=5).all(dim=3)
    return torch.where(~some, 0, torch.where(every, 1, 2)).to(torch.uint8)


def causal_pad(Bm, T, S, pads):
    """HF's mask of a left-padded batch: the causal rule ANDed with the padding columns, [Bm, 1, T, S]."""
    i, j = torch.arange(T)[:, None], torch.arange(S)[None, :]
    keep = j <= i + (S - T)
    return torch.stack([keep & (j >= p) for p in pads[:Bm]])[:, None]


def summary_masks(Bm, Hm, T, S):
    gen = torch.Generator().manual_seed(T * 1000 + S + Bm + Hm)
    yield "all-false", torch.zeros(Bm, Hm, T, S, dtype=torch.bool)
    yield "all-true", torch.ones(Bm, Hm, T, S, dtype=torch.bool)
    q_edge, k_edge = (T - 1) // 32 * 32, (S - 1) // 64 * 64                 # the first query / key of the (partial) edge tile
    for qi in sorted({q_edge, T - 1}):
        for kj in sorted({k_edge, S - 1}):
            one = torch.zeros(Bm, Hm, T, S, dtype=torch.bool)
            one[-1, -1, qi, kj] = True
            yield f"one-true-{qi}-{kj}", one
            yield f"one-false-{qi}-{kj}", ~one
    yield "causal-pad", causal_pad(Bm, T, S, [5, 70, 0, 64]).expand(Bm, Hm, T, S).clone()
    yield "random", torch.rand(Bm, Hm, T, S, generator=gen) < 0.5
    blocks = torch.rand(Bm, Hm, -(-T // 32), -(-S // 64), generator=gen)    # whole tiles of each state, so that 0 and 1 occur
    tiles = blocks.repeat_interleave(32, 2).repeat_interleave(64, 3)[:, :, :T, :S]
    yield "random-tiles", torch.where(tiles < 0.3, False, torch.where(tiles < 0.6, True, torch.rand(Bm, Hm, T, S, generator=gen) < 0.5))


@pytest.mark.parametrize("layout", ["contiguous", "batch-stride-0", "query-stride-0", "per-head", "off-by-one-byte"])
def test_summary_every_byte(ops, dev, layout):
    B, H = 2, 4
    T, S = (70, 77) if layout == "off-by-one-byte" else (70, 200)
    Bm = 1 if layout == "batch-stride-0" else B
    Hm = H if layout == "per-head" else 1
    Tm = 1 if layout == "query-stride-0" else T
    for name, base in summary_masks(Bm, Hm, Tm, S):
        if layout == "off-by-one-byte":                                     # rows of 77 bytes from base + 1: no row is 4-byte aligned
            buf = torch.zeros(base.numel() + 1, dtype=torch.bool, device=dev)
            view = buf[1:].view(base.shape)
            view.copy_(base)
            assert view.data_ptr() % 4 == 1
        else:
            view = base.to(dev)
            assert view.data_ptr() % 4 == 0
        mask = view.expand(B, Hm, T, S)
        assert mask.stride(3) == 1 and (Bm == B or mask.stride(0) == 0) and (Tm == T or mask.stride(2) == 0)
        got = ops.attn_mask_summary(mask, B).cpu()
        want = summary_ref(base.expand(B, Hm, T, S))
        assert tuple(got.shape) == (B, Hm, 3, -(-S // 64)) and got.dtype == torch.uint8
        assert torch.equal(got, want), (layout, name, got.tolist(), want.tolist())
        if name == "random-tiles" and layout == "contiguous":
            assert set(want.flatten().tolist()) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------- identities
def _random_qkv(dt, w, T, S, dev, seed=0):
    r_qk, r_vo, H, KV = w
    gen = torch.Generator().manual_seed(seed + 13 * T + S + r_qk)
    dtype = R.DTYPES[dt]
    q = torch.randn(R.B, H, T, r_qk, generator=gen).to(dtype)
    k = torch.randn(R.B, KV, S, r_qk, generator=gen).to(dtype)
    v = torch.randn(R.B, KV, S, r_vo, generator=gen).to(dtype)
    raw = (q.double() @ k.double().repeat_interleave(H // KV, dim=1).transpose(2, 3)).abs().max().item()
    scale = min(float(r_qk) ** -0.5, 20.0 / raw)
    return q, k, v, scale


@pytest.mark.parametrize("w", WIDTHS + EDGE_WIDTHS, ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_identities_bit_for_bit_prefill(ops, dev, dt, w):
    for T, S in fwd_ts(w):
        q, k, v, scale = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in _random_qkv(dt, w, T, S, dev))
        plain = {c: ops.attn_fwd(q, k, v, scale, causal=c) for c in (True, False)}
        ones = torch.ones(1, 1, T, S, dtype=torch.bool, device=dev).expand(R.B, 1, T, S)
        rule = R.admitted(T, S, True).to(dev)[None, None].expand(R.B, 1, T, S)
        for c in (True, False):
            got = ops.attn_fwd(q, k, v, scale, causal=c, mask=ones)
            assert torch.equal(R.bits(got), R.bits(plain[c])), (T, S, "all-true mask, causal", c)
        for c in (True, False):                                             # the rule in the mask, with or without the flag beside it
            got = ops.attn_fwd(q, k, v, scale, causal=c, mask=rule)
            assert torch.equal(R.bits(got), R.bits(plain[True])), (T, S, "causal rule in the mask, causal", c)


@pytest.mark.parametrize("w", WIDTHS + EDGE_WIDTHS, ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_identities_bit_for_bit_decode(ops, dev, dt, w):
    G = w[2] // w[3]
    for T, S in decode_ts(w):
        if T * G > 32:
            continue
        q, k, v, scale = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in _random_qkv(dt, w, T, S, dev))
        ones = torch.ones(1, 1, T, S, dtype=torch.bool, device=dev).expand(R.B, 1, T, S)
        rule = R.admitted(T, S, True).to(dev)[None, None].expand(R.B, 1, T, S)
        for splits in SPLITS:
            plain = {c: ops.attn_decode(q, k, v, scale, causal=c, splits=splits) for c in (True, False)}
            for c in (True, False):
                got = ops.attn_decode(q, k, v, scale, causal=c, splits=splits, mask=ones)
                assert torch.equal(R.bits(got), R.bits(plain[c])), (T, S, splits, "all-true mask, causal", c)
            for c in (True, False):
                got = ops.attn_decode(q, k, v, scale, causal=c, splits=splits, mask=rule)
                assert torch.equal(R.bits(got), R.bits(plain[True])), (T, S, splits, "causal rule in the mask, causal", c)


# ---------------------------------------------------------------------------------------------------------------- one-hot
def _raw_fwd(q, k, v, scale, causal, mask, dev):
    """mdg_attn_mask_summary + mdg_attn_fwd_masked on a 0xff-filled summary (longer than needed) and a NaN-filled out."""
    from modegpt_amd import _lib
    lib = _lib.load()
    B, H, T, r_qk = q.shape
    KV, S, r_vo = k.shape[1], k.shape[2], v.shape[3]
    Hm = mask.shape[1]
    st = [0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3)]
    need = int(lib.mdg_attn_mask_summary_bytes(B, Hm, T, S))
    summary = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((B, T, H, r_vo), float("nan"), dtype=q.dtype, device=dev)
    dtc = _lib.MDG_BF16 if q.dtype == torch.bfloat16 else _lib.MDG_F16
    _lib.check(lib.mdg_attn_mask_summary(mask.data_ptr(), B, Hm, T, S, st[0], st[1], st[2], summary.data_ptr(), need, None),
               "mdg_attn_mask_summary")
    _lib.check(lib.mdg_attn_fwd_masked(q.data_ptr(), k.data_ptr(), v.data_ptr(), dtc, B, T, S, H, KV, r_qk, r_vo, k.stride(0), k.stride(1),
                                       k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 1 if causal else 0, out.data_ptr(),
                                       H * r_vo, None, mask.data_ptr(), Hm, st[0], st[1], st[2], summary.data_ptr(), need),
               "mdg_attn_fwd_masked")
    torch.cuda.synchronize()
    assert bool((summary[need:] == 0xFF).all()), "the summary kernel wrote beyond mdg_attn_mask_summary_bytes"
    assert bool((summary[:need] <= 2).all())
    return out


def _raw_decode(q, k, v, scale, causal, mask, splits, dev):
    """mdg_attn_decode_masked on a NaN-filled workspace (longer than needed) and a NaN-filled out."""
    from modegpt_amd import _lib
    lib = _lib.load()
    B, H, T, r_qk = q.shape
    KV, S, r_vo = k.shape[1], k.shape[2], v.shape[3]
    Hm = mask.shape[1]
    st = [0 if mask.shape[d] == 1 else mask.stride(d) for d in range(3)]
    need = int(lib.mdg_attn_decode_ws_bytes(B, T, H, r_vo, splits)) // 4
    ws = torch.full((need + 64,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((B, T, H, r_vo), float("nan"), dtype=q.dtype, device=dev)
    dtc = _lib.MDG_BF16 if q.dtype == torch.bfloat16 else _lib.MDG_F16
    _lib.check(lib.mdg_attn_decode_masked(q.data_ptr(), k.data_ptr(), v.data_ptr(), dtc, B, T, S, H, KV, r_qk, r_vo, k.stride(0),
                                          k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, 1 if causal else 0,
                                          splits, ws.data_ptr(), need * 4, out.data_ptr(), H * r_vo, None, mask.data_ptr(), Hm,
                                          st[0], st[1], st[2]), "mdg_attn_decode_masked")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need:]).all()), "the kernel wrote beyond mdg_attn_decode_ws_bytes"
    return out


def one_hot_masked(c, pads):
    """From an exact case: per-head masks [B, H, T, S] that remove every query's winner and the left-padding columns pads[b], and
    -- where that leaves several admitted keys within 120 of the best (the construction's zero-logit keys tie) -- all of those but the
    first, so that the fp32 softmax over the admitted keys is again exactly one-hot.  Returns (mask, want [B, T, H, r_vo])."""
    Bq, H, T, _ = c.q.shape
    KV, S, r_vo = c.k.shape[1], c.k.shape[2], c.v.shape[3]
    G = H // KV
    _, logits = R.reference(c.q, c.k, c.v, c.scale, c.causal)                # -inf beyond the causal limit
    j = torch.arange(S)
    adm = torch.isfinite(logits) & (j[None, None, None, :] != c.winners[..., None])
    adm &= (j[None, :] >= torch.tensor(pads)[:, None])[:, None, None, :]
    masked = logits.masked_fill(~adm, float("-inf"))
    best = masked.argmax(dim=-1, keepdim=True)                               # the first of the largest
    near = masked >= masked.gather(3, best) - 120.0
    adm &= ~near | (j[None, None, None, :] == best)
    masked = logits.masked_fill(~adm, float("-inf"))
    some = adm.any(dim=-1)                                                   # [B, H, T]
    probs = torch.softmax(masked.float(), dim=-1).nan_to_num(0.0)
    onehot = torch.zeros_like(probs).scatter_(3, best, 1.0) * some[..., None]
    assert torch.equal(probs, onehot), "the masked exact case is not one-hot in fp32"
    want = c.v.repeat_interleave(G, dim=1).gather(2, best.expand(-1, -1, -1, r_vo))
    want = torch.where(some[..., None], want, torch.zeros_like(want))
    # with the flag, the rule lives in the kernel: hand over a mask that ignores it where it can (beyond the limit: all true)
    return adm, want.transpose(1, 2).contiguous(), some


@pytest.mark.parametrize("pads", [(0, 5), (64, 70)], ids=["pad0-5", "pad64-70"])
@pytest.mark.parametrize("w", WIDTHS + EDGE_WIDTHS, ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_one_hot_best_admitted_key_bit_for_bit_prefill(dev, dt, w, pads):
    r_qk, r_vo, H, KV = w
    empty_rows = 0
    for T, S in fwd_ts(w):
        c = R.exact_case(dt, (r_qk, r_vo, T, S, H, KV), True)
        adm, want, some = one_hot_masked(c, pads)
        empty_rows += int((~some).sum())
        q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
        beyond = ~R.admitted(T, S, True)
        # causal=False: the mask alone decides; causal=True: the mask says "true" beyond the limit and the kernel's rule removes it
        for causal, mask in ((False, adm), (True, adm | beyond)):
            got = _raw_fwd(q, k, v, c.scale, causal, mask.to(dev), dev).cpu()
            same = R.bits(got) == R.bits(want)
            if not bool(same.all()):
                b, i, h, col = (~same).nonzero()[0].tolist()
                raise AssertionError(f"T={T} S={S} causal={causal}: out[{b}, {i}, {h}, {col}] = {float(got[b, i, h, col])!r}, want "
                                     f"{float(want[b, i, h, col])!r}; {int((~same).sum())} entries differ")
    assert pads != (64, 70) or w not in WIDTHS or empty_rows > 0             # T = S = 100 with 70 pads: 70 queries see nothing


@pytest.mark.parametrize("pads", [(0, 5), (64, 70)], ids=["pad0-5", "pad64-70"])
@pytest.mark.parametrize("w", WIDTHS + EDGE_WIDTHS, ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_one_hot_best_admitted_key_bit_for_bit_decode(dev, dt, w, pads):
    r_qk, r_vo, H, KV = w
    G = H // KV
    empty_rows = 0
    for T, S in [(4, 200), (1, 65), (4, 68)] if w in WIDTHS else EDGE_DECODE_TS:
        assert T * G <= 32
        c = R.exact_case(dt, (r_qk, r_vo, T, S, H, KV), True)
        adm, want, some = one_hot_masked(c, pads)
        empty_rows += int((~some).sum())
        q, k, v = c.q.to(dev), c.k.to(dev), c.v.to(dev)
        beyond = ~R.admitted(T, S, True)
        for splits in SPLITS:
            for causal, mask in ((False, adm), (True, adm | beyond)):
                got = _raw_decode(q, k, v, c.scale, causal, mask.to(dev), splits, dev).cpu()
                same = R.bits(got) == R.bits(want)
                if not bool(same.all()):
                    b, i, h, col = (~same).nonzero()[0].tolist()
                    raise AssertionError(f"T={T} S={S} causal={causal} splits={splits}: out[{b}, {i}, {h}, {col}] = "
                                         f"{float(got[b, i, h, col])!r}, want {float(want[b, i, h, col])!r}; "
                                         f"{int((~same).sum())} entries differ")
    assert pads != (64, 70) or w not in WIDTHS or empty_rows > 0             # S = 65, 68 under 70 pads: nothing admitted at all


# ---------------------------------------------------------------------------------------------------------------- bound
def masked_reference(q, k, v, scale, causal, mask):
    """(fp64 masked softmax attention [B, T, H, r_vo] -- zeros where nothing is admitted --, max |v| over the admitted keys)."""
    Bq, H, T, _ = q.shape
    KV, S, r_vo = k.shape[1], k.shape[2], v.shape[3]
    G = H // KV
    adm = mask.expand(Bq, H, T, S) & R.admitted(T, S, causal)
    logits = scale * (q.double() @ k.double().repeat_interleave(G, dim=1).transpose(2, 3))
    probs = torch.softmax(logits.masked_fill(~adm, float("-inf")), dim=-1).nan_to_num(0.0)
    vv = v.double().repeat_interleave(G, dim=1)
    want = (probs @ vv).transpose(1, 2).contiguous()
    vmax = torch.zeros(Bq, H, T, r_vo, dtype=torch.float64)
    for b in range(Bq):
        for h in range(H):
            vmax[b, h] = (adm[b, h][:, :, None] * vv[b, h].abs()[None]).amax(dim=1)
    return want, vmax.transpose(1, 2).contiguous()


def bound_masks(kind, layout, H, T, S, dev, seed):
    """(mask as handed to the kernel, the same mask on the CPU): `layout` is the mask's own extents before expand."""
    Bm = 1 if layout == "batch-stride-0" else R.B
    Tm = 1 if layout == "query-stride-0" else T
    Hm = H if layout == "per-head" else 1
    gen = torch.Generator().manual_seed(seed)
    if kind == "bernoulli":
        base = torch.rand(Bm, Hm, Tm, S, generator=gen) < 0.5
    elif kind == "causal-pad":                                               # (one shared row cannot hold the causal rule: padding alone)
        base = causal_pad(Bm, T, S, [S // 4, 0])[:, :, T - Tm:].expand(Bm, Hm, Tm, S).clone()
    else:
        base = torch.zeros(Bm, Hm, Tm, S, dtype=torch.bool)
        base[..., S - 1] = True
    return base.to(dev).expand(R.B, Hm, T, S), base.expand(R.B, Hm, T, S)


LAYOUTS = ["contiguous", "batch-stride-0", "query-stride-0", "per-head"]


@pytest.mark.parametrize("w", WIDTHS + EDGE_WIDTHS, ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_random_data_within_the_derived_bound(ops, dev, dt, w):
    u = R.UNIT_ROUNDOFF[dt]
    H, G = w[2], w[2] // w[3]
    worst = {"fwd": 0.0, "decode": 0.0}
    for T, S in FWD_TS + [(4, 300), (1, 65)] if w in WIDTHS else EDGE_FWD_TS + EDGE_DECODE_TS:
        q, k, v, scale = _random_qkv(dt, w, T, S, dev, seed=5)
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        for kind in ("bernoulli", "causal-pad", "last-key"):
            for layout in LAYOUTS:
                mask, cpu_mask = bound_masks(kind, layout, H, T, S, dev, seed=T + S)
                for causal in ((False, True) if kind == "bernoulli" else (False,)):
                    want, vmax = masked_reference(q, k, v, scale, causal, cpu_mask)
                    bound = 4.0 * u * vmax
                    runs = [("fwd", ops.attn_fwd(qd, kd, vd, scale, causal=causal, mask=mask))]
                    if T * G <= 32:
                        runs += [("decode", ops.attn_decode(qd, kd, vd, scale, causal=causal, splits=s, mask=mask)) for s in SPLITS]
                    for name, got in runs:
                        err = (got.cpu().double() - want).abs()
                        ratio = float((err / bound.clamp(min=1e-300)).max()) if bool((bound > 0).any()) else 0.0
                        worst[name] = max(worst[name], ratio)
                        assert bool((err <= bound).all()), f"{name} T={T} S={S} {kind} {layout} causal={causal}: err / bound = {ratio:.3f}"
    print(f"{dt} {wid(w)}: largest |out - fp64| / (4 u max|v|): fwd {worst['fwd']:.3f}, decode {worst['decode']:.3f}")


# ---------------------------------------------------------------------------------------------------------------- not read
@pytest.mark.parametrize("w", WIDTHS[:2], ids=wid)
@pytest.mark.parametrize("dt", sorted(R.DTYPES))
def test_k_rows_at_masked_keys_are_not_read_as_logits(ops, dev, dt, w):
    H, G = w[2], w[2] // w[3]
    for T, S in [(100, 100), (37, 165), (4, 300)]:
        q, k, v, scale = _random_qkv(dt, w, T, S, dev, seed=9)
        keep = causal_pad(R.B, T, S, [0, 70])                                # [B, 1, T, S]; a key column is masked for EVERY query of a
        dead = ~keep.any(dim=2)[:, 0]                                        # batch row exactly when it is padding: [B, S]
        assert bool(dead.any())
        sign = torch.where(torch.arange(S) % 2 == 0, float("inf"), float("-inf"))
        k_inf, k_zero = k.clone(), k.clone()
        k_inf[dead[:, None, :].expand(-1, k.shape[1], -1)] = 0               # (shape check of the index)
        for b in range(R.B):
            k_inf[b, :, dead[b]] = sign[dead[b]][None, :, None].to(k.dtype)
            k_zero[b, :, dead[b]] = 0
        mask = keep.to(dev)
        qd, vd = q.to(dev), v.to(dev)
        a = ops.attn_fwd(qd, k_inf.to(dev), vd, scale, causal=False, mask=mask)
        z = ops.attn_fwd(qd, k_zero.to(dev), vd, scale, causal=False, mask=mask)
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(R.bits(a), R.bits(z)), ("fwd", T, S)
        if T * G <= 32:
            for splits in SPLITS:
                a = ops.attn_decode(qd, k_inf.to(dev), vd, scale, causal=False, splits=splits, mask=mask)
                z = ops.attn_decode(qd, k_zero.to(dev), vd, scale, causal=False, splits=splits, mask=mask)
                assert bool(torch.isfinite(a.float()).all()) and torch.equal(R.bits(a), R.bits(z)), ("decode", T, S, splits)


def test_wrapper_refuses_what_it_cannot_pass_on(ops, dev):
    q = torch.zeros(2, 4, 3, 8, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(2, 2, 9, 8, dtype=torch.bfloat16, device=dev)
    ok = torch.ones(2, 1, 3, 9, dtype=torch.bool, device=dev)
    for bad in (ok.float(), ok[0], ok.cpu(), torch.ones(3, 1, 3, 9, dtype=torch.bool, device=dev),
                torch.ones(2, 2, 3, 9, dtype=torch.bool, device=dev), torch.ones(2, 1, 3, 8, dtype=torch.bool, device=dev),
                torch.ones(2, 1, 3, 18, dtype=torch.bool, device=dev)[..., ::2]):
        for fn in (ops.attn_fwd, ops.attn_decode):
            with pytest.raises(ValueError, match="mask"):
                fn(q, k, k, 1.0, mask=bad)
    assert float(ops.attn_fwd(q, k, k, 1.0, mask=ok).float().abs().max()) == 0.0
