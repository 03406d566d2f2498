"""Cases and the float64 CPU reference for mdg_attn_fwd (tests/test_gpu_attn_fwd.py).

Two kinds of data on one shape list:
  exact    q and k are small exact integers such that every query has ONE admitted key whose scaled logit is more than 120 above
           every other admitted key: every other fp32 probability underflows to exactly zero, the winner's is exactly one, and
           out[b, i, h, :] must equal v[b, g, j*(i), :] bit for bit.  Checked here, on the CPU, when the case is built.
  random   standard normal q, k, v with the scale chosen so that |scale * logit| <= 20; bound 4 u max_j |v| entry-wise.

How the exact case picks its winners with only two logical columns (r_qk = 2 must work).  Key j carries the pair (x_j, y_j):
  x_j = max(0, j - (S - T) + 1)      strictly increasing over the causal limits of the queries: the largest admitted x is the
                                     DIAGONAL key j = i + S - T, and key j + 1, just beyond the limit, carries a larger logit
  y_j = -1 at key 0, +rank at the keys b - 1 and b of every multiple b of 32 (both sides of every key-tile boundary of the
        kernel, 32 and 64), 0 elsewhere
and query (i, h) carries 256 * e with e one of (1, 0): the diagonal (non-causal: the last key); (0, -1): key 0; (0, 1): the last
boundary key it sees (when it sees none: the diagonal).  With scale 0.5 the scaled gap is 128 per unit.  The pair sits in column
pair (i + h) mod (r_qk / 2) of q and is repeated in every column pair of k, so every k-step of the first product is used; kv
head (b, g) carries sign (-1)^(b + g) on k and its queries on q, so the keys of a wrong head or batch select the wrong winner.
v holds bit patterns that differ between neighbours in every index (b, g, j, c)."""
import bisect
import functools
from collections import namedtuple

import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT_ROUNDOFF = {"bf16": 2.0 ** -9, "f16": 2.0 ** -11}

# (r_qk, r_vo, T, S, n_heads, n_kv): every width, every (T, S) and every group size of the issue at least once
SHAPES = [
    (2, 1, 1, 1, 1, 1),
    (2, 7, 5, 70, 4, 1),
    (6, 33, 31, 31, 8, 1),
    (30, 64, 64, 64, 4, 4),
    (64, 77, 65, 65, 8, 2),
    (90, 77, 200, 200, 8, 2),
    (90, 128, 129, 300, 8, 1),
    (128, 128, 200, 200, 4, 1),
    (130, 255, 1, 257, 8, 2),
    (130, 33, 64, 64, 4, 1),
    (256, 256, 129, 300, 2, 2),
    (256, 1, 65, 65, 8, 1),
    (128, 256, 5, 70, 4, 4),
    (30, 129, 65, 65, 4, 2),     # template (4, 8); the first r_vo of the widest v bucket
    (66, 64, 37, 165, 8, 2),     # template (8, 2); the first r_qk of the middle bucket
    (200, 65, 70, 200, 6, 2),    # template (16, 4); the first r_vo of the middle bucket; G = 3
]
B = 2

# The kernels' template buckets: NQ k-steps of 16 over r_qk, NV column tiles of 32 over r_vo.
TEMPLATES = [(nq, nv) for nq in (4, 8, 16) for nv in (2, 4, 8)]


def template_of(r_qk, r_vo):
    """(NQ, NV) of the attn_fwd_kernel / attn_decode_kernel instantiation that serves head widths (r_qk, r_vo): r_qk <= 64 / <= 128 /
    else -> NQ = 4 / 8 / 16 and r_vo <= 64 / <= 128 / else -> NV = 2 / 4 / 8.  These buckets mirror launch_attn_q / launch_attn_v
    (csrc/attn.hip) and launch_decode_q / launch_decode_v (csrc/attn_decode.hip): both must change together, or
    tests/test_attn_templates_host.py stops telling which instantiations the shape lists run."""
    nq = 4 if r_qk <= 64 else 8 if r_qk <= 128 else 16
    nv = 2 if r_vo <= 64 else 4 if r_vo <= 128 else 8
    return nq, nv


# The trip-count sweep: inside a template the k-step loop runs to nq = ceil(r_qk / 16) and the column-tile loop to nv = ceil(r_vo / 32).
# Every nq once with r_qk = 16 nq - 2, paired with nv = ((nq - 1) % 8) + 1 at both ends of the last column tile.
SWEEP = [(16 * nq - 2, r_vo) for nq in range(1, 17) for r_vo in (32 * (((nq - 1) % 8) + 1) - 31, 32 * (((nq - 1) % 8) + 1) - 1)]
SWEEP_HEADS = (2, 1)
SWEEP_FWD_TS = (33, 70)
SWEEP_DECODE_TS = (16, 70)       # the decode kernel's domain is T * G <= 32: with the sweep's group of 2, the full tile


def sweep_shapes(ts):
    return [(r_qk, r_vo) + ts + SWEEP_HEADS for r_qk, r_vo in SWEEP]

Case = namedtuple("Case", "q k v scale causal want vmax winners")


def shape_id(s):
    return "qk%d-vo%d-T%d-S%d-h%d-kv%d" % s


def admitted(T, S, causal):
    """bool [T, S]: key j is seen by query i."""
    if not causal:
        return torch.ones(T, S, dtype=torch.bool)
    i = torch.arange(T)[:, None]
    j = torch.arange(S)[None, :]
    return j <= i + (S - T)


def reference(q, k, v, scale, causal):
    """float64 softmax attention from the 16-bit inputs: [B, T, n_heads, r_vo] float64."""
    Bq, H, T, _ = q.shape
    KV, S = k.shape[1], k.shape[2]
    G = H // KV
    kk = k.double().repeat_interleave(G, dim=1)
    vv = v.double().repeat_interleave(G, dim=1)
    logits = scale * (q.double() @ kk.transpose(2, 3))
    logits = logits.masked_fill(~admitted(T, S, causal), float("-inf"))
    return (torch.softmax(logits, dim=-1) @ vv).transpose(1, 2).contiguous(), logits


def v_max_admitted(v, T, n_heads, causal):
    """max over the admitted keys of |v[b, g, j, c]| as [B, T, n_heads, r_vo] float64."""
    Bv, KV, S, r = v.shape
    run = torch.cummax(v.double().abs(), dim=2).values                       # [B, KV, S, r]
    lim = torch.arange(T) + (S - T) if causal else torch.full((T,), S - 1)
    per_q = run[:, :, lim]                                                   # [B, KV, T, r]
    return per_q.repeat_interleave(n_heads // KV, dim=1).transpose(1, 2).contiguous()


def _distinct_v(dt, KV, S, r_vo):
    """Finite normal values of moderate size whose bit patterns differ between neighbours in b, g, j and c."""
    n = B * KV * S * r_vo
    idx = torch.arange(n, dtype=torch.int64)
    if dt == "bf16":
        lo, span = 0x3000, 0x1f00          # 2^-31 .. 2^31: partial sums of a few hundred stay far from overflow in fp32
    else:
        lo, span = 0x0400, 0x7000          # normal f16 up to 2^13
    bits = lo + (idx * 2477 + (idx // r_vo) * 911 + (idx // (r_vo * S)) * 5003) % span
    bits = bits | ((idx * 7 // 3) % 2) * 0x8000
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return bits.to(torch.int16).view(DTYPES[dt]).reshape(B, KV, S, r_vo).clone()


@functools.lru_cache(maxsize=None)
def exact_case(dt, shape, causal):
    r_qk, r_vo, T, S, H, KV = shape
    G, shift, pairs = H // KV, S - T, r_qk // 2
    dtype = DTYPES[dt]
    j = torch.arange(S)
    x = (j - shift + 1).clamp(min=0).double()
    y = torch.zeros(S, dtype=torch.float64)
    rank = 0
    for b32 in range(32, S, 32):
        for key in (b32 - 1, b32):
            rank += 1
            y[key] = rank
    y[0] = -1.0 if S > 1 else 0.0
    assert x.max() <= 256 and y.max() <= 256
    k = torch.zeros(B, KV, S, r_qk, dtype=torch.float64)
    q = torch.zeros(B, H, T, r_qk, dtype=torch.float64)
    winners = torch.zeros(B, H, T, dtype=torch.int64)
    special = [key for key in range(31, S) if y[key] > 0]
    for b in range(B):
        for g in range(KV):
            sign = -1.0 if (b + g) % 2 else 1.0
            k[b, g, :, 0::2] = sign * x[:, None]
            k[b, g, :, 1::2] = sign * y[:, None]
            for hg in range(G):
                h = g * G + hg
                for i in range(T):
                    lim = i + shift if causal else S - 1
                    mode = (i + h) % 3
                    seen = special[:bisect.bisect_right(special, lim)]
                    if mode == 2 and not seen:
                        mode = 0
                    if mode == 1 and S == 1:
                        mode = 0
                    p = (i + h) % pairs
                    if mode == 0:
                        q[b, h, i, 2 * p], winners[b, h, i] = 256.0 * sign, lim
                    elif mode == 1:
                        q[b, h, i, 2 * p + 1], winners[b, h, i] = -256.0 * sign, 0
                    else:
                        q[b, h, i, 2 * p + 1], winners[b, h, i] = 256.0 * sign, seen[-1]
    q, k = q.to(dtype), k.to(dtype)
    v = _distinct_v(dt, KV, S, r_vo)
    scale = 0.5
    # the reference's fp32 probabilities are exactly one-hot at the chosen key, and the runner-up is more than 120 below
    _, logits = reference(q, k, v, scale, causal)
    probs = torch.softmax(logits.float(), dim=-1)
    onehot = torch.zeros_like(probs).scatter_(3, winners[..., None], 1.0)
    assert torch.equal(probs, onehot), "the exact case is not one-hot in fp32"
    if S > 1:
        top2 = logits.topk(2, dim=-1).values
        gap = top2[..., 0] - top2[..., 1]
        assert bool((gap[torch.isfinite(gap)] > 120).all())
    want = v.repeat_interleave(G, dim=1).gather(2, winners[..., None].expand(-1, -1, -1, r_vo))           # [B, H, T, r_vo]
    return Case(q, k, v, scale, causal, want.transpose(1, 2).contiguous(), None, winners)


@functools.lru_cache(maxsize=None)
def random_case(dt, shape, causal, scale_factor=1.0):
    r_qk, r_vo, T, S, H, KV = shape
    gen = torch.Generator().manual_seed(1000 * r_qk + 7 * r_vo + T + 3 * S + H + (1 if causal else 0))
    dtype = DTYPES[dt]
    q = torch.randn(B, H, T, r_qk, generator=gen).to(dtype)
    k = torch.randn(B, KV, S, r_qk, generator=gen).to(dtype)
    v = torch.randn(B, KV, S, r_vo, generator=gen).to(dtype)
    raw = (q.double() @ k.double().repeat_interleave(H // KV, dim=1).transpose(2, 3)).abs().max().item()
    scale = min(float(r_qk) ** -0.5, 20.0 / max(raw, 1e-30)) * scale_factor
    assert scale * raw <= 20.0
    want, _ = reference(q, k, v, scale, causal)
    return Case(q, k, v, scale, causal, want, v_max_admitted(v, T, H, causal), None)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- the weight probe
# Inputs that make the kernel's output the softmax weight matrix itself (tests/test_gpu_attn_weights.py).  Every key of a kv head
# (b, g) is the SAME row kappa of small integers, so every admitted key of a query has the same fp32 logit: t - m is exactly 0,
# every p is exactly 1, every alpha and every wave's / chunk's 2^(m_s - M) is exactly 1.  v[b, g, j, c] = w(b, g) where j == j0 + c
# and 0 elsewhere, w a power of two: the fp32 accumulator of out[b, i, h, c] is exactly w if key j0 + c is admitted for the query
# and 0 otherwise, the denominator is exactly n = the number of admitted keys of the query, and the stored value is
# (E)(acc * (1.0f / n)).  Windows j0 = 0, r_vo, 2 r_vo, ... read every key's weight back exactly once.
# Accepted per entry (derived, not tuned): where the key is not admitted, or n == 0, the bits of +0; elsewhere one of
# rn_E(x (1 - 2^-22)), rn_E(x (1 + 2^-22)) with x = w / n and rn_E = fp64 -> fp32 -> element type, the way the kernel's value travels:
# 1.0f / den is within one fp32 ulp (2^-23) of 1 / n whether it is a correctly rounded divide or a reciprocal, doubled; the product
# with the power of two w is exact.  For most n the two coincide and the check is bit equality.

# (r_qk, r_vo, n_heads, n_kv): one width per (NQ, NV) template at the bucket edges; groups of 4, 1 and 3
PROBE_WIDTHS = [
    (64, 64, 8, 2),       # (4, 2)
    (62, 65, 4, 4),       # (4, 4)
    (30, 129, 6, 2),      # (4, 8), G = 3
    (66, 33, 8, 2),       # (8, 2)
    (90, 77, 8, 2),       # (8, 4)
    (128, 255, 4, 4),     # (8, 8)
    (130, 64, 8, 2),      # (16, 2)
    (200, 128, 4, 4),     # (16, 4)
    (256, 256, 2, 2),     # (16, 8)
]
PROBE_FWD_TS = [(70, 200), (33, 33)]       # three query tiles and four key tiles, both partial, S - T no multiple of 32; one tile
PROBE_DECODE_TS = [(1, 300), (4, 130)]
PROBE_SPLITS = (1, 3, 7, 256)              # 256: empty chunks and waves without a tile
PROBE_LAYOUTS = ["contiguous", "batch-stride-0", "query-stride-0", "per-head", "off-by-one-byte"]
PROBE_KINDS = ["bernoulli", "causal-pad", "causal-pad-deep", "stripes", "tiles"]

Probe = namedtuple("Probe", "q k scale w windows r_vo")
Admission = namedtuple("Admission", "name causal layout base adm")


def width_id(w):
    return "qk%d-vo%d-h%d-kv%d" % w


@functools.lru_cache(maxsize=None)
def probe_case(dt, width, T, S):
    """q [B, H, T, r_qk], k [B, KV, S, r_qk] of the probe, w [B, KV] and the window starts; v comes from probe_values per window."""
    r_qk, r_vo, H, KV = width
    G = H // KV
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(17 * r_qk + 3 * r_vo + 1000 * T + S + H)
    kappa = torch.randint(-2, 3, (B, KV, 1, r_qk), generator=gen).double()
    for b in range(B):
        for g in range(KV):
            kappa[b, g, 0, 0] = 1.0 + (b + g) % 2                          # never a zero row, and different per (b, g)
    assert len({tuple(kappa[b, g, 0].tolist()) for b in range(B) for g in range(KV)}) == B * KV
    q = torch.randint(-4, 5, (B, H, T, r_qk), generator=gen).double()
    q[..., 0] = torch.where(q.abs().sum(-1) == 0, 1.0, q[..., 0])
    assert float(kappa.abs().max()) <= 2 and float(q.abs().max()) <= 4 and bool((q.abs().sum(-1) > 0).all())
    k = kappa.expand(B, KV, S, r_qk).to(dtype).contiguous()
    q = q.to(dtype)
    scale = float(r_qk) ** -0.5
    # the fp32 logits of each query are bit-identical across keys (and exact: integers below 2^24)
    l32 = q.float() @ k.float().repeat_interleave(G, dim=1).transpose(2, 3)
    l64 = q.double() @ k.double().repeat_interleave(G, dim=1).transpose(2, 3)
    assert torch.equal(l32.double(), l64) and float(l64.abs().max()) < 2 ** 24
    c = torch.tensor(scale * 1.4426950408889634, dtype=torch.float64).float()
    t32 = l32 * c
    assert torch.equal(t32.view(torch.int32), t32[..., :1].expand_as(t32).contiguous().view(torch.int32))
    assert bool(torch.isfinite(t32).all())
    w = torch.tensor([[2.0 ** (b + 2 * g - 3) for g in range(KV)] for b in range(B)], dtype=torch.float64)
    assert w.unique().numel() == B * KV
    # the windows partition the keys
    windows = list(range(0, S, r_vo))
    probed = [j for j0 in windows for j in range(j0, min(j0 + r_vo, S))]
    assert probed == list(range(S))
    return Probe(q, k, scale, w, windows, r_vo)


def probe_values(p, dt, j0):
    """v [B, KV, S, r_vo] of window j0: w(b, g) at (j, c) = (j0 + c, c), 0 elsewhere."""
    Bk, KV, S, _ = p.k.shape
    v = torch.zeros(Bk, KV, S, p.r_vo, dtype=torch.float64)
    c = torch.arange(min(p.r_vo, S - j0))
    v[:, :, j0 + c, c] = p.w[:, :, None]
    out = v.to(DTYPES[dt])
    assert torch.equal(out.double(), v)
    return out


def probe_mask(kind, Bm, Hm, Tm, T, S, gen):
    """bool [Bm, Hm, Tm, S]: the mask's own extents before expand; a row axis of extent 1 stands for every query."""
    from tests.test_gpu_attn_mask import causal_pad       # (imported late: that module imports this one)
    i = torch.arange(Tm)[None, None, :, None]
    h = torch.arange(Hm)[None, :, None, None]
    j = torch.arange(S)[None, None, None, :]
    if kind == "bernoulli":
        return torch.rand(Bm, Hm, Tm, S, generator=gen) < 0.5
    if kind == "causal-pad":                              # HF's left-padded causal mask (one shared row: the padding alone)
        return causal_pad(Bm, T, S, [5, S // 3])[:, :, T - Tm:].expand(Bm, Hm, Tm, S).clone()
    if kind == "causal-pad-deep":                         # pads up to the first query's limit and beyond: rows with n = 1 and n = 0
        return causal_pad(Bm, T, S, [S - T, S - T + 3])[:, :, T - Tm:].expand(Bm, Hm, Tm, S).clone()
    if kind == "stripes":                                 # every lane register and every run of four mask bytes sees both values
        return ((j + i + h) % 5 != 0).expand(Bm, Hm, Tm, S).clone()
    assert kind == "tiles"                                # every 32 x 64 tile whole-none, whole-all or mixed
    nT, nS = -(-Tm // 32), -(-S // 64)
    state = torch.randint(0, 3, (Bm, Hm, nT, nS), generator=gen)
    state[0, 0].view(-1)[:3] = torch.tensor([2, 0, 1])[:state[0, 0].numel()]
    if nT > 1:                                            # a workgroup's four units all none: the uniform tile skip
        state[:, :, :, nS - 1] = 0
        state[:, :, 0, 0] = 1
    per = state.repeat_interleave(32, 2).repeat_interleave(64, 3)[:, :, :Tm, :S]
    return torch.where(per == 0, False, torch.where(per == 1, True, torch.rand(Bm, Hm, Tm, S, generator=gen) < 0.5))


def probe_admissions(T, S, H):
    """Every admission pattern of the probe at (T, S): (name, causal, layout, base mask or None, adm bool [B, H, T, S]).  Unmasked
    causal and full; then every kind of mask in every layout with `causal` on and off.  When the generator is exhausted it asserts
    that the set held a row with no admitted key, one with exactly one and one with all S."""
    seen = set()

    def emit(name, causal, layout, base):
        adm = admitted(T, S, causal)[None, None].expand(B, H, T, S)
        if base is not None:
            adm = adm & base.expand(B, base.shape[1], T, S)
        n = adm.sum(-1)
        assert int(n.max()) <= 2 ** 24
        seen.update(x for x in (0, 1, S) if bool((n == x).any()))
        return Admission(name, causal, layout, base, adm)

    yield emit("unmasked", True, None, None)
    yield emit("unmasked", False, None, None)
    for layout in PROBE_LAYOUTS:
        Bm = 1 if layout == "batch-stride-0" else B
        Tm = 1 if layout == "query-stride-0" else T
        Hm = H if layout == "per-head" else 1
        for kind in PROBE_KINDS:
            gen = torch.Generator().manual_seed(PROBE_KINDS.index(kind) + 10 * PROBE_LAYOUTS.index(layout) + 100 * T + S)
            base = probe_mask(kind, Bm, Hm, Tm, T, S, gen)
            for causal in (False, True):
                yield emit(kind, causal, layout, base)
    assert seen == {0, 1, S}, f"the admission set at T={T} S={S} has no row with n in {sorted({0, 1, S} - seen)}"


def probe_expected(p, dt, adm, width):
    """The two accepted bit patterns per entry, int16 [B, T, H, windows * r_vo] (keys beyond S: +0), and the number of entries where
    they differ."""
    Bq, H, T, S = adm.shape
    r_vo = width[1]
    G = H // p.w.shape[1]
    n = adm.sum(-1)                                                          # [B, H, T]
    assert int(n.max()) <= 2 ** 24
    x = p.w.repeat_interleave(G, dim=1)[:, :, None] / n.clamp(min=1).double()
    P = len(p.windows) * r_vo
    both = []
    for f in (1.0 - 2.0 ** -22, 1.0 + 2.0 ** -22):
        e = (x * f).float().to(DTYPES[dt])                                   # fp64 -> fp32 -> element type
        full = torch.zeros(Bq, H, T, P, dtype=DTYPES[dt])
        full[..., :S] = torch.where(adm, e[..., None].expand(Bq, H, T, S), torch.zeros((), dtype=DTYPES[dt]))
        both.append(bits(full.transpose(1, 2)))
    lo, hi = both
    step = hi.int() - lo.int()
    assert int(step.min()) >= 0 and int(step.max()) <= 1                     # equal or neighbours: the set is the whole interval
    return lo, hi, int(step.sum())
