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
]
B = 2

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
