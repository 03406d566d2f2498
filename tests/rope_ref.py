"""Reference, inputs and case table of the rotary-kernel tests (test_rope_ref_host.py on the CPU, test_gpu_rope.py on the GPU).

Rotation without the norm has one right answer: O.apply_rotary_compressed, bit for bit.

Rotation after the masked RMSNorm has an INTERVAL per output element (norm_rope_interval), because the fp32 sum of squares
of a row has no defined order: torch's, the direct kernel's 16-lane tree and the tile kernel's 4-lane sums may all round
differently.

  inv = 1 / sqrt(ss / r + fp32(eps)) is computed in fp64 from the fp64 sum of squares of the row (exact to ~1e-16) and
  widened to [inv (1 - delta), inv (1 + delta)], rounded outward to fp32, with delta = (r + 8) * 2^-24.
  Why that delta covers every fp32 evaluation (u = 2^-24, the fp32 unit roundoff; all terms are non-negative, so relative
  errors do not amplify):
    * r products and at most r - 1 additions, in any order and any tree shape: every term passes through at most
      1 + (r - 1) roundings, so the sum is off by at most about r u relatively;
    * the division by r and the addition of eps: one rounding each -> (r + 2) u on the radicand;
    * the square root halves the accumulated error and adds a rounding, the reciprocal adds one more:
      (r + 2) / 2 + 2 = r / 2 + 3 roundings' worth on inv;
    * delta is twice that plus 2 u of slack (second-order terms, the outward rounding of the ends).
  Every later op is a correctly rounded, hence monotone (non-decreasing or non-increasing), function of each of its inputs
  with the others fixed: fl(x * inv), dtype(w * ...), the four dtype-rounded products and the dtype-rounded sum of
  x cos + rotate_half(x) sin.  So a normed element lies between its evaluations at the two ends of inv, and an output
  element, which depends on the normed element and on its rotate_half partner, lies between the min and the max over the
  four corner combinations of the two.  The corners are evaluated with the oracle's own dtype-rounded torch expression.
  Where rounding absorbs delta (nearly everywhere for bf16 / f16) the interval is a single number.
"""
import functools

import torch

from oracle import modegpt_oracle as O

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
EPS = 1e-6
U32 = 2.0 ** -24
NONDEGENERATE_CAP = {"bf16": 0.02, "f16": 0.10, "f32": 1.0}     # share of elements whose interval is not a single number


def _outward_f32(v64, up):
    """fp64 -> fp32 rounded towards +inf (up) or -inf; v64 > 0."""
    f = v64.to(torch.float32)
    wrong = (f.double() < v64) if up else (f.double() > v64)
    step = torch.nextafter(f, torch.full_like(f, float("inf") if up else float("-inf")))
    return torch.where(wrong, step, f)


def inv_rms_interval(x_bthr, eps=EPS):
    """x [B, T, H, r] -> (inv_lo, inv_hi) fp32 [B, T, H, 1] enclosing every fp32 evaluation of rsqrt(mean(x^2) + eps)."""
    r = x_bthr.shape[-1]
    ss = x_bthr.double().pow(2).sum(-1, keepdim=True)
    inv = 1.0 / torch.sqrt(ss / r + float(torch.tensor(eps, dtype=torch.float32)))
    delta = (r + 8) * U32
    return _outward_f32(inv * (1 - delta), False), _outward_f32(inv * (1 + delta), True)


def normed_with(x_bthr, inv, weight, mask, groups):
    """O.masked_rms_norm's expression with the reciprocal RMS given: dtype(weight[mask] * (float(x) * inv))."""
    m = torch.repeat_interleave(mask, groups, dim=0) if groups > 1 else mask
    return (weight[m][None, None] * (x_bthr.to(torch.float32) * inv)).to(x_bthr.dtype)


def rotate(x_bhtr, cos, sin, mask, n_kv):
    """O.apply_rotary_compressed of one tensor with n_heads heads over n_kv mask rows."""
    return O.apply_rotary_compressed(x_bhtr, x_bhtr[:, :n_kv], cos, sin, mask)[0]


def norm_rope_interval(x_bthr, weight, eps, mask, n_kv, cos, sin, rope_mask="same"):
    """[lo, hi] per element of rope(masked_rms_norm(x)), both of x's dtype, shape [B, H, T, r].  mask: int64 [n_kv, r]
    (the identity for the mask-free route, then rope_mask=None makes the rotation take per-batch tables as the kernel does)."""
    H, r = x_bthr.shape[2], x_bthr.shape[3]
    half = r // 2
    rmask = mask if rope_mask == "same" else rope_mask
    ends = [normed_with(x_bthr, inv, weight, mask, H // n_kv) for inv in inv_rms_interval(x_bthr, eps)]
    lo = hi = None
    for a in ends:           # the end the first half's elements take
        for b in ends:       # the end their rotate_half partners take
            y = rotate(torch.cat((a[..., :half], b[..., half:]), -1).transpose(1, 2), cos, sin, rmask, n_kv).float()
            lo = y if lo is None else torch.minimum(lo, y)
            hi = y if hi is None else torch.maximum(hi, y)
    return lo.to(x_bthr.dtype), hi.to(x_bthr.dtype)


def oracle_chain(x_bthr, weight, eps, mask, n_kv, cos, sin, rope_mask="same"):
    rmask = mask if rope_mask == "same" else rope_mask
    n = O.masked_rms_norm(x_bthr, weight, eps, mask, x_bthr.shape[2] // n_kv)
    return rotate(n.transpose(1, 2), cos, sin, rmask, n_kv)


def inside(got, lo, hi):
    g = got.double()
    return (g >= lo.double()) & (g <= hi.double())


def nondegenerate_share(lo, hi):
    return (lo.double() != hi.double()).double().mean().item()


# ---------------------------------------------------------------- cases
# name -> (B, T, n_heads, n_kv, head_dim, r, layout).  layout:
#   ""       everything freshly allocated (512-byte aligned), x contiguous, mask a random RoPE-pair selection
#   "perm"   r == head_dim, mask a permutation of the pairs
#   "nomask" r == head_dim, no mask, cos / sin per batch
#   "slice"  x is the column slice [1 : 1 + n_heads * r] of a buffer whose rows are n_heads * r + 3 elements long (odd)
#   "off1"   norm weight = buf[1 : hd + 1], cos / sin views at element offset 1 of a flat buffer, out at element offset 1
#   "off1in" the same without the offset of out (the direct kernel keeps its packs)     "off1nw" only the norm weight is offset
SHAPES = {
    "qwen_full_perm":   (2, 37, 8, 2, 128, 128, "perm"),
    "group5":           (1, 70, 5, 1, 128, 88, ""),
    "vec2_hpt2":        (2, 20, 4, 2, 64, 44, ""),
    "vec2_prepass":     (1, 19, 4, 2, 128, 76, ""),
    "vec4_prepass_mha": (1, 20, 3, 3, 256, 200, ""),
    "vec2_hpt1":        (1, 18, 3, 3, 32, 12, ""),
    "vec2_hpt4":        (1, 9, 4, 1, 64, 20, ""),
    "vec4_hpt2_hd128":  (1, 21, 4, 2, 128, 88, ""),
    "tile_odd_ch4":     (2, 70, 8, 2, 128, 90, ""),
    "tile_odd_ch2":     (1, 33, 6, 3, 64, 42, ""),
    "tile_odd_ch1_wide": (1, 20, 3, 3, 256, 202, ""),
    "tile_even_ch2":    (2, 40, 4, 2, 128, 88, "slice"),
    "tile_even_ch4":    (2, 40, 4, 1, 128, 88, "slice"),
    "tile_even_ch1":    (2, 40, 4, 4, 128, 88, "slice"),
    "one_pair":         (1, 5, 2, 2, 16, 2, ""),
    "nomask_wide":      (2, 7, 2, 1, 256, 256, "nomask"),
    "direct_off1":      (1, 70, 5, 1, 128, 88, "off1"),
    "tile_off1":        (2, 70, 8, 2, 128, 90, "off1"),
    "direct_off1in":    (1, 21, 4, 2, 128, 88, "off1in"),
    "direct_off1nw":    (2, 37, 8, 2, 128, 128, "off1nw"),
}

# What each case reaches WITH the norm weight, per dtype, in variant_of()'s words; without the norm the same with nw0.
# Direct kernel: rope_gather_kernel<DT, VEC, NORM, HPT>; "it" passes over the row (it2 + norm = the sum-of-squares pre-pass);
# "os" one_shot; "cs" / "nw" 16-byte staging of the tables / the norm weight; "big" LDS above 64 KB (attribute call).
# Tile kernel: rope_tile_kernel<DT, NORM, HALF_EVEN> with CH heads and tt tokens per workgroup, copies wi / wo bytes wide.
# "tiles" is the number of token tiles per batch (the last one partial unless T divides).
VARIANTS = {
    # HPT 4, VEC 4, one pass; the half types stage cos / sin (and the weight) through registers; 3 token tiles per batch
    "qwen_full_perm":   {"bf16": "direct hpt4 vec4 it1 os1 cs1 nw1 big0 tiles3", "f16": "direct hpt4 vec4 it1 os1 cs1 nw1 big0 tiles3",
                         "f32": "direct hpt4 vec4 it1 os0 cs1 nw1 big0 tiles3"},
    # Qwen3-14B's group of 5: HPT 1, four tokens per thread group, 70 = 64 + 6 leaves dead tokens; fp32 tables are 66048 B
    "group5":           {"bf16": "direct hpt1 vec4 it1 os1 cs1 nw1 big0 tiles2", "f16": "direct hpt1 vec4 it1 os1 cs1 nw1 big0 tiles2",
                         "f32": "direct hpt1 vec4 it1 os0 cs1 nw1 big1 tiles2"},
    "vec2_hpt2":        {"bf16": "direct hpt2 vec2 it1 os0 cs1 nw1 big0 tiles1", "f16": "direct hpt2 vec2 it1 os0 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt2 vec2 it1 os1 cs1 nw1 big0 tiles1"},
    "vec2_prepass":     {"bf16": "direct hpt2 vec2 it2 os1 cs1 nw1 big0 tiles1", "f16": "direct hpt2 vec2 it2 os1 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt2 vec2 it2 os0 cs1 nw1 big0 tiles1"},
    "vec4_prepass_mha": {"bf16": "direct hpt1 vec4 it2 os0 cs1 nw1 big1 tiles1", "f16": "direct hpt1 vec4 it2 os0 cs1 nw1 big1 tiles1",
                         "f32": "direct hpt1 vec4 it2 os0 cs1 nw1 big1 tiles1"},
    "vec2_hpt1":        {"bf16": "direct hpt1 vec2 it1 os0 cs1 nw1 big0 tiles1", "f16": "direct hpt1 vec2 it1 os0 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt1 vec2 it1 os0 cs1 nw1 big0 tiles1"},
    "vec2_hpt4":        {"bf16": "direct hpt4 vec2 it1 os0 cs1 nw1 big0 tiles1", "f16": "direct hpt4 vec2 it1 os0 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt4 vec2 it1 os1 cs1 nw1 big0 tiles1"},
    "vec4_hpt2_hd128":  {"bf16": "direct hpt2 vec4 it1 os1 cs1 nw1 big0 tiles1", "f16": "direct hpt2 vec4 it1 os1 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt2 vec4 it1 os0 cs1 nw1 big0 tiles1"},
    # 70 = 4 * 16 + 6: five token tiles per batch, the last one 6 tokens, B 2
    "tile_odd_ch4":     {"bf16": "tile ch4 even0 tt16 wi16 wo8 hp1_0 cs1 nw1 big0 tiles5", "f16": "tile ch4 even0 tt16 wi16 wo8 hp1_0 cs1 nw1 big0 tiles5",
                         "f32": "tile ch4 even0 tt16 wi16 wo16 hp1_0 cs1 nw1 big0 tiles5"},
    "tile_odd_ch2":     {"bf16": "tile ch2 even0 tt32 wi8 wo4 hp1_0 cs1 nw1 big0 tiles2", "f16": "tile ch2 even0 tt32 wi8 wo4 hp1_0 cs1 nw1 big0 tiles2",
                         "f32": "tile ch2 even0 tt32 wi16 wo8 hp1_0 cs1 nw1 big0 tiles2"},
    # the tile no longer fits 64 KB at 64 tokens: tt shrinks below 64 / hpt
    "tile_odd_ch1_wide": {"bf16": "tile ch1 even0 tt32 wi4 wo16 hp1_0 cs1 nw1 big0 tiles1", "f16": "tile ch1 even0 tt32 wi4 wo16 hp1_0 cs1 nw1 big0 tiles1",
                          "f32": "tile ch1 even0 tt16 wi8 wo16 hp1_0 cs1 nw1 big0 tiles2"},
    # misaligned x: the packs of the direct kernel cannot address it, the tile kernel runs with an even half; wi = one element
    # (fp32: 64 / hpt tokens of tables and slabs exceed 64 KB, tt halves)
    "tile_even_ch2":    {"bf16": "tile ch2 even1 tt32 wi2 wo16 hp1_0 cs1 nw1 big0 tiles2", "f16": "tile ch2 even1 tt32 wi2 wo16 hp1_0 cs1 nw1 big0 tiles2",
                         "f32": "tile ch2 even1 tt16 wi4 wo16 hp1_0 cs1 nw1 big0 tiles3"},
    "tile_even_ch4":    {"bf16": "tile ch4 even1 tt16 wi2 wo16 hp1_0 cs1 nw1 big0 tiles3", "f16": "tile ch4 even1 tt16 wi2 wo16 hp1_0 cs1 nw1 big0 tiles3",
                         "f32": "tile ch4 even1 tt16 wi4 wo16 hp1_0 cs1 nw1 big0 tiles3"},
    "tile_even_ch1":    {"bf16": "tile ch1 even1 tt64 wi2 wo16 hp1_0 cs1 nw1 big0 tiles1", "f16": "tile ch1 even1 tt64 wi2 wo16 hp1_0 cs1 nw1 big0 tiles1",
                         "f32": "tile ch1 even1 tt32 wi4 wo16 hp1_0 cs1 nw1 big0 tiles2"},
    "one_pair":         {"bf16": "tile ch1 even0 tt64 wi4 wo4 hp1_1 cs1 nw1 big0 tiles1", "f16": "tile ch1 even0 tt64 wi4 wo4 hp1_1 cs1 nw1 big0 tiles1",
                         "f32": "tile ch1 even0 tt64 wi8 wo8 hp1_1 cs1 nw1 big0 tiles1"},
    "nomask_wide":      {"bf16": "direct hpt2 vec4 it2 os0 cs1 nw1 big0 tiles1", "f16": "direct hpt2 vec4 it2 os0 cs1 nw1 big0 tiles1",
                         "f32": "direct hpt2 vec4 it2 os0 cs1 nw1 big1 tiles1"},
    # out at element offset 1: no pack of the direct kernel can address it, so both of these land on the tile kernel with an
    # even half (r = 88) or an odd one (r = 90), wo = one element, and neither the tables nor the weight are 16-byte aligned
    "direct_off1":      {"bf16": "tile ch1 even1 tt64 wi16 wo2 hp1_0 cs0 nw0 big0 tiles2", "f16": "tile ch1 even1 tt64 wi16 wo2 hp1_0 cs0 nw0 big0 tiles2",
                         "f32": "tile ch1 even1 tt32 wi16 wo4 hp1_0 cs0 nw0 big0 tiles3"},
    "tile_off1":        {"bf16": "tile ch4 even0 tt16 wi16 wo2 hp1_0 cs0 nw0 big0 tiles5", "f16": "tile ch4 even0 tt16 wi16 wo2 hp1_0 cs0 nw0 big0 tiles5",
                         "f32": "tile ch4 even0 tt16 wi16 wo4 hp1_0 cs0 nw0 big0 tiles5"},
}


VARIANTS.update({
    # the direct kernel with tables that are not 16-byte aligned (no one_shot even at head_dim 128), and with one_shot
    # tables beside a norm weight that has to take the scalar staging loop
    "direct_off1in": {"bf16": "direct hpt2 vec4 it1 os0 cs0 nw0 big0 tiles1", "f16": "direct hpt2 vec4 it1 os0 cs0 nw0 big0 tiles1",
                      "f32": "direct hpt2 vec4 it1 os0 cs0 nw0 big0 tiles1"},
    "direct_off1nw": {"bf16": "direct hpt4 vec4 it1 os1 cs1 nw0 big0 tiles3", "f16": "direct hpt4 vec4 it1 os1 cs1 nw0 big0 tiles3",
                      "f32": "direct hpt4 vec4 it1 os0 cs1 nw0 big0 tiles3"},
})


def variant_of(plan):
    """A plan dict of ops.rope_plan_at in the words of VARIANTS."""
    tail = f"cs{plan['cs_vec16']} nw{plan['nw_vec16']} big{plan['lds_attr']} tiles{plan['t_tiles']}"
    if plan["route"] == "direct":
        return f"direct hpt{plan['hpt']} vec{plan['vec']} it{plan['iters']} os{plan['one_shot']} {tail}"
    return (f"tile ch{plan['hpt']} even{plan['half_even']} tt{plan['tt']} wi{plan['wi']} wo{plan['wo']} "
            f"hp1_{plan['hp1']} {tail}")


def declared(name, dt, norm):
    v = VARIANTS[name][dt]
    return v if norm else v.replace("nw1", "nw0")


def offsets(name):
    """Element offsets (x, cos / sin, norm weight, out) from an aligned base and x's row pitch in elements."""
    B, T, n_h, n_kv, hd, r, layout = SHAPES[name]
    if layout == "slice":
        return dict(x=1, cs=0, nw=0, out=0, ld_x=n_h * r + 3)
    if layout.startswith("off1"):
        return dict(x=0, cs=int(layout != "off1nw"), nw=1, out=int(layout == "off1"), ld_x=n_h * r)
    return dict(x=0, cs=0, nw=0, out=0, ld_x=n_h * r)


def synthetic_plan(ops, name, dt, norm):
    """The plan of the case at synthetic 512-byte aligned bases plus the case's offsets: no tensor, no device."""
    B, T, n_h, n_kv, hd, r, layout = SHAPES[name]
    o, es = offsets(name), torch.empty(0, dtype=DTYPES[dt]).element_size()
    base = 1 << 32
    return ops.rope_plan_at(DTYPES[dt], B, T, n_h, n_kv, r, hd, o["ld_x"], base + o["x"] * es, 2 * base + o["cs"] * es,
                            3 * base + o["cs"] * es, T * hd if layout == "nomask" else 0, None if layout == "nomask" else 4 * base,
                            5 * base + o["nw"] * es if norm else None, 6 * base + o["out"] * es)


# ---------------------------------------------------------------- inputs
class Inputs:
    """x [B, T, H, r] with a log-normal scale per row, special rows, cos / sin, mask, norm weight -- all on the CPU."""


SPECIAL = {"zero": (0, 0, 0), "rms1e-3": (0, 1, 1), "big": (0, 2, 0)}   # name -> (batch, token, head); every case has T >= 5


@functools.lru_cache(maxsize=None)
def make_inputs(name, dt):
    B, T, n_h, n_kv, hd, r, layout = SHAPES[name]
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name) * 7 + 1)
    # rows at every scale from ~1e-5 to ~10: RMS near 1e-3 (where eps = 1e-6 decides the result) is in the bulk
    scale = 10.0 ** (-2.5 + 1.0 * torch.randn(B, T, n_h, 1, generator=gen)).clamp(-5.0, 1.0)
    x = torch.randn(B, T, n_h, r, generator=gen) * scale
    x[SPECIAL["zero"]] = 0.0
    row = x[SPECIAL["rms1e-3"]]
    x[SPECIAL["rms1e-3"]] = row * (1e-3 / row.pow(2).mean().sqrt())
    x[SPECIAL["big"]][0] = 60000.0            # representable in f16 (max 65504); its square needs the fp32 accumulator
    x = x.to(dtype)
    ang = torch.rand(B, T, hd // 2, generator=gen) * 6.28
    if layout != "nomask":
        ang = ang[:1]
    emb = torch.cat((ang, ang), -1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    if layout == "nomask":        # "perm" needs nothing special: r / 2 of head_dim / 2 pairs drawn without replacement
        idx = torch.arange(hd // 2).repeat(n_kv, 1)
    else:
        idx = torch.stack([torch.randperm(hd // 2, generator=gen)[:r // 2] for _ in range(n_kv)])
    mask = torch.cat((idx, idx + hd // 2), dim=1)
    w = torch.randn(hd, generator=gen)        # both signs
    w[torch.randperm(hd, generator=gen)[:max(1, hd // 8)]] = 0.0
    w[mask[0, 0]] = 1.5                       # (a kept column of the first kv head keeps a weight)
    inp = Inputs()
    inp.x, inp.cos, inp.sin, inp.mask, inp.w = x, cos, sin, mask, w.to(dtype)
    inp.rope_mask = None if layout == "nomask" else mask
    inp.n_kv, inp.hd, inp.dims = n_kv, hd, (B, T, n_h, r)
    return inp


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """(rotation without norm, (lo, hi) with norm), each [B, H, T, r]; computed once per case and dtype, never modified."""
    i = make_inputs(name, dt)
    plain = rotate(i.x.transpose(1, 2), i.cos, i.sin, i.rope_mask, i.n_kv)
    return plain, norm_rope_interval(i.x, i.w, EPS, i.mask, i.n_kv, i.cos, i.sin, rope_mask=i.rope_mask)
