// What the two attention kernels (attn.hip: prefill schedule; attn_decode.hip: split-key decode schedule) share: the MFMA wrapper
// per element type, the 8-element row load with its alignment paths, the key tile and the pitch of the transposed V tile, and the
// mask's arguments and the lane -> key map of a mask load with its 4-byte / byte paths for the masked variants; and the host side of
// the four entries: what a call carries, the argument and overlap checks in their order, the fill of the kernel arguments, the
// (r_qk, r_vo) -> template ladder and the launch.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.hpp"

namespace mdg {
namespace attn {

constexpr int KT = 64;      // keys per LDS stage
constexpr int VP = KT + 8;  // Vs pitch in elements (144 B: 16-byte aligned rows)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int DT> struct Mma;
template <> struct Mma<MDG_BF16> {
  typedef __bf16 E;
  typedef __bf16 frag __attribute__((ext_vector_type(8)));
  __device__ static __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mma<MDG_F16> {
  typedef _Float16 E;
  typedef _Float16 frag __attribute__((ext_vector_type(8)));
  __device__ static __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

// 8 consecutive elements of a row starting at column c0 (a multiple of 8); columns >= width read as zero.  `vec`: the row start
// is 16-byte aligned.  The narrower path reads a whole chunk as 16 bytes at the elements' own 2-byte alignment (global memory takes
// unaligned dword loads; where the target does not, the compiler splits the load) and a row's tail chunk element by element.
typedef unsigned u32x4u __attribute__((ext_vector_type(4), aligned(2)));
template <typename E> __device__ __forceinline__ u32x4 load8(const E* row, int c0, int width, bool vec) {
  u32x4 z = {0u, 0u, 0u, 0u};
  if (c0 >= width) return z;
  if (c0 + 8 <= width) {
    if (vec) return *(const u32x4*)(row + c0);
    const u32x4u w = *(const u32x4u*)(row + c0);
    return (u32x4){w[0], w[1], w[2], w[3]};
  }
  const unsigned short* p = (const unsigned short*)row;
  unsigned e[8];
#pragma unroll
  for (int j = 0; j < 8; j++) e[j] = c0 + j < width ? (unsigned)p[c0 + j] : 0u;
  z.x = e[0] | (e[1] << 16);
  z.y = e[2] | (e[3] << 16);
  z.z = e[4] | (e[5] << 16);
  z.w = e[6] | (e[7] << 16);
  return z;
}

__device__ __forceinline__ unsigned half_of(unsigned w, int odd) { return odd ? (w >> 16) : (w & 0xffffu); }

// ---------------------------------------------------------------- bool masks (mdg_attn_fwd_masked, mdg_attn_decode_masked)
// mask [B, Hm, T, S]: one byte per element, non-zero admits; batch / head / query strides in bytes (0 for an expanded axis), key
// stride 1.  The prefill kernel also reads a tile summary: one byte per (32 queries x 64 keys), written by attn_mask.hip.
constexpr int MASK_QT = 32;  // the summary tile: attn.hip's QT x KT
enum { MASK_NONE = 0, MASK_ALL = 1, MASK_MIXED = 2 };

struct MaskArgs {
  const unsigned char* mask;
  const unsigned char* summary;  // [B][Hm][qtiles][ktiles] (prefill only)
  int64_t mbs, mhs, mqs;         // bytes
  int64_t qtiles, ktiles;
  int per_head;                  // Hm == n_heads (else the one mask head serves every head)
  int vec;                       // every row start is 4-byte aligned
};

// The first product leaves 16 keys of each 32-key half on a lane (lane half hh): register i is key 8 (i >> 2) + 4 hh + (i & 3) of
// the half, four runs of 4 consecutive keys.  Bit i of the result: mask row `row` admits key k0 + 8 (i >> 2) + (i & 3), where
// k0 = the half's first key + 4 hh (a multiple of 4).  Keys >= S are not read and not admitted.  `vec`: row is 4-byte aligned, so
// a run inside the row is one 4-byte load; otherwise, and for the run that crosses S, byte loads.
__device__ __forceinline__ unsigned mask_bits16(const unsigned char* row, int64_t k0, int64_t S, bool vec) {
  // one 64-bit address and small constant offsets from it: nothing per element for the compiler to hoist out of the key loop
  const unsigned char* p = row + k0;
  const int64_t left = S - k0;
  const int rem = left < 32 ? (int)left : 32;  // keys of the row from k0 on (the runs end at offset 28); <= 0: none
  unsigned bits = 0u;
#pragma unroll
  for (int q4 = 0; q4 < 4; q4++) {
    if (vec && 8 * q4 + 4 <= rem) {
      const unsigned w = *(const unsigned*)(p + 8 * q4);
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (w & (0xffu << (8 * i))) bits |= 1u << (4 * q4 + i);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (8 * q4 + i < rem && p[8 * q4 + i]) bits |= 1u << (4 * q4 + i);
    }
  }
  return bits;
}

// the byte range [lo, hi) of a mask; an axis of stride 0 contributes extent 1
static inline void mask_span_of(const void* p, int64_t B, int64_t bs, int64_t H, int64_t hs, int64_t T, int64_t qs, int64_t S,
                                uintptr_t& lo, uintptr_t& hi) {
  lo = (uintptr_t)p;
  hi = lo + (uintptr_t)((B - 1) * bs + (H - 1) * hs + (T - 1) * qs + S);
}

// ---------------------------------------------------------------- the host side of the four entries (attn.hip, attn_decode.hip)
// What every entry receives, in the order of the C signatures, and what the masked entries receive besides.  The order of the checks
// below is part of the interface: of two faults the caller is told the one checked first.
struct Call {
  const void *q, *k, *v;
  int dtype;
  int64_t B, T, S;
  int n_heads, n_kv, r_qk, r_vo;
  int64_t kbs, khs, kts, vbs, vhs, vts;  // elements
  double scale;
  int causal;
  void* out;
  int64_t ld_out;
  void* stream;
};
struct MaskCall {
  const void* mask;
  int Hm;
  int64_t mbs, mhs, mqs;  // bytes
};

// The checks every entry makes, under the caller's name, in three parts: decode's tile and split checks sit between the first two,
// each entry's own overflow bound and the return of an empty call between the last two.
static inline int check_widths(const char* fn, const Call& p) {
  MDG_CHECK_ARG(p.dtype == MDG_BF16 || p.dtype == MDG_F16, "%s: dtype %d (bf16 or f16; fp32 inputs are out of scope)", fn, p.dtype);
  MDG_CHECK_ARG(p.B >= 0 && p.T >= 0 && p.S >= 0, "%s: negative extent", fn);
  MDG_CHECK_ARG(p.n_heads > 0 && p.n_kv > 0 && p.n_heads % p.n_kv == 0, "%s: n_heads=%d is not a positive multiple of n_kv=%d", fn,
                p.n_heads, p.n_kv);
  MDG_CHECK_ARG(p.r_qk >= 2 && p.r_qk <= 256 && p.r_qk % 2 == 0, "%s: r_qk=%d must be even, >= 2 and <= 256", fn, p.r_qk);
  MDG_CHECK_ARG(p.r_vo >= 1 && p.r_vo <= 256, "%s: r_vo=%d must be in 1..256", fn, p.r_vo);
  return MDG_OK;
}
static inline int check_layout(const char* fn, const Call& p) {
  MDG_CHECK_ARG(!(p.causal && p.S < p.T), "%s: causal with S=%lld < T=%lld keys", fn, (long long)p.S, (long long)p.T);
  MDG_CHECK_ARG(p.kts >= p.r_qk, "%s: k token stride %lld < r_qk=%d", fn, (long long)p.kts, p.r_qk);
  MDG_CHECK_ARG(p.vts >= p.r_vo, "%s: v token stride %lld < r_vo=%d", fn, (long long)p.vts, p.r_vo);
  const int64_t width = (int64_t)p.n_heads * p.r_vo;
  MDG_CHECK_ARG(p.ld_out >= width, "%s: ld_out=%lld < n_heads*r_vo=%lld", fn, (long long)p.ld_out, (long long)width);
  MDG_CHECK_ARG(isfinite(p.scale) && p.scale > 0.0, "%s: scale %g must be finite and positive", fn, p.scale);
  return MDG_OK;
}
static inline int check_pointers(const char* fn, const Call& p) {
  MDG_CHECK_ARG(p.q && p.out && (p.S == 0 || (p.k && p.v)), "%s: null pointer", fn);
  return MDG_OK;
}

// The overlap checks as data: an operand's name in the messages and its bytes [lo, hi); lo == hi: nothing to overlap.
struct Span {
  const char* name;
  uintptr_t lo, hi;
};

// `s` lies apart from each of the nt targets (out; in decode out, then the workspace), asked in their order
static inline int apart(const char* fn, const Span* target, int nt, const Span& s) {
  for (int i = 0; i < nt; i++)
    MDG_CHECK_ARG(s.lo == s.hi || s.hi <= target[i].lo || target[i].hi <= s.lo, "%s: %s overlaps %s", fn, target[i].name, s.name);
  return MDG_OK;
}

// the bytes a strided [B, H, N, width] operand spans (none without rows)
static inline Span span_of(const char* name, const void* p, int64_t B, int64_t bs, int64_t H, int64_t hs, int64_t N, int64_t ts,
                           int64_t width, size_t es) {
  if (N == 0) return Span{name, 0, 0};
  int64_t mn = 0, mxe = 0;
  const int64_t ext[3] = {(B - 1) * bs, (H - 1) * hs, (N - 1) * ts};
  for (int i = 0; i < 3; i++) {
    if (ext[i] < 0) mn += ext[i];
    else mxe += ext[i];
  }
  return Span{name, (uintptr_t)p + (uintptr_t)(mn * (int64_t)es), (uintptr_t)p + (uintptr_t)((mxe + width) * (int64_t)es)};
}

// out, then q, k, v in the order the entries check them against it (B, T > 0 here; k and v are empty without keys)
static inline void operand_spans(const Call& p, Span (&sp)[4]) {
  const size_t es = dtype_size(p.dtype);
  sp[0] = span_of("out", p.out, 1, 0, 1, 0, p.B * p.T, p.ld_out, (int64_t)p.n_heads * p.r_vo, es);
  sp[1] = span_of("q", p.q, 1, 0, 1, 0, p.B * p.n_heads * p.T, p.r_qk, p.r_qk, es);
  sp[2] = span_of("k", p.k, p.B, p.kbs, p.n_kv, p.khs, p.S, p.kts, p.r_qk, es);
  sp[3] = span_of("v", p.v, p.B, p.vbs, p.n_kv, p.vhs, p.S, p.vts, p.r_vo, es);
}

// The mask checks the masked entries share (B, T > 0 here), under the caller's name; fills mk's mask fields and the mask's span
// (empty without keys), which the caller then holds against its targets.
static inline int mask_args(const char* fn, const Call& p, const MaskCall& m, MaskArgs& mk, Span& s) {
  MDG_CHECK_ARG(m.Hm == 1 || m.Hm == p.n_heads, "%s: mask heads Hm=%d must be 1 or n_heads=%d", fn, m.Hm, p.n_heads);
  MDG_CHECK_ARG(m.mbs >= 0 && m.mhs >= 0 && m.mqs >= 0, "%s: negative mask stride (%lld, %lld, %lld)", fn, (long long)m.mbs,
                (long long)m.mhs, (long long)m.mqs);
  MDG_CHECK_ARG(m.mask != nullptr || p.S == 0, "%s: null mask", fn);
  s = Span{"mask", 0, 0};
  if (p.S > 0) mask_span_of(m.mask, p.B, m.mbs, m.Hm, m.mhs, p.T, m.mqs, p.S, s.lo, s.hi);
  mk.mask = (const unsigned char*)m.mask;
  mk.summary = nullptr;
  mk.mbs = m.mbs; mk.mhs = m.mhs; mk.mqs = m.mqs;
  mk.qtiles = (p.T + MASK_QT - 1) / MASK_QT;
  mk.ktiles = (p.S + KT - 1) / KT;
  mk.per_head = m.Hm != 1;
  mk.vec = (uintptr_t)m.mask % 4 == 0 && m.mbs % 4 == 0 && m.mhs % 4 == 0 && m.mqs % 4 == 0;
  return MDG_OK;
}

// The fields AttnArgs and DecodeArgs share, from the call: operands, extents and strides as they came, the load path of q, k and v
// (aligned 16-byte loads when base and every stride are multiples of 16 bytes) and c = scale * log2(e).
template <typename A> static inline void fill_args(A& a, const Call& p) {
  a.q = p.q; a.k = p.k; a.v = p.v; a.out = p.out;
  a.T = p.T; a.S = p.S; a.ld_out = p.ld_out;
  a.kbs = p.kbs; a.khs = p.khs; a.kts = p.kts;
  a.vbs = p.vbs; a.vhs = p.vhs; a.vts = p.vts;
  a.n_heads = p.n_heads; a.n_kv = p.n_kv; a.G = p.n_heads / p.n_kv; a.r_qk = p.r_qk; a.r_vo = p.r_vo; a.causal = p.causal != 0;
  a.vec_q = (uintptr_t)p.q % 16 == 0 && p.r_qk % 8 == 0;
  a.vec_k = (uintptr_t)p.k % 16 == 0 && p.kbs % 8 == 0 && p.khs % 8 == 0 && p.kts % 8 == 0;
  a.vec_v = (uintptr_t)p.v % 16 == 0 && p.vbs % 8 == 0 && p.vhs % 8 == 0 && p.vts % 8 == 0;
  a.c = (float)(p.scale * 1.4426950408889634);
}

// The template of a width pair, one statement for both kernels: NQ = 4 / 8 / 16 k-steps for r_qk <= 64 / 128 / 256 and NV = 2 / 4 / 8
// column tiles for r_vo <= 64 / 128 / 256.  Returns f(NQ, NV) with both as integral constants.
template <int N> using Int = std::integral_constant<int, N>;
template <typename F> static inline int with_template(int r_qk, int r_vo, F f) {
  auto nv = [&](auto nq) {
    if (r_vo <= 64) return f(nq, Int<2>{});
    if (r_vo <= 128) return f(nq, Int<4>{});
    return f(nq, Int<8>{});
  };
  if (r_qk <= 64) return nv(Int<4>{});
  if (r_qk <= 128) return nv(Int<8>{});
  return nv(Int<16>{});
}

// One launch of either attention kernel, MASKED or not; dynamic LDS beyond 64 KiB has to be allowed per kernel first.
template <typename A> static inline int launch(void (*kernel)(A, MaskArgs), dim3 grid, int threads, size_t lds, hipStream_t st,
                                               const A& a, const MaskArgs& mk) {
  if (lds > 64 * 1024) MDG_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, a, mk);
  return MDG_OK;
}

}  // namespace attn
}  // namespace mdg
