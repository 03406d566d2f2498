// What the two attention kernels (attn.hip: prefill schedule; attn_decode.hip: split-key decode schedule) share: the MFMA wrapper
// per element type, the 8-element row load with its alignment paths, the key tile and the pitch of the transposed V tile, and the
// byte span of a strided operand for the overlap checks, and for the masked variants the mask's arguments, the lane -> key map of a
// mask load with its 4-byte / byte paths, and the mask checks of the two masked entries.
#pragma once
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

// The mask checks the masked entries share (B, T > 0 here), under the caller's name; fills mk's mask fields.  [ol, oh) is out's span.
static inline int mask_args(const char* fn, const void* mask, int64_t B, int Hm, int n_heads, int64_t T, int64_t S, int64_t mbs,
                            int64_t mhs, int64_t mqs, uintptr_t ol, uintptr_t oh, MaskArgs& mk) {
  MDG_CHECK_ARG(Hm == 1 || Hm == n_heads, "%s: mask heads Hm=%d must be 1 or n_heads=%d", fn, Hm, n_heads);
  MDG_CHECK_ARG(mbs >= 0 && mhs >= 0 && mqs >= 0, "%s: negative mask stride (%lld, %lld, %lld)", fn, (long long)mbs, (long long)mhs,
                (long long)mqs);
  MDG_CHECK_ARG(mask != nullptr || S == 0, "%s: null mask", fn);
  if (S > 0) {
    uintptr_t lo, hi;
    mask_span_of(mask, B, mbs, Hm, mhs, T, mqs, S, lo, hi);
    MDG_CHECK_ARG(hi <= ol || oh <= lo, "%s: out overlaps mask", fn);
  }
  mk.mask = (const unsigned char*)mask;
  mk.summary = nullptr;
  mk.mbs = mbs; mk.mhs = mhs; mk.mqs = mqs;
  mk.qtiles = (T + MASK_QT - 1) / MASK_QT;
  mk.ktiles = (S + KT - 1) / KT;
  mk.per_head = Hm != 1;
  mk.vec = (uintptr_t)mask % 4 == 0 && mbs % 4 == 0 && mhs % 4 == 0 && mqs % 4 == 0;
  return MDG_OK;
}

// the byte range [lo, hi) a strided [B, H, N, width] operand spans
static inline void span_of(const void* p, int64_t B, int64_t bs, int64_t H, int64_t hs, int64_t N, int64_t ts, int64_t width,
                           size_t es, uintptr_t& lo, uintptr_t& hi) {
  int64_t mn = 0, mxe = 0;
  const int64_t ext[3] = {(B - 1) * bs, (H - 1) * hs, (N - 1) * ts};
  for (int i = 0; i < 3; i++) {
    if (ext[i] < 0) mn += ext[i];
    else mxe += ext[i];
  }
  lo = (uintptr_t)p + (uintptr_t)(mn * (int64_t)es);
  hi = (uintptr_t)p + (uintptr_t)((mxe + width) * (int64_t)es);
}

}  // namespace attn
}  // namespace mdg
