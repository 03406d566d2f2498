// What the two attention kernels (attn.hip: prefill schedule; attn_decode.hip: split-key decode schedule) share: the MFMA wrapper
// per element type, the 8-element row load with its alignment paths, the key tile and the pitch of the transposed V tile, and the
// byte span of a strided operand for the overlap checks.
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
