// The device side of the fp8 KV cache's layout (include/modegpt_hip.h states it; kv8.hip writes and reads it back, attn_decode_kv8.hip
// multiplies from it): rows of `pitch` bytes of OCP e4m3, 16 to an aligned load, one power-of-two fp32 scale per row.
#pragma once
#include "attn_tile.hpp"

namespace mdg {
namespace kv8 {

using attn::u32x4;

constexpr int CHUNK = 16;  // elements of one 16-byte load; a row is padded with zero bytes to a whole number of them

static inline int64_t pitch_of(int64_t r) { return (r + CHUNK - 1) / CHUNK * CHUNK; }

// v_cvt_scalef32_pk_{bf16,f16}_fp8: two e4m3 bytes of a word (the low or the high pair) times `s`, rounded to the element type,
// as one dword of two elements.  With s a power of two the product of an e4m3 value (<= 4 significant bits) is exact in bf16.
template <int DT> struct Cvt;
template <> struct Cvt<MDG_BF16> {
  template <bool HI> __device__ static __forceinline__ unsigned pair(unsigned w, float s) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, HI));
  }
};
template <> struct Cvt<MDG_F16> {
  template <bool HI> __device__ static __forceinline__ unsigned pair(unsigned w, float s) {
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, HI));
  }
};

// The 8 elements of two consecutive words, in byte order, as the 4 dwords of an MFMA fragment (or of a 16-byte store).
template <int DT> __device__ __forceinline__ u32x4 dequant8(unsigned w0, unsigned w1, float s) {
  return (u32x4){Cvt<DT>::template pair<false>(w0, s), Cvt<DT>::template pair<true>(w0, s), Cvt<DT>::template pair<false>(w1, s),
                 Cvt<DT>::template pair<true>(w1, s)};
}

// The row quantiser of every kernel that writes the cache (kv8.hip, kv8_paged.hip, rope_kv8_step.hip), after the row's amax is known to
// every lane.  row_scale: amax = m 2^k with 1 <= m < 2 gives e = k - 8 when m <= 1.75 (448 = 1.75 * 2^8) and k - 7 otherwise, clamped
// to the fp32 normal range; the scale is 2^e and `inv` its exact reciprocal; an all-zero row gets scale 1.
__device__ __forceinline__ void row_scale(float amax, float& s, float& inv) {
  const unsigned ab = __float_as_uint(amax);
  int e = (int)(ab >> 23) - 127 - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < -126 ? -126 : e > 127 ? 127 : e;
  const bool zero = amax == 0.f;
  s = zero ? 1.f : __uint_as_float((unsigned)(e + 127) << 23);
  inv = zero ? 1.f : __uint_as_float((unsigned)(127 - e) << 23);  // e <= 121 for any fp32 amax: a normal number
}
// A lane's 16 elements as the 16 e4m3 bytes of its chunk: x * 2^-e is exact, so v_cvt_pk_fp8_f32 rounds x / scale once.
__device__ __forceinline__ u32x4 pack16(const float (&f)[16], float inv) {
  u32x4 p;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w] * inv, f[4 * w + 1] * inv, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2] * inv, f[4 * w + 3] * inv, v, true);
    p[w] = (unsigned)v;
  }
  return p;
}

}  // namespace kv8
}  // namespace mdg
