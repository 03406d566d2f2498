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

}  // namespace kv8
}  // namespace mdg
