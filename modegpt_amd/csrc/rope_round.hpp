// The rotary kernels' arithmetic (rope.hip, rope_rows.hip): torch's eager semantics for the tensor dtype, op by op.  Every product
// and every sum is computed in fp32 and rounded to the element type before the next op uses it, with no FMA contraction, so a
// rotation written with these helpers is bit-identical to the eager expression q * cos + rotate_half(q) * sin.
#pragma once
#include "common.hpp"

// hipcc contracts a*b+c into an FMA by default, and HIP's __fmul_rn / __fadd_rn are plain operators compiled under that
// default: with them the fp32 route would skip the rounding of the products that torch's separate mul / add kernels
// perform.  The arithmetic below therefore uses its own operators, defined after contraction is switched off (the pragma
// holds from here to the end of the including unit).
#pragma STDC FP_CONTRACT OFF

namespace mdg {

__device__ __forceinline__ float mul_r(float a, float b) { return a * b; }
__device__ __forceinline__ float add_r(float a, float b) { return a + b; }

template <int DT> struct Lp;
template <> struct Lp<MDG_BF16> {
  typedef bf16_t T;
  static __device__ __forceinline__ float up(T v) { return __uint_as_float(((unsigned)v) << 16); }
  // v_cvt_pk_bf16_f32: round to nearest even in one instruction
  static __device__ __forceinline__ T down(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
};
template <> struct Lp<MDG_F16> {
  typedef f16_t T;
  static __device__ __forceinline__ float up(T v) { return (float)__builtin_bit_cast(_Float16, v); }
  // The empty asm hides where f came from.  Without it the compiler may select "f16(a * b)" as a mixed-precision FMA with
  // an addend of +0, and (-0) + (+0) = +0: a product that is -0 (an all-zero row, a zero norm weight) lost its sign, and
  // with it the sign of a zero result (the tile kernel with an odd half returned -0 where torch has +0).
  static __device__ __forceinline__ T down(float f) {
    asm("" : "+v"(f));
    return __builtin_bit_cast(unsigned short, (_Float16)f);
  }
};
template <> struct Lp<MDG_F32> {
  typedef float T;
  static __device__ __forceinline__ float up(T v) { return v; }
  static __device__ __forceinline__ T down(float f) { return f; }
};

}  // namespace mdg
