// The fp8 KV cache of compressed heads (layout: include/modegpt_hip.h): the append that quantises new rows into it and the dequantise
// that reads a prefix back for the calls mdg_attn_decode_kv8 does not serve.  Both are one pass over HBM with no LDS.
//
// Append.  A group of LG = 1, 2, 4, 8 or 16 lanes (the least power of two that covers the row's 16-element chunks) takes one source
// row; lane c of the group reads elements [16 c, 16 c + 16) as two 8-element loads (attn_tile.hpp's load8: the source keeps its own
// strides and a row of odd width starts at 2-byte alignment), the row's amax is the maximum over the group by LG - 1 xor-shuffles,
// and every lane derives the same scale from amax's exponent bits:  amax = m 2^k with 1 <= m < 2 gives e = k - 8 when m <= 1.75
// (448 = 1.75 * 2^8) and k - 7 otherwise, clamped to the fp32 normal range; amax == 0 gives scale 1.  x * 2^-e is exact, so
// v_cvt_pk_fp8_f32 (round to nearest even, two elements an instruction) rounds x / scale once.  The lane stores its 16 bytes with one
// aligned store -- elements >= r were read as zero, so the padding is written with the data -- and lane 0 stores the scale.
#include "kv8.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;

struct AppendArgs {
  const void* src;
  unsigned char* data;
  float* scale;
  int64_t rows, T, cap, pitch, pos, sbs, shs, sts;
  int n_kv, r, lg_shift, chunks, vec;  // chunks: 16-byte chunks of a cache row; vec: every source row starts 16-byte aligned
};

template <int DT> __device__ __forceinline__ float elem_f32(unsigned w, int odd) {
  const unsigned h = half_of(w, odd);
  if constexpr (DT == MDG_BF16) return __uint_as_float(h << 16);
  else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

template <int DT> __global__ __launch_bounds__(THREADS) void kv8_append_kernel(AppendArgs a) {
  typedef typename Mma<DT>::E E;
  const int64_t gid = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t row_ = gid >> a.lg_shift;
  const int c = (int)(gid & ((1 << a.lg_shift) - 1));
  const bool live = row_ < a.rows;
  const int64_t row = live ? row_ : a.rows - 1;  // a group beyond the end repeats the last row and stores nothing
  const int64_t bh = row / a.T, t = row - bh * a.T;
  const int64_t b = bh / a.n_kv, g = bh - b * a.n_kv;
  const E* srow = (const E*)a.src + b * a.sbs + g * a.shs + t * a.sts;
  u32x4 x[2];
#pragma unroll
  for (int h = 0; h < 2; h++) x[h] = load8(srow, kv8::CHUNK * c + 8 * h, a.r, a.vec != 0);
  float f[16], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    f[j] = elem_f32<DT>(x[j >> 3][(j >> 1) & 3], j & 1);
    amax = fmaxf(amax, fabsf(f[j]));
  }
  for (int d = (1 << a.lg_shift) >> 1; d; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  float s, inv;
  kv8::row_scale(amax, s, inv);
  const u32x4 p = kv8::pack16(f, inv);
  if (!live) return;
  const int64_t slot = bh * a.cap + a.pos + t;
  unsigned char* drow = a.data + slot * a.pitch;
  if (c < a.chunks) *(u32x4*)(drow + kv8::CHUNK * c) = p;
  // a pitch beyond the row's own chunks (the caller's choice): zero bytes too
  for (int cc = c + (1 << a.lg_shift); cc < a.chunks; cc += 1 << a.lg_shift) *(u32x4*)(drow + kv8::CHUNK * cc) = (u32x4){0u, 0u, 0u, 0u};
  if (c == 0) a.scale[slot] = s;
}

struct DequantArgs {
  const unsigned char* data;
  const float* scale;
  void* out;
  int64_t items, S, cap, pitch;
  int r, chunks, vec;  // chunks: 16-element chunks that hold the r elements; vec: out's rows start 16-byte aligned
};

// One thread per (row, 16-element chunk): a 16-byte load, the row's scale, 8 scaled converts; 16-byte stores where out's rows allow.
template <int DT> __global__ __launch_bounds__(THREADS) void kv8_dequant_kernel(DequantArgs a) {
  typedef typename Mma<DT>::E E;
  const int64_t gid = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (gid >= a.items) return;
  const int64_t row = gid / a.chunks;  // (b * n_kv + g) * S + t
  const int c = (int)(gid - row * a.chunks);
  const int64_t bh = row / a.S, t = row - bh * a.S;
  const int64_t slot = bh * a.cap + t;
  const u32x4 w = *(const u32x4*)(a.data + slot * a.pitch + kv8::CHUNK * c);
  const float s = a.scale[slot];
  E* orow = (E*)a.out + row * a.r;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const u32x4 d = kv8::dequant8<DT>(w[2 * h], w[2 * h + 1], s);
    const int c0 = kv8::CHUNK * c + 8 * h;
    if (a.vec && c0 + 8 <= a.r) {
      *(u32x4*)(orow + c0) = d;
    } else {
      unsigned short* o = (unsigned short*)orow;
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (c0 + j < a.r) o[c0 + j] = (unsigned short)half_of(d[j >> 1], j & 1);
    }
  }
}

// what both entries check of a cache: its dtype-free geometry, under the caller's name
int check_cache(const char* fn, int64_t B, int n_kv, int64_t n, int r, int64_t cap, int64_t pitch) {
  MDG_CHECK_ARG(B >= 0 && n_kv >= 0 && n >= 0 && cap >= 0, "%s: negative extent", fn);
  MDG_CHECK_ARG(r >= 1 && r <= 256, "%s: r=%d must be in 1..256", fn, r);
  MDG_CHECK_ARG(pitch >= kv8::pitch_of(r) && pitch % kv8::CHUNK == 0, "%s: pitch=%lld must be a multiple of 16 and >= mdg_kv8_pitch(%d) = %lld",
                fn, (long long)pitch, r, (long long)kv8::pitch_of(r));
  return MDG_OK;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int64_t mdg_kv8_pitch(int r) { return r <= 0 ? 0 : kv8::pitch_of(r); }

extern "C" int mdg_kv8_append(const void* src, int dtype, int64_t B, int n_kv, int64_t T, int r, int64_t src_batch_stride,
                              int64_t src_head_stride, int64_t src_token_stride, void* data, void* scale, int64_t cap, int64_t pitch,
                              int64_t pos, void* stream) {
  const char* fn = "mdg_kv8_append";
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16, "%s: dtype %d (bf16 or f16)", fn, dtype);
  MDG_TRY(check_cache(fn, B, n_kv, T, r, cap, pitch));
  MDG_CHECK_ARG(pos >= 0 && T <= cap && pos <= cap - T, "%s: pos=%lld + T=%lld rows exceed cap=%lld", fn, (long long)pos, (long long)T,
                (long long)cap);
  if (B == 0 || n_kv == 0 || T == 0) return MDG_OK;
  MDG_CHECK_ARG(B <= INT64_MAX / n_kv / cap / pitch, "%s: B*n_kv*cap*pitch overflows", fn);
  MDG_CHECK_ARG(src && data && scale, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)data % 16 == 0 && (uintptr_t)scale % 4 == 0, "%s: data must be 16-byte and scale 4-byte aligned", fn);
  const Span s = span_of("src", src, B, src_batch_stride, n_kv, src_head_stride, T, src_token_stride, r, dtype_size(dtype));
  const Span target[2] = {Span{"data", (uintptr_t)data, (uintptr_t)data + (uintptr_t)(B * n_kv * cap * pitch)},
                          Span{"scale", (uintptr_t)scale, (uintptr_t)scale + (uintptr_t)(B * n_kv * cap * 4)}};
  MDG_TRY(apart(fn, target, 2, s));
  MDG_TRY(apart(fn, target, 1, target[1]));

  AppendArgs a;
  a.src = src; a.data = (unsigned char*)data; a.scale = (float*)scale;
  a.rows = B * n_kv * T; a.T = T; a.cap = cap; a.pitch = pitch; a.pos = pos;
  a.sbs = src_batch_stride; a.shs = src_head_stride; a.sts = src_token_stride;
  a.n_kv = n_kv; a.r = r;
  const int own = (int)(kv8::pitch_of(r) / kv8::CHUNK);
  a.lg_shift = 0;
  while ((1 << a.lg_shift) < own) a.lg_shift++;
  a.chunks = (int)(pitch / kv8::CHUNK);
  a.vec = (uintptr_t)src % 16 == 0 && src_batch_stride % 8 == 0 && src_head_stride % 8 == 0 && src_token_stride % 8 == 0;
  const int64_t blocks = ceil_div(a.rows << a.lg_shift, THREADS);
  MDG_CHECK_ARG(blocks <= 0x7fffffff, "%s: B*n_kv*T=%lld rows exceed one launch", fn, (long long)a.rows);
  if (dtype == MDG_BF16) hipLaunchKernelGGL(kv8_append_kernel<MDG_BF16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv8_append_kernel<MDG_F16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" int mdg_kv8_dequant(const void* data, const void* scale, int dtype, int64_t B, int n_kv, int64_t S, int r, int64_t cap,
                               int64_t pitch, void* out, void* stream) {
  const char* fn = "mdg_kv8_dequant";
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16, "%s: dtype %d (bf16 or f16)", fn, dtype);
  MDG_TRY(check_cache(fn, B, n_kv, S, r, cap, pitch));
  MDG_CHECK_ARG(S <= cap, "%s: S=%lld rows exceed cap=%lld", fn, (long long)S, (long long)cap);
  if (B == 0 || n_kv == 0 || S == 0) return MDG_OK;
  MDG_CHECK_ARG(B <= INT64_MAX / n_kv / cap / pitch, "%s: B*n_kv*cap*pitch overflows", fn);
  MDG_CHECK_ARG(data && scale && out, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)data % 16 == 0 && (uintptr_t)scale % 4 == 0, "%s: data must be 16-byte and scale 4-byte aligned", fn);
  const Span o = span_of("out", out, 1, 0, 1, 0, B * n_kv * S, r, r, dtype_size(dtype));
  const Span target[2] = {Span{"data", (uintptr_t)data, (uintptr_t)data + (uintptr_t)(B * n_kv * cap * pitch)},
                          Span{"scale", (uintptr_t)scale, (uintptr_t)scale + (uintptr_t)(B * n_kv * cap * 4)}};
  MDG_TRY(apart(fn, target, 2, o));

  DequantArgs a;
  a.data = (const unsigned char*)data; a.scale = (const float*)scale; a.out = out;
  a.S = S; a.cap = cap; a.pitch = pitch; a.r = r;
  a.chunks = (int)(kv8::pitch_of(r) / kv8::CHUNK);
  a.items = B * n_kv * S * a.chunks;
  a.vec = (uintptr_t)out % 16 == 0 && r % 8 == 0;
  const int64_t blocks = ceil_div(a.items, THREADS);
  MDG_CHECK_ARG(blocks <= 0x7fffffff, "%s: B*n_kv*S=%lld rows exceed one launch", fn, (long long)(B * n_kv * S));
  if (dtype == MDG_BF16) hipLaunchKernelGGL(kv8_dequant_kernel<MDG_BF16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv8_dequant_kernel<MDG_F16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
