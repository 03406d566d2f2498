// The paged fp8 KV cache (layout: include/modegpt_hip.h): rows as kv8.hip writes them -- e4m3 bytes zero-padded to `pitch`, one
// power-of-two fp32 scale -- but held in pages of `page` rows that a block table hands to the sequences, with the positions on the
// device.  The append that quantises the new K rows AND the new V rows of a layer in one launch, and the gather that reads a prefix
// back for the calls mdg_attn_decode_paged8 does not serve.  Both are one pass over HBM with no LDS.
//
// Append.  The grid is two runs of workgroups: the first `kblocks` take the K rows, the rest the V rows; a workgroup is of one side,
// so the side's arguments (source, strides, width, lane group, pool) are uniform in it.  The per-row work is kv8.hip's, statement for
// statement: a group of LG = 1 .. 16 lanes per row, lane c reads elements [16 c, 16 c + 16) as two load8, amax by xor-shuffles, the
// scale from amax's exponent bits, v_cvt_pk_fp8_f32 of x * 2^-e, one aligned 16-byte store a lane, lane 0 stores the scale -- the
// same bytes and the same scale as mdg_kv8_append gives that row.  What differs is where the row lands: row t of sequence b goes to
// position p = pos[b] + t, page block_table[b][p / page], offset p % page; each lane of the group loads pos[b] and the table entry
// itself (the same address over the group: one request).  A position outside 0 .. table_len * page - 1 is not written, and a table
// entry is clamped to 0 .. n_pages - 1 for memory safety only: a caller's table holds valid pages where it may be read.
// Gather.  One thread per (row, 16-element chunk) as in kv8.hip, the row found through the table.
#include "kv8.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;

// one side (K or V) of an append: its source, its pool and the lane group of its width
struct AppendSide {
  const void* src;
  unsigned char* data;
  float* scale;
  int64_t rows, pitch, sbs, shs, sts;
  int r, lg_shift, chunks, vec;  // chunks: 16-byte chunks of a pool row; vec: every source row starts 16-byte aligned
};

struct PagedAppendArgs {
  AppendSide side[2];  // K, V
  const int* table;
  const int* pos;
  int64_t T, limit;    // limit = table_len * page: positions at or beyond it are not written
  int64_t table_len, kblocks;
  int n_kv, page, n_pages;
};

template <int DT> __device__ __forceinline__ float elem_f32(unsigned w, int odd) {
  const unsigned h = half_of(w, odd);
  if constexpr (DT == MDG_BF16) return __uint_as_float(h << 16);
  else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

__device__ __forceinline__ int clamp_page(int p, int n_pages) { return p < 0 ? 0 : p >= n_pages ? n_pages - 1 : p; }

template <int DT> __global__ __launch_bounds__(THREADS) void kv8_paged_append_kernel(PagedAppendArgs a) {
  typedef typename Mma<DT>::E E;
  const bool is_v = (int64_t)blockIdx.x >= a.kblocks;
  const AppendSide s = is_v ? a.side[1] : a.side[0];  // uniform: the workgroup's side
  const int64_t gid = ((int64_t)blockIdx.x - (is_v ? a.kblocks : 0)) * THREADS + threadIdx.x;
  const int64_t row_ = gid >> s.lg_shift;
  const int c = (int)(gid & ((1 << s.lg_shift) - 1));
  bool live = row_ < s.rows;
  const int64_t row = live ? row_ : s.rows - 1;  // a group beyond the end repeats the last row and stores nothing
  const int64_t bh = row / a.T, t = row - bh * a.T;
  const int64_t b = bh / a.n_kv, g = bh - b * a.n_kv;
  const E* srow = (const E*)s.src + b * s.sbs + g * s.shs + t * s.sts;
  u32x4 x[2];
#pragma unroll
  for (int h = 0; h < 2; h++) x[h] = load8(srow, kv8::CHUNK * c + 8 * h, s.r, s.vec != 0);
  float f[16], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    f[j] = elem_f32<DT>(x[j >> 3][(j >> 1) & 3], j & 1);
    amax = fmaxf(amax, fabsf(f[j]));
  }
  for (int d = (1 << s.lg_shift) >> 1; d; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  float sc, inv;
  kv8::row_scale(amax, sc, inv);
  const u32x4 p = kv8::pack16(f, inv);
  // where the row lands: position -> (page, offset) through the sequence's table row
  const int64_t at = (int64_t)a.pos[b] + t;
  live = live && at >= 0 && at < a.limit;
  if (!live) return;
  const int64_t pi = at / a.page;
  const int pid = clamp_page(a.table[b * a.table_len + pi], a.n_pages);
  const int64_t slot = ((int64_t)pid * a.n_kv + g) * a.page + (at - pi * a.page);
  unsigned char* drow = s.data + slot * s.pitch;
  if (c < s.chunks) *(u32x4*)(drow + kv8::CHUNK * c) = p;
  // a pitch beyond the row's own chunks (the caller's choice): zero bytes too
  for (int cc = c + (1 << s.lg_shift); cc < s.chunks; cc += 1 << s.lg_shift) *(u32x4*)(drow + kv8::CHUNK * cc) = (u32x4){0u, 0u, 0u, 0u};
  if (c == 0) s.scale[slot] = sc;
}

struct PagedDequantArgs {
  const unsigned char* data;
  const float* scale;
  const int* table;
  void* out;
  int64_t items, S, pitch, table_len;
  int n_kv, page, n_pages;
  int r, chunks, vec;  // chunks: 16-element chunks that hold the r elements; vec: out's rows start 16-byte aligned
};

// One thread per (row, 16-element chunk): the row's page from the table, a 16-byte load, the row's scale, 8 scaled converts.
template <int DT> __global__ __launch_bounds__(THREADS) void kv8_paged_dequant_kernel(PagedDequantArgs a) {
  typedef typename Mma<DT>::E E;
  const int64_t gid = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (gid >= a.items) return;
  const int64_t row = gid / a.chunks;  // (b * n_kv + g) * S + t
  const int c = (int)(gid - row * a.chunks);
  const int64_t bh = row / a.S, t = row - bh * a.S;
  const int64_t b = bh / a.n_kv, g = bh - b * a.n_kv;
  const int64_t pi = t / a.page;
  const int pid = clamp_page(a.table[b * a.table_len + pi], a.n_pages);
  const int64_t slot = ((int64_t)pid * a.n_kv + g) * a.page + (t - pi * a.page);
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

// What both entries check of the pools' geometry (dtype-free), under the caller's name; `what` names the width in the messages.
int check_pool(const char* fn, const char* what, int r, int64_t pitch) {
  MDG_CHECK_ARG(r >= 1 && r <= 256, "%s: %s=%d must be in 1..256", fn, what, r);
  MDG_CHECK_ARG(pitch >= kv8::pitch_of(r) && pitch % kv8::CHUNK == 0, "%s: pitch=%lld must be a multiple of 16 and >= mdg_kv8_pitch(%d) = %lld",
                fn, (long long)pitch, r, (long long)kv8::pitch_of(r));
  return MDG_OK;
}
int check_pages(const char* fn, int64_t n_pages, int64_t page, int64_t table_len) {
  MDG_CHECK_ARG(page > 0 && page % KT == 0, "%s: page=%lld must be a positive multiple of %d", fn, (long long)page, KT);
  MDG_CHECK_ARG(n_pages >= 0 && table_len >= 0, "%s: negative n_pages or table_len", fn);
  MDG_CHECK_ARG(page <= 0x7fffffff && n_pages <= 0x7fffffff && table_len <= INT64_MAX / page, "%s: table_len*page overflows", fn);
  return MDG_OK;
}

int lane_group_shift(int r) {
  const int own = (int)(kv8::pitch_of(r) / kv8::CHUNK);
  int sh = 0;
  while ((1 << sh) < own) sh++;
  return sh;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_kv8_paged_append(const void* k_src, const void* v_src, int dtype, int64_t B, int n_kv, int64_t T, int r_k, int r_v,
                                    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride,
                                    int64_t v_head_stride, int64_t v_token_stride, void* k_data, void* k_scale, void* v_data,
                                    void* v_scale, int64_t n_pages, int64_t page, int64_t k_pitch, int64_t v_pitch,
                                    const void* block_table, int64_t table_len, const void* pos, void* stream) {
  const char* fn = "mdg_kv8_paged_append";
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16, "%s: dtype %d (bf16 or f16)", fn, dtype);
  MDG_CHECK_ARG(B >= 0 && n_kv >= 0 && T >= 0, "%s: negative extent", fn);
  MDG_TRY(check_pool(fn, "r_k", r_k, k_pitch));
  MDG_TRY(check_pool(fn, "r_v", r_v, v_pitch));
  MDG_TRY(check_pages(fn, n_pages, page, table_len));
  if (B == 0 || n_kv == 0 || T == 0) return MDG_OK;
  const int64_t wide = k_pitch > v_pitch ? k_pitch : v_pitch;
  MDG_CHECK_ARG(n_pages == 0 || n_pages <= INT64_MAX / n_kv / page / wide, "%s: n_pages*n_kv*page*pitch overflows", fn);
  MDG_CHECK_ARG(B <= INT64_MAX / 4 / (table_len > 0 ? table_len : 1) && B <= INT64_MAX / n_kv / T / 16, "%s: B*table_len overflows", fn);
  MDG_CHECK_ARG(k_src && v_src && block_table && pos, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)block_table % 4 == 0 && (uintptr_t)pos % 4 == 0, "%s: block_table and pos must be 4-byte aligned", fn);
  if (n_pages == 0 || table_len == 0) return MDG_OK;  // no position can be written
  MDG_CHECK_ARG(k_data && k_scale && v_data && v_scale, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)k_data % 16 == 0 && (uintptr_t)v_data % 16 == 0 && (uintptr_t)k_scale % 4 == 0 && (uintptr_t)v_scale % 4 == 0,
                "%s: data must be 16-byte and scales 4-byte aligned", fn);
  const int64_t rows = n_pages * n_kv * page;
  const Span target[4] = {Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                          Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                          Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                          Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)}};
  const size_t es = dtype_size(dtype);
  const Span in[4] = {span_of("k src", k_src, B, k_batch_stride, n_kv, k_head_stride, T, k_token_stride, r_k, es),
                      span_of("v src", v_src, B, v_batch_stride, n_kv, v_head_stride, T, v_token_stride, r_v, es),
                      Span{"block_table", (uintptr_t)block_table, (uintptr_t)block_table + (uintptr_t)(B * table_len * 4)},
                      Span{"pos", (uintptr_t)pos, (uintptr_t)pos + (uintptr_t)(B * 4)}};
  for (int i = 0; i < 4; i++) MDG_TRY(apart(fn, target, 4, in[i]));
  for (int i = 1; i < 4; i++) MDG_TRY(apart(fn, target, i, target[i]));

  PagedAppendArgs a;
  const void* src[2] = {k_src, v_src};
  unsigned char* data[2] = {(unsigned char*)k_data, (unsigned char*)v_data};
  float* scl[2] = {(float*)k_scale, (float*)v_scale};
  const int64_t st[2][3] = {{k_batch_stride, k_head_stride, k_token_stride}, {v_batch_stride, v_head_stride, v_token_stride}};
  const int r[2] = {r_k, r_v};
  const int64_t pitch[2] = {k_pitch, v_pitch};
  int64_t blocks[2];
  for (int i = 0; i < 2; i++) {
    AppendSide& s = a.side[i];
    s.src = src[i]; s.data = data[i]; s.scale = scl[i];
    s.rows = B * n_kv * T; s.pitch = pitch[i];
    s.sbs = st[i][0]; s.shs = st[i][1]; s.sts = st[i][2];
    s.r = r[i]; s.lg_shift = lane_group_shift(r[i]); s.chunks = (int)(pitch[i] / kv8::CHUNK);
    s.vec = (uintptr_t)src[i] % 16 == 0 && st[i][0] % 8 == 0 && st[i][1] % 8 == 0 && st[i][2] % 8 == 0;
    blocks[i] = ceil_div(s.rows << s.lg_shift, THREADS);
  }
  a.table = (const int*)block_table; a.pos = (const int*)pos;
  a.T = T; a.limit = table_len * page; a.table_len = table_len; a.kblocks = blocks[0];
  a.n_kv = n_kv; a.page = (int)page; a.n_pages = (int)n_pages;
  MDG_CHECK_ARG(blocks[0] + blocks[1] <= 0x7fffffff, "%s: B*n_kv*T=%lld rows exceed one launch", fn, (long long)(B * n_kv * T));
  const dim3 grid((unsigned)(blocks[0] + blocks[1]));
  if (dtype == MDG_BF16) hipLaunchKernelGGL(kv8_paged_append_kernel<MDG_BF16>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv8_paged_append_kernel<MDG_F16>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" int mdg_kv8_paged_dequant(const void* data, const void* scale, int dtype, int64_t B, int n_kv, int64_t S, int r, int64_t n_pages,
                                     int64_t page, int64_t pitch, const void* block_table, int64_t table_len, void* out, void* stream) {
  const char* fn = "mdg_kv8_paged_dequant";
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16, "%s: dtype %d (bf16 or f16)", fn, dtype);
  MDG_CHECK_ARG(B >= 0 && n_kv >= 0 && S >= 0, "%s: negative extent", fn);
  MDG_TRY(check_pool(fn, "r", r, pitch));
  MDG_TRY(check_pages(fn, n_pages, page, table_len));
  MDG_CHECK_ARG(S <= table_len * page, "%s: S=%lld rows exceed table_len*page=%lld", fn, (long long)S, (long long)(table_len * page));
  if (B == 0 || n_kv == 0 || S == 0) return MDG_OK;
  MDG_CHECK_ARG(n_pages > 0, "%s: S=%lld rows of a pool without pages", fn, (long long)S);
  MDG_CHECK_ARG(n_pages <= INT64_MAX / n_kv / page / pitch, "%s: n_pages*n_kv*page*pitch overflows", fn);
  MDG_CHECK_ARG(B <= INT64_MAX / 4 / table_len && B <= INT64_MAX / n_kv / S / 512, "%s: B*table_len overflows", fn);
  MDG_CHECK_ARG(data && scale && out && block_table, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)data % 16 == 0 && (uintptr_t)scale % 4 == 0, "%s: data must be 16-byte and scale 4-byte aligned", fn);
  MDG_CHECK_ARG((uintptr_t)block_table % 4 == 0, "%s: block_table must be 4-byte aligned", fn);
  const int64_t rows = n_pages * n_kv * page;
  const Span o = span_of("out", out, 1, 0, 1, 0, B * n_kv * S, r, r, dtype_size(dtype));
  const Span target[3] = {Span{"data", (uintptr_t)data, (uintptr_t)data + (uintptr_t)(rows * pitch)},
                          Span{"scale", (uintptr_t)scale, (uintptr_t)scale + (uintptr_t)(rows * 4)},
                          Span{"block_table", (uintptr_t)block_table, (uintptr_t)block_table + (uintptr_t)(B * table_len * 4)}};
  MDG_TRY(apart(fn, target, 3, o));

  PagedDequantArgs a;
  a.data = (const unsigned char*)data; a.scale = (const float*)scale; a.table = (const int*)block_table; a.out = out;
  a.S = S; a.pitch = pitch; a.table_len = table_len;
  a.n_kv = n_kv; a.page = (int)page; a.n_pages = (int)n_pages;
  a.r = r;
  a.chunks = (int)(kv8::pitch_of(r) / kv8::CHUNK);
  a.items = B * n_kv * S * a.chunks;
  a.vec = (uintptr_t)out % 16 == 0 && r % 8 == 0;
  const int64_t blocks = ceil_div(a.items, THREADS);
  MDG_CHECK_ARG(blocks <= 0x7fffffff, "%s: B*n_kv*S=%lld rows exceed one launch", fn, (long long)(B * n_kv * S));
  if (dtype == MDG_BF16) hipLaunchKernelGGL(kv8_paged_dequant_kernel<MDG_BF16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(kv8_paged_dequant_kernel<MDG_F16>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
