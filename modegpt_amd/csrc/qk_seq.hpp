// What the two sequence kernels share (qk_pair.hip, qk_causal.hip): one 512-thread workgroup per (sequence b, query head h)
// streams the T post-RoPE rows of its heads through LDS in 16-token stages (threads 0-255 the query rows, threads 256-511 the
// key rows), writes its statistic into the workspace slot of (b, h), and a fold kernel adds the slots onto the caller's
// matrices in ascending b.  Here: the kernel arguments, the stage load and store (common.hpp's Stage<DT>, as cov.hip's cov_tile
// stages), the fold, the workspace size and the host half of an entry point (argument checks, arguments, the two launches).
// Each unit keeps its kernel and its extern "C" names.
#pragma once
#include "common.hpp"

namespace mdg {

constexpr int SEQ_MAX_HD = TILE;

struct SeqArgs {
  const void* q;
  const void* k;
  int64_t ld_q, ld_k, T;
  int n_heads, group, hd;
  int vec_q, vec_k;
  double* part;      // [B, n_heads, hd, hd]
  double* part_raw;  // same, or nullptr
};

// One 16-token stage of one head: rows tok0 .. tok0+15 (below tok_end), columns 0 .. hd-1 of `base` (the head's first element
// of the sequence's first row).  Everything outside stays zero: a ragged hd and a ragged last stage add exact zeros.
template <int DT>
__device__ __forceinline__ void seq_load(const void* base, int64_t ld, int64_t tok0, int64_t tok_end, int hd, int vec_ok,
                                         int tid, typename Stage<DT>::Chunk* regs) {
  typedef Stage<DT> S;
  typedef typename S::T T;
  const T* x = (const T*)base;
#pragma unroll
  for (int p = 0; p < S::CPT; p++) {
    int row, col;
    S::chunk_rc(tid + 256 * p, row, col);
    const int64_t tok = tok0 + row;
    typename S::Chunk ch;
    ch.q = make_uint4(0, 0, 0, 0);
    if (tok < tok_end && col < hd) {
      const T* src = x + tok * ld + col;
      if (vec_ok && col + S::VEC <= hd) {
        ch.q = *(const uint4*)src;
      } else {
#pragma unroll
        for (int e = 0; e < S::VEC; e++)
          if (col + e < hd) ch.e[e] = src[e];
      }
    }
    regs[p] = ch;
  }
}

// The staged chunks as fp64 into LDS rows of ROW_PITCH elements (`dst0`: the stage's first element of this head)
template <int DT, int ROW_PITCH>
__device__ __forceinline__ void seq_store(double* dst0, int tid, const typename Stage<DT>::Chunk* regs) {
  typedef Stage<DT> S;
#pragma unroll
  for (int p = 0; p < S::CPT; p++) {
    int row, col;
    S::chunk_rc(tid + 256 * p, row, col);
    double* dst = dst0 + row * ROW_PITCH + col;
#pragma unroll
    for (int e = 0; e < S::VEC; e += 2) *(d2*)(dst + e) = (d2){load_f64<DT>(regs[p].e, e), load_f64<DT>(regs[p].e, e + 1)};
  }
}

// pair[h][e] = (..((pair[h][e] + part[0][h][e]) + part[1][h][e]) .. + part[B-1][h][e]): ascending b, ONE ADDITION PER SEQUENCE onto
// the running value, so a call over B sequences gives the bits of B calls over one sequence each
static __global__ __launch_bounds__(256) void qk_seq_fold_kernel(const double* part, const double* part_raw, int64_t B, int64_t n,
                                                                 double* pair, double* pair_raw) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double v = pair[e];
  for (int64_t b = 0; b < B; b++) v += part[b * n + e];
  pair[e] = v;
  if (part_raw) {
    double w = pair_raw[e];
    for (int64_t b = 0; b < B; b++) w += part_raw[b * n + e];
    pair_raw[e] = w;
  }
}

struct SeqWs {
  double *part, *part_raw;   // [B][n_heads][hd][hd] each: the slots of SeqArgs; part_raw only where the raw statistic is wanted
  size_t bytes;
};
static inline SeqWs seq_layout(void* ws, int64_t B, int n_heads, int hd, int want_raw) {
  const size_t slots = (size_t)B * (size_t)n_heads * (size_t)hd * (size_t)hd;
  Carve c(ws);
  SeqWs w;
  w.part = c.take<double>(slots);
  w.part_raw = want_raw ? c.take<double>(slots) : nullptr;
  w.bytes = c.off;
  return w;
}
static inline size_t seq_ws_bytes(int64_t B, int n_heads, int hd, int want_raw) {
  if (B <= 0 || n_heads <= 0 || hd <= 0) return 0;
  return seq_layout(nullptr, B, n_heads, hd, want_raw).bytes;
}

// The host half of the entry point `name` (its messages carry it): checks, arguments, then launch(dtype, args, grid, stream) --
// the unit's kernel over B * n_heads workgroups of 512 -- and the fold behind it.
template <class Launch>
static int seq_accum(const char* name, const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T,
                     int n_heads, int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes, void* stream,
                     Launch launch) {
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16 || dtype == MDG_F32, "%s: dtype %d (bf16, f16 or f32)", name, dtype);
  MDG_CHECK_ARG(hd >= 1 && hd <= SEQ_MAX_HD, "%s: head_dim=%d must be >= 1 and <= %d", name, hd, SEQ_MAX_HD);
  MDG_CHECK_ARG(n_heads > 0 && n_kv > 0 && n_heads % n_kv == 0, "%s: n_heads=%d must be a positive multiple of n_kv=%d", name,
                n_heads, n_kv);
  MDG_CHECK_ARG(B >= 0 && T >= 0, "%s: negative extent (B=%lld T=%lld)", name, (long long)B, (long long)T);
  const int64_t wq = (int64_t)n_heads * hd, wk = (int64_t)n_kv * hd;
  MDG_CHECK_ARG(ld_q >= wq, "%s: ld_q=%lld < n_heads*head_dim=%lld", name, (long long)ld_q, (long long)wq);
  MDG_CHECK_ARG(ld_k >= wk, "%s: ld_k=%lld < n_kv*head_dim=%lld", name, (long long)ld_k, (long long)wk);
  if (B == 0 || T == 0) return MDG_OK;
  MDG_CHECK_ARG(B <= 0x7fffffff / (int64_t)n_heads && ceil_div((int64_t)n_heads * hd * hd, 256) <= 0x7fffffff,
                "%s: B*n_heads = %lld x %d exceeds one launch", name, (long long)B, n_heads);
  MDG_CHECK_ARG(q && k && pair && ws, "%s: null pointer", name);
  const size_t need = seq_ws_bytes(B, n_heads, hd, pair_raw != nullptr);
  MDG_CHECK_ARG(ws_bytes >= need, "%s: workspace %zu < required %zu", name, ws_bytes, need);
  MDG_CHECK_ARG((uintptr_t)ws % 8 == 0, "%s: workspace is not 8-byte aligned", name);

  const int64_t es = (int64_t)dtype_size(dtype);
  const int64_t n = (int64_t)n_heads * hd * hd;
  SeqArgs a;
  a.q = q; a.k = k; a.ld_q = ld_q; a.ld_k = ld_k; a.T = T;
  a.n_heads = n_heads; a.group = n_heads / n_kv; a.hd = hd;
  // 16-byte loads: the base, every row and every head start must be 16-byte aligned
  a.vec_q = (uintptr_t)q % 16 == 0 && (ld_q * es) % 16 == 0 && (hd * es) % 16 == 0;
  a.vec_k = (uintptr_t)k % 16 == 0 && (ld_k * es) % 16 == 0 && (hd * es) % 16 == 0;
  const SeqWs w = seq_layout(ws, B, n_heads, hd, pair_raw != nullptr);
  a.part = w.part;
  a.part_raw = w.part_raw;
  hipStream_t st = (hipStream_t)stream;
  launch(dtype, a, dim3((unsigned)(B * n_heads)), st);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(qk_seq_fold_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, a.part, a.part_raw, B, n, pair, pair_raw);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg
