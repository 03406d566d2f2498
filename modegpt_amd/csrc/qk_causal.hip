// Causal Q/K statistic: what dropping the columns D of a head costs the attention logits of a CAUSAL decoder, where query i of a
// sequence multiplies the keys j <= i only and its softmax normalises over n_i = i + 1 of them.  Per sequence of T post-RoPE rows
// (mdg_rope_rows), query head h, kv = h / (n_heads / n_kv), with the running prefix sums over the keys
//   K_i = sum_{j<=i} k_j k_j^T,   m_i = sum_{j<=i} k_j,   n_i = i + 1,
//   pair[h]     += sum_s sum_i (q_i q_i^T) (.) (K_i - m_i m_i^T / n_i) / n_i      (variance over the keys query i can see)
//   pair_raw[h] += sum_s sum_i (q_i q_i^T) (.)  K_i / n_i                         (mean square over them)
// (DESIGN.md "The causal Q/K statistic").  1^T pair[h][D,D] 1 = sum_s sum_i Var_{j<=i}(q_iD . k_jD).
//
// The recurrence is serial in the token and element-wise in (a, b), so it runs on the vector ALU, not on MFMA.  Launch shape: one
// 512-thread workgroup per (sequence b, query head h).  Thread t owns the 4 x 8 entries rows 4 (t >> 4) .. + 3, columns
// (t & 15) + 16 j, j = 0 .. 7 (strided, so that the 16 column lanes of a wave read 16 adjacent LDS words, not 16 words 64 bytes
// apart) of K, pair and pair_raw in registers (32 entries x 3 matrices = 192 VGPRs at two waves per SIMD).  The T
// tokens stream through LDS in 16-token double-buffered stages, converted to fp64 once while staging (threads 0-255 stage the
// query rows of head h, threads 256-511 the key rows of kv head kv), with the next stage's global loads in flight.  At the top of
// a stage threads 0-127 extend the key column sums through the staged rows (column t, ascending token) into the rows' prefix
// sums m_i, and threads 128-143 write the reciprocals r_i = 1.0 / n_i; every thread then reads the same m and r, so there is
// no barrier per token.  Per token and entry, in this order and with these roundings (fma: one rounding):
//   K  = fma(k_a, k_b, K)          qq = q_a * q_b  (exact for bf16 / f16 / f32 rows)       w = qq * r
//   mm = m_a * m_b                 t  = fma(-mm, r, K)        pair = fma(w, t, pair)       pair_raw = fma(w, K, pair_raw)
// -- four fused and three plain operations, 11 flops.  Tokens beyond T are not visited; columns beyond hd are exact zeros and
// their threads idle.  K is recomputed by every query head of a group: the workgroups share nothing, and a non-finite element
// stays in the heads it belongs to.  Each workgroup writes the workspace slot of (b, h); qk_causal_fold_kernel then adds the
// slots onto pair in ascending b, ONE ADDITION PER SEQUENCE onto the running value, so a call over B sequences gives the bits of
// B calls over one sequence each.  No atomics, every sum in a fixed order.
//
// Symmetry to the bit: every operation above is symmetric in (a, b) -- the products commute and m, r, q, k are the same LDS
// values for both entries -- and nothing is contracted or reassociated (FP_CONTRACT OFF, explicit fma), so entry (a, b) and
// entry (b, a) come out equal without a mirror pass.
//
// The staging (CStage, causal_load, causal_store) follows cov.hip's cov_tile by way of qk_pair.hip's PStage, pair_load and
// pair_store -- copied, not shared, so that those units stay as they are.
#include "common.hpp"
#pragma STDC FP_CONTRACT OFF

namespace mdg {
namespace {

constexpr int MAX_HD = TILE;
constexpr int BR = 4, BC = 8;  // a thread's block of entries: BR rows x BC columns; (TILE / BR) * (TILE / BC) = 512 threads
constexpr int CS = TILE / BC;       // the stride between a thread's BC columns
constexpr int ROW = 3 * PITCH;   // fp64 elements of one token's LDS row: q, k and the key prefix sums m
constexpr int STAGE = BK * ROW;

struct CausalArgs {
  const void* q;
  const void* k;
  int64_t ld_q, ld_k, T;
  int n_heads, group, hd;
  int vec_q, vec_k;
  double* part;      // [B, n_heads, hd, hd]
  double* part_raw;  // same, or nullptr
};

// qk_pair.hip PStage<DT> (cov.hip Stage<DT>): the chunk -> (token row, first column) map that spreads a ds_write_b128 group over
// all bank quads
template <int DT> struct CStage {
  typedef typename ElemOf<DT>::type T;
  static constexpr int VEC = 16 / (int)sizeof(T);
  static constexpr int CPR = TILE / VEC;
  static constexpr int CPT = BK * CPR / 256;
  union Chunk {
    uint4 q;
    T e[VEC];
  };
  static constexpr int RG = VEC >= 8 ? 4 : (VEC == 4 ? 2 : 1);
  static constexpr int CG = 8 / RG;
  __device__ static __forceinline__ void chunk_rc(int c, int& row, int& col) {
    const int g = c >> 3, i = c & 7;
    row = (g % (BK / RG)) * RG + (i % RG);
    col = ((g / (BK / RG)) * CG + i / RG) * VEC;
  }
};

// qk_pair.hip pair_load: one 16-token stage of one head, rows tok0 .. tok0+15 (below tok_end), columns 0 .. hd-1 of `base` (the
// head's first element of the sequence's first row).  Everything outside stays zero.
template <int DT>
__device__ __forceinline__ void causal_load(const void* base, int64_t ld, int64_t tok0, int64_t tok_end, int hd, int vec_ok,
                                            int tid, typename CStage<DT>::Chunk* regs) {
  typedef CStage<DT> S;
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

// qk_pair.hip pair_store, into this unit's stage layout (`dst0`: the stage's first q or k element)
template <int DT>
__device__ __forceinline__ void causal_store(double* dst0, int tid, const typename CStage<DT>::Chunk* regs) {
  typedef CStage<DT> S;
#pragma unroll
  for (int p = 0; p < S::CPT; p++) {
    int row, col;
    S::chunk_rc(tid + 256 * p, row, col);
    double* dst = dst0 + row * ROW + col;
#pragma unroll
    for (int e = 0; e < S::VEC; e += 2) *(d2*)(dst + e) = (d2){load_f64<DT>(regs[p].e, e), load_f64<DT>(regs[p].e, e + 1)};
  }
}

template <int DT, bool RAW>
__global__ __launch_bounds__(512) void qk_causal_kernel(CausalArgs a) {
  typedef CStage<DT> S;
  // two stages of 16 token rows; a row is  q[0..127] . .  k[0..127] . .  m[0..127] . .  (m: the key prefix sums m_i), so that
  // one address serves the three operands of an entry's row and one those of its column
  __shared__ __attribute__((aligned(16))) double lds[2 * STAGE];
  __shared__ double rinv[BK];        // 1.0 / n_i of the current stage's tokens
  // wave-uniform, and said so: 0 stages the query rows, 1 the key rows (the head's base pointer and pitch then sit in SGPRs)
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const int tid = threadIdx.x & 255;
  const int b = blockIdx.x / a.n_heads, h = blockIdx.x % a.n_heads, kv = h / a.group;
  const size_t es = sizeof(typename S::T);
  const int64_t ld = role ? a.ld_k : a.ld_q;
  const int vec_ok = role ? a.vec_k : a.vec_q;
  const char* base = role ? (const char*)a.k + ((int64_t)b * a.T * a.ld_k + (int64_t)kv * a.hd) * es
                          : (const char*)a.q + ((int64_t)b * a.T * a.ld_q + (int64_t)h * a.hd) * es;
  const int64_t n_stage = (a.T + BK - 1) / BK;

  const int ra = (int)(threadIdx.x >> 4) * BR, cb = (int)(threadIdx.x & 15);  // columns cb + CS j: the lanes of a wave read adjacent banks
  const bool active = ra < a.hd && cb < a.hd;  // (a block wholly beyond hd holds exact zeros that nobody reads)
  double Kk[BR][BC], Pc[BR][BC], Pr[RAW ? BR : 1][RAW ? BC : 1];
#pragma unroll
  for (int i = 0; i < BR; i++)
#pragma unroll
    for (int j = 0; j < BC; j++) {
      Kk[i][j] = 0.;
      Pc[i][j] = 0.;
      if constexpr (RAW) Pr[i][j] = 0.;
    }

  typename S::Chunk regs[S::CPT];
  causal_load<DT>(base, ld, 0, a.T, a.hd, vec_ok, tid, regs);
  causal_store<DT>(lds + role * PITCH, tid, regs);
  __syncthreads();
  for (int64_t s = 0; s < n_stage; s++) {
    const int cur = (int)(s & 1);
    const bool more = s + 1 < n_stage;
    double* stage = lds + cur * STAGE;
    // the next stage's global loads fly while this one is worked through
    if (more) causal_load<DT>(base, ld, (s + 1) * BK, a.T, a.hd, vec_ok, tid, regs);
    if (threadIdx.x < TILE) {
      // column threadIdx.x: the key sum up to the last stage is the last row of the other stage's m
      double mrun = s ? lds[(cur ^ 1) * STAGE + (BK - 1) * ROW + 2 * PITCH + threadIdx.x] : 0.;
#pragma unroll
      for (int t = 0; t < BK; t++) {
        mrun += stage[t * ROW + PITCH + threadIdx.x];  // (rows beyond T are zeros and are not read below)
        stage[t * ROW + 2 * PITCH + threadIdx.x] = mrun;
      }
    } else if (threadIdx.x < TILE + BK) {
      const int t = (int)threadIdx.x - TILE;
      rinv[t] = 1.0 / (double)(s * BK + t + 1);
    }
    __syncthreads();
    const int64_t left = a.T - s * BK;
    const int nt = left < BK ? (int)left : BK;
    if (active) {
#pragma unroll 1
      for (int t = 0; t < nt; t++) {
        const double* rowp = stage + t * ROW + ra;
        const double* colp = stage + t * ROW + cb;
        const double r = rinv[t];
        double qa[BR], ka[BR], ma[BR];
#pragma unroll
        for (int i = 0; i < BR; i += 2) {
          const d2 x = *(const d2*)(rowp + i), y = *(const d2*)(rowp + PITCH + i), z = *(const d2*)(rowp + 2 * PITCH + i);
          qa[i] = x.x; qa[i + 1] = x.y;
          ka[i] = y.x; ka[i + 1] = y.y;
          ma[i] = z.x; ma[i + 1] = z.y;
        }
#pragma unroll
        for (int j = 0; j < BC; j++) {
          const double qb = colp[CS * j], kb = colp[PITCH + CS * j], mb = colp[2 * PITCH + CS * j];
#pragma unroll
          for (int i = 0; i < BR; i++) {
            Kk[i][j] = __builtin_fma(ka[i], kb, Kk[i][j]);
            const double w = (qa[i] * qb) * r;
            const double mm = ma[i] * mb;
            const double tt = __builtin_fma(-mm, r, Kk[i][j]);
            Pc[i][j] = __builtin_fma(w, tt, Pc[i][j]);
            if constexpr (RAW) Pr[i][j] = __builtin_fma(w, Kk[i][j], Pr[i][j]);
          }
          // (a scheduling fence per column: 192 accumulator registers leave room for the operands of one column at a time)
          asm volatile("" ::: "memory");
        }
      }
    }
    if (more) causal_store<DT>(lds + (cur ^ 1) * STAGE + role * PITCH, tid, regs);
    __syncthreads();
  }

  if (active) {
    const int64_t slot = (int64_t)blockIdx.x * a.hd * a.hd;
#pragma unroll
    for (int i = 0; i < BR; i++)
#pragma unroll
      for (int j = 0; j < BC; j++) {
        const int r = ra + i, c = cb + CS * j;
        if (r < a.hd && c < a.hd) {
          a.part[slot + (int64_t)r * a.hd + c] = Pc[i][j];
          if constexpr (RAW) a.part_raw[slot + (int64_t)r * a.hd + c] = Pr[i][j];
        }
      }
  }
}

// pair[h][e] = (..((pair[h][e] + part[0][h][e]) + part[1][h][e]) .. + part[B-1][h][e]): ascending b, one rounding per sequence
// (qk_pair.hip's fold)
__global__ __launch_bounds__(256) void qk_causal_fold_kernel(const double* part, const double* part_raw, int64_t B, int64_t n,
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

template <int DT>
void causal_launch(const CausalArgs& a, dim3 grid, hipStream_t st) {
  if (a.part_raw) hipLaunchKernelGGL((qk_causal_kernel<DT, true>), grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL((qk_causal_kernel<DT, false>), grid, dim3(512), 0, st, a);
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_qk_causal_ws_bytes(int64_t B, int n_heads, int hd, int want_raw) {
  if (B <= 0 || n_heads <= 0 || hd <= 0) return 0;
  return (size_t)B * (size_t)n_heads * (size_t)hd * (size_t)hd * sizeof(double) * (want_raw ? 2 : 1);
}

extern "C" int mdg_qk_causal_accum(const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T,
                                   int n_heads, int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes,
                                   void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16 || dtype == MDG_F32, "mdg_qk_causal_accum: dtype %d (bf16, f16 or f32)", dtype);
  MDG_CHECK_ARG(hd >= 1 && hd <= MAX_HD, "mdg_qk_causal_accum: head_dim=%d must be >= 1 and <= %d", hd, MAX_HD);
  MDG_CHECK_ARG(n_heads > 0 && n_kv > 0 && n_heads % n_kv == 0, "mdg_qk_causal_accum: n_heads=%d must be a positive multiple of n_kv=%d",
                n_heads, n_kv);
  MDG_CHECK_ARG(B >= 0 && T >= 0, "mdg_qk_causal_accum: negative extent (B=%lld T=%lld)", (long long)B, (long long)T);
  const int64_t wq = (int64_t)n_heads * hd, wk = (int64_t)n_kv * hd;
  MDG_CHECK_ARG(ld_q >= wq, "mdg_qk_causal_accum: ld_q=%lld < n_heads*head_dim=%lld", (long long)ld_q, (long long)wq);
  MDG_CHECK_ARG(ld_k >= wk, "mdg_qk_causal_accum: ld_k=%lld < n_kv*head_dim=%lld", (long long)ld_k, (long long)wk);
  if (B == 0 || T == 0) return MDG_OK;
  MDG_CHECK_ARG(B <= 0x7fffffff / (int64_t)n_heads && ceil_div((int64_t)n_heads * hd * hd, 256) <= 0x7fffffff,
                "mdg_qk_causal_accum: B*n_heads = %lld x %d exceeds one launch", (long long)B, n_heads);
  MDG_CHECK_ARG(q && k && pair && ws, "mdg_qk_causal_accum: null pointer");
  const size_t need = mdg_qk_causal_ws_bytes(B, n_heads, hd, pair_raw != nullptr);
  MDG_CHECK_ARG(ws_bytes >= need, "mdg_qk_causal_accum: workspace %zu < required %zu", ws_bytes, need);
  MDG_CHECK_ARG((uintptr_t)ws % 8 == 0, "mdg_qk_causal_accum: workspace is not 8-byte aligned");

  const int64_t es = (int64_t)dtype_size(dtype);
  const int64_t n = (int64_t)n_heads * hd * hd;
  CausalArgs a;
  a.q = q; a.k = k; a.ld_q = ld_q; a.ld_k = ld_k; a.T = T;
  a.n_heads = n_heads; a.group = n_heads / n_kv; a.hd = hd;
  // 16-byte loads: the base, every row and every head start must be 16-byte aligned
  a.vec_q = (uintptr_t)q % 16 == 0 && (ld_q * es) % 16 == 0 && (hd * es) % 16 == 0;
  a.vec_k = (uintptr_t)k % 16 == 0 && (ld_k * es) % 16 == 0 && (hd * es) % 16 == 0;
  a.part = (double*)ws;
  a.part_raw = pair_raw ? (double*)ws + B * n : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * n_heads));
  if (dtype == MDG_BF16) causal_launch<MDG_BF16>(a, grid, st);
  else if (dtype == MDG_F16) causal_launch<MDG_F16>(a, grid, st);
  else causal_launch<MDG_F32>(a, grid, st);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(qk_causal_fold_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, a.part, a.part_raw, B, n, pair, pair_raw);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
