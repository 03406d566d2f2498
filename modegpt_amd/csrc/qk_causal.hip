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
// stays in the heads it belongs to.  Each workgroup writes the workspace slot of (b, h); qk_seq_fold_kernel then adds the
// slots onto pair in ascending b, ONE ADDITION PER SEQUENCE onto the running value, so a call over B sequences gives the bits of
// B calls over one sequence each.  No atomics, every sum in a fixed order.
//
// Symmetry to the bit: every operation above is symmetric in (a, b) -- the products commute and m, r, q, k are the same LDS
// values for both entries -- and nothing is contracted or reassociated (FP_CONTRACT OFF, explicit fma), so entry (a, b) and
// entry (b, a) come out equal without a mirror pass.
//
// The staging, the fold and the host half of the entry point are qk_seq.hpp's, shared with qk_pair.hip.
#include "qk_seq.hpp"
#pragma STDC FP_CONTRACT OFF

namespace mdg {
namespace {

constexpr int BR = 4, BC = 8;  // a thread's block of entries: BR rows x BC columns; (TILE / BR) * (TILE / BC) = 512 threads
constexpr int CS = TILE / BC;       // the stride between a thread's BC columns
constexpr int ROW = 3 * PITCH;   // fp64 elements of one token's LDS row: q, k and the key prefix sums m
constexpr int STAGE = BK * ROW;

template <int DT, bool RAW>
__global__ __launch_bounds__(512) void qk_causal_kernel(SeqArgs a) {
  typedef Stage<DT> S;
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
  seq_load<DT>(base, ld, 0, a.T, a.hd, vec_ok, tid, regs);
  seq_store<DT, ROW>(lds + role * PITCH, tid, regs);
  __syncthreads();
  for (int64_t s = 0; s < n_stage; s++) {
    const int cur = (int)(s & 1);
    const bool more = s + 1 < n_stage;
    double* stage = lds + cur * STAGE;
    // the next stage's global loads fly while this one is worked through
    if (more) seq_load<DT>(base, ld, (s + 1) * BK, a.T, a.hd, vec_ok, tid, regs);
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
    if (more) seq_store<DT, ROW>(lds + (cur ^ 1) * STAGE + role * PITCH, tid, regs);
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

template <int DT>
void causal_launch(const SeqArgs& a, dim3 grid, hipStream_t st) {
  if (a.part_raw) hipLaunchKernelGGL((qk_causal_kernel<DT, true>), grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL((qk_causal_kernel<DT, false>), grid, dim3(512), 0, st, a);
}

void causal_dispatch(int dtype, const SeqArgs& a, dim3 grid, hipStream_t st) {
  if (dtype == MDG_BF16) causal_launch<MDG_BF16>(a, grid, st);
  else if (dtype == MDG_F16) causal_launch<MDG_F16>(a, grid, st);
  else causal_launch<MDG_F32>(a, grid, st);
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_qk_causal_ws_bytes(int64_t B, int n_heads, int hd, int want_raw) { return seq_ws_bytes(B, n_heads, hd, want_raw); }

extern "C" int mdg_qk_causal_accum(const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T,
                                   int n_heads, int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes,
                                   void* stream) {
  return seq_accum("mdg_qk_causal_accum", q, ld_q, k, ld_k, dtype, B, T, n_heads, n_kv, hd, pair, pair_raw, ws, ws_bytes, stream,
                   causal_dispatch);
}
