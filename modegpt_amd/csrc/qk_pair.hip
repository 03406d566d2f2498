// Within-sequence, shift-invariant Q/K statistic: pair[h] += sum over the sequences b of a calibration batch of
//   G^q_{b,h} (.) (G^k_{b,kv} - m m^T / T),   G^q = Q'^T Q',  G^k = K'^T K',  m = K'^T 1,  kv = h / (n_heads / n_kv),
// on the post-RoPE rows mdg_rope_rows writes (DESIGN.md "The within-sequence Q/K statistic").  1^T pair[h][D,D] 1 is the sum,
// over the queries i of every sequence, of the variance over that sequence's keys j of the logit change q'_iD . k'_jD: the part
// of dropping the columns D that softmax can see.  pair_raw is the same without the centring (the mean square).
//
// Launch shape: one 512-thread workgroup per (sequence b, query head h): waves 0-3 ("role 0") hold G^q of the head, waves 4-7
// ("role 1") hold G^k of the kv head serving it, each role a 2x2 arrangement of 64x64 wave tiles exactly like cov.hip's
// diagonal tile -- one 128x128 fp64 accumulator tile (128 registers per lane) per wave, two waves per SIMD, which is what the
// 512-entry register file holds.  (Both Grams in ONE wave, 256 accumulator registers, leaves the compiler moving accumulators
// between the two halves of the file every stage.)  A role streams the T tokens of its own head through LDS in 16-token
// stages, converted to fp64 once while staging, and multiplies the panel with itself on v_mfma_f64_16x16x4_f64.  G^k is
// recomputed by every query head of a group: the workgroups then share nothing, and a non-finite element stays in the heads it
// belongs to.  The key column sums m are taken from the staged panel by role 1 (thread t: column t & 127, token rows
// 8 (t >> 7) .. + 8 of the stage, in ascending order).  After the token loop role 1 hands S = G^k - m m^T / T (then G^k) to
// role 0 through the LDS the panels no longer need, lane to lane -- wave w and wave w + 4 hold the same entries in the same
// registers -- and role 0 multiplies in the accumulator layout and writes the workspace slot of (b, h).  qk_seq_fold_kernel
// then adds the slots onto pair in ascending b, ONE ADDITION PER SEQUENCE onto the running value, so a call over B sequences
// gives the bits of B calls over one sequence each.  No atomics, every sum in a fixed order.
//
// Symmetry to the bit: entry (a, b) and entry (b, a) of a Gram are the same products accumulated in the same token order by
// the same instruction, m_a m_b and the two further products commute, so both triangles come out equal without a mirror pass.
//
// The staging, the fold and the host half of the entry point are qk_seq.hpp's, shared with qk_causal.hip; the tile core (Acc,
// mma_steps, acc_row / acc_col) is common.hpp's.
#include "qk_seq.hpp"
#pragma STDC FP_CONTRACT OFF

namespace mdg {
namespace {

template <int DT>
__global__ __launch_bounds__(512) void qk_pair_kernel(SeqArgs a) {
  typedef Stage<DT> S;
  __shared__ double lds[4 * PANEL];  // Q[2], K[2]; after the token loop: the exchange buffer
  __shared__ double msum[2 * TILE];
  const int role = threadIdx.x >> 8;  // wave-uniform: 0 = query Gram, 1 = key Gram
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int b = blockIdx.x / a.n_heads, h = blockIdx.x % a.n_heads, kv = h / a.group;
  const size_t es = sizeof(typename S::T);
  const int64_t ld = role ? a.ld_k : a.ld_q;
  const int vec_ok = role ? a.vec_k : a.vec_q;
  const char* base = role ? (const char*)a.k + ((int64_t)b * a.T * a.ld_k + (int64_t)kv * a.hd) * es
                          : (const char*)a.q + ((int64_t)b * a.T * a.ld_q + (int64_t)h * a.hd) * es;
  double* panels = lds + 2 * role * PANEL;
  const int64_t n_stage = (a.T + BK - 1) / BK;

  Acc acc;
  acc_zero(acc);
  double m = 0.;  // role 1: this thread's share of column (tid & 127)'s key sum
  const int mcol = tid & (TILE - 1), mrow = (tid >> 7) * (BK / 2);

  typename S::Chunk regs[S::CPT];
  seq_load<DT>(base, ld, 0, a.T, a.hd, vec_ok, tid, regs);
  seq_store<DT, PITCH>(panels, tid, regs);
  __syncthreads();
  for (int64_t s = 0; s < n_stage; s++) {
    const int cur = (int)(s & 1);
    const bool more = s + 1 < n_stage;
    // the next stage's global loads fly while this one is multiplied
    if (more) seq_load<DT>(base, ld, (s + 1) * BK, a.T, a.hd, vec_ok, tid, regs);
    const double* P = panels + cur * PANEL;
    mma_stage(P, P, wr, wc, lane, acc);
    if (role) {
#pragma unroll
      for (int r = 0; r < BK / 2; r++) m += P[(mrow + r) * PITCH + mcol];
    }
    if (more) seq_store<DT, PITCH>(panels + (cur ^ 1) * PANEL, tid, regs);
    __syncthreads();
  }
  if (role) msum[tid] = m;
  __syncthreads();

  // Epilogue.  Element (sa, sb, reg) of a lane is entry (r, c) of the head's matrices, in both roles.  The exchange buffer
  // holds half a tile per pass, xch[wave][32 values][lane]: passes 0, 1 carry S (rows sa 0-1, then 2-3), passes 2, 3 carry G^k.
  const double Td = (double)a.T;
  const int64_t slot = (int64_t)blockIdx.x * a.hd * a.hd;
  double* xch = lds + wave * (32 * 64) + lane;
  double mc[4] = {0., 0., 0., 0.};
  if (role) {
#pragma unroll
    for (int sb = 0; sb < 4; sb++) {
      const int c = acc_col(wc, lane, sb);
      mc[sb] = msum[c] + msum[TILE + c];
    }
  }
  const int n_pass = a.part_raw ? 4 : 2;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    if (p >= n_pass) break;  // uniform over the workgroup
    double* out = p < 2 ? a.part : a.part_raw;
#pragma unroll
    for (int s2 = 0; s2 < 2; s2++) {
      const int sa = (p & 1) * 2 + s2;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int r = acc_row(wr, lane, sa, reg);
        if (role) {
          const double mr = p < 2 ? msum[r] + msum[TILE + r] : 0.;
#pragma unroll
          for (int sb = 0; sb < 4; sb++) {
            const double kk = acc.v[sa][sb][reg];
            xch[((s2 * 4 + reg) * 4 + sb) * 64] = p < 2 ? kk - (mr * mc[sb]) / Td : kk;
          }
        }
      }
    }
    __syncthreads();
    if (!role) {
#pragma unroll
      for (int s2 = 0; s2 < 2; s2++) {
        const int sa = (p & 1) * 2 + s2;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const int r = acc_row(wr, lane, sa, reg);
#pragma unroll
          for (int sb = 0; sb < 4; sb++) {
            const int c = acc_col(wc, lane, sb);
            const double v = acc.v[sa][sb][reg] * xch[((s2 * 4 + reg) * 4 + sb) * 64];
            if (r < a.hd && c < a.hd) out[slot + (int64_t)r * a.hd + c] = v;
          }
        }
      }
    }
    __syncthreads();
  }
}

void pair_launch(int dtype, const SeqArgs& a, dim3 grid, hipStream_t st) {
  if (dtype == MDG_BF16) hipLaunchKernelGGL(qk_pair_kernel<MDG_BF16>, grid, dim3(512), 0, st, a);
  else if (dtype == MDG_F16) hipLaunchKernelGGL(qk_pair_kernel<MDG_F16>, grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL(qk_pair_kernel<MDG_F32>, grid, dim3(512), 0, st, a);
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_qk_pair_ws_bytes(int64_t B, int n_heads, int hd, int want_raw) { return seq_ws_bytes(B, n_heads, hd, want_raw); }

extern "C" int mdg_qk_pair_accum(const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T,
                                 int n_heads, int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes,
                                 void* stream) {
  return seq_accum("mdg_qk_pair_accum", q, ld_q, k, ld_k, dtype, B, T, n_heads, n_kv, hd, pair, pair_raw, ws, ws_bytes, stream, pair_launch);
}
