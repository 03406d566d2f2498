// What the Q/K pair selection costs the attention logits on the calibration statistic, per query head and at every rank
// (compress_qk.py:355-367, 403-419, 452-464 score a unit from four diagonal entries of sigma_q / sigma_k and report nothing about what
// the selection loses).  Drop the column set D of q and k of one query head: the logit of token pair (i, j) changes by
// sum_{c in D} q_ic k_jc, and its mean square over all token pairs of the calibration set is
//   E(D) = <C_q[D, D], C_k[D, D]>_F = sum_{a, b in D} P[a][b] ,   P = C_q (.) C_k  (entry-wise; PSD by the Schur product theorem)
// -- the CR objective || C_q^1/2 (I - S S^T) C_k^1/2 ||_F^2, of which the reference's scores keep the diagonal.  E is NOT monotone in D.
//
// mdg_qk_rank_curve: one workgroup of 256 threads per kv head, everything of a head in LDS, nothing but plain loads and stores.
//   units           u < ns: the column pair {u, u + hd/2} (RoPE modes, ns = hd/2) or the column u (OPT, ns = hd)
//   T_h (LDS)       the head's unit-block sums, symmetrised and packed: T_h[u][v] = U_h[u][v] + U_h[v][u] for v < u, U_h[u][u] on the
//                   diagonal, U_h[u][v] = sum_{a in cols(u), b in cols(v)} P_h[a][b].  ns (ns + 1) / 2 doubles: 66 KB at ns = 128.  Both
//                   triangles of sigma are READ (the statistic need not be symmetric to the bit), one thread per packed entry.
//   B (LDS)         sum_h T_h in ascending h (only with the greedy outputs): the same thread owns the same entry for every head.
//   curve_h         thread i: inc[i] = sum_{j >= i} T_h[order[i]][order[j]] in ascending j; thread 0: the suffix sums of inc from the
//                   tail.  Every P entry enters a value once, through one product and at most hd^2 - 1 additions.
//   curve           thread 0 adds each head's value to the group's as it writes it: ((c_0 + c_1) + c_2) + ... to the bit.
//   greedy          ONE wave, two units per lane, no barrier inside the ns steps: delta[u] = B[u][u] + sum_{v in D} B[u][v] is kept
//                   in registers, the minimum goes round by a 6-step butterfly, the dropped unit's row of B is added.  The greedy curve
//                   is then evaluated from B along greedy_order exactly as curve_h is from T_h -- not from the running deltas.
// Two packed triangles and 4.6 KB of small arrays: 136.7 KB at ns = 128, within the 160 KB of a CU (dynamic LDS, the > 64 KB attribute
// set on the launch), one workgroup per CU.  No atomics, every sum in a fixed order: bit-identical from run to run.
//
// Non-finite input stays where its entry goes: an entry of one query head's sigma_q in that head's T_h, B and the abs-sum, an entry
// of one kv head's sigma_k in every T_h of that group; other kv heads are other workgroups.  `order` is clamped to 0 .. ns-1 when it
// is read; greedy_order is built from the lanes' own unit numbers, so it is a permutation whatever the values are.
#include "common.hpp"

namespace mdg {

struct QkCurveArgs {
  const double* cov_q;
  const double* cov_k;
  const int64_t* order;
  double* curve_h;
  double* curve;
  double* terms;
  double* scale;
  double* greedy_curve;
  int64_t* greedy_order;
  double ridge_q, ridge_k, terms_ridge_q, terms_ridge_k;
  int n_heads, n_kv, hd, mode;
};

constexpr int QKC_THREADS = 256;
constexpr int QKC_SMALL = 128 + 136 + QKC_THREADS + 64 + 64;     // inc, gsum, red, ord (int), gord (int): doubles of LDS ahead of T

__device__ __forceinline__ int qkc_tri(int u, int v) { return u >= v ? u * (u + 1) / 2 + v : v * (v + 1) / 2 + u; }

// P_h[a][b] = (C_q + rho_q I)[a][b] (C_k + rho_k I)[a][b]
__device__ __forceinline__ double qkc_p(const double* Cq, const double* Ck, int hd, int a, int b, double rq, double rk) {
  const double q = Cq[a * hd + b], k = Ck[a * hd + b];
  return a == b ? (q + rq) * (k + rk) : q * k;
}

// candidate (d, u) goes before (e, v): u < 0 marks "none"; otherwise a < b, ties to the lower unit, NaN last (before_asc of select.hip:8-12)
__device__ __forceinline__ bool qkc_before(double d, int u, double e, int v) {
  if (u < 0) return false;
  if (v < 0) return true;
  const bool dn = d != d, en = e != e;
  if (dn || en) return (!dn && en) || (dn && en && u < v);
  return d < e || (d == e && u < v);
}

// inc[i] = sum_{j >= i} M[ord[i]][ord[j]] (thread i, ascending j), then thread 0: out[m] = sum_{i >= m} inc[i] from the tail, out[ns] = +0.0;
// with gsum, the value is also added to gsum[m] (first: stored).  M must be complete (a barrier behind its last write); a barrier
// separates the two halves; NO barrier at the end (inc is next written behind the caller's next barrier).
template <class I>
__device__ __forceinline__ void qkc_curve_along(const double* M, const I* ord, int ns, double* inc, double* out, double* gsum, bool first) {
  const int tid = threadIdx.x;
  if (tid < ns) {
    const int u = (int)ord[tid];
    double s = M[qkc_tri(u, u)];
    for (int j = tid + 1; j < ns; j++) s += M[qkc_tri(u, (int)ord[j])];
    inc[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.;
    out[ns] = s;
    if (gsum) gsum[ns] = 0.;
    for (int i = ns - 1; i >= 0; i--) {
      s += inc[i];
      out[i] = s;
      if (gsum) gsum[i] = first ? s : gsum[i] + s;
    }
  }
}

__global__ __launch_bounds__(QKC_THREADS) void qk_rank_curve_kernel(QkCurveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double qkc_lds[];
  double* inc = qkc_lds;                    // [128]
  double* gsum = inc + 128;                 // [ns + 1]
  double* red = gsum + 136;                 // [256]
  int* ord = (int*)(red + QKC_THREADS);     // [128]
  int* gord = ord + 128;                    // [128]
  double* T = qkc_lds + QKC_SMALL;          // [nt]
  const int kv = blockIdx.x, tid = threadIdx.x;
  const int hd = a.hd, g = a.n_heads / a.n_kv;
  const bool opt = a.mode == MDG_QK_OPT;
  const int ns = opt ? hd : hd / 2, w = opt ? 1 : 2;
  const int nt = ns * (ns + 1) / 2;
  const bool greedy = a.greedy_order != nullptr;
  double* B = T + nt;                       // [nt], allocated with the greedy outputs only
  const double* Ck = a.cov_k + (int64_t)kv * hd * hd;

  if (tid < ns) {
    const int64_t o = a.order[(int64_t)kv * ns + tid];
    ord[tid] = (int)(o < 0 ? 0 : (o > ns - 1 ? ns - 1 : o));
  }
  double sabs = 0.;
  for (int q = 0; q < g; q++) {
    const int h = kv * g + q;
    const double* Cq = a.cov_q + (int64_t)h * hd * hd;
    // (T of the previous head is dead: its last readers passed the barrier inside qkc_curve_along)
    for (int p = tid; p < nt; p += QKC_THREADS) {
      int u = (int)((sqrtf(8.f * (float)p + 1.f) - 1.f) * 0.5f);
      while (u * (u + 1) / 2 > p) u--;
      while ((u + 1) * (u + 2) / 2 <= p) u++;
      const int v = p - u * (u + 1) / 2;    // v <= u
      double t = 0.;
      for (int ia = 0; ia < w; ia++)
        for (int ib = 0; ib < w; ib++) {
          const double x = qkc_p(Cq, Ck, hd, u + ia * ns, v + ib * ns, a.ridge_q, a.ridge_k);
          t += x;
          sabs += fabs(x);
        }
      if (u != v)
        for (int ia = 0; ia < w; ia++)
          for (int ib = 0; ib < w; ib++) {
            const double x = qkc_p(Cq, Ck, hd, v + ib * ns, u + ia * ns, a.ridge_q, a.ridge_k);
            t += x;
            sabs += fabs(x);
          }
      T[p] = t;
      if (greedy) B[p] = q == 0 ? t : B[p] + t;
    }
    __syncthreads();
    qkc_curve_along(T, ord, ns, inc, a.curve_h + (int64_t)h * (ns + 1), gsum, q == 0);
    __syncthreads();
  }

  // the abs-sum of everything the group's values were added from: a fixed tree
  red[tid] = sabs;
  __syncthreads();
  for (int o = QKC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0 && a.scale) a.scale[kv] = red[0];
  if (tid <= ns) a.curve[(int64_t)kv * (ns + 1) + tid] = gsum[tid];

  if (a.terms && tid < ns) {                // the diagonal share of unit order[tid], as select.hip:140-153 forms it
    const int j1 = ord[tid], j2 = j1 + hd / 2;
    double acc;
    if (opt) {
      const double* Cq = a.cov_q + (int64_t)kv * hd * hd;
      const double nq2 = fmax(Cq[j1 * hd + j1] + a.terms_ridge_q, 0.), nk2 = fmax(Ck[j1 * hd + j1] + a.terms_ridge_k, 0.);
      acc = nq2 * nk2;
    } else {
      const double nk1 = fmax(Ck[j1 * hd + j1] + a.terms_ridge_k, 0.), nk2 = fmax(Ck[j2 * hd + j2] + a.terms_ridge_k, 0.);
      acc = 0.;
      for (int q = 0; q < g; q++) {
        const double* Cq = a.cov_q + (int64_t)(kv * g + q) * hd * hd;
        const double nq1 = fmax(Cq[j1 * hd + j1] + a.terms_ridge_q, 0.), nq2 = fmax(Cq[j2 * hd + j2] + a.terms_ridge_q, 0.);
        acc += nq1 * nk1 + nq2 * nk2;
      }
    }
    a.terms[(int64_t)kv * ns + tid] = acc;
  }
  if (!greedy) return;                      // (uniform over the workgroup)

  // greedy: start from nothing dropped; drop the unit whose move into D raises the group's E least.  B is complete (the barriers above).
  if (tid < 64) {
    const int u0 = tid, u1 = tid + 64;
    bool alive0 = u0 < ns, alive1 = u1 < ns;
    double d0 = alive0 ? B[qkc_tri(u0, u0)] : 0., d1 = alive1 ? B[qkc_tri(u1, u1)] : 0.;
    for (int s = 0; s < ns; s++) {
      double bd = d0;
      int bu = alive0 ? u0 : -1;
      if (qkc_before(d1, alive1 ? u1 : -1, bd, bu)) { bd = d1; bu = u1; }
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int ou = __shfl_xor(bu, o, 64);
        if (qkc_before(od, ou, bd, bu)) { bd = od; bu = ou; }
      }
      // (every lane holds the same winner: the order is total)
      if (tid == 0) gord[ns - 1 - s] = bu;
      if (bu == u0) alive0 = false;
      if (bu == u1) alive1 = false;
      if (alive0) d0 += B[qkc_tri(u0, bu)];
      if (alive1) d1 += B[qkc_tri(u1, bu)];
    }
  }
  __syncthreads();
  if (tid < ns) a.greedy_order[(int64_t)kv * ns + tid] = gord[tid];
  qkc_curve_along(B, gord, ns, inc, a.greedy_curve + (int64_t)kv * (ns + 1), (double*)nullptr, false);
}

}  // namespace mdg

using namespace mdg;

extern "C" int mdg_qk_rank_curve(const double* cov_q, const double* cov_k, int n_heads, int n_kv, int hd, double ridge_q, double ridge_k,
                                 int mode, const int64_t* order, double terms_ridge_q, double terms_ridge_k, double* curve_h,
                                 double* curve, double* terms, double* scale, double* greedy_curve, int64_t* greedy_order,
                                 void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(cov_q && cov_k && order && curve_h && curve, "mdg_qk_rank_curve: null pointer");
  MDG_CHECK_ARG((greedy_curve == nullptr) == (greedy_order == nullptr), "mdg_qk_rank_curve: greedy_curve and greedy_order go together");
  MDG_CHECK_ARG(n_kv > 0 && n_heads >= n_kv && n_heads % n_kv == 0, "mdg_qk_rank_curve: n_heads %d not a multiple of n_kv %d", n_heads,
                n_kv);
  MDG_CHECK_ARG(hd > 0 && hd <= 256, "mdg_qk_rank_curve: bad head_dim %d", hd);
  MDG_CHECK_ARG(mode >= MDG_QK_ROPE_GROUPED && mode <= MDG_QK_OPT, "mdg_qk_rank_curve: unknown mode %d", mode);
  if (mode != MDG_QK_OPT) {
    MDG_CHECK_ARG(hd % 2 == 0, "mdg_qk_rank_curve: RoPE modes need even head_dim");
    MDG_CHECK_ARG(hd / 2 <= 128, "mdg_qk_rank_curve: head_dim %d too large", hd);
  } else {
    MDG_CHECK_ARG(hd <= 128 && n_heads == n_kv, "mdg_qk_rank_curve: OPT mode needs head_dim <= 128 and n_heads == n_kv");
  }
  if (mode == MDG_QK_ROPE_MHA) MDG_CHECK_ARG(n_heads == n_kv, "mdg_qk_rank_curve: ROPE_MHA needs n_heads == n_kv");
  QkCurveArgs a;
  a.cov_q = cov_q; a.cov_k = cov_k; a.order = order;
  a.curve_h = curve_h; a.curve = curve; a.terms = terms; a.scale = scale;
  a.greedy_curve = greedy_curve; a.greedy_order = greedy_order;
  a.ridge_q = ridge_q; a.ridge_k = ridge_k; a.terms_ridge_q = terms_ridge_q; a.terms_ridge_k = terms_ridge_k;
  a.n_heads = n_heads; a.n_kv = n_kv; a.hd = hd; a.mode = mode;
  const int ns = mode == MDG_QK_OPT ? hd : hd / 2;
  const size_t lds = ((size_t)QKC_SMALL + (size_t)(greedy_order ? 2 : 1) * (size_t)(ns * (ns + 1) / 2)) * sizeof(double);
  if (lds > 64 * 1024) MDG_HIP(hipFuncSetAttribute((const void*)qk_rank_curve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(qk_rank_curve_kernel, dim3(n_kv), dim3(QKC_THREADS), lds, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
