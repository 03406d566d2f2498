// The error-versus-rank curve of the Nystrom refit of down_proj (compress_mlp.py:52-62), for EVERY rank from one factorisation:
//   M = C + eps I,  pi = the columns in ridge-score order,  M[pi, pi] = L L^T,  Z = W_d[:, pi] L,  c_j = ||Z[:, j]||^2,
//   curve[r] = sum_{j >= r} c_j = tr(W_d (M - M[:, S] M_SS^-1 M[S, :]) W_d^T),  S = pi[:r]      ("The error-versus-rank curve")
// -- the trailing block L[r:, r:] of the factor IS the Cholesky factor of the Schur complement of M_SS, for every r at once.
// clamp / check the order -> gather M[pi, pi] (from the lower triangle of C) -> blocked Cholesky -> gather the columns of W_d -> triangular GEMM ->
// column norms over the d rows -> suffix sum.  No atomics; every sum in a fixed order: bit-identical from run to run.
//
// The product Z = W_pi L runs with MDG_GEMM_B_LOWER_TRI, which skips k < j0 per 128-wide tile column (d n^2 flops instead of
// 2 d n^2: 0.84 instead of 1.68 TFLOP at n = 14336, d = 4096) but READS the strict upper part of L's 128 x 128 diagonal blocks
// and needs zeros there -- potrf_lower may leave anything in those entries (it stores diagonal tiles whole), and the gathered
// copy never wrote them.  So the strict upper part of the diagonal blocks is CLEARED between the factorisation and the product
// (n / 128 blocks of 8128 entries: 0.9 MB of stores at n = 14336) rather than paying for the full GEMM.
//
// A repeated index makes M[pi, pi] exactly singular, but rounding can leave the second occurrence a pivot of order +2^-53 c_jj and
// let the factorisation through.  The order check therefore writes a NaN onto the diagonal entry of every position whose index
// occurs more than once, and the factorisation reports the first of them as the failed pivot (a NaN pivot counts).
#include "common.hpp"

namespace mdg {
int gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i, int64_t sa_k,
             const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k, int64_t sb_j, double beta, void* C,
             int c_dtype, int64_t ldc, int64_t batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int flags,
             hipStream_t st);
int potrf_lower(double* A, int64_t n, int64_t lda, double* inv_diag, hipStream_t st);

constexpr int RC_NB = 128;   // the factorisation's diagonal block (chol.hip NB)

// oc[j] = order[j] clamped into [0, n) (memory safety only, as mdg_rope_gather clamps its mask); seen[oc[j]] = j.  Where an index
// repeats, which of its positions the plain stores leave in `seen` is not defined -- order_check_kernel does not depend on it.
__global__ __launch_bounds__(256) void order_clamp_kernel(const int64_t* order, int64_t n, int64_t* oc, int* seen) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int64_t v = order[j];
  v = v < 0 ? 0 : (v >= n ? n - 1 : v);
  oc[j] = v;
  seen[v] = (int)j;
}

// Mg lower triangle (incl. diagonal) = C[oc, oc] + eps I.  chol.hip's copy_lower reads C[oc[i], oc[j]] for j <= i, which with an
// UNSORTED gather lies above the diagonal of C half of the time; here entry (a, b) is always taken from the lower triangle,
// C[max(a, b), min(a, b)], so that a statistic whose upper triangle was never mirrored gives the same curve.  The ridge is added as
// copy_lower adds it: one fp64 addition per diagonal entry.
// Rows are folded in pairs so that every workgroup has the same work: pair y holds row y (y + 1 entries) and row n - 1 - y (n - y
// entries), n + 1 entries together; the middle row of an odd n stands alone.  blockIdx.y strides over the pairs (any n fits the grid).
__global__ __launch_bounds__(256) void gather_lower_kernel(const double* C, int64_t ldc, const int64_t* oc, double* Mg, int64_t ldm,
                                                           int64_t n, double eps) {
  const int64_t pairs = (n + 1) / 2;
  for (int64_t y = blockIdx.y; y < pairs; y += gridDim.y) {
    const int64_t i0 = y, i1 = n - 1 - y;
    const int64_t len = i1 > i0 ? n + 1 : i0 + 1;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (int64_t)gridDim.x * 256) {
      const int64_t i = e <= i0 ? i0 : i1, j = e <= i0 ? e : e - i0 - 1;
      const int64_t si = oc[i], sj = oc[j];
      double v = si >= sj ? C[si * ldc + sj] : C[sj * ldc + si];
      if (j == i) v += eps;
      Mg[i * ldm + j] = v;
    }
  }
}

// A position that does not find itself in `seen` shares its index with the position that is there: both get a NaN pivot.  Every
// position of a repeated index is either the one in `seen` (poisoned by the others) or not (poisons itself): the result is the
// same whichever store won.
__global__ __launch_bounds__(256) void order_check_kernel(const int64_t* oc, const int* seen, int64_t n, double* Mg, int64_t ldm) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t w = seen[oc[j]];
  if (w != j) {
    const double bad = __longlong_as_double(0x7ff8000000000000ll);
    Mg[j * ldm + j] = bad;
    Mg[w * ldm + w] = bad;
  }
}

// zeros strictly above the diagonal inside the 128 x 128 diagonal blocks (what MDG_GEMM_B_LOWER_TRI reads there)
__global__ __launch_bounds__(256) void clear_diag_upper_kernel(double* L, int64_t ldl, int64_t n) {
  const int64_t b0 = (int64_t)blockIdx.x * RC_NB;
  for (int e = threadIdx.x; e < RC_NB * RC_NB; e += 256) {
    const int64_t i = b0 + e / RC_NB, j = b0 + e % RC_NB;
    if (j > i && j < n) L[i * ldl + j] = 0.;
  }
}

// out[i, j] = fp64(W[i, oc[j]]): the columns of W_d in the order of the factorisation (the existing gathers take rows)
template <int DT>
__global__ __launch_bounds__(256) void gather_cols_kernel(const void* W, int64_t ldw, const int64_t* oc, int64_t d, int64_t n,
                                                          double* out, int64_t ldo) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int64_t src = oc[j];
  for (int64_t i = blockIdx.y; i < d; i += gridDim.y) out[i * ldo + j] = load_f64<DT>(W, i * ldw + src);
}

// c[j] = sum_i Z[i, j]^2: one workgroup per 64 columns, wave w takes the rows w, w + 4, ... in ascending order, the four partial
// sums are added in the order 0, 1, 2, 3.
__global__ __launch_bounds__(256) void colnorm2_kernel(const double* Z, int64_t ldz, int64_t d, int64_t n, double* c) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;
  double s = 0.;
  if (j < n)
    for (int64_t i = wave; i < d; i += 4) {
      const double v = Z[i * ldz + j];
      s += v * v;
    }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && j < n) c[j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// curve[r] = sum_{j >= r} c[j], curve[n] = +0, as a two-level sum in one workgroup.  Thread t owns the contiguous chunk
// [t m, (t + 1) m) and forms its LOCAL suffix sums from the chunk's last entry downwards; thread 0 then adds the chunk totals from the
// last chunk downwards, off[t] = the sum of the chunks behind chunk t; entry j of chunk t is fl(local suffix of j + off[t]).  So the
// far tail is summed on its own, tail first, before it meets anything of chunk t, while inside chunk t the entries between j and the
// chunk's end are added to one another before that tail joins them.  All terms are non-negative, so whatever the order every
// entry is within (m + 256) 2^-53 of its exact value relative to ITSELF, not to curve[0]: a small tail is not absorbed by the head.
// Non-increasing exactly: inside a chunk the local sums are (rounded additions of non-negative terms are monotone) and adding the
// same off[t] keeps the order; across a chunk edge because off[t] = fl(total[t + 1] + off[t + 1]) is bit for bit the first entry of
// chunk t + 1, and the last entry of chunk t is fl(c + off[t]) >= off[t].
constexpr int SCAN_T = 256;
__global__ __launch_bounds__(SCAN_T) void suffix_sum_kernel(const double* c, int64_t n, double* curve) {
  __shared__ double total[SCAN_T], off[SCAN_T];
  const int t = threadIdx.x;
  const int64_t m = (n + SCAN_T - 1) / SCAN_T;
  const int64_t lo = (int64_t)t * m, hi = lo + m < n ? lo + m : n;
  double s = 0.;
  for (int64_t j = hi - 1; j >= lo; j--) {
    s += c[j];
    curve[j] = s;
  }
  total[t] = s;     // (+0 for a chunk behind the end)
  __syncthreads();
  if (t == 0) {
    double a = 0.;
    for (int u = SCAN_T - 1; u >= 0; u--) {
      off[u] = a;
      a += total[u];
    }
    curve[n] = 0.;
  }
  __syncthreads();
  const double o = off[t];
  for (int64_t j = lo; j < hi; j++) curve[j] += o;   // (the thread's own stores of the first pass)
}

static int64_t rc_pitch(int64_t n) { return (n + 15) / 16 * 16; }   // rows of L, W_pi and Z on 16-byte boundaries (mlp.hip ckk_pitch)

// L [n][np], inv_diag, W_pi [d][np], Z [d][np], c [np] (doubles); the clamped order [n] (int64); seen [np] (int)
struct RankCurveWs {
  double *L, *inv, *Wp, *Z, *c;
  int64_t* oc;
  int* seen;
  size_t bytes;
};
static RankCurveWs rank_curve_layout(void* ws, int64_t n, int64_t d) {
  const size_t np = (size_t)rc_pitch(n);
  Carve c(ws);
  RankCurveWs w;
  w.L = c.take<double>((size_t)n * np);
  w.inv = c.take<double>(mdg_potrf_inv_diag_elems(n));
  w.Wp = c.take<double>((size_t)d * np);
  w.Z = c.take<double>((size_t)d * np);
  w.c = c.take<double>(np);
  w.oc = c.take<int64_t>((size_t)n);
  w.seen = c.take<int>(np);
  w.bytes = c.off;
  return w;
}

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_nystrom_rank_curve_ws_bytes(int64_t n, int64_t d) {
  if (n <= 0 || d <= 0) return 0;
  return rank_curve_layout(nullptr, n, d).bytes;
}

extern "C" int mdg_nystrom_rank_curve(const double* C, int64_t n, int64_t ldc, const int64_t* order, const void* Wd, int64_t d,
                                      int64_t ld_wd, int w_dtype, double eps, double* curve, void* ws, size_t ws_bytes,
                                      void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(C && order && Wd && curve, "mdg_nystrom_rank_curve: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_nystrom_rank_curve: W_d must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n > 0 && d > 0 && ldc >= n && ld_wd >= n, "mdg_nystrom_rank_curve: bad sizes (n=%lld d=%lld ldc=%lld ld_wd=%lld)",
                (long long)n, (long long)d, (long long)ldc, (long long)ld_wd);
  MDG_CHECK_ARG(n <= INT32_MAX, "mdg_nystrom_rank_curve: n = %lld is beyond the limit of 2^31 - 1 columns", (long long)n);
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_nystrom_rank_curve_ws_bytes(n, d), "mdg_nystrom_rank_curve: workspace %zu < required %zu",
                ws_bytes, mdg_nystrom_rank_curve_ws_bytes(n, d));
  hipStream_t st = (hipStream_t)stream;
  const int64_t np = rc_pitch(n);
  const RankCurveWs w = rank_curve_layout(ws, n, d);
  double *L = w.L, *inv = w.inv, *Wp = w.Wp, *Z = w.Z, *c = w.c;
  int64_t* oc = w.oc;
  int* seen = w.seen;
  const unsigned gn = (unsigned)ceil_div(n, 256);
  hipLaunchKernelGGL(order_clamp_kernel, dim3(gn), dim3(256), 0, st, order, n, oc, seen);
  MDG_LAUNCH_CHECK();
  // M[pi, pi] = C[pi, pi] + eps I  (lower; the ridge added in fp64, one rounding per diagonal entry)   compress_mlp.py:52,56
  {
    const int64_t pairs = (n + 1) / 2, gx = ceil_div(n + 1, 256);
    hipLaunchKernelGGL(gather_lower_kernel, dim3((unsigned)(gx < 64 ? gx : 64), (unsigned)(pairs < 32768 ? pairs : 32768)), dim3(256), 0, st, C,
                       ldc, oc, L, np, n, eps);
  }
  hipLaunchKernelGGL(order_check_kernel, dim3(gn), dim3(256), 0, st, oc, seen, n, L, np);
  MDG_LAUNCH_CHECK();
  MDG_TRY(potrf_lower(L, n, np, inv, st));      // (the call's one host round trip, or none in deferred-status mode)
  hipLaunchKernelGGL(clear_diag_upper_kernel, dim3((unsigned)ceil_div(n, RC_NB)), dim3(256), 0, st, L, np, n);
  const dim3 gg(gn, (unsigned)(d < 1024 ? d : 1024));
  if (w_dtype == MDG_BF16) hipLaunchKernelGGL(gather_cols_kernel<MDG_BF16>, gg, dim3(256), 0, st, Wd, ld_wd, oc, d, n, Wp, np);
  else hipLaunchKernelGGL(gather_cols_kernel<MDG_F64>, gg, dim3(256), 0, st, Wd, ld_wd, oc, d, n, Wp, np);
  MDG_LAUNCH_CHECK();
  // Z = W_pi L, L lower triangular
  MDG_TRY(gemm_f64(d, n, n, 1.0, Wp, MDG_F64, np, 1, nullptr, L, MDG_F64, np, 1, 0.0, Z, MDG_F64, np, 1, 0, 0, 0,
                   MDG_GEMM_B_LOWER_TRI, st));
  hipLaunchKernelGGL(colnorm2_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(256), 0, st, Z, np, d, n, c);
  hipLaunchKernelGGL(suffix_sum_kernel, dim3(1), dim3(SCAN_T), 0, st, c, n, curve);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
