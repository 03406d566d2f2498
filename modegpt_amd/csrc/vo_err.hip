// What the stored V/O factors lose of the attention output on the calibration statistic, per head and output channel, and what the
// truncation costs at every rank (compress_vo.py:112-223 cuts the SVD at `rank` and reports nothing about either).  The objective
// the reference works on is the map x -> W_o,h W_v,g x per query head h of kv group g (no token mixing).  With
//   delta_{h,k} = W_o,h[k, :] W_v,g - o'_h[k, :] v'_g                                (a row of length d; never formed)
//   e[h][k] = delta C delta^T ,   dnorm2[h][k] = ||delta||^2 ,                       (q: the same with nothing subtracted)
// the stacked Gram does it in (hd + r)-sized pieces: V_g = [W_v,g ; -v'_g]  [(hd + r), d],  y_{h,k} = [W_o,h[k, :], o'_h[k, :]],
//   e[h][k] = y (V_g C V_g^T) y^T ,   dnorm2[h][k] = y (V_g V_g^T) y^T .
//
// mdg_vo_output_error:
//   T_g = V_g C            gemm_f64, batched over the kv heads (the rows of -v'_g with alpha = -1; bf16 operands read directly)
//   Gc_g = T_g V_g^T, Gn_g = V_g V_g^T     gemm_f64, batched; only the blocks on and below the block diagonal are computed
//   vo_quad_kernel         one workgroup = a 128-row block of output channels of one head x one 128-wide tile COLUMN J of one Gram:
//                          P = sum_{I >= J} y[:, I] G[I, J] on v_mfma_f64_16x16x4_f64 with the diagonal tile masked to its STRICT lower
//                          part while staging (the Gram's upper triangle is never loaded), y stitched from W_o,h and o'_h in the
//                          A-operand staging (both widened exactly); epilogue y_kj (2 P_kj + G_jj y_kj) summed along the tile's
//                          columns in a fixed tree.  P is never written.  grid = (row blocks, Gram x J, heads).
//                          Tile scheme, epilogue and reduction: quad_form.hpp.
//   quad_reduce_kernel     adds the (at most two) tile-column partials of a channel in ascending J.
// No atomics: two runs are bit-identical.  e is accurate relative to a[h][k] = (|y| |V_g|) |C| (|y| |V_g|)^T, not to itself.
//
// mdg_vo_rank_curve: from the eigen-decomposition (lambda_i, v_i) the last mdg_vo_compress left in its workspace,
//   grouped: c_i = max(lambda_i, 0) sum_{h in g} ||W_o,h v_i||^2 ,   MHA: c_i = max(lambda2_i, 0)   (the second spectrum)
//   curve[g][r] = sum_{i >= r} c_i , accumulated from the tail; curve[g][hd] = +0.0.
// ||W_o,h v_i||^2 as column norms of Z_h = W_o,h V_g (gemm_f64): every term of the norm is a square, so it is accurate to
// (hd + d) u relative to ITSELF -- the route v_i^T (W_o,h^T W_o,h) v_i would be accurate to d u ||W_o,h||^2 only, which says nothing
// about a direction W_o,h nearly annihilates.  Rows are summed in 256-row chunks, chunks, then heads, in ascending order.
//
// Non-finite input: a NaN in row k of one head's W_o or o' stays in row k of y, P and the sums -- e[h][k] alone; a NaN in one kv
// head's W_v or v' reaches that group's Grams, i.e. every channel of that group's heads, and no other group; a NaN in C reaches
// everything.  Out-of-range rows / columns are never loaded (selects, not multiplications by zero).
#include "common.hpp"
#include "quad_form.hpp"
#include "vo_ws.hpp"

namespace mdg {
int gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i, int64_t sa_k,
             const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k, int64_t sb_j, double beta, void* C,
             int c_dtype, int64_t ldc, int64_t batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int flags,
             hipStream_t st);

struct VoQuadArgs {
  const void* Wo;       // [d, n_heads * hd]
  int64_t ld_wo;
  const void* o_new;    // [d, n_heads * r]   (not read when r == 0)
  int64_t ld_o;
  const double* gram;   // [planes][n_kv][n][n]: plane 0 = V C V^T, plane 1 = V V^T; the lower triangles are read
  double* part;         // [planes][tiles_n][n_heads][d]
  int64_t d;
  int hd, r, n, group, n_heads, n_kv, tiles_n;
};

// y_{h,k}[col]: W_o,h for col < hd, o'_h behind it
template <int WDT, int NDT>
struct VoQuadRows {
  typedef int Idx;
  struct Col {};        // (nothing to look up per column)
  const VoQuadArgs g;   // (a copy: through a reference the kernel compiles to branches where this gives selects, a third more code)
  int h;
  __device__ __forceinline__ Col prepare(int) const { return {}; }
  __device__ __forceinline__ double at(int64_t row, int col, Col) const {
    return col < g.hd ? load_f64<WDT>(g.Wo, row * g.ld_wo + (int64_t)h * g.hd + col)
                      : load_f64<NDT>(g.o_new, row * g.ld_o + (int64_t)h * g.r + (col - g.hd));
  }
};

template <int WDT, int NDT>
__global__ __launch_bounds__(256, 2) void vo_quad_kernel(VoQuadArgs g) {
  __shared__ double lds[4 * PANEL];
  const int tid = threadIdx.x;
  const int bi = blockIdx.x, plane = blockIdx.y / g.tiles_n, bj = blockIdx.y % g.tiles_n, h = blockIdx.z;
  const int64_t i0 = (int64_t)bi * TILE;
  const double* G = g.gram + ((size_t)plane * g.n_kv + (size_t)(h / g.group)) * (size_t)g.n * g.n;
  double se, unused;
  quad_form_tile_column<false>(VoQuadRows<WDT, NDT>{g, h}, G, g.n, g.n, g.d, i0, bj * TILE, lds, se, unused);
  if (tid < TILE && i0 + tid < g.d)
    g.part[(((size_t)plane * g.tiles_n + bj) * g.n_heads + h) * (size_t)g.d + i0 + tid] = se;
}

struct VoErrWs {
  double *T, *gram, *part;
  size_t bytes;
};

static VoErrWs vo_err_layout(void* ws, int64_t d, int n_heads, int n_kv, int hd, int rank) {
  VoErrWs w;
  Carve c(ws);
  const size_t n = (size_t)hd + (size_t)rank;
  w.T = c.take<double>((size_t)n_kv * n * (size_t)d);                                            // V_g C
  w.gram = c.take<double>(2 * (size_t)n_kv * n * n);                                             // V_g C V_g^T, V_g V_g^T
  w.part = c.take<double>(2 * (size_t)ceil_div((int64_t)n, TILE) * (size_t)n_heads * (size_t)d);   // the tile-column partials of e and dnorm2
  w.bytes = c.off;
  return w;
}

// ---------------------------------------------------------------- the curve
constexpr int VO_CURVE_CHUNK = 256;

// pn[h][chunk][i] = sum over the chunk's rows k of Z[h][k][i]^2: two threads per column, each every other row, ascending
__global__ __launch_bounds__(256) void vo_colnorm_kernel(const double* Z, int64_t d, int hd, int n_chunk, double* pn) {
  __shared__ double half_[2][128];
  const int col = threadIdx.x & 127, half = threadIdx.x >> 7;
  const int chunk = blockIdx.x, h = blockIdx.y;
  const double* Zh = Z + (size_t)h * (size_t)d * hd;
  const int64_t k_lo = (int64_t)chunk * VO_CURVE_CHUNK;
  const int64_t k_hi = k_lo + VO_CURVE_CHUNK < d ? k_lo + VO_CURVE_CHUNK : d;
  double s = 0.;
  if (col < hd)
    for (int64_t k = k_lo + half; k < k_hi; k += 2) {
      const double z = Zh[(size_t)k * hd + col];
      s += z * z;
    }
  half_[half][col] = s;
  __syncthreads();
  if (half == 0 && col < hd) pn[((size_t)h * n_chunk + chunk) * hd + col] = half_[0][col] + half_[1][col];
}

// one workgroup per kv head: c_i = max(lambda_i, 0) * (sum over the group's heads, in head order, of the head's chunks in order), then
// the suffix sum from the tail by one thread (hd <= 128 additions).  pn == nullptr (MHA): c_i = max(lambda_i, 0).
__global__ __launch_bounds__(128) void vo_curve_kernel(const double* lam_all, const double* pn, int hd, int group, int n_chunk,
                                                       double* curve) {
  __shared__ double c_[128];
  const int kv = blockIdx.x, i = threadIdx.x;
  if (i < hd) {
    const double l = lam_all[(size_t)kv * hd + i];
    double w = 1.;
    if (pn) {
      w = 0.;
      for (int j = 0; j < group; j++) {
        const double* ph = pn + (size_t)(kv * group + j) * n_chunk * hd;
        double s = 0.;
        for (int c = 0; c < n_chunk; c++) s += ph[(size_t)c * hd + i];
        w += s;
      }
    }
    c_[i] = (l < 0. ? 0. : l) * w;          // (a NaN eigenvalue stays a NaN)
  }
  __syncthreads();
  if (i == 0) {
    double* out = curve + (size_t)kv * (hd + 1);
    double s = 0.;
    out[hd] = s;
    for (int a = hd - 1; a >= 0; a--) {
      s += c_[a];
      out[a] = s;
    }
  }
}

// Z [n_heads][d][hd] and the chunk partials of its column norms [n_heads][ceil(d / 256)][hd]
struct VoCurveWs {
  double *Z, *pn;
  size_t bytes;
};
static VoCurveWs vo_curve_layout(void* ws, int64_t d, int n_heads, int hd) {
  VoCurveWs w;
  Carve c(ws);
  w.Z = c.take<double>((size_t)n_heads * (size_t)d * hd);
  w.pn = c.take<double>((size_t)n_heads * (size_t)ceil_div(d, VO_CURVE_CHUNK) * hd);
  w.bytes = c.off;
  return w;
}

static bool vo_head_layout_ok(int n_heads, int n_kv, int hd) {
  return n_kv > 0 && n_heads > 0 && n_heads % n_kv == 0 && hd >= 2 && hd <= 128 && hd % 2 == 0;
}

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_vo_output_error_ws_bytes(int64_t d, int n_heads, int n_kv, int hd, int rank) {
  if (d <= 0 || !vo_head_layout_ok(n_heads, n_kv, hd) || rank < 0 || rank > hd) return 0;
  return vo_err_layout(nullptr, d, n_heads, n_kv, hd, rank).bytes;
}

extern "C" int mdg_vo_output_error(const double* cov_x, int64_t d, int64_t ldc, const void* Wv, int64_t ld_wv, const void* Wo,
                                   int64_t ld_wo, int w_dtype, int n_heads, int n_kv, int hd, int rank, const void* v_new,
                                   int64_t ld_v, const void* o_new, int64_t ld_o, int new_dtype, double* e, double* dnorm2, void* ws,
                                   size_t ws_bytes, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(cov_x && Wv && Wo && e, "mdg_vo_output_error: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_vo_output_error: weights must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(vo_head_layout_ok(n_heads, n_kv, hd), "mdg_vo_output_error: unsupported head layout (n_heads=%d n_kv=%d hd=%d)",
                n_heads, n_kv, hd);
  MDG_CHECK_ARG(rank >= 0 && rank <= hd, "mdg_vo_output_error: rank %d outside [0, %d]", rank, hd);
  MDG_CHECK_ARG(rank == 0 || (v_new && o_new), "mdg_vo_output_error: rank %d needs v_new and o_new", rank);
  const int r = (v_new && o_new) ? rank : 0;                      // v_new == NULL: nothing is subtracted, as rank == 0
  MDG_CHECK_ARG(r == 0 || new_dtype == MDG_BF16 || new_dtype == MDG_F64, "mdg_vo_output_error: factors must be bf16 or f64 (got %d)",
                new_dtype);
  MDG_CHECK_ARG(d > 0 && ldc >= d && ld_wv >= d && ld_wo >= (int64_t)n_heads * hd &&
                    (r == 0 || (ld_v >= d && ld_o >= (int64_t)n_heads * r)), "mdg_vo_output_error: bad leading dimensions");
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_vo_output_error_ws_bytes(d, n_heads, n_kv, hd, r),
                "mdg_vo_output_error: workspace %zu < required %zu", ws_bytes, mdg_vo_output_error_ws_bytes(d, n_heads, n_kv, hd, r));
  const int64_t tiles_d = ceil_div(d, TILE);
  MDG_CHECK_ARG(tiles_d < (1ll << 31) && n_heads < 65536, "mdg_vo_output_error: grid too large");
  hipStream_t st = (hipStream_t)stream;
  VoErrWs w = vo_err_layout(ws, d, n_heads, n_kv, hd, r);
  if (r == 0) new_dtype = w_dtype;                                // (one instantiation less to reach; o_new is not read)
  const int64_t n = hd + r, nn = n * n, nd = n * d;
  double* Gc = w.gram;
  double* Gn = w.gram + (size_t)n_kv * nn;
  // T_g = V_g C: rows 0 .. hd-1 from W_v,g, rows hd .. n-1 from -v'_g                                   [n, d] per kv head
  MDG_TRY(gemm_f64(hd, d, d, 1.0, Wv, w_dtype, ld_wv, 1, nullptr, cov_x, MDG_F64, ldc, 1, 0.0, w.T, MDG_F64, d, n_kv,
                   (int64_t)hd * ld_wv, 0, nd, 0, st));
  if (r)
    MDG_TRY(gemm_f64(r, d, d, -1.0, v_new, new_dtype, ld_v, 1, nullptr, cov_x, MDG_F64, ldc, 1, 0.0, w.T + (size_t)hd * d, MDG_F64, d,
                     n_kv, (int64_t)r * ld_v, 0, nd, 0, st));
  // Gc_g = T_g V_g^T: the block column of W_v (all n rows), then rows hd .. n-1 of the block column of -v'   [n, n] per kv head
  MDG_TRY(gemm_f64(n, hd, d, 1.0, w.T, MDG_F64, d, 1, nullptr, Wv, w_dtype, 1, ld_wv, 0.0, Gc, MDG_F64, n, n_kv, nd,
                   (int64_t)hd * ld_wv, nn, 0, st));
  if (r)
    MDG_TRY(gemm_f64(r, r, d, -1.0, w.T + (size_t)hd * d, MDG_F64, d, 1, nullptr, v_new, new_dtype, 1, ld_v, 0.0,
                     Gc + (size_t)hd * n + hd, MDG_F64, n, n_kv, nd, (int64_t)r * ld_v, nn, 0, st));
  if (dnorm2) {
    // Gn_g = V_g V_g^T: W_v W_v^T, -v' W_v^T, v' v'^T (what lies above the block diagonal is never read)
    MDG_TRY(gemm_f64(hd, hd, d, 1.0, Wv, w_dtype, ld_wv, 1, nullptr, Wv, w_dtype, 1, ld_wv, 0.0, Gn, MDG_F64, n, n_kv,
                     (int64_t)hd * ld_wv, (int64_t)hd * ld_wv, nn, 0, st));
    if (r) {
      MDG_TRY(gemm_f64(r, hd, d, -1.0, v_new, new_dtype, ld_v, 1, nullptr, Wv, w_dtype, 1, ld_wv, 0.0, Gn + (size_t)hd * n, MDG_F64,
                       n, n_kv, (int64_t)r * ld_v, (int64_t)hd * ld_wv, nn, 0, st));
      MDG_TRY(gemm_f64(r, r, d, 1.0, v_new, new_dtype, ld_v, 1, nullptr, v_new, new_dtype, 1, ld_v, 0.0,
                       Gn + (size_t)hd * n + hd, MDG_F64, n, n_kv, (int64_t)r * ld_v, (int64_t)r * ld_v, nn, 0, st));
    }
  }
  VoQuadArgs g;
  g.Wo = Wo; g.ld_wo = ld_wo;
  g.o_new = o_new; g.ld_o = ld_o;
  g.gram = w.gram; g.part = w.part;
  g.d = d;
  g.hd = hd; g.r = r; g.n = (int)n; g.group = n_heads / n_kv; g.n_heads = n_heads; g.n_kv = n_kv;
  g.tiles_n = (int)ceil_div(n, TILE);
  const int planes = dnorm2 ? 2 : 1;
  const dim3 grid((unsigned)tiles_d, (unsigned)(planes * g.tiles_n), (unsigned)n_heads);
  const bool n64 = new_dtype == MDG_F64;
  if (w_dtype == MDG_BF16 && !n64) hipLaunchKernelGGL((vo_quad_kernel<MDG_BF16, MDG_BF16>), grid, dim3(256), 0, st, g);
  else if (w_dtype == MDG_BF16) hipLaunchKernelGGL((vo_quad_kernel<MDG_BF16, MDG_F64>), grid, dim3(256), 0, st, g);
  else if (!n64) hipLaunchKernelGGL((vo_quad_kernel<MDG_F64, MDG_BF16>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((vo_quad_kernel<MDG_F64, MDG_F64>), grid, dim3(256), 0, st, g);
  MDG_LAUNCH_CHECK();
  const int64_t total = (int64_t)n_heads * d;
  // (the partials are laid out [plane][J][head][d]: plane 1 starts tiles_n * total behind plane 0)
  hipLaunchKernelGGL(quad_reduce_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, w.part, total, g.tiles_n, e, dnorm2);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" size_t mdg_vo_rank_curve_ws_bytes(int64_t d, int n_heads, int n_kv, int hd) {
  if (d <= 0 || !vo_head_layout_ok(n_heads, n_kv, hd) || n_heads == n_kv) return 0;       // MHA: the second spectrum alone
  return vo_curve_layout(nullptr, d, n_heads, hd).bytes;
}

extern "C" int mdg_vo_rank_curve(const void* vo_ws, size_t vo_ws_bytes, const void* Wo, int64_t ld_wo, int w_dtype, int64_t d,
                                 int n_heads, int n_kv, int hd, double* curve, void* ws, size_t ws_bytes, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(vo_ws && Wo && curve, "mdg_vo_rank_curve: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_vo_rank_curve: weights must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(vo_head_layout_ok(n_heads, n_kv, hd), "mdg_vo_rank_curve: unsupported head layout (n_heads=%d n_kv=%d hd=%d)", n_heads,
                n_kv, hd);
  MDG_CHECK_ARG(d > 0 && ld_wo >= (int64_t)n_heads * hd, "mdg_vo_rank_curve: bad leading dimensions");
  MDG_CHECK_ARG(vo_ws_bytes >= mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd), "mdg_vo_rank_curve: mdg_vo_compress workspace too small");
  const size_t need = mdg_vo_rank_curve_ws_bytes(d, n_heads, n_kv, hd);
  MDG_CHECK_ARG((need == 0 || ws) && ws_bytes >= need, "mdg_vo_rank_curve: workspace %zu < required %zu", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  VoWs w = vo_layout(const_cast<void*>(vo_ws), d, n_heads, n_kv, hd);
  const int group = n_heads / n_kv;
  if (group == 1) {
    hipLaunchKernelGGL(vo_curve_kernel, dim3(n_kv), dim3(128), 0, st, w.evals2, (const double*)nullptr, hd, 1, 0, curve);
    MDG_LAUNCH_CHECK();
    return MDG_OK;
  }
  const int64_t n_chunk = ceil_div(d, VO_CURVE_CHUNK);
  MDG_CHECK_ARG(n_chunk < (1ll << 31) && n_heads < 65536, "mdg_vo_rank_curve: grid too large");
  const VoCurveWs cw = vo_curve_layout(ws, d, n_heads, hd);
  double *Z = cw.Z, *pn = cw.pn;
  const int64_t wsz = w_dtype == MDG_BF16 ? 2 : 8, hh = (int64_t)hd * hd;
  // Z[kv * group + j] = W_o,h V_kv                                                                     [d, hd] per query head
  for (int j = 0; j < group; j++)
    MDG_TRY(gemm_f64(d, hd, hd, 1.0, (const char*)Wo + (int64_t)j * hd * wsz, w_dtype, ld_wo, 1, nullptr, w.evecs, MDG_F64, hd, 1, 0.0,
                     Z + (size_t)j * d * hd, MDG_F64, hd, n_kv, (int64_t)group * hd, hh, (int64_t)group * d * hd, 0, st));
  hipLaunchKernelGGL(vo_colnorm_kernel, dim3((unsigned)n_chunk, (unsigned)n_heads), dim3(256), 0, st, Z, d, hd, (int)n_chunk, pn);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(vo_curve_kernel, dim3(n_kv), dim3(128), 0, st, w.evals, pn, hd, group, (int)n_chunk, curve);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
