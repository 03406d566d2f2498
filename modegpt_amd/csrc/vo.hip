// VO compression (compress_vo.py:14-223) on the Gram matrix.
//
// Reference: A_h = sqrt(C) W_v,h^T = U S V^T (thin SVD), W_v' = (C^-1/2 U_r)^T, W_o'[j] = (S_r V_r^T W_o,j^T)^T.
// Identity used here (C := Sigma_x + rho I, symmetric PD so sqrt(C)^2 = C):
//   G_h := A_h^T A_h = W_v,h C W_v,h^T = V S^2 V^T          (128 x 128, batched Jacobi)
//   C^-1/2 U_r = C^-1/2 A_h V_r S_r^-1 = W_v,h^T V_r S_r^-1  => W_v' = S_r^-1 V_r^T W_v,h
//   W_o'[j]   = W_o,j V_r S_r
// so the d x d eigensolve and LU inverse of compress_vo.py:43-45 never happen.  The MHA variant (two SVDs,
// :162-223) reduces the same way: B = S V^T W_o,h^T, B B^T = (S V^T)(W_o,h^T W_o,h)(V S) = U_p S_p^2 U_p^T,
// W_v' = U_p,r^T S^-1 V^T W_v,h,  W_o' = W_o,h V S U_p,r.
#include "common.hpp"
#include "row_dots.hpp"
#include "vo_ws.hpp"

namespace mdg {
int gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i, int64_t sa_k,
             const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k, int64_t sb_j, double beta, void* C,
             int c_dtype, int64_t ldc, int64_t batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int flags,
             hipStream_t st);
int syevj_batched(double* A, int64_t n, int64_t batch, double* evals, double* evecs, int* dflag, hipStream_t st,
                  int max_sweeps = 40, int sorted = 1);
int check_flag(int* dflag, hipStream_t st, const char* what);

// dst (f64, ld) = scale * src (bf16 or f64, ld_src)
template <int DT>
__global__ __launch_bounds__(256) void scale_to_f64_kernel(const void* src, int64_t ld_src, int64_t cols, double scale,
                                                           double* dst, int64_t ld) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < cols; c += 256) dst[r * ld + c] = scale * load_f64<DT>(src, r * ld_src + c);
}

// grouped: P[h][a][k] = V[k][a] / S_a, Q[h][k][a] = V[k][a] * S_a  (a < r)
__global__ __launch_bounds__(256) void vo_factors_grouped_kernel(const double* evals, const double* evecs, int hd, int r,
                                                                 double* P, double* Q) {
  const int h = blockIdx.x;
  const double* lam = evals + (int64_t)h * hd;
  const double* V = evecs + (int64_t)h * hd * hd;
  for (int e = threadIdx.x; e < r * hd; e += 256) {
    const int a = e / hd, k = e % hd;
    const double l = lam[a];
    const double s = sqrt(l > 0. ? l : 0.);
    const double v = V[k * hd + a];
    P[(int64_t)h * r * hd + a * hd + k] = s > 0. ? v / s : 0.;
    Q[(int64_t)h * hd * r + k * r + a] = v * s;
  }
}

// Y[h][a][k] = S_a V[k][a]   (all hd components)
__global__ __launch_bounds__(256) void vo_sv_kernel(const double* evals, const double* evecs, int hd, double* Y) {
  const int h = blockIdx.x;
  const double* lam = evals + (int64_t)h * hd;
  const double* V = evecs + (int64_t)h * hd * hd;
  for (int e = threadIdx.x; e < hd * hd; e += 256) {
    const int a = e / hd, k = e % hd;
    const double l = lam[a];
    Y[(int64_t)h * hd * hd + e] = sqrt(l > 0. ? l : 0.) * V[k * hd + a];
  }
}

// MHA: P[h][a][k] = sum_b Up[b][a] / S_b * V[k][b],  Q[h][k][a] = sum_b V[k][b] * S_b * Up[b][a]   (a < r)
__global__ __launch_bounds__(256) void vo_factors_mha_kernel(const double* evals, const double* evecs, const double* up,
                                                             int hd, int r, double* P, double* Q) {
  __shared__ double s_[128], is_[128];
  const int h = blockIdx.x;
  const double* lam = evals + (int64_t)h * hd;
  const double* V = evecs + (int64_t)h * hd * hd;
  const double* U = up + (int64_t)h * hd * hd;
  if (threadIdx.x < hd) {
    const double l = lam[threadIdx.x];
    const double s = sqrt(l > 0. ? l : 0.);
    s_[threadIdx.x] = s;
    is_[threadIdx.x] = s > 0. ? 1. / s : 0.;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < r * hd; e += 256) {
    const int a = e / hd, k = e % hd;
    double p = 0., q = 0.;
    for (int b = 0; b < hd; b++) {
      const double u = U[b * hd + a], v = V[k * hd + b];
      p += u * is_[b] * v;
      q += v * s_[b] * u;
    }
    P[(int64_t)h * r * hd + a * hd + k] = p;
    Q[(int64_t)h * hd * r + k * r + a] = q;
  }
}

// What the truncation at `rank` did to the spectrum mdg_vo_compress left in its workspace (lam: [n_kv][hd], descending): one
// workgroup per kv head, out[h][8] as documented at mdg_vo_spectrum.  grouped: also the Weyl bound eps * || |W_v,h| s ||_2^2,
// s_a = sqrt(sigma_x,aa).  The diagonal of sigma_x is a strided read: it is staged through LDS once per chunk of VO_SPEC_CHUNK
// columns; a wave owns every fourth row of the head's hd x d slice of W_v (hd <= 128: at most 32 rows, their partial sums in
// registers), lanes along the row (coalesced), fixed summation order.  vec (bf16 weights, 16-byte aligned rows, d % 8 == 0): eight
// weights per lane and load.
constexpr int VO_SPEC_CHUNK = 2048;
template <int DT>
__global__ __launch_bounds__(256) void vo_spectrum_kernel(const double* lam_all, const double* cov_x, int64_t d, int64_t ldc,
                                                          const void* Wv, int64_t ld_wv, int hd, int rank, int grouped, double eps,
                                                          int vec, double* out) {
  __shared__ double s_[VO_SPEC_CHUNK];
  __shared__ double part[4];
  const int h = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const double* lam = lam_all + (int64_t)h * hd;
  double mine = 0.;
  if (grouped) {
    double acc[32];
#pragma unroll
    for (int ii = 0; ii < 32; ii++) acc[ii] = 0.;
    for (int64_t a0 = 0; a0 < d; a0 += VO_SPEC_CHUNK) {
      const int len = (int)(d - a0 < VO_SPEC_CHUNK ? d - a0 : VO_SPEC_CHUNK);
      __syncthreads();
      for (int e = tid; e < len; e += 256) s_[e] = sqrt(fmax(cov_x[(a0 + e) * ldc + a0 + e], 0.));
      __syncthreads();
#pragma unroll
      for (int ii = 0; ii < 32; ii++) {
        const int i = w + 4 * ii;
        if (i < hd) {
          const int64_t row = ((int64_t)h * hd + i) * ld_wv + a0;
          double s = 0.;
          if (DT == MDG_BF16 && vec) {
            const uint4* rp = (const uint4*)((const bf16_t*)Wv + row);
            for (int v = lane; v < len / 8; v += 64) {
              const uint4 u = rp[v];
              const double* sp = s_ + 8 * v;
              const unsigned q[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
              for (int t = 0; t < 4; t++)   // (|x|: the sign bit masked off; element 2t in the low half)
                s += bf16_to_f64((bf16_t)(q[t] & 0x7fffu)) * sp[2 * t] + bf16_to_f64((bf16_t)((q[t] >> 16) & 0x7fffu)) * sp[2 * t + 1];
            }
          } else {
            for (int e = lane; e < len; e += 64) s += fabs(load_f64<DT>(Wv, row + e)) * s_[e];
          }
          acc[ii] += s;
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < 32; ii++) {
      double s = acc[ii];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      mine += s * s;     // (rows beyond hd contribute exact zeros)
    }
  }
  if (lane == 0) part[w] = mine;
  __syncthreads();
  if (tid == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double l_r = lam[rank - 1], l_next = rank < hd ? lam[rank] : 0.;
    const double s_r = sqrt(fmax(l_r, 0.)), s_next = sqrt(fmax(l_next, 0.));
    double kept = 0., all = 0.;
    for (int i = 0; i < hd; i++) {
      all += lam[i];
      if (i == rank - 1) kept = all;
    }
    const double b = eps * (((part[0] + part[1]) + part[2]) + part[3]);
    double* o8 = out + (int64_t)h * 8;
    o8[0] = l_r; o8[1] = l_next;
    o8[2] = s_r > 0. ? (s_r - s_next) / s_r : 0.;
    o8[3] = kept / all;
    o8[4] = grouped ? b : nan;
    o8[5] = grouped ? (l_r - l_next > 2. * b ? 1. : 0.) : nan;
    o8[6] = lam[0]; o8[7] = lam[hd - 1];
  }
}

// ---- the projection biases through the truncation (mdg_vo_bias) ----
// Scratch of mdg_vo_bias inside the T block of the workspace (T = W_v C is dead once the Gram matrices are formed):
// [0, a) b_v widened, [a, 2a) u = (I - Q P) b_v, [2a, 2a + d) s_i = W_o[i, :] b_v, [2a + d, 2a + 2d) rho_i = W_o[i, :] u;  a = n_kv hd.
template <int DT>
__global__ __launch_bounds__(128) void vo_bias_head_kernel(const double* P, const double* Q, const void* b_v, int hd, int r,
                                                           double* v_bias, double* bw, double* u) {
  __shared__ double b_[128], c_[128];
  const int g = blockIdx.x, tid = threadIdx.x;
  const double* Pg = P + (int64_t)g * r * hd;
  const double* Qg = Q + (int64_t)g * hd * r;
  if (tid < hd) bw[(int64_t)g * hd + tid] = b_[tid] = load_f64<DT>(b_v, (int64_t)g * hd + tid);
  __syncthreads();
  if (tid < r) {                       // c = P_g b_v,g: the bias of the truncated v_proj
    double s = 0.;
    for (int k = 0; k < hd; k++) s += Pg[tid * hd + k] * b_[k];
    c_[tid] = s;
    if (v_bias) v_bias[(int64_t)g * r + tid] = s;
  }
  __syncthreads();
  if (tid < hd) {                      // u = b_v,g - Q_g c: what no bias of the truncated v_proj can carry
    double s = 0.;
    for (int a = 0; a < r; a++) s += Qg[tid * r + a] * c_[a];
    u[(int64_t)g * hd + tid] = b_[tid] - s;
  }
}

// s_i and rho_i for RD_ROWS rows of W_o per workgroup: one pass of row_dots (row_dots.hpp) carries both vectors, staged already
// expanded to the query heads' columns, so that W_o is read once.
template <int DT>
__global__ __launch_bounds__(256) void vo_bias_rows_kernel(const void* Wo, int64_t ld_wo, int64_t d, int n_cols, int hd, int group,
                                                           const double* bw, const double* u, const void* b_o, int bo_dtype, int vec,
                                                           double* o_bias, double* s_out, double* rho_out) {
  __shared__ double sv_[2 * RD_CHUNK];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + (int64_t)w * RD_RPW;
  double st[2 * RD_RPW];                // s, then rho
  row_dots<DT, 2>(Wo, ld_wo, d, row0, n_cols, StageHeads<2>{{bw, u}, hd, group}, vec, sv_, st);
#pragma unroll
  for (int rr = 0; rr < RD_RPW; rr++) {
    const int64_t row = row0 + rr;
    if (lane == 0 && row < d) {
      s_out[row] = st[rr];
      rho_out[row] = st[RD_RPW + rr];
      if (o_bias) o_bias[row] = load_any(b_o, bo_dtype, row) + st[rr];
    }
  }
}

template <int DT>
static int vo_bias_launch(const VoWs& w, const void* Wo, int64_t ld_wo, int64_t d, const void* b_v, const void* b_o, int b_dtype,
                          int n_heads, int n_kv, int hd, int rank, double* o_bias, double* v_bias, double* resid, int vec,
                          hipStream_t st) {
  const VoBiasWs sw = vo_bias_layout(w.T, d, n_kv, hd);
  double *bw = sw.bw, *u = sw.u, *s_rows = sw.s_rows, *rho_rows = sw.rho_rows;
  switch (b_dtype) {
    case MDG_BF16: hipLaunchKernelGGL(vo_bias_head_kernel<MDG_BF16>, dim3(n_kv), dim3(128), 0, st, w.P, w.Q, b_v, hd, rank, v_bias, bw, u); break;
    case MDG_F16: hipLaunchKernelGGL(vo_bias_head_kernel<MDG_F16>, dim3(n_kv), dim3(128), 0, st, w.P, w.Q, b_v, hd, rank, v_bias, bw, u); break;
    case MDG_F32: hipLaunchKernelGGL(vo_bias_head_kernel<MDG_F32>, dim3(n_kv), dim3(128), 0, st, w.P, w.Q, b_v, hd, rank, v_bias, bw, u); break;
    default: hipLaunchKernelGGL(vo_bias_head_kernel<MDG_F64>, dim3(n_kv), dim3(128), 0, st, w.P, w.Q, b_v, hd, rank, v_bias, bw, u); break;
  }
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(vo_bias_rows_kernel<DT>, dim3((unsigned)ceil_div(d, RD_ROWS)), dim3(256), 0, st, Wo, ld_wo, d, n_heads * hd, hd,
                     n_heads / n_kv, bw, u, b_o, b_dtype, vec, o_bias, s_rows, rho_rows);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_norms_kernel, dim3(1), dim3(256), 0, st, rho_rows, s_rows, d, resid);      // (||rho||^2, ||s||^2)
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_vo_compress_ws_bytes(int64_t d, int n_heads, int n_kv, int hd) {
  return vo_layout(nullptr, d, n_heads, n_kv, hd).bytes;
}

extern "C" int mdg_vo_compress(const double* cov_x, int64_t d, int64_t ldc, const void* Wv, int64_t ld_wv, const void* Wo,
                               int64_t ld_wo, int w_dtype, int n_heads, int n_kv, int hd, int rank, double ridge, void* v_out,
                               int64_t ld_v, void* o_out, int64_t ld_o, double* v_f64, double* o_f64, void* ws,
                               size_t ws_bytes, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(cov_x && Wv && Wo && v_out && o_out, "mdg_vo_compress: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_vo_compress: weights must be bf16 or f64 (got %d)", w_dtype);
  const int64_t wsz = w_dtype == MDG_BF16 ? 2 : 8;
  MDG_CHECK_ARG(n_kv > 0 && n_heads % n_kv == 0 && hd >= 2 && hd <= 128 && hd % 2 == 0,
                "mdg_vo_compress: unsupported head layout (n_heads=%d n_kv=%d hd=%d)", n_heads, n_kv, hd);
  MDG_CHECK_ARG(rank >= 1 && rank <= hd, "mdg_vo_compress: rank %d outside [1, %d]", rank, hd);
  MDG_CHECK_ARG(d > 0 && ldc >= d && ld_wv >= d && ld_wo >= (int64_t)n_heads * hd && ld_v >= d &&
                    ld_o >= (int64_t)n_heads * rank, "mdg_vo_compress: bad leading dimensions");
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd), "mdg_vo_compress: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  VoWs w = vo_layout(ws, d, n_heads, n_kv, hd);
  const int g = n_heads / n_kv;
  const bool mha = (g == 1);
  const int64_t rows = (int64_t)n_kv * hd, hh = (int64_t)hd * hd;
  // T = W_v (Sigma_x + rho I) = rho W_v + W_v Sigma_x                       [n_kv*hd, d]
  if (w_dtype == MDG_BF16)
    hipLaunchKernelGGL(scale_to_f64_kernel<MDG_BF16>, dim3((unsigned)rows), dim3(256), 0, st, Wv, ld_wv, d, ridge, w.T, d);
  else
    hipLaunchKernelGGL(scale_to_f64_kernel<MDG_F64>, dim3((unsigned)rows), dim3(256), 0, st, Wv, ld_wv, d, ridge, w.T, d);
  MDG_LAUNCH_CHECK();
  MDG_TRY(gemm_f64(rows, d, d, 1.0, Wv, w_dtype, ld_wv, 1, nullptr, cov_x, MDG_F64, ldc, 1, 1.0, w.T, MDG_F64, d, 1, 0, 0,
                   0, 0, st));
  // G_h = T_h W_v,h^T                                                        [hd, hd] per kv head
  MDG_TRY(gemm_f64(hd, hd, d, 1.0, w.T, MDG_F64, d, 1, nullptr, Wv, w_dtype, 1, ld_wv, 0.0, w.G, MDG_F64, hd, n_kv,
                   (int64_t)hd * d, (int64_t)hd * ld_wv, hh, 0, st));
  MDG_TRY(syevj_batched(w.G, hd, n_kv, w.evals, w.evecs, w.flag, st));
  if (!mha) {
    hipLaunchKernelGGL(vo_factors_grouped_kernel, dim3(n_kv), dim3(256), 0, st, w.evals, w.evecs, hd, rank, w.P, w.Q);
    MDG_LAUNCH_CHECK();
  } else {
    MDG_TRY(check_flag(w.flag, st, "mdg_vo_compress (first SVD)"));
    // M_h = W_o,h^T W_o,h
    MDG_TRY(gemm_f64(hd, hd, d, 1.0, Wo, w_dtype, 1, ld_wo, nullptr, Wo, w_dtype, ld_wo, 1, 0.0, w.Mh, MDG_F64, hd,
                     n_heads, hd, hd, hh, 0, st));
    hipLaunchKernelGGL(vo_sv_kernel, dim3(n_kv), dim3(256), 0, st, w.evals, w.evecs, hd, w.Y);
    MDG_LAUNCH_CHECK();
    // B B^T = Y M Y^T
    MDG_TRY(gemm_f64(hd, hd, hd, 1.0, w.Y, MDG_F64, hd, 1, nullptr, w.Mh, MDG_F64, hd, 1, 0.0, w.tmp, MDG_F64, hd, n_kv, hh,
                     hh, hh, 0, st));
    MDG_TRY(gemm_f64(hd, hd, hd, 1.0, w.tmp, MDG_F64, hd, 1, nullptr, w.Y, MDG_F64, 1, hd, 0.0, w.Mh, MDG_F64, hd, n_kv, hh,
                     hh, hh, 0, st));
    MDG_TRY(syevj_batched(w.Mh, hd, n_kv, w.evals2, w.evecs2, w.flag, st));
    hipLaunchKernelGGL(vo_factors_mha_kernel, dim3(n_kv), dim3(256), 0, st, w.evals, w.evecs, w.evecs2, hd, rank, w.P, w.Q);
    MDG_LAUNCH_CHECK();
  }
  // W_v'[h] = P_h W_v,h   -> rows [h*rank, (h+1)*rank) of v_out
  for (int pass = 0; pass < (v_f64 ? 2 : 1); pass++) {
    void* out = pass ? (void*)v_f64 : v_out;
    int64_t ld = pass ? d : ld_v;
    MDG_TRY(gemm_f64(rank, d, hd, 1.0, w.P, MDG_F64, hd, 1, nullptr, Wv, w_dtype, ld_wv, 1, 0.0, out,
                     pass ? MDG_F64 : MDG_BF16, ld, n_kv, (int64_t)rank * hd, (int64_t)hd * ld_wv, (int64_t)rank * ld, 0,
                     st));
  }
  // W_o'[h*g + j] = W_o[:, head] Q_h  -> columns [(h*g+j)*rank, +rank) of o_out
  for (int pass = 0; pass < (o_f64 ? 2 : 1); pass++) {
    for (int j = 0; j < g; j++) {
      char* out = pass ? (char*)(o_f64 + (int64_t)j * rank) : (char*)o_out + (int64_t)j * rank * 2;
      int64_t ld = pass ? (int64_t)n_heads * rank : ld_o;
      MDG_TRY(gemm_f64(d, rank, hd, 1.0, (const char*)Wo + (int64_t)j * hd * wsz, w_dtype, ld_wo, 1, nullptr, w.Q, MDG_F64,
                       rank, 1, 0.0, out, pass ? MDG_F64 : MDG_BF16, ld, n_kv, (int64_t)g * hd, (int64_t)hd * rank,
                       (int64_t)g * rank, 0, st));
    }
  }
  return check_flag(w.flag, st, "mdg_vo_compress");
}

extern "C" int mdg_vo_spectrum(const void* ws, size_t ws_bytes, const double* cov_x, int64_t d, int64_t ldc, const void* Wv,
                               int64_t ld_wv, int w_dtype, int n_heads, int n_kv, int hd, int rank, double ridge, double eps,
                               double* out, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(cov_x && Wv && out, "mdg_vo_spectrum: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_vo_spectrum: weights must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n_kv > 0 && n_heads % n_kv == 0 && hd >= 2 && hd <= 128 && hd % 2 == 0,
                "mdg_vo_spectrum: unsupported head layout (n_heads=%d n_kv=%d hd=%d)", n_heads, n_kv, hd);
  MDG_CHECK_ARG(rank >= 1 && rank <= hd, "mdg_vo_spectrum: rank %d outside [1, %d]", rank, hd);
  MDG_CHECK_ARG(d > 0 && ldc >= d && ld_wv >= d, "mdg_vo_spectrum: bad leading dimensions");
  MDG_CHECK_ARG(eps >= 0. && ridge == ridge, "mdg_vo_spectrum: bad error bound / ridge");
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd), "mdg_vo_spectrum: workspace too small");
  VoWs w = vo_layout(const_cast<void*>(ws), d, n_heads, n_kv, hd);
  const int grouped = n_heads != n_kv;
  // the spectrum the last mdg_vo_compress on this workspace truncated: the Gram matrix's (grouped) / the second SVD's (MHA)
  const double* lam = grouped ? w.evals : w.evals2;
  const int vec = w_dtype == MDG_BF16 && (uintptr_t)Wv % 16 == 0 && ld_wv % 8 == 0 && d % 8 == 0;   // eight weights per load
  if (w_dtype == MDG_BF16)
    hipLaunchKernelGGL(vo_spectrum_kernel<MDG_BF16>, dim3(n_kv), dim3(256), 0, (hipStream_t)stream, lam, cov_x, d, ldc, Wv, ld_wv, hd,
                       rank, grouped, eps, vec, out);
  else
    hipLaunchKernelGGL(vo_spectrum_kernel<MDG_F64>, dim3(n_kv), dim3(256), 0, (hipStream_t)stream, lam, cov_x, d, ldc, Wv, ld_wv, hd,
                       rank, grouped, eps, 0, out);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" int mdg_vo_bias(void* ws, size_t ws_bytes, const void* Wo, int64_t ld_wo, int w_dtype, int64_t d, const void* b_v,
                           const void* b_o, int b_dtype, int n_heads, int n_kv, int hd, int rank, double* o_bias, double* v_bias,
                           double* resid, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(Wo && b_v && resid, "mdg_vo_bias: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F16 || w_dtype == MDG_F64, "mdg_vo_bias: W_o must be bf16, fp16 or f64 (got %d)",
                w_dtype);
  MDG_CHECK_ARG(b_dtype == MDG_BF16 || b_dtype == MDG_F16 || b_dtype == MDG_F32 || b_dtype == MDG_F64,
                "mdg_vo_bias: unsupported bias dtype %d", b_dtype);
  MDG_CHECK_ARG(n_kv > 0 && n_heads > 0 && n_heads % n_kv == 0 && hd >= 2 && hd <= 128 && hd % 2 == 0,
                "mdg_vo_bias: unsupported head layout (n_heads=%d n_kv=%d hd=%d)", n_heads, n_kv, hd);
  MDG_CHECK_ARG(rank >= 1 && rank <= hd, "mdg_vo_bias: rank %d outside [1, %d]", rank, hd);
  MDG_CHECK_ARG(d > 0 && d < (1ll << 31) && ld_wo >= (int64_t)n_heads * hd && (int64_t)n_heads * hd < (1ll << 31),
                "mdg_vo_bias: bad leading dimensions");
  MDG_CHECK_ARG(b_o ? o_bias != nullptr : v_bias != nullptr, "mdg_vo_bias: o_bias is required with b_o, v_bias without it");
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_vo_compress_ws_bytes(d, n_heads, n_kv, hd), "mdg_vo_bias: workspace too small");
  // (the scratch lives in the workspace's T block, n_kv hd d doubles: see vo_bias_head_kernel)
  MDG_CHECK_ARG(vo_bias_layout(nullptr, d, n_kv, hd).bytes / sizeof(double) <= (size_t)n_kv * hd * (size_t)d,
                "mdg_vo_bias: d = %lld too small for the scratch", (long long)d);
  VoWs w = vo_layout(ws, d, n_heads, n_kv, hd);
  hipStream_t st = (hipStream_t)stream;
  const int vec = w_dtype != MDG_F64 && (uintptr_t)Wo % 16 == 0 && ld_wo % 8 == 0;
  // with b_o the v bias is folded into o_bias and v_bias is not written; without it o_bias is not written
  double* ob = b_o ? o_bias : nullptr;
  double* vb = b_o ? nullptr : v_bias;
  if (w_dtype == MDG_BF16)
    return vo_bias_launch<MDG_BF16>(w, Wo, ld_wo, d, b_v, b_o, b_dtype, n_heads, n_kv, hd, rank, ob, vb, resid, vec, st);
  if (w_dtype == MDG_F16)
    return vo_bias_launch<MDG_F16>(w, Wo, ld_wo, d, b_v, b_o, b_dtype, n_heads, n_kv, hd, rank, ob, vb, resid, vec, st);
  return vo_bias_launch<MDG_F64>(w, Wo, ld_wo, d, b_v, b_o, b_dtype, n_heads, n_kv, hd, rank, ob, vb, resid, 0, st);
}
