// First moments of the MLP statistic and what is done with them (not upstream: the reference's refit has no intercept):
//   mdg_col_sum_accum      sum[j] += sum_t f(x[t, j])   in fp64, one pass over x                        (HBM-bound: the bytes of x)
//   mdg_cov_center         S_ij = fma(-mu_i, mu_j, C_ij), both triangles from the lower one of C          (HBM-bound: 1.5 n^2 8 bytes)
//   mdg_nystrom_intercept  delta_i = W_d[i, :] mu - D^[i, :] mu[idx], the bias b_d + delta and two norms  (one read of W_d and D^;
//                          the rows and the norms through row_dots.hpp, shared with mdg_vo_intercept and mdg_vo_bias)
// No atomics anywhere; every sum is taken in an order that depends on the shapes alone, so the bits repeat from run to run.
#include "common.hpp"
#include "row_dots.hpp"

using namespace mdg;

namespace mdg {

// ---------------------------------------------------------------- column sums
// A workgroup owns COL_SUM_CHUNK tokens and 256 column slots.  A slot is a 16-byte vector of the row (8 / 4 / 2 columns) where the
// rows allow aligned vector loads, otherwise one column: the `head` columns in front of the first 16-byte boundary, the columns
// behind the last whole vector, or every column when ld is no multiple of the vector.  Slots 0 .. nvec-1 are vectors, the scalar
// columns follow.  Every thread adds its tokens in ascending order; the partial row of chunk c goes to part[c][0 .. n).
constexpr int COL_SUM_CHUNK = 128, COL_SUM_UNROLL = 4;

template <bool RELU>
__device__ __forceinline__ double col_f(double v) {
  return RELU ? (v > 0. ? v : (v != v ? v : 0.)) : v;      // ReLU keeps a NaN (it stays in its column) and turns -0 into +0
}

template <int DT, int VEC>
__device__ __forceinline__ void unpack16(const uint4& q, double* v) {
  if (DT == MDG_BF16 || DT == MDG_F16) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {                            // (element 2k in the low half)
      const unsigned short lo = (unsigned short)(w[k] & 0xffffu), hi = (unsigned short)(w[k] >> 16);
      v[2 * k] = DT == MDG_BF16 ? bf16_to_f64(lo) : f16_to_f64(lo);
      v[2 * k + 1] = DT == MDG_BF16 ? bf16_to_f64(hi) : f16_to_f64(hi);
    }
  } else if (DT == MDG_F32) {
    v[0] = (double)__uint_as_float(q.x);
    v[1] = (double)__uint_as_float(q.y);
    v[2] = (double)__uint_as_float(q.z);
    v[3] = (double)__uint_as_float(q.w);
  } else {
    v[0] = __hiloint2double((int)q.y, (int)q.x);
    v[1] = __hiloint2double((int)q.w, (int)q.z);
  }
}

template <int DT, bool RELU>
__global__ __launch_bounds__(256) void col_sum_partial_kernel(const void* x, int64_t tokens, int64_t n, int64_t ld, int head,
                                                              int64_t nvec, double* part) {
  typedef typename ElemOf<DT>::type elem_t;
  constexpr int VEC = 16 / (int)sizeof(elem_t);
  const int64_t g = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const int64_t c = blockIdx.x, t0 = c * COL_SUM_CHUNK;
  const int64_t t1 = t0 + COL_SUM_CHUNK < tokens ? t0 + COL_SUM_CHUNK : tokens;
  const int64_t nsc = n - nvec * VEC;
  double* prow = part + c * n;
  if (g < nvec) {
    const int64_t col = head + g * VEC;
    const elem_t* p = (const elem_t*)x + col;
    double acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) acc[k] = 0.;
    int64_t t = t0;
    for (; t + COL_SUM_UNROLL <= t1; t += COL_SUM_UNROLL) {
      uint4 q[COL_SUM_UNROLL];
#pragma unroll
      for (int u = 0; u < COL_SUM_UNROLL; u++) q[u] = *(const uint4*)(p + (t + u) * ld);
#pragma unroll
      for (int u = 0; u < COL_SUM_UNROLL; u++) {
        double v[VEC];
        unpack16<DT, VEC>(q[u], v);
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] += col_f<RELU>(v[k]);
      }
    }
    for (; t < t1; t++) {
      const uint4 q = *(const uint4*)(p + t * ld);
      double v[VEC];
      unpack16<DT, VEC>(q, v);
#pragma unroll
      for (int k = 0; k < VEC; k++) acc[k] += col_f<RELU>(v[k]);
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) prow[col + k] = acc[k];
  } else if (g < nvec + nsc) {
    const int64_t s = g - nvec;
    const int64_t col = s < head ? s : head + nvec * VEC + (s - head);
    double acc = 0.;
    for (int64_t t = t0; t < t1; t++) acc += col_f<RELU>(load_f64<DT>(x, t * ld + col));
    prow[col] = acc;
  }
}

// sum[j] += part[0][j] + part[1][j] + ... in ascending chunk order (the partials are added to each other first, then to sum)
__global__ __launch_bounds__(256) void col_sum_reduce_kernel(const double* part, int64_t chunks, int64_t n, double* sum) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = part[j];
  for (int64_t c = 1; c < chunks; c++) s += part[c * n + j];
  sum[j] += s;
}

template <int DT>
static int col_sum_launch(const void* x, int64_t tokens, int64_t n, int64_t ld, int relu, double* sum, double* part, hipStream_t st) {
  constexpr int VEC = 16 / (int)sizeof(typename ElemOf<DT>::type);
  constexpr int ES = (int)sizeof(typename ElemOf<DT>::type);
  // aligned 16-byte loads need every row to start at the same offset from a boundary: ld a multiple of the vector
  int head = (int)n;
  int64_t nvec = 0;
  if (ld % VEC == 0) {
    const int lead = (int)(((16 - (uintptr_t)x % 16) % 16) / ES);     // (x is aligned to its element: checked by the caller)
    if (lead <= n) {
      head = lead;
      nvec = (n - head) / VEC;
    }
  }
  if (nvec == 0) head = (int)n;
  const int64_t chunks = ceil_div(tokens, COL_SUM_CHUNK);
  const int64_t slots = nvec + (n - nvec * VEC);
  const dim3 grid((unsigned)chunks, (unsigned)ceil_div(slots, 256));
  if (relu)
    hipLaunchKernelGGL((col_sum_partial_kernel<DT, true>), grid, dim3(256), 0, st, x, tokens, n, ld, head, nvec, part);
  else
    hipLaunchKernelGGL((col_sum_partial_kernel<DT, false>), grid, dim3(256), 0, st, x, tokens, n, ld, head, nvec, part);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(col_sum_reduce_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, part, chunks, n, sum);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

// ---------------------------------------------------------------- centring
// One workgroup per 64 x 64 tile (bi, bj) of the LOWER block triangle (bj <= bi; the grid is square, the upper blocks leave at
// once).  The tile of S is computed from the tile of C, written in place and -- transposed through LDS -- at (bj, bi); a diagonal
// tile computes its entries at and below the diagonal and writes each to both places.  Nothing above the diagonal of C is read,
// so S is symmetric bit for bit whatever the upper triangle of C holds.
constexpr int CENTER_TILE = 64;

__global__ __launch_bounds__(256) void cov_center_kernel(const double* C, int64_t n, int64_t ldc, const double* mu, double* S,
                                                         int64_t lds) {
  __shared__ double tile_[CENTER_TILE][CENTER_TILE + 1];
  __shared__ double mi_[CENTER_TILE], mj_[CENTER_TILE];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)bi * CENTER_TILE, j0 = (int64_t)bj * CENTER_TILE;
  if (tid < CENTER_TILE) {
    mi_[tid] = i0 + tid < n ? mu[i0 + tid] : 0.;
  } else if (tid < 2 * CENTER_TILE) {
    const int b = tid - CENTER_TILE;
    mj_[b] = j0 + b < n ? mu[j0 + b] : 0.;
  }
  __syncthreads();
  const int b = tid & 63;
  for (int a = tid >> 6; a < CENTER_TILE; a += 4) {
    const int64_t i = i0 + a, j = j0 + b;
    if (i < n && j < n && j <= i) {
      const double v = fma(-mi_[a], mj_[b], C[i * ldc + j]);
      tile_[a][b] = v;
      S[i * lds + j] = v;
    }
  }
  __syncthreads();
  // the mirror image: entry (j, i) of S for every strictly-lower (i, j) of this tile; lanes run along i (a row of S)
  for (int bb = tid >> 6; bb < CENTER_TILE; bb += 4) {
    const int a = tid & 63;
    const int64_t i = i0 + a, j = j0 + bb;
    if (i < n && j < n && j < i) S[j * lds + i] = tile_[a][bb];
  }
}

// ---------------------------------------------------------------- intercept
// The rows of W_d against mu and of D^ against mu[idx] through row_dots (row_dots.hpp), one after the other on the same LDS chunk.
template <int DT>
__global__ __launch_bounds__(256) void intercept_rows_kernel(const void* Wd, int64_t ld_wd, int64_t d, int64_t n, const void* Dh,
                                                             int64_t ld_dh, int64_t r, const int64_t* idx, const double* mu, int vec_w,
                                                             int vec_d, const void* b_d, int b_dtype, void* bias_out, int out_dtype,
                                                             double* bias_f64, double* delta_rows, double* wmu_rows) {
  __shared__ double sv_[RD_CHUNK];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + (int64_t)w * RD_RPW;
  double a[RD_RPW], b[RD_RPW];
  row_dots<DT, 1>(Wd, ld_wd, d, row0, (int)n, StageGather{mu, n, nullptr}, vec_w, sv_, a);
  row_dots<MDG_BF16, 1>(Dh, ld_dh, d, row0, (int)r, StageGather{mu, n, idx}, vec_d, sv_, b);
#pragma unroll
  for (int rr = 0; rr < RD_RPW; rr++) {
    const int64_t row = row0 + rr;
    if (lane == 0 && row < d) {
      const double delta = a[rr] - b[rr];
      const double bias = (b_d ? load_any(b_d, b_dtype, row) : 0.) + delta;
      delta_rows[row] = delta;
      wmu_rows[row] = a[rr];
      bias_f64[row] = bias;
      if (bias_out) store_any(bias_out, out_dtype, row, bias);
    }
  }
}

struct ColSumWs {
  double* part;   // [ceil(n_tokens / COL_SUM_CHUNK)][n]: the partial row of every chunk
  size_t bytes;
};
static ColSumWs col_sum_layout(void* ws, int64_t n_tokens, int64_t n) {
  Carve c(ws);
  ColSumWs w;
  w.part = c.take<double>((size_t)ceil_div(n_tokens, COL_SUM_CHUNK) * (size_t)n);
  w.bytes = c.off;
  return w;
}

struct InterceptWs {
  double *delta_rows, *wmu_rows;   // [d] each
  size_t bytes;
};
static InterceptWs intercept_layout(void* ws, int64_t d) {
  Carve c(ws);
  InterceptWs w;
  w.delta_rows = c.take<double>((size_t)d);
  w.wmu_rows = c.take<double>((size_t)d);
  w.bytes = c.off;
  return w;
}

}  // namespace mdg

extern "C" size_t mdg_col_sum_ws_bytes(int64_t n_tokens, int64_t n) {
  if (n_tokens <= 0 || n <= 0) return 0;
  return col_sum_layout(nullptr, n_tokens, n).bytes;
}

extern "C" int mdg_col_sum_accum(const void* x, int dtype, int64_t n_tokens, int64_t n, int64_t ld, int relu, double* sum, void* ws,
                                 size_t ws_bytes, void* stream) {
  MDG_CHECK_ARG(known_dtype(dtype), "mdg_col_sum_accum: unsupported dtype %d", dtype);
  MDG_CHECK_ARG(x && sum, "mdg_col_sum_accum: null pointer");
  MDG_CHECK_ARG(n_tokens > 0 && n > 0 && ld >= n, "mdg_col_sum_accum: bad sizes (tokens=%lld n=%lld ld=%lld)", (long long)n_tokens,
                (long long)n, (long long)ld);
  MDG_CHECK_ARG((uintptr_t)x % dtype_size(dtype) == 0 && (uintptr_t)sum % 8 == 0 && (uintptr_t)ws % 8 == 0,
                "mdg_col_sum_accum: x, sum and ws must be aligned to their elements");
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_col_sum_ws_bytes(n_tokens, n), "mdg_col_sum_accum: workspace %zu < required %zu", ws_bytes,
                mdg_col_sum_ws_bytes(n_tokens, n));
  MDG_CHECK_ARG(ceil_div(n_tokens, COL_SUM_CHUNK) < (1ll << 31) && ceil_div(n, 256) < 65536, "mdg_col_sum_accum: grid too large");
  MDG_CLEAR();
  hipStream_t st = (hipStream_t)stream;
  double* part = col_sum_layout(ws, n_tokens, n).part;
  switch (dtype) {
    case MDG_BF16: return col_sum_launch<MDG_BF16>(x, n_tokens, n, ld, relu, sum, part, st);
    case MDG_F16: return col_sum_launch<MDG_F16>(x, n_tokens, n, ld, relu, sum, part, st);
    case MDG_F32: return col_sum_launch<MDG_F32>(x, n_tokens, n, ld, relu, sum, part, st);
    default: return col_sum_launch<MDG_F64>(x, n_tokens, n, ld, relu, sum, part, st);
  }
}

extern "C" int mdg_cov_center(const double* C, int64_t n, int64_t ldc, const double* mu, double* S, int64_t lds, void* stream) {
  MDG_CHECK_ARG(C && mu && S, "mdg_cov_center: null pointer");
  MDG_CHECK_ARG(n > 0 && ldc >= n && lds >= n, "mdg_cov_center: bad sizes (n=%lld ldc=%lld lds=%lld)", (long long)n, (long long)ldc,
                (long long)lds);
  const int64_t nb = ceil_div(n, CENTER_TILE);
  MDG_CHECK_ARG(nb < 65536, "mdg_cov_center: n = %lld too large", (long long)n);
  MDG_CLEAR();
  hipLaunchKernelGGL(cov_center_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, C, n, ldc, mu, S, lds);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" size_t mdg_nystrom_intercept_ws_bytes(int64_t d) { return d > 0 ? intercept_layout(nullptr, d).bytes : 0; }

extern "C" int mdg_nystrom_intercept(const void* Wd, int64_t d, int64_t n, int64_t ld_wd, int w_dtype, const void* down_hat, int64_t r,
                                     int64_t ld_down, const int64_t* idx, const double* mu, const void* b_d, int b_dtype,
                                     void* bias_out, int out_dtype, double* bias_f64, double* norms, void* ws, size_t ws_bytes,
                                     void* stream) {
  MDG_CHECK_ARG(Wd && down_hat && idx && mu && bias_f64 && norms, "mdg_nystrom_intercept: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_nystrom_intercept: W_d must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG((!b_d || known_dtype(b_dtype)) && (!bias_out || known_dtype(out_dtype)), "mdg_nystrom_intercept: unsupported bias dtype");
  MDG_CHECK_ARG(d > 0 && n > 0 && r > 0 && r <= n && ld_wd >= n && ld_down >= r,
                "mdg_nystrom_intercept: bad sizes (d=%lld n=%lld r=%lld ld_wd=%lld ld_down=%lld)", (long long)d, (long long)n, (long long)r,
                (long long)ld_wd, (long long)ld_down);
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_nystrom_intercept_ws_bytes(d) && (uintptr_t)ws % 8 == 0,
                "mdg_nystrom_intercept: workspace %zu < required %zu", ws_bytes, mdg_nystrom_intercept_ws_bytes(d));
  MDG_CHECK_ARG(ceil_div(d, RD_ROWS) < (1ll << 31) && n < (1ll << 31), "mdg_nystrom_intercept: too many rows or columns");
  MDG_CLEAR();
  hipStream_t st = (hipStream_t)stream;
  const InterceptWs w = intercept_layout(ws, d);
  double *delta_rows = w.delta_rows, *wmu_rows = w.wmu_rows;
  const int vec_w = w_dtype == MDG_BF16 && (uintptr_t)Wd % 16 == 0 && ld_wd % 8 == 0;
  const int vec_d = (uintptr_t)down_hat % 16 == 0 && ld_down % 8 == 0;
  const dim3 grid((unsigned)ceil_div(d, RD_ROWS));
  if (w_dtype == MDG_BF16)
    hipLaunchKernelGGL(intercept_rows_kernel<MDG_BF16>, grid, dim3(256), 0, st, Wd, ld_wd, d, n, down_hat, ld_down, r, idx, mu, vec_w,
                       vec_d, b_d, b_dtype, bias_out, out_dtype, bias_f64, delta_rows, wmu_rows);
  else
    hipLaunchKernelGGL(intercept_rows_kernel<MDG_F64>, grid, dim3(256), 0, st, Wd, ld_wd, d, n, down_hat, ld_down, r, idx, mu, vec_w,
                       vec_d, b_d, b_dtype, bias_out, out_dtype, bias_f64, delta_rows, wmu_rows);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_norms_kernel, dim3(1), dim3(256), 0, st, delta_rows, wmu_rows, d, norms);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
