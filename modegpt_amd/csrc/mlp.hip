// Nystrom refit of down_proj (compress_mlp.py:52-62,97):
//   W_d' = (C[idx,idx] + eps I)^-1  C[idx,:]  W_d^T      -> stored transposed as [d, r] bf16
// With k = idx, k' its complement and M = C_kk + eps I:  M^-1 C_kk = I - eps M^-1, so
//   W_d' = W_d[:,k]^T + M^-1 ( C[k,k'] W_d[:,k']^T - eps W_d[:,k]^T )
// the selected columns' share is the weights themselves and only the n - r unselected columns are multiplied:
// gather -> complement list -> compaction of C[k,k'] and W_d[:,k'] -> GEMM onto the -eps W right-hand side
// (beside the blocked Cholesky) -> blocked substitution -> add W_d[:,k]^T, transpose-cast.
#include "common.hpp"

namespace mdg {
int gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i, int64_t sa_k,
             const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k, int64_t sb_j, double beta, void* C,
             int c_dtype, int64_t ldc, int64_t batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int flags,
             hipStream_t st);
int potrf_lower(double* A, int64_t n, int64_t lda, double* inv_diag, hipStream_t st);
int potrs_lower(const double* L, int64_t n, int64_t ldl, const double* inv_diag, double* X, int64_t nrhs, int64_t ldx,
                const PotrsWs& ws, hipStream_t st);
int copy_lower(const double* src, int64_t ld_src, const int64_t* idx, double* dst, int64_t ldd, int64_t n,
               double ridge, hipStream_t st);
}  // namespace mdg

using namespace mdg;

// Row pitch of C_kk in the workspace: r rounded up to 16 doubles.  With pitch r an odd rank (10035 of 14336 at 30 %) leaves every
// second row off a 16-byte boundary, and every GEMM of the factorisation and the substitution on the element-wise staging path --
// potrf_lower 15.1 -> 14.3 ms, potrs_lower 17.8 -> 16.9 ms at r = 10035 (scripts/probes/decomp_phases.py).
static int64_t ckk_pitch(int64_t r) { return (r + 15) / 16 * 16; }
// The compacted operands' row pitch: n - r rounded up to a whole number of GEMM stages (BK = 16 elements: also a multiple of the
// 16-byte staging unit of either dtype), so that every tile of the product takes the vector staging path.
static int64_t comp_pitch(int64_t n, int64_t r) { return (n - r + BK - 1) / BK * BK; }
// The solve part, doubles: C_kk [r][ckk_pitch] | inverted diagonal blocks | X [r][d] | the substitution's workspace.  Then the
// tail, each block from a 16-byte boundary: C[k,k'] fp64 [r][Kp] | W_d[:,k'] [d][Kp] (sized for fp64) | k' int64 [n - r] | marks
// int32 [n].  The tail starts on a 16-byte ADDRESS (the vector staging path of the product reads it), while ws itself need only
// hold doubles: NYS_ALIGN_SLACK bytes are reserved for what moving the tail up to that address can cost.  For a 16-byte aligned
// ws the tail sits at the solve part's size rounded up to 16 and the slack lies unused behind the marks.
constexpr size_t NYS_ALIGN_SLACK = 16;
struct NystromWs {
  double *Ckk, *inv, *X;
  PotrsWs solve;
  double* Cbar;
  void* Wbar;
  int64_t* comp;
  int* marks;
  size_t bytes;
};
static NystromWs nystrom_layout(void* ws, int64_t n, int64_t r, int64_t d) {
  const size_t Kp = (size_t)comp_pitch(n, r);
  NystromWs w;
  Carve c(ws);
  w.Ckk = c.take<double>((size_t)r * ckk_pitch(r));
  w.inv = c.take<double>(mdg_potrf_inv_diag_elems(r));
  w.X = c.take<double>((size_t)r * d);
  w.solve = potrs_layout(c, r, d);
  Carve t(ws ? (void*)align_up((size_t)((uintptr_t)ws + c.off), 16) : nullptr);
  w.Cbar = t.take<double>((size_t)r * Kp);
  w.Wbar = t.take<double>((size_t)d * Kp, 16);
  w.comp = t.take<int64_t>((size_t)(n - r), 16);
  w.marks = t.take<int>((size_t)n, 16);
  w.bytes = align_up(c.off, 16) + NYS_ALIGN_SLACK + align_up(t.off, 16);
  return w;
}
extern "C" size_t mdg_nystrom_down_ws_bytes(int64_t n, int64_t r, int64_t d) { return nystrom_layout(nullptr, n, r, d).bytes; }

namespace mdg {

__device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// comp[0 .. K) = the indices of 0 .. n-1 that idx[0 .. r) does not name, ascending (K = n - r when idx is distinct and in range;
// more unnamed indices than K: the first K).  One workgroup: clear the marks, mark, ordered compaction by a scan of per-thread
// counts -- no atomics, the list does not depend on the order of idx.  Entries of idx outside 0 .. n-1 mark nothing.
__global__ __launch_bounds__(1024) void complement_kernel(const int64_t* idx, int64_t r, int64_t n, int64_t K, int* marks, int64_t* comp) {
  __shared__ int sums[1024];
  const int tid = threadIdx.x;
  for (int64_t i = tid; i < n; i += 1024) marks[i] = 0;
  __syncthreads();
  for (int64_t p = tid; p < r; p += 1024) {
    const int64_t i = idx[p];
    if (i >= 0 && i < n) marks[i] = 1;
  }
  __syncthreads();
  const int64_t per = (n + 1023) / 1024;
  const int64_t b = min((int64_t)tid * per, n), e = min(b + per, n);
  int c = 0;
  for (int64_t i = b; i < e; i++) c += marks[i] ? 0 : 1;
  sums[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    int v = tid >= o ? sums[tid - o] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  int64_t pos = sums[tid] - c;
  for (int64_t i = b; i < e && pos < K; i++)
    if (!marks[i]) comp[pos++] = i;
}

// dst[p][q] = src[rows[p]][comp[q]] for q < K, 0 for K <= q < Kp (rows == nullptr: row p).  One workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void compact_cols_kernel(const T* src, int64_t ld_src, const int64_t* rows, int64_t n, const int64_t* comp,
                                                           int64_t K, int64_t Kp, T* dst) {
  const int64_t p = blockIdx.x;
  const T* s = src + (rows ? clamp_index(rows[p], n) : p) * ld_src;
  T* o = dst + p * Kp;
  for (int64_t q = threadIdx.x; q < Kp; q += 256) o[q] = q < K ? s[comp[q]] : (T)0;
}

// X[p][j] = -eps_p W_d[j][idx[p]], eps_p = fl(c_pp + eps) - c_pp: what copy_lower really added to that diagonal entry.
// 32 x 32 tiles: W_d is read along p (neighbouring selected columns), X written along j.
template <int DT>
__global__ __launch_bounds__(256) void ridge_rhs_kernel(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd,
                                                        int64_t d, int64_t ld_wd, double eps, double* X) {
  __shared__ double t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t p0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  const int64_t col = p0 + tx < r ? clamp_index(idx[p0 + tx], n) : -1;
  double eps_p = 0.;
  if (col >= 0) {
    const double c = C[col * ldc + col];
    eps_p = (c + eps) - c;
  }
  for (int j = ty; j < 32; j += 8)
    if (col >= 0 && j0 + j < d) t[j][tx] = -(eps_p * load_f64<DT>(Wd, (j0 + j) * ld_wd + col));
  __syncthreads();
  for (int p = ty; p < 32; p += 8)
    if (p0 + p < r && j0 + tx < d) X[(p0 + p) * d + j0 + tx] = t[tx][p];
}

// X[p][j] <- W_d[j][idx[p]] + X[p][j] (the weight widened exactly: one rounding per entry), out[j][p] = bf16 of the same value,
// f64_out[p][j] (optional) the value itself.
template <int DT>
__global__ __launch_bounds__(256) void add_cast_transpose_kernel(const double* X, const int64_t* idx, int64_t r, int64_t n, const void* Wd,
                                                                 int64_t d, int64_t ld_wd, bf16_t* out, int64_t ld_out, double* f64_out) {
  __shared__ double t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t p0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  for (int p = ty; p < 32; p += 8)
    t[p][tx] = (p0 + p < r && j0 + tx < d) ? X[(p0 + p) * d + j0 + tx] : 0.;
  __syncthreads();
  const int64_t col = p0 + tx < r ? clamp_index(idx[p0 + tx], n) : -1;
  for (int j = ty; j < 32; j += 8)
    if (col >= 0 && j0 + j < d) {
      const double v = load_f64<DT>(Wd, (j0 + j) * ld_wd + col) + t[tx][j];
      out[(j0 + j) * ld_out + p0 + tx] = f64_to_bf16(v);
      t[tx][j] = v;
    }
  if (!f64_out) return;
  __syncthreads();
  for (int p = ty; p < 32; p += 8)
    if (p0 + p < r && j0 + tx < d) f64_out[(p0 + p) * d + j0 + tx] = t[p][tx];
}

}  // namespace mdg

static int nystrom_down(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd, int64_t d, int64_t ld_wd,
                        int w_dtype, double eps, void* down_out, int64_t ld_out, double* down_f64, void* ws, size_t ws_bytes,
                        void* side_stream, void* ev_fork, void* ev_join, void* stream);

extern "C" int mdg_nystrom_down(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd,
                                int64_t d, int64_t ld_wd, int w_dtype, double eps, void* down_out, int64_t ld_out,
                                double* down_f64, void* ws, size_t ws_bytes, void* stream) {
  return nystrom_down(C, n, ldc, idx, r, Wd, d, ld_wd, w_dtype, eps, down_out, ld_out, down_f64, ws, ws_bytes, nullptr, nullptr, nullptr, stream);
}

extern "C" int mdg_nystrom_down_overlapped(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd,
                                           int64_t d, int64_t ld_wd, int w_dtype, double eps, void* down_out, int64_t ld_out,
                                           double* down_f64, void* ws, size_t ws_bytes, void* side_stream, void* ev_fork, void* ev_join,
                                           void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(side_stream && ev_fork && ev_join && side_stream != stream,
                "mdg_nystrom_down_overlapped: needs a second stream and two events of the caller's");
  return nystrom_down(C, n, ldc, idx, r, Wd, d, ld_wd, w_dtype, eps, down_out, ld_out, down_f64, ws, ws_bytes, side_stream, ev_fork, ev_join, stream);
}

static int nystrom_down(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd, int64_t d, int64_t ld_wd,
                        int w_dtype, double eps, void* down_out, int64_t ld_out, double* down_f64, void* ws, size_t ws_bytes,
                        void* side_stream, void* ev_fork, void* ev_join, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(C && idx && Wd && down_out, "mdg_nystrom_down: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_nystrom_down: W_d must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n > 0 && r > 0 && r <= n && d > 0 && ldc >= n && ld_wd >= n && ld_out >= r,
                "mdg_nystrom_down: bad sizes (n=%lld r=%lld d=%lld)", (long long)n, (long long)r, (long long)d);
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_nystrom_down_ws_bytes(n, r, d), "mdg_nystrom_down: workspace %zu < required %zu",
                ws_bytes, mdg_nystrom_down_ws_bytes(n, r, d));
  hipStream_t st = (hipStream_t)stream;
  const NystromWs w = nystrom_layout(ws, n, r, d);
  double *Ckk = w.Ckk, *inv = w.inv, *X = w.X, *Cbar = w.Cbar;
  void* Wbar = w.Wbar;
  int64_t* comp = w.comp;
  int* marks = w.marks;
  const int64_t ldk = ckk_pitch(r);
  const int64_t K = n - r, Kp = comp_pitch(n, r);
  const bool w_bf16 = w_dtype == MDG_BF16;
  dim3 tiles((unsigned)ceil_div(d, 32), (unsigned)ceil_div(r, 32));
  MDG_CHECK_ARG(tiles.y < 65536 && d < (1ll << 31), "mdg_nystrom_down: too many rows");
  // C_kk + eps I  (lower)                                           compress_mlp.py:52,56
  MDG_TRY(copy_lower(C, ldc, idx, Ckk, ldk, r, eps, st));
  // rhs = C[k,k'] W_d[:,k']^T - eps W_d[:,k]^T  -> [r, d]           (compress_mlp.py:54 less what the solve would cancel)
  // (with a second stream: beside the factorisation of C_kk, which does not need it -- the chain of 79 diagonal-block steps
  // leaves most of the chip idle between its GEMMs)
  hipStream_t cross_st = st;
  if (side_stream) {
    cross_st = (hipStream_t)side_stream;
    MDG_HIP(hipEventRecord((hipEvent_t)ev_fork, st));
    MDG_HIP(hipStreamWaitEvent(cross_st, (hipEvent_t)ev_fork, 0));
  }
  if (w_bf16) hipLaunchKernelGGL(ridge_rhs_kernel<MDG_BF16>, tiles, dim3(256), 0, cross_st, C, n, ldc, idx, r, Wd, d, ld_wd, eps, X);
  else hipLaunchKernelGGL(ridge_rhs_kernel<MDG_F64>, tiles, dim3(256), 0, cross_st, C, n, ldc, idx, r, Wd, d, ld_wd, eps, X);
  MDG_LAUNCH_CHECK();
  if (K > 0) {
    hipLaunchKernelGGL(complement_kernel, dim3(1), dim3(1024), 0, cross_st, idx, r, n, K, marks, comp);
    MDG_LAUNCH_CHECK();
    hipLaunchKernelGGL(compact_cols_kernel<double>, dim3((unsigned)r), dim3(256), 0, cross_st, C, ldc, idx, n, comp, K, Kp, Cbar);
    MDG_LAUNCH_CHECK();
    if (w_bf16)
      hipLaunchKernelGGL(compact_cols_kernel<bf16_t>, dim3((unsigned)d), dim3(256), 0, cross_st, (const bf16_t*)Wd, ld_wd, (const int64_t*)nullptr,
                         n, comp, K, Kp, (bf16_t*)Wbar);
    else
      hipLaunchKernelGGL(compact_cols_kernel<double>, dim3((unsigned)d), dim3(256), 0, cross_st, (const double*)Wd, ld_wd, (const int64_t*)nullptr,
                         n, comp, K, Kp, (double*)Wbar);
    MDG_LAUNCH_CHECK();
    MDG_TRY(gemm_f64(r, d, Kp, 1.0, Cbar, MDG_F64, Kp, 1, nullptr, Wbar, w_dtype, 1, Kp, 1.0, X, MDG_F64, d, 1, 0, 0, 0, 0, cross_st));
  }
  if (side_stream) MDG_HIP(hipEventRecord((hipEvent_t)ev_join, cross_st));
  const int rc_potrf = potrf_lower(Ckk, r, ldk, inv, st);         // compress_mlp.py:56
  if (side_stream) MDG_HIP(hipStreamWaitEvent(st, (hipEvent_t)ev_join, 0));   // (also on failure: the workspace is the caller's to free)
  if (rc_potrf != MDG_OK) return rc_potrf;
  MDG_TRY(potrs_lower(Ckk, r, ldk, inv, X, d, d, w.solve, st));  // compress_mlp.py:57
  // W_d[:,k]^T + X: [r, d] fp64 -> down_f64, and [d, r] bf16       compress_mlp.py:61,97
  if (w_bf16)
    hipLaunchKernelGGL(add_cast_transpose_kernel<MDG_BF16>, tiles, dim3(256), 0, st, X, idx, r, n, Wd, d, ld_wd, (bf16_t*)down_out, ld_out, down_f64);
  else
    hipLaunchKernelGGL(add_cast_transpose_kernel<MDG_F64>, tiles, dim3(256), 0, st, X, idx, r, n, Wd, d, ld_wd, (bf16_t*)down_out, ld_out, down_f64);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
