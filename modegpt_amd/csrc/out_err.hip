// The realised output error of a stored down projection on the calibration statistic (compress_mlp.py:52-62 computes the refit and
// reports nothing about what it lost).  With U [d, n] the residual weights -- column j of U is W_d[:, j] where j is not kept and
// W_d[:, j] - down[:, pos(j)] where j = idx[pos(j)] -- the call gives one quadratic form per output channel,
//   e_k = u_k C u_k^T = sum_i C_ii u_ki^2 + 2 sum_{i > j} C_ij u_ki u_kj ,      unorm2_k = ||u_k||^2 ,
// read from the LOWER triangle of C alone.  sum_k e_k is the E_D of the sandwich in DESIGN.md section 7 ("The error-versus-rank
// curve"): E_D + eps ||U||^2 - eps ||W_S||^2 <= curve[r] <= E_D + eps ||U||^2 -- here for ANY down tensor, the bf16 artefact included.
//
// Tile scheme, epilogue and reduction: quad_form.hpp (a workgroup = a 128-row block of U x one tile column of C; U is formed in the
// A-operand staging, a bf16 - bf16 difference being exact in fp64; `pos` [n] int32 is the inverse index map, -1: not kept).
//
// Work: d n (n + 1) flop (half of the full product U C), 0.84 TFLOP at n = 14336, d = 4096.  Workspace: the inverse map + two planes
// of partials, 4 n + 16 d ceil(n / 128) bytes (7.4 MB there; the route through a materialised U, a mirrored C and U C needs 2.6 GB).
//
// Non-finite input: a NaN in row k of W_d or down stays in row k of U, of P and of the sums -- e[k] alone is NaN; a NaN in the lower
// triangle of C reaches every row.  Out-of-range rows / columns are never loaded (selects, not multiplications by zero).
#include "common.hpp"
#include "quad_form.hpp"

namespace mdg {

// pos[j] = the HIGHEST position p with clamp(idx[p]) == j, or -1: every column scans the whole index list (n r comparisons, 1.4e8
// at Llama-3-8B shapes -- microseconds) so that a repeated index resolves the same way in every run without an atomic.
__global__ __launch_bounds__(256) void oe_pos_kernel(const int64_t* idx, int64_t r, int64_t n, int* pos) {
  __shared__ int64_t chunk[256];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int best = -1;
  for (int64_t p0 = 0; p0 < r; p0 += 256) {
    const int64_t p = p0 + threadIdx.x;
    int64_t v = -1;
    if (p < r) {
      v = idx[p];
      v = v < 0 ? 0 : (v >= n ? n - 1 : v);      // memory safety only, as mdg_nystrom_rank_curve clamps its order
    }
    __syncthreads();                             // (the previous chunk has been read by everyone)
    chunk[threadIdx.x] = v;
    __syncthreads();
    const int m = (int)(r - p0 < 256 ? r - p0 : 256);
    for (int q = 0; q < m; q++)
      if (chunk[q] == j) best = (int)(p0 + q);
  }
  if (j < n) pos[j] = best;
}

struct OutErrArgs {
  const double* C;
  int64_t n, ldc;
  const void* W;
  int64_t d, ldw;
  const int* pos;      // nullptr: nothing is subtracted (U = W_d)
  const void* down;
  int64_t sd_row, sd_col;
  double* part_e;      // [tiles_n][d]
  double* part_u;      // [tiles_n][d]
  int tiles_d;
};

// row k of U: W_d[k, col], minus down[k, pos[col]] where the column is kept (pos looked up once per column)
template <int WDT, int DDT>
struct OutErrRows {
  typedef int64_t Idx;
  typedef int Col;
  const OutErrArgs g;   // (a copy, as in vo_err.hip: through a reference the kernel compiles to more code)
  __device__ __forceinline__ Col prepare(int64_t col) const { return g.pos ? g.pos[col] : -1; }
  __device__ __forceinline__ double at(int64_t row, int64_t col, Col p) const {
    double u = load_f64<WDT>(g.W, row * g.ldw + col);
    if (p >= 0) u -= load_f64<DDT>(g.down, row * g.sd_row + (int64_t)p * g.sd_col);
    return u;
  }
};

template <int WDT, int DDT>
__global__ __launch_bounds__(256, 2) void out_err_kernel(OutErrArgs g) {
  __shared__ double lds[4 * PANEL];
  const int tid = threadIdx.x;
  const int bj = blockIdx.x / g.tiles_d, bi = blockIdx.x % g.tiles_d;     // tile column of C (longest first), row block of U
  const int64_t i0 = (int64_t)bi * TILE;
  double se, su;
  quad_form_tile_column<true>(OutErrRows<WDT, DDT>{g}, g.C, g.ldc, g.n, g.d, i0, (int64_t)bj * TILE, lds, se, su);
  if (tid < TILE && i0 + tid < g.d) {
    const int64_t o = (int64_t)bj * g.d + i0 + tid;
    g.part_e[o] = se;
    g.part_u[o] = su;
  }
}

// pos [n] (int32, padded to 16 bytes); the partials of e and of unorm2, [ceil(n / 128)][d] doubles each, part_u right behind
// part_e: the two plane sets of quad_reduce_kernel
struct OutErrWs {
  int* pos;
  double *part_e, *part_u;
  size_t bytes;
};
static OutErrWs out_err_layout(void* ws, int64_t n, int64_t d) {
  const size_t plane = (size_t)ceil_div(n, TILE) * (size_t)d;
  Carve c(ws);
  OutErrWs w;
  w.pos = c.take<int>((size_t)n);
  w.part_e = c.take<double>(plane, 16);
  w.part_u = c.take<double>(plane);
  w.bytes = c.off;
  return w;
}

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_mlp_output_error_ws_bytes(int64_t n, int64_t d) {
  if (n <= 0 || d <= 0) return 0;
  return out_err_layout(nullptr, n, d).bytes;
}

extern "C" int mdg_mlp_output_error(const double* C, int64_t n, int64_t ldc, const void* Wd, int64_t d, int64_t ld_wd, int w_dtype,
                                    const int64_t* idx, int64_t r, const void* down, int64_t sd_row, int64_t sd_col, int down_dtype,
                                    double* e, double* unorm2, void* ws, size_t ws_bytes, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(C && Wd && e, "mdg_mlp_output_error: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_mlp_output_error: W_d must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n > 0 && d > 0 && ldc >= n && ld_wd >= n, "mdg_mlp_output_error: bad sizes (n=%lld d=%lld ldc=%lld ld_wd=%lld)",
                (long long)n, (long long)d, (long long)ldc, (long long)ld_wd);
  MDG_CHECK_ARG(n <= INT32_MAX, "mdg_mlp_output_error: n = %lld is beyond the limit of 2^31 - 1 columns", (long long)n);
  MDG_CHECK_ARG(r >= 0 && r <= n, "mdg_mlp_output_error: rank %lld outside 0 .. n = %lld", (long long)r, (long long)n);
  const bool sub = down != nullptr && r > 0;
  MDG_CHECK_ARG(r == 0 || (down && idx), "mdg_mlp_output_error: rank %lld needs down and idx", (long long)r);
  MDG_CHECK_ARG(!sub || down_dtype == MDG_BF16 || down_dtype == MDG_F64, "mdg_mlp_output_error: down must be bf16 or f64 (got %d)",
                down_dtype);
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_mlp_output_error_ws_bytes(n, d), "mdg_mlp_output_error: workspace %zu < required %zu", ws_bytes,
                mdg_mlp_output_error_ws_bytes(n, d));
  const int64_t tiles_n = ceil_div(n, TILE), tiles_d = ceil_div(d, TILE);
  MDG_CHECK_ARG(tiles_n * tiles_d < (1ll << 31), "mdg_mlp_output_error: grid too large");
  hipStream_t st = (hipStream_t)stream;
  const OutErrWs w = out_err_layout(ws, n, d);
  int* pos = w.pos;
  double *part_e = w.part_e, *part_u = w.part_u;
  if (sub) {
    hipLaunchKernelGGL(oe_pos_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, idx, r, n, pos);
    MDG_LAUNCH_CHECK();
  }
  OutErrArgs g;
  g.C = C; g.n = n; g.ldc = ldc;
  g.W = Wd; g.d = d; g.ldw = ld_wd;
  g.pos = sub ? pos : nullptr;
  g.down = down; g.sd_row = sd_row; g.sd_col = sd_col;
  g.part_e = part_e; g.part_u = part_u;
  g.tiles_d = (int)tiles_d;
  const dim3 grid((unsigned)(tiles_n * tiles_d));
  const bool d64 = sub && down_dtype == MDG_F64;
  if (w_dtype == MDG_BF16 && !d64) hipLaunchKernelGGL((out_err_kernel<MDG_BF16, MDG_BF16>), grid, dim3(256), 0, st, g);
  else if (w_dtype == MDG_BF16) hipLaunchKernelGGL((out_err_kernel<MDG_BF16, MDG_F64>), grid, dim3(256), 0, st, g);
  else if (!d64) hipLaunchKernelGGL((out_err_kernel<MDG_F64, MDG_BF16>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((out_err_kernel<MDG_F64, MDG_F64>), grid, dim3(256), 0, st, g);
  MDG_LAUNCH_CHECK();
  // (part_u starts tiles_n * d behind part_e: the two plane sets of quad_reduce_kernel)
  hipLaunchKernelGGL(quad_reduce_kernel, dim3((unsigned)ceil_div(d, 256)), dim3(256), 0, st, part_e, d, (int)tiles_n, e, unorm2);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
