// The realised output error of a stored down projection on the calibration statistic (compress_mlp.py:52-62 computes the refit and
// reports nothing about what it lost).  With U [d, n] the residual weights -- column j of U is W_d[:, j] where j is not kept and
// W_d[:, j] - down[:, pos(j)] where j = idx[pos(j)] -- the call gives one quadratic form per output channel,
//   e_k = u_k C u_k^T = sum_i C_ii u_ki^2 + 2 sum_{i > j} C_ij u_ki u_kj ,      unorm2_k = ||u_k||^2 ,
// read from the LOWER triangle of C alone.  sum_k e_k is the E_D of the sandwich in DESIGN.md section 7 ("The error-versus-rank
// curve"): E_D + eps ||U||^2 - eps ||W_S||^2 <= curve[r] <= E_D + eps ||U||^2 -- here for ANY down tensor, the bf16 artefact included.
//
// Tile scheme (the shared 128 x 128 / 4-wave / LDS-fp64-panel core of common.hpp).  A workgroup owns a 128-row block of U and one
// 128-wide tile COLUMN J of C and walks the tiles (I, J), I = J .. T-1, of the lower triangle down that column:
//   P[128, 128] = sum_{I >= J} U[:, I] C[I, J]     (v_mfma_f64_16x16x4_f64; the diagonal tile C_JJ masked to its STRICT lower part
//                                                   while staging, so what lies on or above the diagonal of C is never loaded)
// -- one accumulator for the whole column, so the epilogue runs once per workgroup and the partial sums are d * T numbers, not
// d * T (T + 1) / 2.  U is formed in the A-operand staging: the weight and the down entry are widened exactly to fp64 and subtracted
// there (a bf16 - bf16 difference is exact in fp64); `pos` [n] int32 is the inverse index map (-1: not kept).  Epilogue, per entry
// (k, j) of the tile:  u_kj (2 P_kj + C_jj u_kj)  -- the factor 2 on the strict lower part, the diagonal term without it -- and
// u_kj^2, summed along the tile's 128 columns (4 in the lane, 16 lanes by shuffles in a fixed tree, the two wave columns through
// LDS).  P is never written to memory.  A second small kernel adds each row's T partials in ascending tile order.  No atomics:
// two runs are bit-identical.  Tile columns are handed out longest first (J ascending): T - J tiles each.
//
// Work: d n (n + 1) flop (half of the full product U C), 0.84 TFLOP at n = 14336, d = 4096.  Workspace: the inverse map + two planes
// of partials, 4 n + 16 d ceil(n / 128) bytes (7.4 MB there; the route through a materialised U, a mirrored C and U C needs 2.6 GB).
//
// Non-finite input: a NaN in row k of W_d or down stays in row k of U, of P and of the sums -- e[k] alone is NaN; a NaN in the lower
// triangle of C reaches every row.  Out-of-range rows / columns are never loaded (selects, not multiplications by zero).
#include "common.hpp"

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

template <int WDT, int DDT>
__device__ __forceinline__ double oe_u(const OutErrArgs& g, int64_t row, int64_t col, int p) {
  double u = load_f64<WDT>(g.W, row * g.ldw + col);
  if (p >= 0) u -= load_f64<DDT>(g.down, row * g.sd_row + (int64_t)p * g.sd_col);
  return u;
}

template <int WDT, int DDT>
__global__ __launch_bounds__(256, 2) void out_err_kernel(OutErrArgs g) {
  __shared__ double lds[4 * PANEL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bj = blockIdx.x / g.tiles_d, bi = blockIdx.x % g.tiles_d;     // tile column of C (longest first), row block of U
  const int64_t i0 = (int64_t)bi * TILE, j0 = (int64_t)bj * TILE;
  const int64_t n_stage = (g.n - j0 + BK - 1) / BK;                       // k runs over the columns j0 .. n-1 of U (>= 1 stage)

  // A panel: element (x = row of U, k); W_d is k-contiguous, so consecutive threads walk k: a thread keeps one k and 8 rows
  const int ak = tid & 15, ax = tid >> 4;
  // B panel: element (k = row of C, y = column of C); C is y-contiguous: a thread keeps one column and 8 rows
  const int bk = tid >> 7, by = tid & 127;
  const int64_t gcb = j0 + by;
  double rg[8];  // one panel's prefetch at a time: A rides under the first half of a stage, B under the second (gemm.hip)

  auto load_a = [&](int64_t k0) {
    const int64_t col = k0 + ak;
    const bool ok = col < g.n;
    const int p = (ok && g.pos) ? g.pos[col] : -1;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int64_t row = i0 + ax + 16 * q;
      rg[q] = (ok && row < g.d) ? oe_u<WDT, DDT>(g, row, col, p) : 0.;
    }
  };
  auto store_a = [&](double* panel) {
#pragma unroll
    for (int q = 0; q < 8; q++) panel[ak * PITCH + ax + 16 * q] = rg[q];
  };
  auto load_b = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int64_t gr = k0 + bk + 2 * q;
      rg[q] = (gr < g.n && gr > gcb) ? g.C[gr * g.ldc + gcb] : 0.;       // strictly below the diagonal only (gcb < gr < n)
    }
  };
  auto store_b = [&](double* panel) {
#pragma unroll
    for (int q = 0; q < 8; q++) panel[(bk + 2 * q) * PITCH + by] = rg[q];
  };

  Acc acc;
  acc_zero(acc);
  load_a(j0);
  store_a(lds);
  load_b(j0);
  store_b(lds + 2 * PANEL);
  __syncthreads();
  for (int64_t s = 0; s < n_stage; s++) {
    const int cur = (int)(s & 1);
    const bool more = s + 1 < n_stage;
    const int64_t k0 = j0 + (s + 1) * BK;
    const double* As = lds + cur * PANEL;
    const double* Bs = lds + (2 + cur) * PANEL;
    if (more) load_a(k0);
    mma_steps<0, BK / 8>(As, Bs, wr, wc, lane, acc);
    if (more) {
      store_a(lds + (cur ^ 1) * PANEL);
      load_b(k0);
    }
    mma_steps<BK / 8, BK / 4>(As, Bs, wr, wc, lane, acc);
    if (more) store_b(lds + (2 + (cur ^ 1)) * PANEL);
    __syncthreads();
  }

  // epilogue: sum_j u_kj (2 P_kj + C_jj u_kj) and sum_j u_kj^2 over the tile's columns
  double* red_e = lds;                 // [2][TILE]  (the panels are dead: the loop ended with a barrier)
  double* red_u = lds + 2 * TILE;      // [2][TILE]
  const int64_t gc0 = j0 + acc_col(wc, lane, 0);
  bool cok[4];
  int pj[4];
  double cd[4];
#pragma unroll
  for (int sb = 0; sb < 4; sb++) {
    const int64_t col = gc0 + sb;
    cok[sb] = col < g.n;
    pj[sb] = (cok[sb] && g.pos) ? g.pos[col] : -1;
    cd[sb] = cok[sb] ? g.C[col * g.ldc + col] : 0.;
  }
#pragma unroll
  for (int sa = 0; sa < 4; sa++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int lr = acc_row(wr, lane, sa, reg);
      const int64_t row = i0 + lr;
      double se = 0., su = 0.;
      if (row < g.d) {
#pragma unroll
        for (int sb = 0; sb < 4; sb++) {
          if (!cok[sb]) continue;
          const double u = oe_u<WDT, DDT>(g, row, gc0 + sb, pj[sb]);
          se += u * (2. * acc.v[sa][sb][reg] + cd[sb] * u);
          su += u * u;
        }
      }
      // the 16 lanes that share (lane >> 4) hold this row's other columns: a fixed butterfly, the same value in all of them
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        se += __shfl_xor(se, m);
        su += __shfl_xor(su, m);
      }
      if ((lane & 15) == 0) {
        red_e[wc * TILE + lr] = se;
        red_u[wc * TILE + lr] = su;
      }
    }
  }
  __syncthreads();
  if (tid < TILE && i0 + tid < g.d) {
    const int64_t o = (int64_t)bj * g.d + i0 + tid;
    g.part_e[o] = red_e[tid] + red_e[TILE + tid];
    g.part_u[o] = red_u[tid] + red_u[TILE + tid];
  }
}

// e[k] = sum_J part_e[J][k] in ascending J (and unorm2 likewise): one thread per output channel, coalesced along k
__global__ __launch_bounds__(256) void oe_reduce_kernel(const double* part_e, const double* part_u, int64_t d, int tiles_n, double* e,
                                                        double* unorm2) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= d) return;
  double se = 0., su = 0.;
  for (int t = 0; t < tiles_n; t++) {
    se += part_e[(int64_t)t * d + k];
    su += part_u[(int64_t)t * d + k];
  }
  e[k] = se;
  if (unorm2) unorm2[k] = su;
}

static size_t oe_pos_bytes(int64_t n) { return align_up((size_t)n * sizeof(int), 16); }

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_mlp_output_error_ws_bytes(int64_t n, int64_t d) {
  if (n <= 0 || d <= 0) return 0;
  // pos [n] (int32, padded to 16 bytes); the partials of e and of unorm2, [ceil(n / 128)][d] doubles each
  return oe_pos_bytes(n) + 2 * (size_t)ceil_div(n, TILE) * (size_t)d * sizeof(double);
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
  int* pos = (int*)ws;
  double* part_e = (double*)((char*)ws + oe_pos_bytes(n));
  double* part_u = part_e + (size_t)tiles_n * (size_t)d;
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
  hipLaunchKernelGGL(oe_reduce_kernel, dim3((unsigned)ceil_div(d, 256)), dim3(256), 0, st, part_e, part_u, d, (int)tiles_n, e, unorm2);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
