// The tile-column quadratic form y G y^T of the error reports (out_err.hip: y = a row of the residual weights, G = the statistic;
// vo_err.hip: y = a row of [W_o,h | o'_h], G = a stacked Gram), read from the LOWER triangle of the symmetric G alone.
//
// Tile scheme (the shared 128 x 128 / 4-wave / LDS-fp64-panel core of common.hpp).  A workgroup owns a 128-row block of the row
// source y and one 128-wide tile COLUMN J of G and walks the tiles (I, J), I = J .. T-1, of the lower triangle down that column:
//   P[128, 128] = sum_{I >= J} y[:, I] G[I, J]     (v_mfma_f64_16x16x4_f64; the diagonal tile G_JJ masked to its STRICT lower part
//                                                   while staging, so what lies on or above the diagonal of G is never loaded)
// -- one accumulator for the whole column, so the epilogue runs once per workgroup and the partial sums are rows * T numbers, not
// rows * T (T + 1) / 2.  y is formed in the A-operand staging by the row source (every input widened exactly to fp64 there).
// Epilogue, per entry (k, j) of the tile:  y_kj (2 P_kj + G_jj y_kj)  -- the factor 2 on the strict lower part, the diagonal term
// without it -- and, where asked for, y_kj^2, summed along the tile's 128 columns (4 in the lane, 16 lanes by shuffles in a fixed
// tree, the two wave columns through LDS).  P is never written to memory.  quad_reduce_kernel adds each row's T partials in ascending
// tile order.  No atomics: two runs are bit-identical.  Tile columns are best handed out longest first (J ascending): T - J tiles each.
//
// A row source has an index type Idx (int or int64_t: what holds n), a type Col (default-constructible) and two steps, so that what
// depends on the column alone is looked up once:
//   Col prepare(Idx col) const                        for a column col < n
//   double at(int64_t row, Idx col, Col c) const      y[row][col] with c = prepare(col), row below the caller's row limit
// Out-of-range rows / columns are never loaded (selects, not multiplications by zero): a NaN in row k of the source stays in row k of
// P and of the sums; a NaN in the lower triangle of G reaches every row.
#pragma once
#include "common.hpp"

namespace mdg {

// For tid < TILE: qf = sum_j y_kj (2 P_kj + G_jj y_kj) and, with NORM2, n2 = sum_j y_kj^2 over the columns j0 .. j0 + 127 (below n)
// of row k = i0 + tid (0 for k >= rows).  All 256 threads of the workgroup call it; lds: 4 * PANEL doubles.
template <bool NORM2, class Src>
__device__ __forceinline__ void quad_form_tile_column(const Src& src, const double* __restrict__ G, typename Src::Idx ldg,
                                                      typename Src::Idx n, int64_t rows, int64_t i0, typename Src::Idx j0, double* lds,
                                                      double& qf, double& n2) {
  typedef typename Src::Idx Idx;         // of a column of y / a row or column of G: int where n allows it (registers)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const Idx n_stage = (n - j0 + BK - 1) / BK;                         // k runs over the columns j0 .. n-1 of y (>= 1 stage)

  // A panel: element (x = row of y, k); y is k-contiguous, so consecutive threads walk k: a thread keeps one k and 8 rows
  const int ak = tid & 15, ax = tid >> 4;
  // B panel: element (k = row of G, y = column of G); G is column-contiguous: a thread keeps one column and 8 rows
  const int bk = tid >> 7, by = tid & 127;
  const Idx gcb = j0 + by;
  double rg[8];  // one panel's prefetch at a time: A rides under the first half of a stage, B under the second (gemm.hip)

  auto load_a = [&](Idx k0) {
    const Idx col = k0 + ak;
    const bool ok = col < n;
    typename Src::Col c{};
    if (ok) c = src.prepare(col);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int64_t row = i0 + ax + 16 * q;
      rg[q] = (ok && row < rows) ? src.at(row, col, c) : 0.;
    }
  };
  auto store_a = [&](double* panel) {
#pragma unroll
    for (int q = 0; q < 8; q++) panel[ak * PITCH + ax + 16 * q] = rg[q];
  };
  auto load_b = [&](Idx k0) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const Idx gr = k0 + bk + 2 * q;
      rg[q] = (gr < n && gr > gcb) ? G[(size_t)gr * ldg + gcb] : 0.;              // strictly below the diagonal only (gcb < gr < n)
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
  for (Idx s = 0; s < n_stage; s++) {
    const int cur = (int)(s & 1);
    const bool more = s + 1 < n_stage;
    const Idx k0 = j0 + (s + 1) * BK;
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

  // epilogue: sum_j y_kj (2 P_kj + G_jj y_kj) and sum_j y_kj^2 over the tile's columns
  double* red_e = lds;                 // [2][TILE]  (the panels are dead: the loop ended with a barrier)
  double* red_u = lds + 2 * TILE;      // [2][TILE]
  const Idx gc0 = j0 + acc_col(wc, lane, 0);
  bool cok[4];
  typename Src::Col cj[4];
  double gd[4];
#pragma unroll
  for (int sb = 0; sb < 4; sb++) {
    const Idx col = gc0 + sb;
    cok[sb] = col < n;
    cj[sb] = typename Src::Col{};
    if (cok[sb]) cj[sb] = src.prepare(col);
    gd[sb] = cok[sb] ? G[(size_t)col * ldg + col] : 0.;
  }
#pragma unroll
  for (int sa = 0; sa < 4; sa++) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int lr = acc_row(wr, lane, sa, reg);
      const int64_t row = i0 + lr;
      double se = 0., su = 0.;
      if (row < rows) {
#pragma unroll
        for (int sb = 0; sb < 4; sb++) {
          if (!cok[sb]) continue;
          const double y = src.at(row, gc0 + sb, cj[sb]);
          se += y * (2. * acc.v[sa][sb][reg] + gd[sb] * y);
          if (NORM2) su += y * y;
        }
      }
      // the 16 lanes that share (lane >> 4) hold this row's other columns: a fixed butterfly, the same value in all of them
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        se += __shfl_xor(se, m);
        if (NORM2) su += __shfl_xor(su, m);
      }
      if ((lane & 15) == 0) {
        red_e[wc * TILE + lr] = se;
        if (NORM2) red_u[wc * TILE + lr] = su;
      }
    }
  }
  __syncthreads();
  if (tid < TILE) {
    qf = red_e[tid] + red_e[TILE + tid];
    if (NORM2) n2 = red_u[tid] + red_u[TILE + tid];
  }
}

// e[i] = sum_J part[J][i] in ascending J over `tiles` planes of `total` entries; with e2, e2[i] likewise from the second plane set,
// which starts tiles * total behind the first.  One thread per entry, coalesced along i.  (static: one copy per including file.)
static __global__ __launch_bounds__(256) void quad_reduce_kernel(const double* part, int64_t total, int tiles, double* e, double* e2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  double se = 0., s2 = 0.;
  for (int t = 0; t < tiles; t++) {
    se += part[(size_t)t * total + i];
    if (e2) s2 += part[(size_t)(tiles + t) * total + i];
  }
  e[i] = se;
  if (e2) e2[i] = s2;
}

}  // namespace mdg
