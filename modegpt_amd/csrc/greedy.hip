// Block-greedy column selection for the MLP on the objective the Nystrom refit minimises (include/modegpt_hip.h,
// mdg_nystrom_greedy_select; DESIGN.md section 7, "Greedy MLP selection"):
//   M = C + eps I,  R = M - M[:, S] M_SS^-1 M[S, :],  B = W R,  J = sum B o W = tr(W R W^T),  gain g_j = ||B[:, j]||^2 / R_jj.
// Hybrid form: R is never stored.  Yt [|S|, n] holds R = M - Yt^T Yt (one row per pick, in pick order), diag(R) is kept as a
// vector, a round's panel R[P, :] = M[P, :] - Yt[:, P]^T Yt is built for its picks only, and B is downdated right-looking:
//   K = R[P, P] = L L^T,  Ynew = L^-1 R[P, :]  (the new rows of Yt),  diag(R) -= column sums of Ynew o Ynew,
//   B -= (B[:, P] L^-T) Ynew.
// A round's pick count m_t is known on the host, how many of the picks are DEAD (ineligible columns that fill a round when the
// eligible ones run out) is not: a dead pick keeps its slot with a zero panel row, a unit diagonal in K and a zero column of
// B[:, P], which makes it an exact no-op of the downdate without a host round trip.
// Every round is ordinary launches on one stream; no atomics, every sum in a fixed order: bit-identical from run to run.
#include "common.hpp"

namespace mdg {
int gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i, int64_t sa_k,
             const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k, int64_t sb_j, double beta, void* C,
             int c_dtype, int64_t ldc, int64_t batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int flags,
             hipStream_t st);
int potrf_lower(double* A, int64_t n, int64_t lda, double* inv_diag, hipStream_t st);
int tri_inverse_doubling(const double* L, int64_t n, int64_t ldl, const double* inv_diag, double* X, int64_t ldx, double* T,
                         int64_t s_limit, hipStream_t st);

constexpr int GR_RS = 16;          // row slabs of the column statistics (partial sums, added in slab order)
constexpr int GR_CHUNK = 2048;     // rows of M per panel of the initial product B = W M
constexpr int GR_SPLIT_MAX = 8;    // K-splits of a round's panel product at most ...
constexpr int GR_SPLIT_TILES = 1024;   // ... and only while splits x 128-square output tiles stay at or under this (four per CU)
constexpr int GR_SPLIT_DEPTH = 64;     // ... and every split is at least this deep

// dM[j] = C[j, j] + eps (one fp64 addition, as mdg_nystrom_down adds the ridge), dR = dM, nothing taken, no dead pick yet.
__global__ __launch_bounds__(256) void greedy_init_kernel(const double* C, int64_t ldc, int64_t n, double eps, double* dM, double* dR,
                                                          int* taken, int64_t* n_dead) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j == 0) n_dead[0] = 0;
  if (j >= n) return;
  const double v = C[j * ldc + j] + eps;
  dM[j] = v;
  dR[j] = v;
  taken[j] = 0;
}

// out[a, j] = M[row_a, j], row_a = rows ? rows[a] : row0 + a, always from the lower triangle of C (C[max, min]), the ridge on the
// diagonal; a dead pick (elig given and elig[row_a] == 0) gets a zero row.  blockIdx.y strides over the rows.
__global__ __launch_bounds__(256) void sym_rows_kernel(const double* C, int64_t ldc, const int64_t* rows, int64_t row0, int64_t m, int64_t n,
                                                       double eps, const int* elig, double* out, int64_t ldo) {
  for (int64_t a = blockIdx.y; a < m; a += gridDim.y) {
    const int64_t i = rows ? rows[a] : row0 + a;
    const bool dead = elig && !elig[i];
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
      double v = 0.;
      if (!dead) {
        v = j <= i ? C[i * ldc + j] : C[j * ldc + i];
        if (j == i) v += eps;
      }
      out[a * ldo + j] = v;
    }
  }
}

// Column statistics of B over the row slab blockIdx.y: sq[slab][j] = sum_i B_ij^2, bw[slab][j] = sum_i B_ij W_ij.  One workgroup per
// 64 columns and slab; wave w takes the slab's rows w, w + 4, ... in ascending order, the four partial sums are added in the order
// 0, 1, 2, 3 (rank_curve.hip colnorm2_kernel).
template <int DT>
__global__ __launch_bounds__(256) void colstat_kernel(const double* B, int64_t ldb, const void* W, int64_t ldw, int64_t d, int64_t n,
                                                      int64_t slab_rows, double* sq, double* bw, int64_t lds_) {
  __shared__ double red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + lane;
  const int64_t i0 = (int64_t)blockIdx.y * slab_rows, i1 = i0 + slab_rows < d ? i0 + slab_rows : d;
  double s = 0., t = 0.;
  if (j < n)
    for (int64_t i = i0 + wave; i < i1; i += 4) {
      const double b = B[i * ldb + j];
      s += b * b;
      t += b * load_f64<DT>(W, i * ldw + j);
    }
  red[0][wave][lane] = s;
  red[1][wave][lane] = t;
  __syncthreads();
  if (wave == 0 && j < n) {
    sq[blockIdx.y * lds_ + j] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    bw[blockIdx.y * lds_ + j] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
  }
}

// gain, eligibility and the ranking key of every column (the slabs added in ascending order); cbw[j] = the column's share of J.
// key: -gain for an eligible column, +inf for an ineligible one that is not taken, NaN for a taken one -- under
// mdg_select_smallest_sorted's order (ties: lower index; NaN last) the first m are the round's picks.
__global__ __launch_bounds__(256) void greedy_key_kernel(const double* sq, const double* bw, int64_t lds_, int slabs, const double* dR,
                                                         const double* dM, const int* taken, int64_t n, double floor_rel, double* gain,
                                                         double* key, int* elig, double* cbw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = 0., t = 0.;
  for (int k = 0; k < slabs; k++) {
    s += sq[k * lds_ + j];
    t += bw[k * lds_ + j];
  }
  cbw[j] = t;
  const double r = dR[j], g = s / r;
  const bool fin = fabs(g) <= 1.7976931348623157e308;       // (false for NaN and Inf)
  const bool ok = !taken[j] && r > floor_rel * dM[j] && fin;
  gain[j] = g;
  elig[j] = ok ? 1 : 0;
  key[j] = taken[j] ? __longlong_as_double(0x7ff8000000000000ll) : (ok ? -g : __longlong_as_double(0x7ff0000000000000ll));
}

// out[0 .. copies) = sum_j c[j]: thread t sums its contiguous chunk in ascending order, thread 0 adds the 256 chunk totals in ascending order.
__global__ __launch_bounds__(256) void greedy_objective_kernel(const double* c, int64_t n, double* out, int64_t copies) {
  __shared__ double total[256];
  const int t = threadIdx.x;
  const int64_t m = (n + 255) / 256;
  const int64_t lo = (int64_t)t * m, hi = lo + m < n ? lo + m : n;
  double s = 0.;
  for (int64_t j = lo; j < hi; j++) s += c[j];
  total[t] = s;
  __syncthreads();
  if (t == 0) {
    double a = 0.;
    for (int u = 0; u < 256; u++) a += total[u];
    for (int64_t k = 0; k < copies; k++) out[k] = a;
  }
}

// The masked top-m pick under mdg_select_smallest_sorted's order (a before b: a < b, or equal and the lower index; NaN is largest),
// as a rank by counting that fills the chip: that entry's rank_threshold_kernel gives a thread ALL n compares (n / 256 workgroups:
// 1.4 ms at n = 14336, a third of a 128-round call); here workgroup (x, y) counts, for its 256 keys, how many of the 1024 keys of
// slab y come before each -- n^2 / 2^18 workgroups -- and one workgroup adds the slab counts (integers) and compacts.
__device__ __forceinline__ bool key_before(double a, int64_t ia, double b, int64_t ib) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return (!an && bn) || (an && bn && ia < ib);
  return a < b || (a == b && ia < ib);
}

constexpr int PK_SLAB = 1024;

__global__ __launch_bounds__(256) void pick_count_kernel(const double* key, int64_t n, int* part, int64_t ldp) {
  __shared__ double tile[PK_SLAB];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, j0 = (int64_t)blockIdx.y * PK_SLAB;
  for (int e = threadIdx.x; e < PK_SLAB; e += 256) tile[e] = (j0 + e < n) ? key[j0 + e] : 0.;
  __syncthreads();
  if (i >= n) return;
  const double mine = key[i];
  const int lim = (int)(n - j0 < PK_SLAB ? n - j0 : PK_SLAB);
  int c = 0;
  for (int e = 0; e < lim; e++) c += key_before(tile[e], j0 + e, mine, i) ? 1 : 0;
  part[blockIdx.y * ldp + i] = c;
}

// picks[0 .. m) = the indices whose rank (the sum of their slab counts) is below m, in ascending order: one workgroup, thread t owns
// a contiguous range of indices, an exclusive scan of the per-thread counts places them.  Exactly m indices qualify (the order is total).
__global__ __launch_bounds__(1024) void pick_compact_kernel(const int* part, int64_t ldp, int slabs, int64_t n, int64_t m, int64_t* picks) {
  __shared__ int sums[1024];
  const int tid = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t b = tid * per, e = (b + per < n) ? b + per : n;
  auto selected = [&](int64_t i) {
    int64_t rank = 0;
    for (int s = 0; s < slabs; s++) rank += part[s * ldp + i];
    return rank < m;
  };
  int c = 0;
  for (int64_t i = b; i < e; i++) c += selected(i) ? 1 : 0;
  sums[tid] = c;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele inclusive scan
    const int v = tid >= o ? sums[tid - o] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  int64_t pos = sums[tid] - c;
  for (int64_t i = b; i < e; i++)
    if (selected(i) && pos < m) picks[pos++] = i;
}

// One workgroup, after the round's picks are known: marks them taken, counts the dead ones, and leaves the round's cut --
// cut[0] = the smallest picked gain, cut[1] = the largest eligible gain not picked, NaN where there is none.
__global__ __launch_bounds__(1024) void greedy_cut_kernel(const int64_t* picks, int64_t m, const double* gain, const int* elig, int* taken,
                                                          int64_t n, int round, double* cut, int64_t* n_dead) {
  __shared__ double lo[1024], hi[1024];
  __shared__ int cnt[1024];
  const int tid = threadIdx.x;
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);
  double mn = inf;
  int dead = 0;
  for (int64_t a = tid; a < m; a += 1024) {
    const int64_t j = picks[a];
    taken[j] = round + 1;
    if (elig[j]) mn = fmin(mn, gain[j]); else dead++;
  }
  __syncthreads();     // (the marks above are this workgroup's own stores)
  double mx = -inf;
  for (int64_t j = tid; j < n; j += 1024)
    if (!taken[j] && elig[j]) mx = fmax(mx, gain[j]);
  lo[tid] = mn; hi[tid] = mx; cnt[tid] = dead;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) {
      lo[tid] = fmin(lo[tid], lo[tid + o]);
      hi[tid] = fmax(hi[tid], hi[tid + o]);
      cnt[tid] += cnt[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (cut) {
      cut[0] = lo[0] < inf ? lo[0] : nan;
      cut[1] = hi[0] > -inf ? hi[0] : nan;
    }
    n_dead[0] += cnt[0];
  }
}

// out[i, a] = src[i, picks[a]] for the rows i < rows (0 for a dead pick): the picked columns of Yt or of B.
__global__ __launch_bounds__(256) void pick_cols_kernel(const double* src, int64_t lds_, const int64_t* picks, const int* elig, int64_t rows,
                                                        int64_t m, double* out, int64_t ldo) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a >= m) return;
  const int64_t j = picks[a];
  const bool dead = !elig[j];
  for (int64_t i = blockIdx.y; i < rows; i += gridDim.y) out[i * ldo + a] = dead ? 0. : src[i * lds_ + j];
}

// K (lower triangle) = R[P, P] from the panel Pt = R[P, :]; a dead pick has a unit diagonal and zeros in its row and column.
__global__ __launch_bounds__(256) void pick_block_kernel(const double* Pt, int64_t ldp, const int64_t* picks, const int* elig, int64_t m,
                                                         double* K, int64_t ldk) {
  for (int64_t a = blockIdx.y; a < m; a += gridDim.y) {
    const bool dead_a = !elig[picks[a]];
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b <= a; b += (int64_t)gridDim.x * 256) {
      const int64_t jb = picks[b];
      const bool dead = dead_a || !elig[jb];
      K[a * ldk + b] = dead ? (a == b ? 1. : 0.) : Pt[a * ldp + jb];
    }
  }
}

// dR[j] -= sum_a Y[a, j]^2 over the round's m new rows, a ascending, one subtraction.
__global__ __launch_bounds__(256) void diag_downdate_kernel(const double* Y, int64_t ldy, int64_t m, int64_t n, double* dR) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = 0.;
  for (int64_t a = 0; a < m; a++) {
    const double v = Y[a * ldy + j];
    s += v * v;
  }
  dR[j] -= s;
}

// Pt[a, j] -= sum_b parts[b][a, j], b ascending: the K-split partial products of a round's panel.
__global__ __launch_bounds__(256) void panel_reduce_kernel(double* Pt, const double* parts, int64_t part_stride, int64_t count, int64_t m,
                                                           int64_t n, int64_t ldp) {
  for (int64_t a = blockIdx.y; a < m; a += gridDim.y)
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
      double s = 0.;
      for (int64_t b = 0; b < count; b++) s += parts[b * part_stride + a * ldp + j];
      Pt[a * ldp + j] -= s;
    }
}

__global__ void greedy_copy_count_kernel(const int64_t* src, int64_t* dst) { dst[0] = src[0]; }

__global__ __launch_bounds__(256) void greedy_fill_kernel(double* p, int64_t count, double v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) p[i] = v;
}

static int64_t gr_pitch(int64_t n) { return (n + 15) / 16 * 16; }

// the workspace (every block starts on a 16-byte boundary)
struct GreedyWs {
  int64_t np, mp, dp, m_max, pm, rounds;
  double *B, *Yt, *Pt, *K, *inv, *Linv, *T, *YP, *parts, *BP, *Gt, *dM, *dR, *gain, *key, *cbw, *sq, *bw;
  int *taken, *elig, *part;
  int64_t* ndead;
  size_t bytes;
};
static GreedyWs greedy_layout(void* ws, int64_t n, int64_t d, int64_t r, int64_t rounds_in) {
  GreedyWs w;
  w.rounds = r < rounds_in ? r : rounds_in;                       // (T > r counts as r)
  w.m_max = w.rounds > 0 ? ceil_div(r, w.rounds) : 0;
  w.np = gr_pitch(n); w.mp = gr_pitch(w.m_max > 0 ? w.m_max : 1); w.dp = gr_pitch(d);
  const int64_t chunk = n < GR_CHUNK ? n : GR_CHUNK;
  w.pm = w.m_max > chunk ? w.m_max : chunk;
  const int64_t np = w.np, mp = w.mp, dp = w.dp, m_max = w.m_max, rounds = w.rounds;
  Carve c(ws);
  auto take = [&](size_t elems) { return c.take<double>(elems, 16); };
  auto take_int = [&](size_t elems) { return c.take<int>(elems, 16); };
  w.B = take((size_t)d * np);
  w.Yt = take((size_t)r * np);
  w.Pt = take((size_t)w.pm * np);
  w.K = take((size_t)m_max * mp);
  w.inv = take(m_max > 0 ? mdg_potrf_inv_diag_elems(m_max) : 0);
  w.Linv = take((size_t)m_max * mp + mp);
  w.T = take(tri_inverse_scratch_elems(m_max, m_max));
  w.YP = take(rounds > 1 ? (size_t)(r - m_max) * mp : 0);       // (the last round's picks meet at most r - m_last rows of Yt)
  {   // the K-split partial panels: splits x m x np <= GR_SPLIT_TILES tiles of 128 x 128 by the rule that picks the split count
    const size_t cap = (size_t)GR_SPLIT_TILES * 128 * 128, all = (size_t)GR_SPLIT_MAX * m_max * np;
    w.parts = take(rounds > 1 ? (all < cap ? all : cap) : 0);
  }
  w.BP = take((size_t)d * mp);
  w.Gt = take((size_t)m_max * dp);
  w.dM = take(np); w.dR = take(np); w.gain = take(np); w.key = take(np); w.cbw = take(np);
  w.sq = take((size_t)GR_RS * np); w.bw = take((size_t)GR_RS * np);
  w.taken = take_int(np); w.elig = take_int(np);
  w.part = take_int((size_t)ceil_div(n, PK_SLAB) * np);         // (the pick's slab counts)
  w.ndead = c.take<int64_t>(2, 16);                             // (one used)
  w.bytes = c.off;
  return w;
}

}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_nystrom_greedy_ws_bytes(int64_t n, int64_t d, int64_t r, int64_t rounds) {
  if (n <= 0 || d <= 0 || r < 0 || r > n || rounds < 1) return 0;
  return greedy_layout(nullptr, n, d, r, rounds).bytes;
}

extern "C" int mdg_nystrom_greedy_select(const double* C, int64_t n, int64_t ldc, const void* Wd, int64_t d, int64_t ld_wd, int w_dtype,
                                         double eps, int64_t r, int64_t rounds, int64_t* order, double* objective, double* cut,
                                         int64_t* n_dead, void* ws, size_t ws_bytes, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(C && Wd && objective, "mdg_nystrom_greedy_select: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_nystrom_greedy_select: W_d must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n > 0 && d > 0 && ldc >= n && ld_wd >= n, "mdg_nystrom_greedy_select: bad sizes (n=%lld d=%lld ldc=%lld ld_wd=%lld)",
                (long long)n, (long long)d, (long long)ldc, (long long)ld_wd);
  MDG_CHECK_ARG(n <= INT32_MAX, "mdg_nystrom_greedy_select: n = %lld is beyond the limit of 2^31 - 1 columns", (long long)n);
  MDG_CHECK_ARG(r >= 0 && r <= n, "mdg_nystrom_greedy_select: rank %lld outside 0 .. n = %lld", (long long)r, (long long)n);
  MDG_CHECK_ARG(rounds >= 1, "mdg_nystrom_greedy_select: rounds = %lld, need at least 1", (long long)rounds);
  MDG_CHECK_ARG(order || r == 0, "mdg_nystrom_greedy_select: null order with rank %lld", (long long)r);
  MDG_CHECK_ARG(ws && ws_bytes >= mdg_nystrom_greedy_ws_bytes(n, d, r, rounds), "mdg_nystrom_greedy_select: workspace %zu < required %zu",
                ws_bytes, mdg_nystrom_greedy_ws_bytes(n, d, r, rounds));
  hipStream_t st = (hipStream_t)stream;
  const GreedyWs L = greedy_layout(ws, n, d, r, rounds);
  double *B = L.B, *Yt = L.Yt, *Pt = L.Pt, *Km = L.K, *inv = L.inv, *Linv = L.Linv, *Tt = L.T, *YP = L.YP, *parts = L.parts, *BP = L.BP,
         *Gt = L.Gt, *dM = L.dM, *dR = L.dR, *gain = L.gain, *key = L.key, *cbw = L.cbw, *sq = L.sq, *bw = L.bw;
  int *taken = L.taken, *elig = L.elig, *part = L.part;
  int64_t* ndead = L.ndead;
  const int64_t np = L.np, mp = L.mp, dp = L.dp, T = L.rounds;
  const unsigned gn = (unsigned)ceil_div(n, 256);
  const int64_t slab_rows = ceil_div(ceil_div(d, GR_RS), 4) * 4;         // (whole groups of the four waves' rows)
  const int slabs = (int)ceil_div(d, slab_rows);
  const size_t wsz = dtype_size(w_dtype);
  const int pslabs = (int)ceil_div(n, PK_SLAB);
  int status = MDG_OK;

  hipLaunchKernelGGL(greedy_init_kernel, dim3(gn), dim3(256), 0, st, C, ldc, n, eps, dM, dR, taken, ndead);
  MDG_LAUNCH_CHECK();
  // B = W M, by panels of GR_CHUNK rows of M (symmetrised from the lower triangle), accumulated in panel order
  for (int64_t c0 = 0; c0 < n; c0 += GR_CHUNK) {
    const int64_t kc = n - c0 < GR_CHUNK ? n - c0 : GR_CHUNK;
    hipLaunchKernelGGL(sym_rows_kernel, dim3(gn < 64 ? gn : 64, (unsigned)(kc < 4096 ? kc : 4096)), dim3(256), 0, st, C, ldc,
                       (const int64_t*)nullptr, c0, kc, n, eps, (const int*)nullptr, Pt, np);
    MDG_LAUNCH_CHECK();
    MDG_TRY(gemm_f64(d, n, kc, 1.0, (const char*)Wd + (size_t)c0 * wsz, w_dtype, ld_wd, 1, nullptr, Pt, MDG_F64, np, 1, c0 ? 1.0 : 0.0, B,
                     MDG_F64, np, 1, 0, 0, 0, 0, st));
  }
  // the column statistics of the current B: the gains of the next round and the objective after the last one
  auto stats = [&]() -> int {
    const dim3 g((unsigned)ceil_div(n, 64), (unsigned)slabs);
    if (w_dtype == MDG_BF16) hipLaunchKernelGGL(colstat_kernel<MDG_BF16>, g, dim3(256), 0, st, B, np, Wd, ld_wd, d, n, slab_rows, sq, bw, np);
    else hipLaunchKernelGGL(colstat_kernel<MDG_F64>, g, dim3(256), 0, st, B, np, Wd, ld_wd, d, n, slab_rows, sq, bw, np);
    hipLaunchKernelGGL(greedy_key_kernel, dim3(gn), dim3(256), 0, st, sq, bw, np, slabs, dR, dM, taken, n, (double)n * 0x1p-52, gain, key,
                       elig, cbw);
    MDG_LAUNCH_CHECK();
    return MDG_OK;
  };
  int64_t off = 0;
  for (int64_t t = 0; t < T; t++) {
    const int64_t m = r * (t + 1) / T - r * t / T;                       // (>= 1: T <= r)
    int64_t* picks = order + off;
    MDG_TRY(stats());
    hipLaunchKernelGGL(greedy_objective_kernel, dim3(1), dim3(256), 0, st, cbw, n, objective + t, (int64_t)1);
    MDG_LAUNCH_CHECK();
    hipLaunchKernelGGL(pick_count_kernel, dim3(gn, (unsigned)pslabs), dim3(256), 0, st, key, n, part, np);
    hipLaunchKernelGGL(pick_compact_kernel, dim3(1), dim3(1024), 0, st, part, np, pslabs, n, m, picks);     // ascending index within the round
    MDG_LAUNCH_CHECK();
    hipLaunchKernelGGL(greedy_cut_kernel, dim3(1), dim3(1024), 0, st, picks, m, gain, elig, taken, n, (int)t, cut ? cut + 2 * t : nullptr,
                       ndead);
    MDG_LAUNCH_CHECK();
    // the panel Pt = R[P, :] = M[P, :] - Yt[:, P]^T Yt
    hipLaunchKernelGGL(sym_rows_kernel, dim3(gn < 64 ? gn : 64, (unsigned)(m < 4096 ? m : 4096)), dim3(256), 0, st, C, ldc, picks, (int64_t)0,
                       m, n, eps, elig, Pt, np);
    MDG_LAUNCH_CHECK();
    if (off > 0) {
      hipLaunchKernelGGL(pick_cols_kernel, dim3((unsigned)ceil_div(m, 256), (unsigned)(off < 1024 ? off : 1024)), dim3(256), 0, st, Yt, np,
                         picks, elig, off, m, YP, mp);
      MDG_LAUNCH_CHECK();
      // Yt[:, P]^T Yt is m x n x |S|: with few picks its output tiles cannot fill the chip (79 x 14336: one tile row of 112), so
      // K = |S| is split over the batch dimension into partial panels, which are then subtracted in split order
      const int64_t tiles = ceil_div(m, TILE) * ceil_div(n, TILE);
      int64_t nb = GR_SPLIT_TILES / tiles;
      nb = nb > GR_SPLIT_MAX ? GR_SPLIT_MAX : nb;
      nb = nb > off / GR_SPLIT_DEPTH ? off / GR_SPLIT_DEPTH : nb;
      if (nb >= 2) {
        const int64_t kc = ceil_div(ceil_div(off, nb), 16) * 16, full = off / kc, rem = off - full * kc, pbs = m * np;
        MDG_TRY(gemm_f64(m, n, kc, 1.0, YP, MDG_F64, 1, mp, nullptr, Yt, MDG_F64, np, 1, 0.0, parts, MDG_F64, np, full, kc * mp, kc * np, pbs,
                         0, st));
        if (rem > 0)
          MDG_TRY(gemm_f64(m, n, rem, 1.0, YP + (size_t)full * kc * mp, MDG_F64, 1, mp, nullptr, Yt + (size_t)full * kc * np, MDG_F64, np, 1, 0.0,
                           parts + (size_t)full * pbs, MDG_F64, np, 1, 0, 0, 0, 0, st));
        hipLaunchKernelGGL(panel_reduce_kernel, dim3(gn < 64 ? gn : 64, (unsigned)(m < 4096 ? m : 4096)), dim3(256), 0, st, Pt, parts, pbs,
                           full + (rem > 0 ? 1 : 0), m, n, np);
        MDG_LAUNCH_CHECK();
      } else {
        MDG_TRY(gemm_f64(m, n, off, -1.0, YP, MDG_F64, 1, mp, nullptr, Yt, MDG_F64, np, 1, 1.0, Pt, MDG_F64, np, 1, 0, 0, 0, 0, st));
      }
    }
    // K = R[P, P] = L L^T and L^-1
    hipLaunchKernelGGL(pick_block_kernel, dim3((unsigned)(ceil_div(m, 256) < 64 ? ceil_div(m, 256) : 64), (unsigned)(m < 4096 ? m : 4096)),
                       dim3(256), 0, st, Pt, np, picks, elig, m, Km, mp);
    MDG_LAUNCH_CHECK();
    {
      // a pivot that fails leaves NaN behind, the picks stay distinct all the same: the remaining rounds run, the status is kept
      const int s = potrf_lower(Km, m, mp, inv, st);
      if (s == MDG_ERR_NOT_PD) status = s;
      else if (s != MDG_OK) return s;
    }
    MDG_TRY(tri_inverse_doubling(Km, m, mp, inv, Linv, mp, Tt, m, st));
    // the new rows of Yt: Ynew = L^-1 Pt, and diag(R) -= their column norms
    double* Ynew = Yt + (size_t)off * np;
    MDG_TRY(gemm_f64(m, n, m, 1.0, Linv, MDG_F64, mp, 1, nullptr, Pt, MDG_F64, np, 1, 0.0, Ynew, MDG_F64, np, 1, 0, 0, 0, MDG_GEMM_A_LOWER_TRI,
                     st));
    hipLaunchKernelGGL(diag_downdate_kernel, dim3(gn), dim3(256), 0, st, Ynew, np, m, n, dR);
    MDG_LAUNCH_CHECK();
    // B -= (B[:, P] L^-T) Ynew:  Gt = L^-1 B[:, P]^T  [m, d]
    hipLaunchKernelGGL(pick_cols_kernel, dim3((unsigned)ceil_div(m, 256), (unsigned)(d < 1024 ? d : 1024)), dim3(256), 0, st, B, np, picks, elig,
                       d, m, BP, mp);
    MDG_LAUNCH_CHECK();
    MDG_TRY(gemm_f64(m, d, m, 1.0, Linv, MDG_F64, mp, 1, nullptr, BP, MDG_F64, 1, mp, 0.0, Gt, MDG_F64, dp, 1, 0, 0, 0, MDG_GEMM_A_LOWER_TRI, st));
    MDG_TRY(gemm_f64(d, n, m, -1.0, Gt, MDG_F64, 1, dp, nullptr, Ynew, MDG_F64, np, 1, 1.0, B, MDG_F64, np, 1, 0, 0, 0, 0, st));
    off += m;
  }
  // the objective after the last round, repeated for the rounds beyond r (which take nothing and have no cut)
  MDG_TRY(stats());
  hipLaunchKernelGGL(greedy_objective_kernel, dim3(1), dim3(256), 0, st, cbw, n, objective + T, rounds - T + 1);
  MDG_LAUNCH_CHECK();
  if (r > 0) {
    if (cut && rounds > T)
      hipLaunchKernelGGL(greedy_fill_kernel, dim3((unsigned)ceil_div(2 * (rounds - T), 256)), dim3(256), 0, st, cut + 2 * T, 2 * (rounds - T),
                         __builtin_nan(""));
    if (n_dead) hipLaunchKernelGGL(greedy_copy_count_kernel, dim3(1), dim3(1), 0, st, ndead, n_dead);
    MDG_LAUNCH_CHECK();
  }
  return status;
}
