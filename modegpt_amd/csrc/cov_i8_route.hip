// int8 covariance, the route (the map of the units is at the head of cov_i8.hip): which product a statistic takes and which of
// its columns leave the int8 path (i8_route_kernel), the clearing of those columns' digits, and -- enqueued after the products --
// their rows / columns of sigma in plain fp64.
#include <algorithm>

#include "cov_i8.hpp"

namespace mdg {
namespace {

// ---- the route of a statistic (host model with the derivation: tests/i8_model.py).
// With alpha_s(j) = 256^(5 - s) ||d_s(., j)|| / ||N_j|| (plane energies over the column norm) and rho_j = sqrt(rounded_j) / (2 ||N_j||),
// Cauchy-Schwarz over the tokens bounds the error of the P-plane product entry-wise, for ANY input:
//     |sigma_ij(P) - sigma_ij| / sqrt(sigma_ii sigma_jj)  <=  sum_{s + t >= P} alpha_s(i) alpha_t(j) + rho_i + rho_j + rho_i rho_j  <=  SQ_P + X_P
//     SQ_P = sum_{2 s >= P} A_s^2 + 2 R + R^2   (attained on the diagonal)        X_P = sum_{s != t, s + t >= P} A_s A_t   (cross terms)
// with A_s, R the maxima over the columns that stay on the int8 path.  The route is the smallest P in {5, 6} for which
// SQ_P <= TAU_SQ and X_P <= tau_x(tokens) hold after at most ROUTE_JMAX columns have been handed to the fp64 column kernel -- greedily,
// each time the column whose removal lowers the violation most (a column dominated by a few massive activations carries a bulk
// that lives entirely in the deep planes: it alone sets A_2 .. A_4) -- else the whole statistic goes through mdg_cov_accum.  Columns
// holding an Inf / NaN always leave (only the fp64 arithmetic propagates those the way the reference does).
// ||N_j|| enters through the integer lower bound 2^32 (||256 d_0 + d_1|| - sqrt(nonzeros) / 2): every decision is a function of
// integer sums, hence run-to-run bit-identical.  One workgroup per statistic.
// Element type: checked for fp16 (F16Elem, cov_i8.hpp) -- nothing here assumes an 8-bit significand.  The kernel sees integer plane
// energies and emax only.  The lower bound on ||N_j|| holds for any integers below 2^47 (what lies under the top two digits is at
// most half a unit of d_1 per nonzero element); it is positive because the column maximum's significand sits right below bit 46
// for either type (|d_0| >= 16 there, or a column of subnormals whose N are multiples of 2^35: |256 d_0 + d_1| >= 8 per nonzero
// element against the 1/2 subtracted).  Inf / NaN columns are recognised by emax 255, which is what F16Elem reports for exponent
// field 31; a finite fp16 column never counts a rounded element, so its rho is 0.
// TAU_SQ bounds the attained part.  The cross part is attained only by columns whose digit sequences are proportional over the
// tokens; for uncorrelated columns the sums behind it grow like sqrt(tokens) where Cauchy-Schwarz allows tokens, so the measured
// error sits ~4.5 / sqrt(tokens) below X_P (0.02 - 0.035 at 32768 tokens on every family of scripts/probes/i8_error_bound.py).
// Short calls have no such averaging (33 tokens: measured / X_P ~ 0.3), and neither have sparse columns (the sums run over a
// column's nonzero elements: 7033 tokens at 1 % density measured 0.23), hence the threshold on X_P grows with the EFFECTIVE token
// count -- the smallest number of nonzero elements any column of the statistic has:
// guaranteed <= TAU_SQ + tau_x <= 1.1e-11 for any input, and <= 1e-12 measured also on the uncorrelated data of a short or sparse call.
constexpr double TAU_SQ = 1e-12, TAU_X_MIN = 1e-12, TAU_X_MAX = 1e-11, TAU_X_TOKENS = 1024.0;
// The `tolerance` argument of mdg_cov_accum_i8 / _multi: one factor on both thresholds (1 = the figures above), per CALL -- the
// library keeps no accuracy state (two host threads with different factors each get the route of their own factor).  A caller
// who accepts `f` times the guarantee gets five planes where the default asks for six (SiLU-gated activations: X_5 = 3.7e-10,
// i.e. f >= 37); the bound every call computes (RouteOut::sq, ::x) says what was guaranteed either way.
__host__ __device__ inline double tau_x_of(int64_t tokens) {
  return fmin(TAU_X_MAX, fmax(TAU_X_MIN, TAU_X_MIN * ((double)tokens / TAU_X_TOKENS)));
}
constexpr int NVAL = 7;                     // alpha_0 .. alpha_5, rho
constexpr int ROUTE_THREADS = 512;

__device__ __forceinline__ void route_terms(const double (&A)[NVAL], int P, double& sq, double& x) {
  sq = 2.0 * A[6] + A[6] * A[6];
  x = 0.0;
#pragma unroll
  for (int s = 0; s < NP; s++)
#pragma unroll
    for (int t = 0; t < NP; t++)
      if (s + t >= P) {
        if (s == t) sq += A[s] * A[t];
        else x += A[s] * A[t];
      }
}
__device__ __forceinline__ double route_violation(const double (&A)[NVAL], int P, double tau_x) {
  double sq, x;
  route_terms(A, P, sq, x);
  return fmax(sq / TAU_SQ, x / tau_x);
}

struct Top2 { double m1; int a1; double m2; };
__device__ __forceinline__ void top2_merge(Top2& a, const Top2& b) {   // (lowest index wins among equals: the model's argmax)
  if (b.m1 > a.m1 || (b.m1 == a.m1 && b.a1 < a.a1)) {
    a.m2 = fmax(a.m1, b.m2);
    a.m1 = b.m1;
    a.a1 = b.a1;
  } else {
    a.m2 = fmax(a.m2, b.m1);
  }
}

// Scratch of the multi-workgroup first pass, per workgroup: the top two of its columns and the maxima of the 64 column classes.
struct RoutePartial {
  Top2 top[NVAL];
  unsigned long long cls[NVAL][64];
  unsigned min_nnz;              // fewest nonzero elements of any (not all-zero) column
};

// Grid: one workgroup per ROUTE_THREADS columns.  Every workgroup turns its columns' integers into alpha_s / rho (kept in `vals`
// for the greedy) and leaves its partial maxima in `partial`; the LAST one to finish (ticket) merges them and decides -- so the
// ~10 fp64 square roots per column are spread over the chip and the common case (nothing has to leave) ends there.
__global__ __launch_bounds__(ROUTE_THREADS) void i8_route_kernel(const unsigned long long* __restrict__ stats, int* emax, int n, int64_t n_tokens,
                                                                 double* __restrict__ vals, RoutePartial* partial, RouteScratch* scratch,
                                                                 int* flag, RouteOut* out, int* route_counts, double tolerance) {
  __shared__ unsigned long long group_max[NVAL][64];   // per quantity: maxima of the 64 column classes j % 64 (bit patterns of doubles >= 0)
  __shared__ Top2 wave_top[ROUTE_THREADS / 64][NVAL];
  __shared__ Top2 top[NVAL];
  __shared__ double floor_of[NVAL];
  __shared__ int decision;   // -1: keep going; 0: accepted; 1: this P cannot be reached
  __shared__ int forced_total, my_ticket;
  __shared__ unsigned min_nnz;
  __shared__ double tau_x_shared;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < NVAL * 64; i += ROUTE_THREADS) (&group_max[0][0])[i] = 0ull;
  if (tid == 0) min_nnz = 0xffffffffu;
  __syncthreads();
  // top two of every quantity over the columns still on the int8 path: block reduction of per-thread results into top[]
  auto reduce_top = [&](Top2 (&t)[NVAL]) {
#pragma unroll
    for (int i = 0; i < NVAL; i++) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        Top2 o;
        o.m1 = __shfl_xor(t[i].m1, off);
        o.a1 = __shfl_xor(t[i].a1, off);
        o.m2 = __shfl_xor(t[i].m2, off);
        top2_merge(t[i], o);
      }
      if (lane == 0) wave_top[wave][i] = t[i];
    }
    __syncthreads();
    if (tid < NVAL) {
      Top2 r = wave_top[0][tid];
      for (int w = 1; w < ROUTE_THREADS / 64; w++) top2_merge(r, wave_top[w][tid]);
      top[tid] = r;
    }
    __syncthreads();
  };
  // pass 1 (every workgroup): alpha_s(j), rho_j of its column from the integers; columns with an Inf / NaN (emax 255) leave at once
  Top2 t[NVAL];
#pragma unroll
  for (int i = 0; i < NVAL; i++) t[i] = Top2{-1.0, 0x7fffffff, -1.0};
  {
    const int j = blockIdx.x * ROUTE_THREADS + tid;
    bool nonfinite = false;
    if (j < n) {
      double q[NSTAT];
#pragma unroll
      for (int i = 0; i < NSTAT - 1; i++) q[i] = i == STAT_D0D1 ? (double)(long long)stats[(int64_t)i * n + j] : (double)stats[(int64_t)i * n + j];
      const unsigned long long counts = stats[(int64_t)STAT_COUNTS * n + j];
      const int ex = emax[j];
      const double nnz = (double)(unsigned)counts, rounded = (double)(unsigned)(counts >> 32);
      const double hi2 = 65536.0 * q[0] + 512.0 * q[STAT_D0D1] + q[1];
      const double norm = (sqrt(fmax(hi2, 0.0)) - 0.5 * sqrt(nnz)) * 4294967296.0;
      // (norm <= 0 can only happen for a column of denormals, which has nothing below plane 1; 1e300 keeps the test conservative)
      const double inv = nnz > 0 ? (norm > 0 ? 1.0 / norm : 1e300) : 0.0;
      double a[NVAL];
#pragma unroll
      for (int s2 = 0; s2 < NP; s2++) a[s2] = q[s2] > 0 ? sqrt(q[s2]) * ldexp(1.0, 8 * (NP - 1 - s2)) * inv : 0.0;
      a[6] = rounded > 0 ? 0.5 * sqrt(rounded) * inv : 0.0;
      nonfinite = (ex & 255) == 255;
      if ((unsigned)counts) atomicMin(&min_nnz, (unsigned)counts);
#pragma unroll
      for (int i = 0; i < NVAL; i++) {
        vals[(int64_t)i * n + j] = a[i];
        if (!nonfinite) t[i] = Top2{a[i], j, -1.0};
      }
      if (nonfinite) emax[j] = ex | EMAX_COLUMN_OUT;
    }
#pragma unroll
    for (int i = 0; i < NVAL; i++)
      if (t[i].m1 > 0.0) atomicMax(&group_max[i][lane], (unsigned long long)__double_as_longlong(t[i].m1));   // (column j is in class j % 64 = lane)
    const unsigned long long nf = __ballot(nonfinite);
    if (lane == 0 && nf) atomicAdd(&scratch->forced, __popcll(nf));
  }
  reduce_top(t);
  // hand the partial results over; the last workgroup to arrive goes on
  RoutePartial& mine = partial[blockIdx.x];
  if (tid < NVAL) mine.top[tid] = top[tid];
  if (tid == 0) mine.min_nnz = min_nnz;
  for (int i = tid; i < NVAL * 64; i += ROUTE_THREADS) (&mine.cls[0][0])[i] = (&group_max[0][0])[i];
  __threadfence();
  __syncthreads();
  if (tid == 0) my_ticket = atomicAdd(&scratch->ticket, 1);
  __syncthreads();
  if (my_ticket != (int)gridDim.x - 1) return;
  __threadfence();
  // (the merges take the partials four workgroups at a time: four independent loads in flight instead of a chain of gridDim.x
  //  dependent round trips -- the merge order does not enter the result, top2_merge breaks ties by column index)
  const unsigned nwg = gridDim.x;
  if (tid < NVAL) {
    Top2 r = partial[0].top[tid];
    unsigned w = 1;
    for (; w + 4 <= nwg; w += 4) {
      const Top2 b0 = partial[w].top[tid], b1 = partial[w + 1].top[tid], b2 = partial[w + 2].top[tid], b3 = partial[w + 3].top[tid];
      top2_merge(r, b0); top2_merge(r, b1); top2_merge(r, b2); top2_merge(r, b3);
    }
    for (; w < nwg; w++) top2_merge(r, partial[w].top[tid]);
    r.m1 = fmax(r.m1, 0.0);
    r.m2 = fmax(r.m2, 0.0);
    top[tid] = r;
  }
  for (int i = tid; i < NVAL * 64; i += ROUTE_THREADS) {
    unsigned long long m = 0ull;
    unsigned w = 0;
    for (; w + 4 <= nwg; w += 4) {
      const unsigned long long v0 = (&partial[w].cls[0][0])[i], v1 = (&partial[w + 1].cls[0][0])[i], v2 = (&partial[w + 2].cls[0][0])[i],
                               v3 = (&partial[w + 3].cls[0][0])[i];
      m = max(max(m, v0), max(max(v1, v2), v3));
    }
    for (; w < nwg; w++) m = max(m, (&partial[w].cls[0][0])[i]);
    (&group_max[0][0])[i] = m;
  }
  if (tid == 0) {
    forced_total = scratch->forced;
    unsigned m = 0xffffffffu;
    unsigned w = 0;
    for (; w + 4 <= nwg; w += 4) {
      const unsigned v0 = partial[w].min_nnz, v1 = partial[w + 1].min_nnz, v2 = partial[w + 2].min_nnz, v3 = partial[w + 3].min_nnz;
      m = min(min(m, v0), min(min(v1, v2), v3));
    }
    for (; w < nwg; w++) m = min(m, partial[w].min_nnz);
    tau_x_shared = tau_x_of(min(n_tokens, (int64_t)m));
  }
  __syncthreads();
  const double tau_x = tau_x_shared;
  int n_out = 0;
  if (forced_total > ROUTE_JMAX) {      // too many: the whole statistic goes through the fp64 kernel
    if (tid == 0) {
      out->planes = 0; out->n_out = 0; out->sq = out->x = out->rho = 0.0;
      atomicOr(flag, 2);
    }
    for (int j = tid; j < n; j += ROUTE_THREADS) emax[j] &= 255;
    return;
  }
  if (forced_total) {                   // (rare: listed in index order by one thread)
    if (tid == 0)
      for (int j = 0; j < n; j++)
        if (emax[j] & EMAX_COLUMN_OUT) out->out[n_out++] = j;
    __syncthreads();
  }
  const int n_forced = forced_total;
  // Whatever ROUTE_JMAX columns leave, the (ROUTE_JMAX + 1)-th largest value of every quantity stays.  A lower bound on it without
  // sorting: the (ROUTE_JMAX + 1 - forced)-th largest of the 64 class maxima (that many DISTINCT columns are at least as large).
  if (wave == 0) {
    const int want = ROUTE_JMAX - n_forced;        // 0-based rank among the class maxima
#pragma unroll 1
    for (int i = 0; i < NVAL; i++) {
      const unsigned long long mine = group_max[i][lane];
      int rank = 0;
      for (int k = 0; k < 64; k++) {
        const unsigned long long o = group_max[i][k];
        rank += (o > mine || (o == mine && k < lane));
      }
      if (rank == want) floor_of[i] = __longlong_as_double((long long)mine);
    }
  }
  __syncthreads();
  double fl[NVAL];
#pragma unroll
  for (int i = 0; i < NVAL; i++) fl[i] = floor_of[i];
  bool top_valid = true;
  for (int P = 5; P <= 6; P++) {
    if (n > 64 && route_violation(fl, P, tau_x) > tolerance) continue;   // hopeless for this P (uniform: every thread computes the same)
    n_out = n_forced;
    for (;;) {
      if (!top_valid) {             // (the first look uses pass 1's result)
        top_valid = true;
#pragma unroll
        for (int i = 0; i < NVAL; i++) t[i] = Top2{-1.0, 0x7fffffff, -1.0};
        constexpr int PASS1_COLS = 4;     // (four columns' loads in flight per thread)
        for (int j0 = tid; j0 < n; j0 += ROUTE_THREADS * PASS1_COLS) {
          double v[PASS1_COLS][NVAL];
          int ex[PASS1_COLS];
#pragma unroll
          for (int c = 0; c < PASS1_COLS; c++) {
            const int j = j0 + c * ROUTE_THREADS;
            ex[c] = j < n ? emax[j] : EMAX_COLUMN_OUT;
#pragma unroll
            for (int i = 0; i < NVAL; i++) v[c][i] = j < n ? vals[(int64_t)i * n + j] : 0.0;
          }
#pragma unroll
          for (int c = 0; c < PASS1_COLS; c++)
            if (!(ex[c] & EMAX_COLUMN_OUT)) {
#pragma unroll
              for (int i = 0; i < NVAL; i++) top2_merge(t[i], Top2{v[c][i], j0 + c * ROUTE_THREADS, -1.0});
            }
        }
        reduce_top(t);
      }
      if (tid == 0) {
        double A[NVAL];
#pragma unroll
        for (int i = 0; i < NVAL; i++) {
          top[i].m1 = fmax(top[i].m1, 0.0);
          top[i].m2 = fmax(top[i].m2, 0.0);
          A[i] = top[i].m1;
        }
        decision = -1;
        if (route_violation(A, P, tau_x) <= tolerance) {
          out->planes = P;
          out->n_out = n_out;
          route_terms(A, P, out->sq, out->x);
          out->rho = 2.0 * A[6] + A[6] * A[6];
          if (P == 6) atomicOr(flag, 1);
          if (route_counts && n_out) atomicAdd(route_counts + 3, n_out);
          decision = 0;
        } else if (n_out == ROUTE_JMAX) {
          decision = 1;
        } else {
          int best = -1;
          double best_v = 1e308;
          for (int qi = 0; qi < NVAL; qi++) {      // candidates: the columns that hold a maximum, in quantity order
            const int c = top[qi].a1;
            if (c == 0x7fffffff) continue;
            double A2[NVAL];
#pragma unroll
            for (int i = 0; i < NVAL; i++) A2[i] = top[i].a1 == c ? top[i].m2 : top[i].m1;
            const double v = route_violation(A2, P, tau_x);
            if (v < best_v) { best_v = v; best = c; }
          }
          if (best < 0) decision = 1;              // (no column left)
          else {
            emax[best] |= EMAX_COLUMN_OUT;
            out->out[n_out] = best;
          }
        }
      }
      __syncthreads();
      const int dec = decision;
      __syncthreads();
      if (dec == 0) return;
      if (dec == 1) break;
      n_out++;
      top_valid = false;
    }
    // this P cannot be reached: take the greedy picks back (the forced columns stay out)
    if (n_out > n_forced) {
      for (int j = tid; j < n; j += ROUTE_THREADS)
        if ((emax[j] & EMAX_COLUMN_OUT) && (emax[j] & 255) != 255) emax[j] &= 255;
      top_valid = false;
      __syncthreads();
    }
  }
  if (tid == 0) {
    out->planes = 0; out->n_out = 0; out->sq = out->x = out->rho = 0.0;
    atomicOr(flag, 2);
  }
  for (int j = tid; j < n; j += ROUTE_THREADS) emax[j] &= 255;
}

// Columns the route took off the int8 path no longer matter to the product -- but their digits would still cost it: a bulk 12
// binades under its spikes puts a nonzero into plane 3 of every piece of its 32-row group, and the five-plane kernel then runs
// that group's deep-plane blocks in every k-step of every tile of its row and column block (measured: +2 % on the whole launch
// for four such columns, through the tiles' per-step barrier).  So their rows of the digit planes are zeroed and the piece masks
// of their groups recomputed: one wave per (column, k-step), lane = (half, row) -- a piece is read as the product kernel reads
// it, 1 KB per plane.  Enqueued with every call; every workgroup exits at once when no column left.
__global__ __launch_bounds__(256) void i8_clear_columns_kernel(const RouteOut* route, const int* flag, const int* emax, signed char* planes,
                                                               unsigned char* zmask, int n, int nk) {
  if ((*flag & 2) || (int)blockIdx.x >= route->n_out) return;
  const int j = route->out[blockIdx.x];
  const int64_t groups = n / 32;
  const int G = j >> 5, lane = threadIdx.x & 63, row = lane & 31;
  const bool row_out = (emax[G * 32 + row] & EMAX_COLUMN_OUT) != 0;     // (every column of this group that left, not only j)
  for (int kt = blockIdx.y * 4 + (threadIdx.x >> 6); kt < nk; kt += gridDim.y * 4) {
    const unsigned old_mask = zmask[(int64_t)kt * groups + G];
    unsigned new_mask = 0;
#pragma unroll
    for (int s = 0; s < NP; s++) {
      // planes the split pass did not write here (all-zero pieces of planes 4, 5) are not touched: nothing reads them
      if (s >= ALWAYS_WRITTEN_PLANES && (old_mask >> s) == 0) continue;
      i32x4* p = (i32x4*)(planes + ((s * groups + G) * (int64_t)nk + kt) * 1024) + lane;
      i32x4 v = *p;
      if (row_out) {
        v = (i32x4)0;
        *p = v;
      }
      if (__ballot((v[0] | v[1] | v[2] | v[3]) != 0)) new_mask |= 1u << s;
    }
    if (lane == 0) zmask[(int64_t)kt * groups + G] = (unsigned char)new_mask;
  }
}

// ---- the fp64 column kernel: the rows / columns of sigma that belong to the columns the route took off the int8 path
// (RouteOut::out, at most ROUTE_JMAX per statistic): v_k[c] = sum over tokens of x[t, out[k]] x[t, c] in plain fp64 -- the
// reference's arithmetic (LlamaAdapter.py:127-147) -- for every column c.  One pass over X serves COLK_GROUP such columns: a lane
// owns 8 consecutive columns c (one 16-byte load per token) x the group's columns (64 accumulators), a one-wave workgroup 512
// columns x one of COLK_CHUNKS token chunks; 8 tokens' loads are in flight together, and the group's own values for the next 64
// tokens are fetched while the current 64 are multiplied.  The chunk partials are reduced in chunk order by
// i8_columns_reduce_kernel (run-to-run bit-identical), which adds v_k[c] to sigma[max(c, j)][min(c, j)].  Both launches are
// enqueued with every call and exit at once when the route left every column on the int8 path.  2 x tokens x n flop per column:
// 0.94 GFLOP at the sigma_mlp shape; one pass reads X once (0.94 GB).
constexpr int COLK_GROUP = 8, COLK_CHUNKS = 64, COLK_WG_COLS = 512, COLK_STAGE = 64, COLK_BATCH = 8;
struct ColArgs {
  const bf16_t* x;
  int64_t ld, T;
  int n, vec;                 // vec: rows are 16-byte addressable
  const RouteOut* route;
  const int* flag;            // the statistic's route bits (bit 1: the whole statistic went to the fp64 kernel)
  double* part;               // [ROUTE_JMAX][COLK_CHUNKS][n]
  const unsigned* rowmask;    // MDG_I8_ROWS: tokens that left for the fp64 row kernel read as +0 here (the row kernel adds them for ALL columns)
};

template <class EL, bool RELU, bool ROWS>
__global__ __launch_bounds__(64) void i8_columns_kernel(ColArgs a) {
  const int pass = blockIdx.z;
  const int n_out = a.route->n_out;
  if ((*a.flag & 2) || pass * COLK_GROUP >= n_out) return;
  const int nj = min(COLK_GROUP, n_out - pass * COLK_GROUP);
  __shared__ __attribute__((aligned(16))) double xj[COLK_STAGE][COLK_GROUP];
  const int lane = threadIdx.x;
  const int my_k = lane % COLK_GROUP;                       // staging: lane l fetches column l % 8 of the group for tokens l / 8 + 8 i
  const int my_col = my_k < nj ? a.route->out[pass * COLK_GROUP + my_k] : -1;
  const int c0 = blockIdx.x * COLK_WG_COLS + lane * 8;
  const bool active = c0 < a.n;
  const int64_t chunk_len = (a.T + COLK_CHUNKS - 1) / COLK_CHUNKS;
  const int64_t t0 = blockIdx.y * chunk_len, t1 = min(a.T, t0 + chunk_len);
  const unsigned short* xs = (const unsigned short*)a.x;
  auto fetch_group = [&](int64_t t, unsigned short (&g)[COLK_STAGE / 8]) {
#pragma unroll
    for (int i = 0; i < COLK_STAGE / 8; i++) {
      const int64_t tok = t + lane / COLK_GROUP + 8 * i;
      g[i] = (my_col >= 0 && tok < t1 && !row_left<ROWS>(a.rowmask, tok)) ? (unsigned short)relu_bits<EL, RELU>(xs[tok * a.ld + my_col])
                                                                         : (unsigned short)0;
    }
  };
  double acc[COLK_GROUP][8] = {};
  unsigned short g[COLK_STAGE / 8];
  if (t0 < t1) fetch_group(t0, g);
  for (int64_t t = t0; t < t1; t += COLK_STAGE) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < COLK_STAGE / 8; i++) xj[lane / COLK_GROUP + 8 * i][my_k] = EL::to_f64(g[i]);
    __syncthreads();
    if (t + COLK_STAGE < t1) fetch_group(t + COLK_STAGE, g);
    if (!active) continue;
    const int steps = (int)min((int64_t)COLK_STAGE, t1 - t);
    for (int tb = 0; tb < steps; tb += COLK_BATCH) {
      unsigned w[COLK_BATCH][4];
#pragma unroll
      for (int i = 0; i < COLK_BATCH; i++) {
        const bool in_chunk = t + tb + i < t1;
        const int64_t tok = in_chunk ? t + tb + i : t1 - 1;    // (the address stays inside the chunk ...)
        const bool live = in_chunk && !row_left<ROWS>(a.rowmask, tok);
        if (a.vec) {
          const i32x4 v = *(const i32x4*)(xs + tok * a.ld + c0);
          w[i][0] = v[0]; w[i][1] = v[1]; w[i][2] = v[2]; w[i][3] = v[3];
        } else {
#pragma unroll
          for (int h = 0; h < 4; h++) w[i][h] = xs[tok * a.ld + c0 + 2 * h] | ((unsigned)xs[tok * a.ld + c0 + 2 * h + 1] << 16);
        }
        // ... and a slot beyond the chunk's end contributes exact zeros: the group's staged values are zero there, but the re-read
        // last token may hold an Inf / NaN -- the very columns this kernel exists for -- and 0 * Inf would turn the +-Inf the
        // reference's fp64 product gives into NaN (the same holds for a token that left for the row kernel)
        if (!live) w[i][0] = w[i][1] = w[i][2] = w[i][3] = 0u;
      }
#pragma unroll
      for (int i = 0; i < COLK_BATCH; i++) {
        double xc[8];
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const unsigned wr = relu_pair<EL, RELU>(w[i][h]);
          xc[2 * h] = EL::to_f64(wr & 0xFFFFu);
          xc[2 * h + 1] = EL::to_f64(wr >> 16);
        }
#pragma unroll
        for (int k = 0; k < COLK_GROUP; k++) {
          const double xk = xj[tb + i][k];
#pragma unroll
          for (int c = 0; c < 8; c++) acc[k][c] += xk * xc[c];
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int k = 0; k < COLK_GROUP; k++)
    if (k < nj) {
      double* o = a.part + ((int64_t)(pass * COLK_GROUP + k) * COLK_CHUNKS + blockIdx.y) * a.n + c0;
#pragma unroll
      for (int c = 0; c < 8; c++) o[c] = acc[k][c];
    }
}

__global__ __launch_bounds__(256) void i8_columns_reduce_kernel(ColArgs a, const int* emax, double* sigma, int64_t ld_sigma, int block) {
  const int k = blockIdx.y;
  if ((*a.flag & 2) || k >= a.route->n_out) return;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.n) return;
  const int j = a.route->out[k];
  if (block && c / block != j / block) return;                 // per-head statistics: only the head's own 128 x 128 block exists
  if ((emax[c] & EMAX_COLUMN_OUT) && c < j) return;            // a pair of two such columns belongs to the pass of the smaller index
  double v = 0.0;
  for (int q = 0; q < COLK_CHUNKS; q++) v += a.part[((int64_t)k * COLK_CHUNKS + q) * a.n + c];   // chunk order: reproducible
  const int row = max(c, j), col = min(c, j);
  sigma[(int64_t)row * ld_sigma + col - (block ? row / block * block : 0)] += v;
}

}  // namespace

size_t route_vals_bytes(int64_t n) { return (size_t)(NVAL * n) * sizeof(double) + (size_t)ceil_div(n, (int64_t)ROUTE_THREADS) * sizeof(RoutePartial); }
size_t column_partials_bytes(int64_t n) { return (size_t)ROUTE_JMAX * COLK_CHUNKS * (size_t)n * sizeof(double); }

// a flag per statistic: the launch takes the deepest route any statistic still on the int8 path asks for (launch_route)
int enqueue_route(const I8Call& c, int i, double tolerance) {
  const I8Stat& s = c.stat[i];
  const int n = s.n;
  RoutePartial* partial = (RoutePartial*)(s.vals + (size_t)NVAL * n);
  RouteScratch* scratch = (RouteScratch*)(s.stats() + (size_t)NSTAT * n);      // (inside the region the split stage zeroed)
  hipLaunchKernelGGL(i8_route_kernel, dim3((unsigned)ceil_div(n, ROUTE_THREADS)), dim3(ROUTE_THREADS), 0, c.st, s.stats(), s.emax, n,
                     c.n_tokens, s.vals, partial, scratch, s.route_flag, s.route, c.route_counts, tolerance);
  hipLaunchKernelGGL(i8_clear_columns_kernel, dim3(ROUTE_JMAX, (unsigned)std::min(64, (c.nk + 3) / 4)), dim3(256), 0, c.st,
                     (const RouteOut*)s.route, (const int*)s.route_flag, (const int*)s.emax, s.planes, s.zmask, n, c.nk);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

// the columns the route took off the int8 path: their rows / columns of sigma from the fp64 column kernel (both launches exit at
// once when there are none)
int enqueue_columns(const I8Call& c, int i) {
  const I8Stat& s = c.stat[i];
  ColArgs a;
  a.x = s.x; a.ld = s.ld; a.T = c.n_tokens; a.n = s.n;
  a.vec = s.vec();
  a.route = s.route;
  a.flag = s.route_flag;
  a.part = s.colpart;
  a.rowmask = s.rowmask;
  MDG_I8_DISPATCH_ROWS(c, i8_columns_kernel, dim3((unsigned)ceil_div(s.n, COLK_WG_COLS), COLK_CHUNKS, ROUTE_JMAX / COLK_GROUP), dim3(64), 0, c.st, a);
  hipLaunchKernelGGL(i8_columns_reduce_kernel, dim3((unsigned)ceil_div(s.n, 256), ROUTE_JMAX), dim3(256), 0, c.st, a, (const int*)s.emax, s.sigma,
                     s.ld_sigma, s.block);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg
