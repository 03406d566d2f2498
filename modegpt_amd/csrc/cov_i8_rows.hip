// int8 covariance, outlier token rows (flag MDG_I8_ROWS; the map of the units is at the head of cov_i8.hip): which rows leave the
// int8 path, and their contribution to sigma in plain fp64.
//
// WHY.  The split measures every element against its COLUMN's maximum exponent E_j.  A handful of tokens whose activations are
// large across many columns raises every E_j at once, the bulk of every column then sits deeper under its maximum, the exact
// route's event lists overflow and the bound of the truncated product fails in more columns than the fp64 column kernel takes:
// the whole statistic drops to the fp64 kernel.  Rows are the easy direction out: X^T X = sum_t x_t x_t^T is additive over the
// tokens, so for any row set R
//     X^T X = X_rest^T X_rest + X_R^T X_R                     (no cross terms)
// -- the int8 path runs on X with the rows of R read as +0 (column maxima, split, route statistics, event lists, fp64 column
// kernel: `row_left` in cov_i8.hpp), and i8_rows_product_kernel adds the rank-|R| update in the reference's own arithmetic
// (fp64 sums of products, LlamaAdapter.py:127-147).
//
// THE RULE (host model: tests/i8_rows_model.py).  A deterministic function of the exponent fields of x -- integers only, no
// floating-point sum, no host round trip; run-to-run bit-identical:
//   1. E_j = the column maxima over ALL rows (the maximum pass of cov_i8_split.hip, as without the flag).
//   2. Votes: v_t = the number of columns j in which x_tj is nonzero and ee(x_tj) >= E_j - ROW_WINDOW (ee: the effective
//      exponent of the element traits; ReLU on load is honoured; ROW_WINDOW = 4 binades).
//   3. Row t is DOMINANT when v_t >= n / ROW_SHARE (ROW_SHARE = 8): it comes within four binades of the maximum in an eighth of
//      all columns.  On ordinary data most rows are dominant -- each column's maximum has thousands of rows within a few binades
//      of it; when a few tokens are far larger than the rest, only those are.
//   4. If 1 .. MDG_I8_MAX_ROWS (64) rows are dominant AND they are at most an eighth of the call (dominant x ROW_MINORITY <=
//      tokens: without this a call of 64 tokens or fewer, where every row is dominant, would leave as a whole), they leave:
//      listed in ascending token order (RowsOut), their bits set in the row bitmask.
//   5. Otherwise -- no dominant row, more than 64, or not a minority -- nothing leaves and the call proceeds exactly as without
//      the flag: every kernel after this one sees an all-zero mask and the column maxima of step 1.
//   6. When rows left, the column maxima are computed again over the rows that stayed (the second maximum pass; it exits on its
//      first instruction otherwise).
// ONE ROUND ONLY.  Two tiers of outliers (rows x 2^16 and rows x 2^8 together: only the upper tier is dominant, the lower one
// stays and sets the maxima of the rest) and a continuum of token scales (the lognormal family, scripts/probes/i8_fuzz.py kind 7:
// no gap between "the few" and "the rest") are out of scope -- such statistics take the route they took without the flag.
// The constants come from a sweep of the host model over the families of tests/test_gpu_i8_f16.py and the outlier scenarios of
// tests/test_i8_rows_host.py (W in 2 .. 8, share 1/4 .. 1/32): see DESIGN.md section 7.
//
// THE ROW KERNEL.  sigma += X_R^T X_R over the rows that left, for ALL columns (the column kernel skips those rows: nothing is
// counted twice), on v_mfma_f64_16x16x4_f64: one workgroup per 128 x 128 tile of the lower triangle (per-head statistics: the
// diagonal tiles), the rows staged in LDS 16 at a time, widened exactly to fp64, k in ascending token order, no atomics -- run-to-run
// bit-identical.  Like the int8 fold it writes the entries with column <= row only; the upper half of a diagonal tile is not
// touched.  Bound by the read-modify-write of the triangle: 8 n^2 bytes.  Every workgroup exits on its first instruction when no
// row left or when the statistic went to the fp64 kernel as a whole (flag bit 1): that kernel reads every row of x itself.
// Rounding: products of two bf16 / fp16 values are exact in fp64; each of the |R| additions (and the one into sigma) rounds once,
// relative to a partial sum that Cauchy-Schwarz bounds by sqrt(sigma_ii sigma_jj): (|R| + 1) 2^-53, which mdg_cov_accum_i8_route
// adds to bound[0].
#include <algorithm>

#include "cov_i8.hpp"

namespace mdg {
namespace {

constexpr int ROW_WINDOW = 4;        // binades under the column maximum within which an element votes for its row
constexpr int ROW_SHARE = 8;         // a row is dominant when it votes in n / ROW_SHARE columns
constexpr int ROW_MINORITY = 8;      // rows leave only when dominant x ROW_MINORITY <= tokens
constexpr int VOTE_SPAN = 1024;      // columns a workgroup of the vote pass walks per token
constexpr int VOTE_TOKENS = 128;     // tokens per workgroup of the vote pass
constexpr int SELECT_THREADS = 1024;

// lane = (token lane tl, column group cg): 16 tokens x 16 groups of 8 columns per step, VOTE_SPAN / 128 steps per token; the votes
// of a token are summed over its 16 lanes and leave the workgroup as one integer atomic.
template <class EL, bool RELU>
__global__ __launch_bounds__(256) void i8_row_votes_kernel(const bf16_t* x, int64_t ld, int64_t T, int n, int vec, const int* emax,
                                                           int* votes) {
  __shared__ __attribute__((aligned(16))) int thr[VOTE_SPAN];
  const int c_begin = blockIdx.y * VOTE_SPAN;
  const int span = min(VOTE_SPAN, n - c_begin);          // a multiple of 128
  // a nonzero element has ee >= 1 and a zero reports 0: with the threshold at least 1, zeros never vote
  for (int i = threadIdx.x; i < span; i += 256) thr[i] = max((emax[c_begin + i] & 255) - ROW_WINDOW, 1);
  __syncthreads();
  const int cg = threadIdx.x & 15, tl = threadIdx.x >> 4;
  const int64_t slab0 = (int64_t)blockIdx.x * VOTE_TOKENS, t1 = min(T, slab0 + VOTE_TOKENS);
  for (int64_t tb = slab0; tb < t1; tb += 16) {
    const int64_t t = tb + tl;
    const bool live = t < t1;
    int cnt = 0;
    if (live) {
      const bf16_t* row = x + t * ld + c_begin;
#pragma unroll
      for (int cb = 0; cb < VOTE_SPAN / 128; cb++) {
        const int jl = cb * 128 + cg * 8;
        if (jl >= span) break;
        unsigned w[4];
        if (vec) {
          const i32x4 v = *(const i32x4*)(row + jl);
          w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
        } else {
#pragma unroll
          for (int h = 0; h < 4; h++) w[h] = row[jl + 2 * h] | ((unsigned)row[jl + 2 * h + 1] << 16);
        }
        const i32x4 h0 = *(const i32x4*)(thr + jl), h1 = *(const i32x4*)(thr + jl + 4);
        const int th[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const unsigned wr = relu_pair<EL, RELU>(w[q]);
          cnt += (EL::ee_if_nonzero(wr & 0xFFFFu) >= th[2 * q]) + (EL::ee_if_nonzero(wr >> 16) >= th[2 * q + 1]);
        }
      }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) cnt += __shfl_xor(cnt, off);
    if (live && cg == 0 && cnt) atomicAdd(votes + t, cnt);
  }
}

// One workgroup: thread i owns a contiguous range of tokens, so that an exclusive scan of the per-thread counts puts the dominant
// rows into the list in ascending token order.
__global__ __launch_bounds__(SELECT_THREADS) void i8_row_select_kernel(const int* votes, int64_t T, int n, unsigned* rowmask, RowsOut* out,
                                                                       int* emax) {
  __shared__ int cnt[SELECT_THREADS];
  const int tid = threadIdx.x;
  const int64_t chunk = (T + SELECT_THREADS - 1) / SELECT_THREADS;
  const int64_t a = min(T, tid * chunk), b = min(T, a + chunk);
  const int need = n / ROW_SHARE;                        // (n is a multiple of 128)
  int mine = 0;
  for (int64_t t = a; t < b; t++) mine += votes[t] >= need;
  cnt[tid] = mine;
  __syncthreads();
  for (int off = 1; off < SELECT_THREADS; off <<= 1) {
    const int v = tid >= off ? cnt[tid - off] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  const int n_dom = cnt[SELECT_THREADS - 1];
  const bool leave = n_dom >= 1 && n_dom <= ROWS_MAX && (int64_t)n_dom * ROW_MINORITY <= T;
  if (tid == 0) {
    out->n_dominant = n_dom;
    out->n_rows = leave ? n_dom : 0;
  }
  if (!leave) return;
  int k = cnt[tid] - mine;
  if (mine)
    for (int64_t t = a; t < b; t++)
      if (votes[t] >= need) {
        out->rows[k++] = (int)t;
        atomicOr(rowmask + (t >> 5), 1u << (t & 31));
      }
  for (int j = tid; j < n; j += SELECT_THREADS) emax[j] = 0;      // the second maximum pass starts from zero
}

struct RowArgs {
  const bf16_t* x;
  int64_t ld;
  int block;                  // 0: n x n lower triangle; 128: per-head statistics, diagonal tiles only
  const RowsOut* rows;
  const int* flag;            // the statistic's route bits (bit 1: the whole statistic went to the fp64 kernel)
  double* sigma;
  int64_t ld_sigma;
  int* route_counts;
};

template <class EL, bool RELU>
__global__ __launch_bounds__(256) void i8_rows_product_kernel(RowArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[2 * PANEL];
  __shared__ int tok[ROWS_MAX];
  const int nr = a.rows->n_rows;
  if (nr == 0 || (*a.flag & 2)) return;
  int bi, bj;
  if (a.block) bi = bj = blockIdx.x;
  else tri_decode(blockIdx.x, bi, bj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  if (tid < ROWS_MAX) tok[tid] = tid < nr ? a.rows->rows[tid] : -1;
  if (blockIdx.x == 0 && tid == 0 && a.route_counts) atomicAdd(a.route_counts + 5, nr);
  __syncthreads();
  const bool diag = bi == bj;
  double* const As = lds;
  double* const Bs = diag ? lds : lds + PANEL;
  const unsigned short* xs = (const unsigned short*)a.x;
  Acc acc;
  acc_zero(acc);
  for (int k0 = 0; k0 < nr; k0 += BK) {    // BK rows at a time, ascending; rows past the list are exact zeros
    if (k0) __syncthreads();
#pragma unroll
    for (int i = 0; i < BK / 2; i++) {
      const int k = (tid >> 7) + 2 * i, f = tid & 127;
      const int t = tok[k0 + k];
      double va = 0., vb = 0.;
      if (t >= 0) {
        const unsigned short* row = xs + (int64_t)t * a.ld;
        va = EL::to_f64(relu_bits<EL, RELU>(row[bi * TILE + f]));
        if (!diag) vb = EL::to_f64(relu_bits<EL, RELU>(row[bj * TILE + f]));
      }
      As[k * PITCH + f] = va;
      if (!diag) Bs[k * PITCH + f] = vb;
    }
    __syncthreads();
    mma_stage(As, Bs, wr, wc, lane, acc);
  }
#pragma unroll
  for (int sa = 0; sa < 4; sa++)
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int gr = bi * TILE + acc_row(wr, lane, sa, reg);
      const int gc0 = bj * TILE + acc_col(wc, lane, 0);
      double* row = a.sigma + (int64_t)gr * a.ld_sigma + gc0 - (a.block ? gr / a.block * a.block : 0);
#pragma unroll
      for (int sb = 0; sb < 4; sb++)
        if (gc0 + sb <= gr) row[sb] += acc.v[sa][sb][reg];     // the fold's footprint: nothing above the diagonal
    }
}

}  // namespace

RowsWsBytes rows_ws_bytes(int64_t n_tokens) {
  RowsWsBytes b;
  b.mask = align_up((size_t)ceil_div(n_tokens, (int64_t)32) * sizeof(unsigned), 256);      // T / 8 bytes
  b.votes = align_up((size_t)n_tokens * sizeof(int), 256);
  b.out = align_up(sizeof(RowsOut), 256);
  return b;
}

// after the first maximum pass: votes against those maxima, the selection, the bitmask
int enqueue_row_selection(const I8Call& c, int i) {
  const I8Stat& s = c.stat[i];
  const RowsWsBytes b = rows_ws_bytes(c.n_tokens);
  MDG_HIP(hipMemsetAsync(s.rowmask, 0, b.mask + b.votes + b.out, c.st));     // (one region: mask, votes, list)
  MDG_I8_DISPATCH(c, i8_row_votes_kernel, dim3((unsigned)ceil_div(c.n_tokens, (int64_t)VOTE_TOKENS), (unsigned)ceil_div(s.n, VOTE_SPAN)),
                  dim3(256), 0, c.st, s.x, s.ld, c.n_tokens, s.n, (int)s.vec(), (const int*)s.emax, s.votes);
  hipLaunchKernelGGL(i8_row_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, c.st, (const int*)s.votes, c.n_tokens, s.n, s.rowmask,
                     s.rows_out, s.emax);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

// after the products: the rows that left, in fp64 (exits at once when there are none)
int enqueue_rows_product(const I8Call& c, int i) {
  const I8Stat& s = c.stat[i];
  RowArgs a;
  a.x = s.x; a.ld = s.ld; a.block = s.block;
  a.rows = s.rows_out;
  a.flag = s.route_flag;
  a.sigma = s.sigma; a.ld_sigma = s.ld_sigma;
  a.route_counts = c.route_counts;
  const int64_t nb = s.n / TILE;
  MDG_I8_DISPATCH(c, i8_rows_product_kernel, dim3((unsigned)(s.block ? nb : nb * (nb + 1) / 2)), dim3(256), 0, c.st, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg
