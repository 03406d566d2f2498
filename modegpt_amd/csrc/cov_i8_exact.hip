// int8 covariance, the exact route's remainder (the map of the units is at the head of cov_i8.hip): the event lists of the
// elements with digits below plane 2, built before the product launches, and the fp64 remainder products, enqueued after them.
#include <algorithm>

#include "cov_i8.hpp"

namespace mdg {

struct __attribute__((aligned(16))) LoEntry {
  double v;                        // x_lo(token, column) = L 2^(E_column - 172): exact (|L| < 2^24)
  unsigned off, aux;               // byte offset of the token's row in x (token x row pitch x 2);  aux: the same in the x_d copy (token x n x
                                   // 2) -- in a sparse (group, residue) list: the column's index in its group.  The call refuses the exact
                                   // route when x spans 4 GB or more: the walk then spends no 64-bit scalar arithmetic on an address
};

namespace {

// ---- the exact route: no plane pair is dropped.
// An element's 48-bit integer N splits into its top three balanced digits and the rest, N = N_d + L with N_d = d_0 2^40 + d_1 2^32 +
// d_2 2^24 and L = d_3 2^16 + d_4 2^8 + d_5 in [-8421504, 8355711]; X = X_d + X_lo accordingly.  On real activations L is zero for
// almost every element: planes 3 .. 5 are reached only by elements 17 binades and more below their column's maximum -- 3e-5 of a
// Gaussian column, 0.5 % of a SiLU-gated one (whose 1 KB pieces of plane 3 nevertheless hold a nonzero 95 % of the time, which is why
// the truncated six-plane product spends 6 of its 15 plane pairs multiplying a 99.5 %-zero operand).  So
//     X^T X = X_d^T X_d  +  X_lo^T X  +  X_d^T X_lo
//   * X_d^T X_d: the NINE plane pairs of the top three planes, all of them (classes 0 .. 4) -- i8_syrk_kernel<3>, the product
//     kernel's tile code on planes 0 .. 2 alone: exact int32 class sums as before, 9 instead of 9.4 / 15.1 executed pairs;
//   * the two remainder products: every element with L != 0 is an EVENT (token, column, x_lo = L 2^(E - 172)), listed per COLUMN in
//     token order by i8_extract_lo_kernel / i8_compact_lo_kernel.  Two implementations, picked on the device from the list lengths
//     (i8_lo_mode_kernel):
//       sparse lists (Gaussian columns: two events per column) -- i8_lo_product_kernel, one workgroup per 128 x 128 tile of the lower
//         triangle: the lists of the tile's row block (sigma[r][c] += x_lo(t, r) x(t, c), the partner x in full) and of its column
//         block (+= x_d(t, r) x_lo(t, c), the partner's top three planes recomputed from x where it has deeper digits: x_d = 2^24 q
//         floor(x / (2^24 q) + 8421504 / 2^24), the balanced digits' rounding), summed into an fp64 tile in LDS, sigma read and
//         written once;
//       dense lists (SiLU-gated: 156 per column) -- i8_lo_wide_kernel<false / true>, one wave per (column, block of 512 partner
//         columns), eight partner columns per lane, the sums in registers; the second product reads its partner from a bf16 copy of
//         x in which every listed element is replaced by x_d (i8_copy_xd_kernel, i8_patch_xd_kernel).
//     Either way fp64 products of exact operands, every sum owned by ONE wave that adds its events in list order -- run-to-run
//     bit-identical -- and folded into sigma once per product.
// Nothing is truncated: what is left is fp64 rounding (one rounding per fold of the class sums and per event sum) and the rho term
// of the elements more than 38 binades under their column maximum, which the split rounds to an integer (RouteOut::sq keeps it).
// The route kernel's decisions stay as they are -- which columns leave for the fp64 column kernel, whether the whole statistic
// does -- and the exact route then REPLACES the truncated five- or six-plane product whenever every remainder list fits its
// list (LO_CAP events per column and 2048 tokens = 6.2 % of the elements; cubed Gaussians, Student-t: no -- the truncated
// product with its bound takes those as before).  Cost at the sigma_mlp shape (profiles/r04_exact_route_kernels_*.csv): lists 0.08 /
// 0.25 ms, remainder products 0.7 ms (Gaussian; 1.0 with the tile kernel's longer chain of round trips) / 5.4 + 0.5 ms for the copy (SiLU-gated) against 0.4 x 2.1 ... 6.1 x 2.1 ms of
// plane-pair products saved.
constexpr int LO_CHUNK_STEPS = 64;       // k-steps (2048 tokens) per segment of a column's event list
constexpr int LO_CAP = 128;              // events per segment: 6.2 % of its 2048 tokens
constexpr double LO_ROUND = 8421504.0 / 16777216.0;   // (128 (1 + 256 + 65536)) / 2^24: where the balanced digits d_3 d_4 d_5 round
// LoArgs::state is the start of the workspace's shared block as ints: where its three words of the exact route sit
constexpr int EXACT_OVERFLOW = offsetof(SharedBlock, exact_overflow) / sizeof(int), EXACT_RAN = offsetof(SharedBlock, exact_ran) / sizeof(int),
              EXACT_MODE = offsetof(SharedBlock, exact_mode) / sizeof(int);
#ifndef MDG_LO_SPARSE_MEAN
#define MDG_LO_SPARSE_MEAN 32
#endif
#ifndef MDG_LO_SPARSE_MAX
#define MDG_LO_SPARSE_MAX 256
#endif
constexpr int LO_SPARSE_MAX = MDG_LO_SPARSE_MAX;      // sparse lists: at most this many events in any column, LO_SPARSE_MEAN on average
constexpr int LO_SUB = 4, LO_RCAP = 8 * LO_SPARSE_MAX;   // one merged list per (32-column group, column mod 4)
constexpr int LO_TILE = 128, LO_PITCH = LO_TILE + 1;

struct LoProblem {
  const bf16_t* x;
  int64_t ld;
  const signed char* planes;
  const unsigned char* zmask;
  const int* emax;
  LoEntry* entries;                // [n][nch][LO_CAP]: one list per COLUMN, written per segment by i8_extract_lo_kernel, then closed up
                                   // to one contiguous list by i8_compact_lo_kernel
  int* counts;                     // [n][nch] segment lengths, then [n] list lengths (totals)
  double* sigma;
  int64_t ld_sigma;
  bf16_t* xd;                      // [tokens][n]: x with every listed element replaced by its top three digit planes x_d = x - x_lo (which is
                                   // a bf16 again: a rounding of 8 significant bits to a coarser grid) -- the partner of the second product
  int n, block;
  LoEntry* rentries;               // sparse mode: [n / 32][LO_SUB][LO_RCAP] merged lists (i8_residue_lo_kernel) and their lengths
  int* rtotals;
  int tile0[3];                    // this statistic's first workgroup in the grids of the two wide products and of the tile kernel
  int pairs;                       // rows of x are 4-byte addressable: a lane of the tile kernel fetches two neighbouring columns with one load
};
struct LoArgs {
  LoProblem prob[MAX_PROBLEMS];
  int nprob, nk, nch, tiles[3];
  int64_t n_tokens;
  int always;                      // MDG_I8_EXACT_ALWAYS: the exact route for launches of the five-plane class too
  const int* route_flag;
  int* state;                      // shared block of the workspace: [EXACT_OVERFLOW], [EXACT_RAN], [EXACT_MODE]
};
__device__ __forceinline__ int* lo_totals(const LoProblem& pr, int nch) { return pr.counts + (int64_t)pr.n * nch; }
// Is the exact route on offer for this launch?  Always when the caller asks for it; by default where it is the faster product:
// launches of the six-plane class (9 executed plane pairs + the remainder kernel against 15.1), and five-plane launches of a large
// statistic (9 against 9.4 pairs on a kernel without masks or conditional blocks: 21.6 against 22.2 ms per sigma_mlp call on
// Gaussian columns; with two k-steps per stage 20.6) -- below LO_AUTO_MIN_N features the remainder kernel's fixed costs (a workgroup
// per tile, two list walks, one fold) outweigh 0.4 plane pairs (4096 features, 32768 tokens: 2.13 against 2.15 ms on Gaussian, 3.25
// against 3.42 on SiLU-gated columns; 8192: 7.18 / 7.72 and 10.6 / 12.5 -- profiles/r04_exact_route_timing.log).
constexpr int LO_AUTO_MIN_N = 4096;
__device__ __forceinline__ bool lo_offered(const LoArgs& a) {
  if (a.always) return true;
  if (a.prob[0].n >= LO_AUTO_MIN_N && !a.prob[0].block) return true;
  for (int p = 0; p < a.nprob; p++)
    if ((a.route_flag[p] & 3) == 1) return true;
  return false;
}

// One wave per (32-column group, segment of LO_CHUNK_STEPS k-steps): reads the pieces of planes 3 .. 5 the piece masks say are
// there -- as the product kernel would -- and appends every element with L != 0 to ITS COLUMN's segment, in token order (lane r
// holds tokens 0 .. 15 of a k-step of column r, lane 32 + r tokens 16 .. 31: the second appends behind the first).
// (Reads planes and emax only -- the unit 2^(E - 172) is the same for bf16 and fp16, see the element traits -- so it is one kernel
// for both element types.)
__global__ __launch_bounds__(64) void i8_extract_lo_kernel(LoArgs a) {
  const LoProblem& pr = a.prob[blockIdx.z];
  const int64_t groups = pr.n / 32;
  const int G = blockIdx.x, ch = blockIdx.y, lane = threadIdx.x;
  if (!lo_offered(a)) return;
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && lane == 0) a.state[EXACT_RAN] = 1;
  if (G >= groups || (a.route_flag[blockIdx.z] & 2)) return;     // (a statistic that went to the fp64 kernel has no lists)
  const int col = G * 32 + (lane & 31);
  LoEntry* out = pr.entries + ((int64_t)col * a.nch + ch) * LO_CAP;
  const double scale = ldexp(1.0, (pr.emax[col] & 255) - 172);
  int count = 0;                                                  // events of this lane's column so far (the same in both of its lanes)
  const int kt1 = min(a.nk, (ch + 1) * LO_CHUNK_STEPS);
  for (int kt = ch * LO_CHUNK_STEPS; kt < kt1; kt++) {
    const unsigned m = pr.zmask[(int64_t)kt * groups + G];
    if ((m >> 3) == 0) continue;
    const i32x4 zero = (i32x4)0;
    const i32x4 d3 = *((const i32x4*)(pr.planes + ((3 * groups + G) * (int64_t)a.nk + kt) * 1024) + lane);
    const i32x4 d4 = (m >> 4) ? *((const i32x4*)(pr.planes + ((4 * groups + G) * (int64_t)a.nk + kt) * 1024) + lane) : zero;
    const i32x4 d5 = (m >> 5) ? *((const i32x4*)(pr.planes + ((5 * groups + G) * (int64_t)a.nk + kt) * 1024) + lane) : zero;
    const unsigned tok0 = (unsigned)kt * KS + (lane >> 5) * 16;
    int L[16], mine = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int sh = 8 * (q & 3);
      L[q] = (int)(signed char)((unsigned)d3[q >> 2] >> sh) * 65536 + (int)(signed char)((unsigned)d4[q >> 2] >> sh) * 256 +
             (int)(signed char)((unsigned)d5[q >> 2] >> sh);
      mine += L[q] != 0;
    }
    if (__ballot(mine != 0) == 0) continue;
    const int other = __shfl_xor(mine, 32);
    int at = count + ((lane >> 5) ? other : 0);
#pragma unroll
    for (int q = 0; q < 16; q++)
      if (L[q] != 0) {
        if (at < LO_CAP) out[at] = LoEntry{(double)L[q] * scale, (tok0 + q) * (unsigned)(pr.ld * 2), (tok0 + q) * (unsigned)(pr.n * 2)};
        at++;
      }
    count += mine + other;
  }
  if (lane < 32) {
    pr.counts[(int64_t)col * a.nch + ch] = min(count, LO_CAP);
    if (count > LO_CAP) a.state[EXACT_OVERFLOW] = 1;
  }
}

// One wave per column: closes the segments of its list up into one contiguous list, in place (a segment only ever moves towards
// the front, and the wave copies in order), and leaves its length in lo_totals.  The remainder kernel then walks full batches
// whatever the density.
__global__ __launch_bounds__(64) void i8_compact_lo_kernel(LoArgs a) {
  if (!lo_offered(a) || a.state[EXACT_OVERFLOW] != 0) return;
  const LoProblem& pr = a.prob[blockIdx.y];
  const int col = blockIdx.x, lane = threadIdx.x;
  if (col >= pr.n || (a.route_flag[blockIdx.y] & 2)) return;
  const int* counts = pr.counts + (int64_t)col * a.nch;
  LoEntry* base = pr.entries + (int64_t)col * a.nch * LO_CAP;
  int total = 0;
  for (int ch = 0; ch < a.nch; ch++) {
    const int cnt = counts[ch];
    const LoEntry* src = base + (int64_t)ch * LO_CAP;
    if (total != ch * LO_CAP)
      for (int i = 0; i < cnt; i += 64) {
        LoEntry e = LoEntry{0., 0u, 0u};
        if (i + lane < cnt) e = src[i + lane];
        if (i + lane < cnt) base[total + i + lane] = e;      // (the 64 loads of a round are complete before its stores: same wave, in order)
      }
    total += cnt;
  }
  if (lane == 0) lo_totals(pr, a.nch)[col] = total;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// Which remainder kernels run, from the list lengths (one workgroup; read by everything below): SPARSE lists -- at most LO_SPARSE_MAX
// events in any column and LO_SPARSE_MEAN per column on average: Gaussian columns have two per 32768 tokens -- go to the 128 x 128-tile
// kernel, where a tile is one chain of memory round trips around a handful of products and sigma is read and written ONCE for both
// products; anything denser (SiLU-gated: 164 per column and 32768 tokens) to the wide kernels, which need 2.4 x fewer instructions per
// product but pay 0.5 ms for the x_d copy and a dependent chain per (column, partner block).  Measured at the sigma_mlp width, whole
// call, SiLU-gated columns, 2048 / 4096 / 8192 / 16384 / 32768 tokens = 10 / 20 / 41 / 82 / 164 events per column
// (scripts/probes/lo_mode_crossover.sh, profiles/r04_lo_mode_crossover.log): tiles 3.11 / 4.78 / 8.23 / 15.3 / 29.8 ms, wide 3.79 /
// 5.25 / 8.15 / 14.0 / 26.6 -- they cross at ~38; Gaussian columns at 32768 tokens: tiles 1.0 ms, wide 1.8 + 0.5.
constexpr int LO_SPARSE_MEAN = MDG_LO_SPARSE_MEAN;
__global__ __launch_bounds__(1024) void i8_lo_mode_kernel(LoArgs a) {
  if (!lo_offered(a) || a.state[EXACT_OVERFLOW] != 0) return;
  __shared__ long long sums[16];
  __shared__ int maxs[16];
  long long sum = 0, cols = 0;
  int mx = 0;
  for (int p = 0; p < a.nprob; p++) {
    if (a.route_flag[p] & 2) continue;
    const LoProblem& pr = a.prob[p];
    cols += pr.n;
    for (int c = threadIdx.x; c < pr.n; c += 1024) {
      const int t = lo_totals(pr, a.nch)[c];
      sum += t;
      mx = max(mx, t);
    }
  }
  for (int o = 32; o; o >>= 1) {
    sum += __shfl_xor(sum, o);
    mx = max(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) { sums[threadIdx.x >> 6] = sum; maxs[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) { sum += sums[w]; mx = max(mx, maxs[w]); }
    a.state[EXACT_MODE] = (mx <= LO_SPARSE_MAX && sum <= LO_SPARSE_MEAN * cols) ? 1 : 2;
  }
}

// SPARSE: the lists of the eight columns 4 k + sub of a group, one behind the other, as ONE list per (group, residue) -- the unit a wave
// of the tile kernel walks (it owns the accumulators of those rows / columns); `aux` = the column's index in its group.  One wave
// per list; at most 8 x 64 entries.
__global__ __launch_bounds__(64) void i8_residue_lo_kernel(LoArgs a) {
  if (a.state[EXACT_MODE] != 1) return;
  const LoProblem& pr = a.prob[blockIdx.y];
  const int id = blockIdx.x, lane = threadIdx.x;
  if (id >= pr.n / 32 * LO_SUB || (a.route_flag[blockIdx.y] & 2)) return;
  const int G = id / LO_SUB, sub = id % LO_SUB;
  LoEntry* out = pr.rentries + (int64_t)id * LO_RCAP;
  int at = 0;
  for (int k = 0; k < 8; k++) {
    const int col = G * 32 + 4 * k + sub;
    const int cnt = lo_totals(pr, a.nch)[col];           // <= LO_SPARSE_MAX (the mode says so)
    for (int i = lane; i < cnt; i += 64) {
      LoEntry e = pr.entries[(int64_t)col * a.nch * LO_CAP + i];
      e.aux = 4 * k + sub;
      out[at + i] = e;
    }
    at += cnt;
  }
  if (lane == 0) pr.rtotals[id] = at;
}

// DENSE: x_d starts as a copy of x (16 bytes per thread and step; n is a multiple of 128), then every listed element is replaced by
// x_d = x - x_lo -- exactly (both are multiples of the column's unit, below 2^48 of them), and a value of x's type again: a
// rounding of x's significand to a coarser grid.  bf16: 8 significant bits at most, exponent range of the column.  fp16: a listed
// element lies k = sh - 11 >= 1 bits under the grid 2^24 units = 2^(E - 148), so x_d = M 2^(E - 148) with |M| = round(|sig| / 2^k) <=
// 2^(11 - k): at most 11 significant bits, no larger than the column maximum, and the grid is no finer than fp16's own 2^-24 -- in a
// column with E < 124 every element is a multiple of 2^24 units and nothing is listed.  (Checked over every bit pattern and shift:
// tests/test_i8_f16_host.py.)  ReLU is applied by the copy; a listed element is nonzero after it, hence positive and unchanged.
// One wave per column for the second step.
template <class EL, bool RELU>
__global__ __launch_bounds__(256) void i8_copy_xd_kernel(LoArgs a) {
  if (a.state[EXACT_MODE] != 2) return;
  const LoProblem& pr = a.prob[blockIdx.y];
  if (a.route_flag[blockIdx.y] & 2) return;
  const int64_t per_row = pr.n / 8, total = a.n_tokens * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / per_row, c = (i - t * per_row) * 8;
    typedef unsigned u32x4u __attribute__((ext_vector_type(4), aligned(2)));
    const u32x4u v = *(const u32x4u*)(pr.x + t * pr.ld + c);
    *(u32x4*)(pr.xd + t * pr.n + c) = (u32x4){relu_pair<EL, RELU>(v[0]), relu_pair<EL, RELU>(v[1]), relu_pair<EL, RELU>(v[2]), relu_pair<EL, RELU>(v[3])};
  }
}
template <class EL, bool RELU>
__global__ __launch_bounds__(64) void i8_patch_xd_kernel(LoArgs a) {
  if (a.state[EXACT_MODE] != 2) return;
  const LoProblem& pr = a.prob[blockIdx.y];
  const int col = blockIdx.x, lane = threadIdx.x;
  if (col >= pr.n || (a.route_flag[blockIdx.y] & 2)) return;
  const int total = lo_totals(pr, a.nch)[col];
  const LoEntry* list = pr.entries + (int64_t)col * a.nch * LO_CAP;
  for (int i = lane; i < total; i += 64) {
    const LoEntry e = list[i];
    const double xd = EL::to_f64(*(const bf16_t*)((const char*)pr.x + e.off + 2 * col)) - e.v;
    *(bf16_t*)((char*)pr.xd + e.aux + 2 * col) = (bf16_t)EL::from_f64(xd);
  }
}

__device__ __forceinline__ void lds_add_f64(double* p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_f64, returnless: issued in order per wave
}
// Where row (column) i of the tile sits in the LDS accumulator: even indices in the first half, odd ones in the second.  A lane
// fetches two NEIGHBOURING partner columns with one load; stored side by side its two ds_add_f64 would put the 64 lanes on a 16-byte
// stride -- four lanes per bank pair, a four-way conflict on every atomic of the kernel (the walk was bound by exactly that:
// 10.6 ms at the sigma_mlp shape on SiLU-gated data).  Permuted, the lanes of an atomic cover 512 contiguous bytes (row-event) or
// one 8-byte word per 1032-byte row (column-event): the two passes a 64-lane fp64 access needs anyway.
__device__ __forceinline__ int lo_perm(int i) { return (i >> 1) + 64 * (i & 1); }

// The events of ONE list -- 32-column group G, columns with (column mod 4) == sub -- in list order, by ONE wave, which thereby owns
// the accumulators they touch.  COLS = false: G is row group g of the tile's row block: acc[g 32 + r][c] += x_lo(t, r) x(t, c) for
// the 128 columns c of the tile's column block (lane: c = 2 lane, 2 lane + 1).  COLS = true: G is column group g of the column
// block: acc[r][g 32 + c] += x_d(t, r) x_lo(t, c) for the 128 rows r of the row block (lane: r = 2 lane, 2 lane + 1), x_d the
// partner's top three digit planes -- which IS x for every element within 14 binades of its column maximum (no digit below plane
// 2), so the rounding is taken only when a lane meets a deeper one.  partner0: first column of the partner block.
// The walk is bound by the latency of the partner loads (one 4-byte load per event and lane, rows scattered over the tokens) and
// by the VALU and the LDS atomics (7 - 14 operations per event): the events go in batches of LO_UN whose loads are all issued
// before the previous batch is multiplied (two batches in flight per wave, sixteen waves per CU).  A Gaussian list holds ~16
// events: at 32 slots per batch half of them were padding -- a partner load and two ds_add_f64 of an exact zero each -- so a batch
// is 16 slots, and a list's last (or only) batch 8 when no more are left (LO_SHORT; wave-uniform).  Leaving padding out changes
// no bit: an accumulator is never -0 (it starts at +0, and a sum that cancels gives +0), so adding +-0 to it is the identity
// (0 x Inf is not +-0, but a column that holds an Inf or a NaN has left for the fp64 column kernel and its sums are not stored).
constexpr int LO_UN = 16;
#ifndef MDG_LO_SHORT
#define MDG_LO_SHORT 8
#endif
constexpr int LO_SHORT = MDG_LO_SHORT;       // 0: every batch LO_UN wide
constexpr int LO_HEAD = 64;                  // entries of a list's head: one per lane, i.e. batches 0 .. LO_HEAD / LO_UN - 1
// The length of a list and its head, one entry per lane (lanes beyond the list's end: the last entry's token, v = 0: exact
// zeros) -- fetched for BOTH passes of a tile before the first one starts.  The kernel has the length already (its first round
// trip), so the head is ONE dependent load, and a list of up to 64 events never fetches entries again.  The load is not
// conditional (an empty list reads its slot's first entry, which is inside the buffer, and uses nothing of it): behind a branch
// each of a wave's two heads was waited for inside its branch, one round trip after the other.
struct LoFirst {
  int cnt;
  LoEntry m;
};
__device__ __forceinline__ LoFirst lo_first(const LoProblem& pr, const int list_id, const int cnt, const int lane) {
  LoFirst f;
  f.cnt = cnt;
  f.m = pr.rentries[(int64_t)list_id * LO_RCAP + min(lane, max(cnt, 1) - 1)];
  if (lane >= cnt) f.m.v = 0.;
  return f;
}
// The partner loads of the slots U0 .. U1 - 1 of a batch, whose entries sit in lanes e0 .. of m_off (the entries' row offsets);
// col0 = the lane's first partner column.
template <class EL, bool RELU, int U0, int U1>
__device__ __forceinline__ void lo_issue_n(const LoProblem& pr, const unsigned m_off, const int e0, const int col0, unsigned (&xv)[LO_UN]) {
  if (pr.pairs) {
#pragma unroll
    for (int u = U0; u < U1; u++) {
      const unsigned off = (unsigned)__builtin_amdgcn_readlane((int)m_off, e0 + u);
      xv[u] = relu_pair<EL, RELU>(*(const unsigned*)((const unsigned short*)((const char*)pr.x + off) + col0));
    }
  } else {
#pragma unroll
    for (int u = U0; u < U1; u++) {
      const unsigned off = (unsigned)__builtin_amdgcn_readlane((int)m_off, e0 + u);
      const unsigned short* row = (const unsigned short*)((const char*)pr.x + off) + col0;
      xv[u] = relu_pair<EL, RELU>((unsigned)row[0] | ((unsigned)row[1] << 16));
    }
  }
}
// ... of a batch with `left` events still to go (wave-uniform): the short width when they fit it.  (Written as "the first slots,
// then perhaps the rest", not as two whole batches of either width: hipcc merges the equal tails of two such branches into stores
// at a variable index, and the batch then lives in scratch.)
constexpr int LO_FIRST_SLOTS = LO_SHORT ? LO_SHORT : LO_UN;
template <class EL, bool RELU>
__device__ __forceinline__ void lo_issue(const LoProblem& pr, const unsigned m_off, const int e0, const int left, const int col0,
                                         unsigned (&xv)[LO_UN]) {
  lo_issue_n<EL, RELU, 0, LO_FIRST_SLOTS>(pr, m_off, e0, col0, xv);
  if (LO_SHORT && left > LO_SHORT) lo_issue_n<EL, RELU, LO_FIRST_SLOTS, LO_UN>(pr, m_off, e0, col0, xv);
}
// ... and its products: acc += x_lo (the entry's v, broadcast) x partner, two per lane.  COLS: the partner's top three digit planes;
// its rows' digit grid is 2^24 units of their own scale, q = 2^(E - 148) = 2^sa, 2^sb (kept as exponents: the scalings are
// v_ldexp_f64 in the rare branch that needs them, not four fp64 registers held through the walk); an element has a digit below
// plane 2 iff its exponent field is below a limit set by E (and it is not zero): 0 < |bits| < deep_limit(E) = lim_a, lim_b
template <class EL, bool COLS, int U0, int U1>
__device__ __forceinline__ void lo_multiply_n(double* acc, const LoEntry& m, const int e0, const unsigned (&xv)[LO_UN], const int g, const int lane,
                                              const int sa, const int sb, const unsigned lim_a, const unsigned lim_b) {
#pragma unroll
  for (int u = U0; u < U1; u++) {
    const double v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(m.v), e0 + u), __builtin_amdgcn_readlane(__double2loint(m.v), e0 + u));
    const int col = __builtin_amdgcn_readlane((int)m.aux, e0 + u);
    double pa = EL::to_f64(xv[u] & 0xFFFFu), pb = EL::to_f64(xv[u] >> 16);
    if (COLS) {
      const bool deep = ((xv[u] & 0x7FFFu) - 1u < lim_a - 1u) || (((xv[u] >> 16) & 0x7FFFu) - 1u < lim_b - 1u);
      if (__ballot(deep)) {
        pa = ldexp(floor(ldexp(pa, -sa) + LO_ROUND), sa);                // exact (powers of two, one floor)
        pb = ldexp(floor(ldexp(pb, -sb) + LO_ROUND), sb);
      }
      lds_add_f64(acc + lane * LO_PITCH + lo_perm(g * 32 + col), v * pa);            // rows 2 lane, 2 lane + 1
      lds_add_f64(acc + (64 + lane) * LO_PITCH + lo_perm(g * 32 + col), v * pb);
    } else {
      lds_add_f64(acc + lo_perm(g * 32 + col) * LO_PITCH + lane, v * pa);            // columns 2 lane, 2 lane + 1
      lds_add_f64(acc + lo_perm(g * 32 + col) * LO_PITCH + 64 + lane, v * pb);
    }
  }
}
// x0: the partner loads of the list's first batch, issued by the kernel (lo_issue with e0 = 0, left = the list's length) before
// the tile's first barrier -- for both passes, so that the second does not start with a memory round trip of its own.
// ea, eb (COLS): emax of the lane's two partner rows.
template <class EL, bool RELU, bool COLS>
__device__ __forceinline__ void lo_events(const LoProblem& pr, const int list_id, const int partner0, const int g, const int lane, double* acc,
                                          const LoFirst& first, const unsigned (&x0)[LO_UN], const int ea, const int eb) {
  const int cnt = first.cnt;
  if (cnt == 0) return;
  const int sa = (ea & 255) - 148, sb = (eb & 255) - 148;
  const unsigned lim_a = COLS ? EL::deep_limit(ea & 255) : 0u, lim_b = COLS ? EL::deep_limit(eb & 255) : 0u;
  const int col0 = partner0 + 2 * lane;
  const LoEntry* list = pr.rentries + (int64_t)list_id * LO_RCAP;
  // batch k: events [k LO_UN, ...).  Its entries: lanes e0 .. of the head while that lasts, then one entry per lane (mod LO_UN) of
  // a fetch of its own (lanes beyond the list's end: the last entry's token, v = 0: exact zeros)
  auto entries = [&](int k, LoEntry& m, int& e0) {
    if (k < LO_HEAD / LO_UN) {
      m = first.m;
      e0 = k * LO_UN;
    } else {
      m = list[min(k * LO_UN + (lane & (LO_UN - 1)), cnt - 1)];
      if (k * LO_UN + (lane & (LO_UN - 1)) >= cnt) m.v = 0.;
      e0 = 0;
    }
  };
  auto multiply = [&](const LoEntry& m, const int e0, const int left, const unsigned (&xv)[LO_UN]) {
    lo_multiply_n<EL, COLS, 0, LO_FIRST_SLOTS>(acc, m, e0, xv, g, lane, sa, sb, lim_a, lim_b);
    if (LO_SHORT && left > LO_SHORT) lo_multiply_n<EL, COLS, LO_FIRST_SLOTS, LO_UN>(acc, m, e0, xv, g, lane, sa, sb, lim_a, lim_b);
  };
  const int nb = (cnt + LO_UN - 1) / LO_UN;
  LoEntry mA = first.m, mB = first.m;
  int eA = 0, eB = 0;
  unsigned xA[LO_UN], xB[LO_UN];
#pragma unroll
  for (int u = 0; u < LO_UN; u++) xA[u] = x0[u];
  for (int k = 0; k < nb; k += 2) {
    if (k + 1 < nb) {
      entries(k + 1, mB, eB);
      lo_issue<EL, RELU>(pr, mB.off, eB, cnt - (k + 1) * LO_UN, col0, xB);
    }
    __builtin_amdgcn_sched_barrier(0);    // (batch B's loads are out before batch A's are waited for: hipcc would sink each load to its use)
    multiply(mA, eA, cnt - k * LO_UN, xA);
    if (k + 1 >= nb) break;
    if (k + 2 < nb) {
      entries(k + 2, mA, eA);
      lo_issue<EL, RELU>(pr, mA.off, eA, cnt - (k + 2) * LO_UN, col0, xA);
    }
    __builtin_amdgcn_sched_barrier(0);
    multiply(mB, eB, cnt - (k + 1) * LO_UN, xB);
  }
}

// One workgroup of sixteen waves per 128 x 128 tile of the lower triangle (per-head statistics: the diagonal tiles; a head is one
// tile, block == LO_TILE): wave (g, sub) takes the list `sub` of row group g, then of column group g.
// A tile is a chain of memory round trips around a handful of products, and one workgroup fills a CU (132 KB of LDS), so the chain
// is what a tile costs.  It is three long: (1) the launch's state words and, beside them, the lengths of the wave's two lists (which
// also decide the early exit) and emax of the tile's rows and columns; (2) the heads of both lists -- and, issued before them, the
// thread's 16 elements of sigma for the fold, whether or not they will be stored; (3) the first batch of partner rows of BOTH
// passes.  The fold then has everything in registers.  (It used to be seven: state, the lengths, the lengths again, the two
// heads one after the other, each pass's partners with emax, emax before the fold, sigma behind emax.)  No load leaves the
// statistic's buffers: n is a multiple of LO_TILE, so every row and column of a tile exists; the elements above the diagonal of a
// diagonal tile read sigma[0][0] instead.  Measured at the sigma_mlp shape, Gaussian columns, per launch
// (profiles/lo_sparse_*_kernel_trace_bygrid.csv): 0.98 ms before, 0.69 - 0.71 with all of this; with every batch 16 slots wide (no short
// last batch) 0.74; with the sigma loads behind the first partner loads instead of at entry (a wave's loads return in order, so at
// entry the list heads wait for them, behind the partners only the second batches do) 0.72 -- entry it is.  Not built: two
// workgroups of 128 x 64 per CU.
constexpr int LO_THREADS = 1024;
template <class EL, bool RELU>
__global__ __launch_bounds__(LO_THREADS) void i8_lo_product_kernel(LoArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lo_acc[];     // [128][LO_PITCH]
  int p = 0;
  while (p + 1 < a.nprob && (int)blockIdx.x >= a.prob[p + 1].tile0[2]) p++;
  const LoProblem& pr = a.prob[p];
  const int t = blockIdx.x - pr.tile0[2];
  int bi, bj;
  if (pr.block) {
    bi = bj = t;
  } else {
    bi = (int)((sqrtf(8.f * t + 1.f) - 1.f) * 0.5f);
    while ((bi + 1) * (bi + 2) / 2 <= t) bi++;
    while (bi * (bi + 1) / 2 > t) bi--;
    bj = t - bi * (bi + 1) / 2;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave & 3, sub = wave >> 2;
  constexpr int PER = LO_TILE * LO_TILE / LO_THREADS, ROWS = LO_THREADS / LO_TILE;      // 16 elements per thread, 8 rows apart
  // ---- round trip 1: the launch's state words and, beside them, the small loads of the tile (they lie in the workspace whatever
  // the state says, and a workgroup that leaves at once has spent a few cached loads on them) ...
  const int ran = a.state[EXACT_RAN], overflow = a.state[EXACT_OVERFLOW], mode = a.state[EXACT_MODE], flag = a.route_flag[p];
  const int list_r = (4 * bi + g) * LO_SUB + sub, list_c = (4 * bj + g) * LO_SUB + sub;
  const int len_r = pr.rtotals[list_r], len_c = pr.rtotals[list_c];
  const int ea = pr.emax[bi * LO_TILE + 2 * lane], eb = pr.emax[bi * LO_TILE + 2 * lane + 1];      // rows 2 lane, 2 lane + 1 of the tile
  const int c = tid % LO_TILE, col = bj * LO_TILE + c, row0 = bi * LO_TILE + tid / LO_TILE;
  const int e_col = pr.emax[col];
  __builtin_amdgcn_sched_barrier(0);
  if (ran != 1 || overflow != 0 || mode != 1 || (flag & 2)) return;
  // ... then sigma (128 KB per tile: only for a launch that runs), in flight until the fold
  double* const sigma = pr.sigma;
  const int64_t ld_sigma = pr.ld_sigma, at0 = (int64_t)row0 * ld_sigma + col - (pr.block ? bi * LO_TILE : 0);
  double old[PER];
#pragma unroll
  for (int u = 0; u < PER; u++) {      // (every row of the tile exists; above the diagonal: offset 0, by a mask -- no branch around a load)
    const int64_t at = at0 + (int64_t)u * ROWS * ld_sigma;
    old[u] = sigma[at & -(int64_t)(col <= row0 + u * ROWS)];
  }
  for (int i = tid; i < LO_TILE * LO_PITCH; i += LO_THREADS) lo_acc[i] = 0.;      // (under the loads; the early exit's barrier is theirs too)
  __builtin_amdgcn_sched_barrier(0);      // (all of the above is issued before the first of it is waited for)
  // anything to do?  (the sixteen waves hold the lists of the tile's four row groups and four column groups between them)
  const int cnt_r = __builtin_amdgcn_readfirstlane(len_r), cnt_c = __builtin_amdgcn_readfirstlane(len_c);
  if (!__syncthreads_or(cnt_r | cnt_c)) return;
  // ---- round trip 2: the heads of both lists;  3: their first batches of partner rows
  const LoFirst first_rows = lo_first(pr, list_r, cnt_r, lane), first_cols = lo_first(pr, list_c, cnt_c, lane);
  unsigned x_rows[LO_UN], x_cols[LO_UN];
  if (cnt_r) lo_issue<EL, RELU>(pr, first_rows.m.off, 0, cnt_r, bj * LO_TILE + 2 * lane, x_rows);
  if (cnt_c) lo_issue<EL, RELU>(pr, first_cols.m.off, 0, cnt_c, bi * LO_TILE + 2 * lane, x_cols);
  __builtin_amdgcn_sched_barrier(0);
  lo_events<EL, RELU, false>(pr, list_r, bj * LO_TILE, g, lane, lo_acc, first_rows, x_rows, 0, 0);
  __syncthreads();      // an accumulator changes owner between the two passes: the wave of its row, then the wave of its column
  lo_events<EL, RELU, true>(pr, list_c, bi * LO_TILE, g, lane, lo_acc, first_cols, x_cols, ea, eb);
  __syncthreads();
  // the fold: sigma and emax are here already; the tests decide only the store (rows / columns of the fp64 column kernel are not ours)
  const int e_rows = (wave & 2) ? eb : ea;      // the thread's rows tid / 128 + 8 u: all of one parity, row r in lane r / 2
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int r = tid / LO_TILE + u * ROWS, row = bi * LO_TILE + r;
    const double v = lo_acc[lo_perm(r) * LO_PITCH + lo_perm(c)];
    const int e_row = __builtin_amdgcn_readlane(e_rows, (wave >> 2) + u * (ROWS / 2));
    if (col <= row && v != 0. && !((e_row | e_col) & EMAX_COLUMN_OUT)) sigma[at0 + (int64_t)u * ROWS * ld_sigma] = old[u] + v;
  }
}

// The two remainder products.  One workgroup = the 16 columns of group G against a block of LW_BLOCK = 512 partner columns; wave w
// owns column G 16 + w, and every lane EIGHT neighbouring partner columns (one 16-byte load
// per event), whose eight sums it keeps in registers while it walks the column's list -- one v_fma_f64 per product, events in list
// order (run-to-run bit-identical; no atomics, no LDS) -- and adds to sigma when the column is done:
//   TR = false   sigma[r][c] += sum_t x_lo(t, r) x(t, c)      for the partner columns c <= r   (X_lo^T X, lower part; a contiguous row)
//   TR = true    sigma[c][r] += sum_t x_lo(t, r) x_d(t, c)    for the partner columns c >= r   (X_d^T X_lo, lower part; partner x_d from
//                the copy, so both products are the same loop: the first versions recomputed x_d from x whenever a lane met an
//                element with digits below plane 2 -- at eight columns per lane nearly every event does)
// Two launches, the second after the first (an entry of sigma gets a sum from each).  Why this shape: the kernel is bound by its
// INSTRUCTION stream -- per event and wave three broadcasts and an address, then per product an unpack, a conversion and the fma; at
// two partner columns per lane (the 128 x 128-tile versions: profiles/r04_exact_route_kernels_silu_gated.csv, 9.3 ms) the fixed part
// and two LDS atomics per event were most of it.  Workgroups run partner block by partner block (P-major): the 256 that are
// resident walk their lists in token order over the SAME 512 columns of x -- 32 MB that stay in the memory-side cache.
#ifndef MDG_LW_UN
#define MDG_LW_UN 8
#endif
#ifndef MDG_LW_OCC
#define MDG_LW_OCC 0      // 8: two workgroups per CU (64 VGPRs)
#endif
#if MDG_LW_OCC
#define LW_OCC_ATTR __attribute__((amdgpu_waves_per_eu(MDG_LW_OCC, MDG_LW_OCC)))
#else
#define LW_OCC_ATTR
#endif
constexpr int LW_COLS = 8, LW_BLOCK = 64 * LW_COLS, LW_UN = MDG_LW_UN, LW_GROUP = 16, LW_TP = LW_GROUP + 1;
template <class EL, bool RELU, bool TR>
__global__ __launch_bounds__(LO_THREADS) LW_OCC_ATTR void i8_lo_wide_kernel(LoArgs a) {
  if (a.state[EXACT_RAN] != 1 || a.state[EXACT_OVERFLOW] != 0 || a.state[EXACT_MODE] != 2) return;
  int p = 0;
  while (p + 1 < a.nprob && (int)blockIdx.x >= a.prob[p + 1].tile0[TR]) p++;
  if (a.route_flag[p] & 2) return;
  const LoProblem& pr = a.prob[p];
  const int n = pr.n, nG = n / LW_GROUP;
  constexpr int PER = LW_BLOCK / LW_GROUP;     // groups per partner block
  int t = blockIdx.x - pr.tile0[TR], G, P = 0;
  if (pr.block) {            // per-head statistics: the one partner block is the head
    G = t;
  } else {                   // partner block P of 512 columns, then the groups that have a column on the right side of it
    for (;;) {
      const int cnt = TR ? min(nG, PER * (P + 1)) : nG - PER * P;
      if (t < cnt) break;
      t -= cnt;
      P++;
    }
    G = TR ? t : PER * P + t;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const char* const xs = TR ? (const char*)pr.xd : (const char*)pr.x;
  typedef unsigned u32x4u __attribute__((ext_vector_type(4), aligned(2)));
  __shared__ double tr_tile[TR ? LW_BLOCK * LW_TP : 1];      // TR: [partner row][column of the group], for the transposed fold
  const int r = G * LW_GROUP + wave;
  const int total = __builtin_amdgcn_readfirstlane(lo_totals(pr, a.nch)[r]);
  const bool r_ours = total != 0 && !(pr.emax[r] & EMAX_COLUMN_OUT);
  const LoEntry* list = pr.entries + (int64_t)r * a.nch * LO_CAP;
  LoEntry m0 = LoEntry{0., 0u, 0u};            // the first 64 entries of the column's list: one per lane
  if (r_ours) {
    m0 = list[min(lane, min(total, 64) - 1)];
    if (lane >= total) m0.v = 0.;              // (padding: the last entry's row, exact zeros)
  }
  {
    const int p0 = pr.block ? G * LW_GROUP / pr.block * pr.block : P * LW_BLOCK;
    const int pend = pr.block ? p0 + pr.block : min(n, p0 + LW_BLOCK);
    const int c0 = p0 + LW_COLS * lane;                                   // this lane's partner columns c0 .. c0 + 7
    // which of them exist, are ours (columns of the fp64 column kernel are not) and lie on this product's side of the diagonal
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < LW_COLS; j++)
      if (c0 + j < pend && !(pr.emax[c0 + j] & EMAX_COLUMN_OUT) && (TR ? c0 + j >= r : c0 + j <= r)) mine |= 1u << j;
    const unsigned lane_off = (unsigned)(c0 + LW_COLS <= pend ? c0 : p0) * 2u;   // (lanes beyond the block read its first columns; never used)
    const bool walk = r_ours && __ballot(mine != 0) != 0;
    double acc[LW_COLS];
#pragma unroll
    for (int j = 0; j < LW_COLS; j++) acc[j] = 0.;
    if (walk) {
      // super-batches of 64 entries (one per lane, broadcast with v_readlane), batches of LW_UN events whose partner loads are all
      // issued before the previous batch is multiplied
      for (int sb = 0; sb < total; sb += 64) {
        const int len = min(64, total - sb);
        LoEntry m = m0;
        if (sb) {
          m = list[sb + min(lane, len - 1)];
          if (lane >= len) m.v = 0.;
        }
        const unsigned moff = TR ? m.aux : m.off;
        u32x4 xa[LW_UN], xb[LW_UN];
        auto issue = [&](int b, u32x4 (&xv)[LW_UN]) {
#pragma unroll
          for (int u = 0; u < LW_UN; u++) {
            const unsigned o = (unsigned)__builtin_amdgcn_readlane((int)moff, b * LW_UN + u) + lane_off;
            const u32x4u q = *(const u32x4u*)(xs + o);
            xv[u] = (u32x4){q[0], q[1], q[2], q[3]};
          }
        };
        auto multiply = [&](int b, const u32x4 (&xv)[LW_UN]) {
#pragma unroll
          for (int u = 0; u < LW_UN; u++) {
            const double v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(m.v), b * LW_UN + u),
                                              __builtin_amdgcn_readlane(__double2loint(m.v), b * LW_UN + u));
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const unsigned w = TR ? xv[u][q] : relu_pair<EL, RELU>(xv[u][q]);      // (the x_d copy has the ReLU in it)
              acc[2 * q] = fma(v, EL::lo_f64(w), acc[2 * q]);
              acc[2 * q + 1] = fma(v, EL::hi_f64(w), acc[2 * q + 1]);
            }
          }
        };
        const int nb = (len + LW_UN - 1) / LW_UN;      // 1 .. 8 batches
        issue(0, xa);
        for (int b = 0; b < nb; b += 2) {
          __builtin_amdgcn_sched_barrier(0);
          if (b + 1 < nb) issue(b + 1, xb);
          __builtin_amdgcn_sched_barrier(0);
          multiply(b, xa);
          if (b + 1 >= nb) break;
          __builtin_amdgcn_sched_barrier(0);
          if (b + 2 < nb) issue(b + 2, xa);
          __builtin_amdgcn_sched_barrier(0);
          multiply(b + 1, xb);
        }
      }
    }
    if (!TR) {
      if (!walk) return;
      // the column's sums into its row of sigma (64 contiguous bytes per lane): all loads first
      double* s[LW_COLS];
      double old[LW_COLS];
#pragma unroll
      for (int j = 0; j < LW_COLS; j++) {
        s[j] = (mine >> j & 1) ? pr.sigma + (int64_t)r * pr.ld_sigma + c0 + j - (pr.block ? r / pr.block * pr.block : 0) : nullptr;
        old[j] = s[j] ? *s[j] : 0.;
      }
#pragma unroll
      for (int j = 0; j < LW_COLS; j++)
        if (s[j]) *s[j] = old[j] + acc[j];
      return;
    }
    // TR: the sums belong to COLUMN r of sigma.  Written from here they are 8-byte accesses a row pitch apart, sixteen waves on the
    // same 128-byte lines one after the other (measured: the fold's L2 requests were 80 % of the walk's); through LDS every thread
    // folds eight neighbouring columns of one partner row, 64 contiguous bytes.
#pragma unroll
    for (int j = 0; j < LW_COLS; j++) tr_tile[(LW_COLS * lane + j) * LW_TP + wave] = (walk && (mine >> j & 1)) ? acc[j] : 0.;
    __syncthreads();
    {
      const int i = p0 + (threadIdx.x >> 1), half = threadIdx.x & 1;      // partner row i, columns G 16 + 8 half ..
      if (i < pend && !(pr.emax[i] & EMAX_COLUMN_OUT)) {
        double v[8], old[8];
        double* s[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int col = G * LW_GROUP + 8 * half + k;
          v[k] = tr_tile[(i - p0) * LW_TP + 8 * half + k];
          s[k] = (v[k] != 0. && col <= i) ? pr.sigma + (int64_t)i * pr.ld_sigma + col - (pr.block ? i / pr.block * pr.block : 0) : nullptr;
          old[k] = s[k] ? *s[k] : 0.;
        }
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (s[k]) *s[k] = old[k] + v[k];
      }
    }
  }
}

template <bool TR>
void launch_lo_wide(const I8Call& c, const LoArgs& lo) {
  const dim3 grid((unsigned)lo.tiles[TR]), block(LO_THREADS);
  if (c.f16) {
    if (c.relu) hipLaunchKernelGGL((i8_lo_wide_kernel<F16Elem, true, TR>), grid, block, 0, c.st, lo);
    else hipLaunchKernelGGL((i8_lo_wide_kernel<F16Elem, false, TR>), grid, block, 0, c.st, lo);
  } else {
    if (c.relu) hipLaunchKernelGGL((i8_lo_wide_kernel<Bf16Elem, true, TR>), grid, block, 0, c.st, lo);
    else hipLaunchKernelGGL((i8_lo_wide_kernel<Bf16Elem, false, TR>), grid, block, 0, c.st, lo);
  }
}

int lo_chunks(int64_t T) { return (int)ceil_div(ceil_div(T, (int64_t)KS), (int64_t)LO_CHUNK_STEPS); }

LoArgs lo_args(const I8Call& c, bool always) {
  LoArgs lo;
  lo.nprob = c.count;
  lo.nk = c.nk;
  lo.nch = lo_chunks(c.n_tokens);
  lo.route_flag = c.shared->route_flag;
  lo.state = c.shared->reserved;
  lo.always = always ? 1 : 0;
  lo.n_tokens = c.n_tokens;
  int tiles[3] = {0, 0, 0};
  for (int i = 0; i < c.count; i++) {
    const I8Stat& s = c.stat[i];
    LoProblem& l = lo.prob[i];
    l.x = s.x; l.ld = s.ld;
    l.planes = s.planes; l.zmask = s.zmask; l.emax = s.emax;
    l.entries = s.lo_entries;
    l.xd = s.lo_xd;
    l.rentries = s.lo_rentries;
    l.rtotals = s.lo_rtotals;
    l.pairs = ((uintptr_t)s.x % 4 == 0) && (s.ld % 2 == 0);
    l.counts = s.lo_counts;
    l.sigma = s.sigma; l.ld_sigma = s.ld_sigma;
    l.n = s.n; l.block = s.block;
    const int nG = s.n / LW_GROUP, per = LW_BLOCK / LW_GROUP;
    for (int tr = 0; tr < 2; tr++) {
      l.tile0[tr] = tiles[tr];
      if (s.block) {
        tiles[tr] += nG;
      } else {
        for (int P = 0; P * per < nG; P++) tiles[tr] += tr ? std::min(nG, per * (P + 1)) : nG - per * P;
      }
    }
    l.tile0[2] = tiles[2];
    const int rbi = s.n / TI;
    tiles[2] += s.block ? rbi : rbi * (rbi + 1) / 2;
  }
  for (int i = c.count; i < MAX_PROBLEMS; i++) lo.prob[i] = lo.prob[0];
  for (int k = 0; k < 3; k++) lo.tiles[k] = tiles[k];
  return lo;
}

}  // namespace

LoWsBytes lo_ws_bytes(int64_t n_tokens, int64_t n) {
  LoWsBytes b;
  b.entries = (size_t)n * lo_chunks(n_tokens) * LO_CAP * sizeof(LoEntry);      // [n][chunks][LO_CAP] x 16 bytes
  b.counts = (size_t)n * (lo_chunks(n_tokens) + 1) * sizeof(int);
  b.xd = (size_t)n * (size_t)n_tokens * sizeof(bf16_t);
  b.rentries = (size_t)(n / 32) * LO_SUB * LO_RCAP * sizeof(LoEntry);
  b.rtotals = (size_t)(n / 32) * LO_SUB * sizeof(int);
  return b;
}

// the remainder lists of every statistic (planes 3 .. 5, after the route's columns were cleared); the product launches then read
// the outcome -- {overflow, ran} -- from the shared block
int enqueue_lo_lists(const I8Call& c, bool always) {
  const LoArgs lo = lo_args(c, always);
  int max_groups = 0;
  for (int i = 0; i < c.count; i++) max_groups = std::max(max_groups, c.stat[i].n / 32);
  const unsigned count = (unsigned)c.count;
  hipLaunchKernelGGL(i8_extract_lo_kernel, dim3((unsigned)max_groups, (unsigned)lo.nch, count), dim3(64), 0, c.st, lo);
  hipLaunchKernelGGL(i8_compact_lo_kernel, dim3((unsigned)(max_groups * 32), count), dim3(64), 0, c.st, lo);
  hipLaunchKernelGGL(i8_lo_mode_kernel, dim3(1), dim3(1024), 0, c.st, lo);
  hipLaunchKernelGGL(i8_residue_lo_kernel, dim3((unsigned)(max_groups * LO_SUB), count), dim3(64), 0, c.st, lo);
  MDG_I8_DISPATCH(c, i8_copy_xd_kernel, dim3(2048u, count), dim3(256), 0, c.st, lo);
  MDG_I8_DISPATCH(c, i8_patch_xd_kernel, dim3((unsigned)(max_groups * 32), count), dim3(64), 0, c.st, lo);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

// the remainder products (every workgroup exits at once when the truncated product ran instead)
int enqueue_lo_products(const I8Call& c, bool always) {
  const LoArgs lo = lo_args(c, always);
  const size_t lds = (size_t)LO_TILE * LO_PITCH * sizeof(double);
  const void* tile_kernel = c.f16 ? (c.relu ? (const void*)i8_lo_product_kernel<F16Elem, true> : (const void*)i8_lo_product_kernel<F16Elem, false>)
                                  : (c.relu ? (const void*)i8_lo_product_kernel<Bf16Elem, true> : (const void*)i8_lo_product_kernel<Bf16Elem, false>);
  MDG_HIP(hipFuncSetAttribute(tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  MDG_I8_DISPATCH(c, i8_lo_product_kernel, dim3((unsigned)lo.tiles[2]), dim3(LO_THREADS), lds, c.st, lo);          // sparse lists
  launch_lo_wide<false>(c, lo);       // dense lists: X_lo^T X,
  launch_lo_wide<true>(c, lo);        // then X_d^T X_lo
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg
