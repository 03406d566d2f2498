// int8 covariance, first stage (the map of the units is at the head of cov_i8.hip): column maxima, the split of the bf16 or fp16
// activations into six digit planes with the route statistics and the piece masks.  Every kernel here is a template on the
// element traits (EL: Bf16Elem / F16Elem, cov_i8.hpp), on ReLU-on-load and on ROWS (MDG_I8_ROWS: a token whose bit is set in
// `rowmask` reads as +0; the ROWS = false instantiations never look at the pointer).
#include <algorithm>

#include "cov_i8.hpp"

namespace mdg {
namespace {

// An element more than EL::TOP binades under its column maximum (bf16 only; in an fp16 column only beside an Inf / NaN, and such a
// column leaves the int8 path) is rounded to an integer: the magnitude half up; nothing survives a shift by more than SIG_BITS + 1.
template <class EL>
__device__ __forceinline__ long long fixed_point(int sig, int sh, bool& rounded) {
  rounded = sh > EL::TOP;
  if (!rounded) return (long long)sig << (EL::TOP - sh);
  const int dn = sh - EL::TOP;
  const int mag = dn > EL::SIG_BITS + 1 ? 0 : ((sig < 0 ? -sig : sig) + (1 << (dn - 1))) >> dn;
  return sig < 0 ? -mag : mag;
}

template <class EL, bool RELU, bool ROWS>
__global__ __launch_bounds__(256) void i8_colmax_kernel(const bf16_t* x, int64_t ld, int64_t T, int n, int64_t rows_per_block,
                                                        int* emax, const unsigned* rowmask, const RowsOut* rows_out) {
  if (ROWS && rows_out->n_rows == 0) return;     // (the second maximum pass: no row left, the first pass's maxima stand)
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int64_t t0 = (int64_t)blockIdx.y * rows_per_block + (threadIdx.x >> 6);
  const int64_t t1 = min(T, (int64_t)(blockIdx.y + 1) * rows_per_block);
  int best = 1;
  if (j < n)
    for (int64_t t = t0; t < t1; t += 4) {
      int sig, ee;
      EL::parts(relu_bits<EL, RELU>(x[t * ld + j]), sig, ee);
      if (sig != 0 && !row_left<ROWS>(rowmask, t)) best = max(best, ee);
    }
  if (j < n) atomicMax(emax + j, best);
}

// Piece mask: one byte per (k-step, 32-row group), bit s set when the 1 KB piece of plane s there holds any nonzero digit.  An
// element is two full digits and a carry digit (see FLUSH_STEPS), so on real activations whole pieces of the lower planes are
// zero -- Gaussian columns: plane 3 in 90 % of the pieces, planes 4 and 5 always; SiLU-gated: plane 4 in 98 % -- and the
// product kernel neither loads nor multiplies those.  Called with the 32 rows of a piece in the 32 lanes of a half-wave.
__device__ __forceinline__ unsigned write_piece_mask(const unsigned (&any)[NP], unsigned char* zmask, int64_t index) {
  unsigned byte = 0;
#pragma unroll
  for (int s = 0; s < NP; s++) {
    const unsigned long long b = __ballot(any[s] != 0);
    const unsigned half = (threadIdx.x & 32) ? (unsigned)(b >> 32) : (unsigned)b;
    byte |= (half != 0) << s;
  }
  if ((threadIdx.x & 31) == 0) zmask[index] = (unsigned char)byte;
  return byte;     // the mask of the caller's own piece (its half-wave)
}

// One thread = one feature row of a 32-row group x one k-step (32 tokens) at a time: two 16-byte stores per plane and
// k-step.  A workgroup walks SPLIT_STEPS k-steps of its row group, 8 at a time.
constexpr int SPLIT_STEPS = 64;
template <class EL, bool RELU, bool ROWS>
__global__ __launch_bounds__(256) void i8_split_kernel(const bf16_t* x, int64_t ld, int64_t T, int n, int nk, const int* emax,
                                                       signed char* planes, unsigned long long* stats, unsigned char* zmask,
                                                       const unsigned* rowmask) {
  __shared__ unsigned long long st_lds[NSTAT][32];
  const int r = threadIdx.x & 31;
  const int G = blockIdx.x;
  const int j = G * 32 + r;
  const int E = emax[j];
  const int64_t groups = n / 32;
  for (int i = threadIdx.x; i < NSTAT * 32; i += 256) (&st_lds[0][0])[i] = 0;
  __syncthreads();
  long long q[NSTAT] = {};
  for (int kq = 0; kq < SPLIT_STEPS; kq += 8) {
    const int kt = blockIdx.y * SPLIT_STEPS + kq + (threadIdx.x >> 5);
    if (kt >= nk) break;
    unsigned any[NP] = {};       // per plane: does this row hold a nonzero digit in this k-step
#pragma unroll
    for (int h = 0; h < 2; h++) {
      unsigned dig[NP][4] = {};  // 16 bytes per plane
#pragma unroll
      for (int qq = 0; qq < 16; qq++) {
        const int64_t t = (int64_t)kt * KS + h * 16 + qq;
        int sig = 0, ee = 1;
        if (t < T && !row_left<ROWS>(rowmask, t)) EL::parts(relu_bits<EL, RELU>(x[t * ld + j]), sig, ee);
        bool rounded;
        long long N = fixed_point<EL>(sig, E - ee, rounded);
        q[STAT_COUNTS] += (long long)(sig != 0) + ((long long)(sig != 0 && rounded) << 32);
        int d[NP];
#pragma unroll
        for (int s = NP - 1; s >= 1; s--) {
          d[s] = (int)((N + 128) & 255) - 128;  // balanced digit in [-128, 127]
          dig[s][qq >> 2] |= (unsigned)(d[s] & 255) << (8 * (qq & 3));
          N = (N - d[s]) >> 8;
        }
        d[0] = (int)N;
        dig[0][qq >> 2] |= (unsigned)(d[0] & 255) << (8 * (qq & 3));
#pragma unroll
        for (int s = 0; s < NP; s++) q[s] += d[s] * d[s];
        q[STAT_D0D1] += d[0] * d[1];
      }
#pragma unroll
      for (int s = 0; s < NP; s++) {
        signed char* piece = planes + ((s * groups + G) * (int64_t)nk + kt) * 1024;
        *(i32x4*)(piece + h * 512 + r * 16) = (i32x4){(int)dig[s][0], (int)dig[s][1], (int)dig[s][2], (int)dig[s][3]};
        any[s] |= dig[s][0] | dig[s][1] | dig[s][2] | dig[s][3];
      }
    }
    write_piece_mask(any, zmask, (int64_t)kt * groups + G);   // the 32 lanes of a half-wave hold the 32 rows of the piece
  }
#pragma unroll
  for (int i = 0; i < NSTAT; i++)
    if (q[i]) atomicAdd(&st_lds[i][r], (unsigned long long)q[i]);
  __syncthreads();
  for (int i = threadIdx.x; i < NSTAT * 32; i += 256)
    if (st_lds[i >> 5][i & 31]) atomicAdd(stats + (int64_t)(i >> 5) * n + G * 32 + (i & 31), st_lds[i >> 5][i & 31]);
}

// ---- the same two passes for the usual case of 16-byte addressable rows (ld % 8 == 0, aligned base): 16-byte loads.
// The scalar kernels above read 2 bytes per lane in 64-byte row segments and run at ~2 TB/s; these read whole 256-byte
// segments and are bound by the 6 bytes per element the split writes.
#ifndef MDG_COLMAX_WGS
#define MDG_COLMAX_WGS 4096
#endif
template <class EL, bool RELU, bool ROWS>
__global__ __launch_bounds__(256) void i8_colmax_vec_kernel(const bf16_t* x, int64_t ld, int64_t T, int64_t rows_per_block, int* emax,
                                                            const unsigned* rowmask, const RowsOut* rows_out) {
  __shared__ int best_lds[128];
  if (ROWS && rows_out->n_rows == 0) return;     // (the second maximum pass: no row left, the first pass's maxima stand)
  const int cg = threadIdx.x & 15, tl = threadIdx.x >> 4;  // 16 column groups of 8 columns x 16 token lanes
  const int j0 = blockIdx.x * 128 + cg * 8;
  const int64_t t0 = (int64_t)blockIdx.y * rows_per_block + tl;
  const int64_t t1 = min(T, (int64_t)(blockIdx.y + 1) * rows_per_block);
  if (threadIdx.x < 128) best_lds[threadIdx.x] = 1;
  __syncthreads();
  int best[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  for (int64_t t = t0; t < t1; t += 16) {
    i32x4 v = *(const i32x4*)(x + t * ld + j0);
    if (row_left<ROWS>(rowmask, t)) v = (i32x4)0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const unsigned w = relu_pair<EL, RELU>((unsigned)v[q]);
      best[2 * q] = max(best[2 * q], EL::ee_if_nonzero(w & 0xFFFF));
      best[2 * q + 1] = max(best[2 * q + 1], EL::ee_if_nonzero(w >> 16));
    }
  }
#pragma unroll
  for (int q = 0; q < 8; q++) atomicMax(&best_lds[cg * 8 + q], best[q]);
  __syncthreads();
  if (threadIdx.x < 128) atomicMax(emax + blockIdx.x * 128 + threadIdx.x, best_lds[threadIdx.x]);
}

// workgroup = 128 features (4 row groups) x SPLIT_TILES tiles of 64 tokens (2 k-steps): a tile goes through LDS (the next one's
// loads are in flight meanwhile), one thread then owns one feature of one k-step.  The column statistics of the route are kept
// in registers over the tiles and leave the workgroup as 8 atomics per feature.
constexpr int SPLIT_TILES = 8;
template <class EL, bool RELU, bool ROWS>
__global__ __launch_bounds__(256) void i8_split_vec_kernel(const bf16_t* x, int64_t ld, int64_t T, int n, int nk, const int* emax,
                                                           signed char* planes, unsigned long long* stats, unsigned char* zmask,
                                                           const unsigned* rowmask) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64 * 128];
  __shared__ int st_lds[NSTAT + 1][128];
  const int f0 = blockIdx.x * 128;
  const int f = threadIdx.x & 127, ks = threadIdx.x >> 7;
  const int E = emax[f0 + f];
  const int64_t groups = n / 32;
  const int G = (f0 + f) >> 5, r = f & 31;
  for (int i = threadIdx.x; i < (NSTAT + 1) * 128; i += 256) (&st_lds[0][0])[i] = 0;
  int q[NSTAT + 1] = {};   // q_0 .. q_5, sum d_0 d_1, nonzero elements, rounded elements: < 2^23 each over 8 tiles
  auto load_tile = [&](int tile_index, i32x4 (&v)[4]) {
    const int64_t tok0 = (int64_t)tile_index * 2 * KS;
#pragma unroll
    for (int c4 = 0; c4 < 4; c4++) {
      const int c = threadIdx.x + 256 * c4;  // 16-byte chunk: token c / 16, columns (c % 16) * 8 ..
      const int64_t t = tok0 + (c >> 4);
      v[c4] = (i32x4)0;
      if (t < T && !row_left<ROWS>(rowmask, t)) v[c4] = *(const i32x4*)(x + t * ld + f0 + (c & 15) * 8);
    }
  };
  const int tile0 = blockIdx.y * SPLIT_TILES, tiles = (nk + 1) / 2;
  for (int it = 0; it < SPLIT_TILES && tile0 + it < tiles; it++) {
    __syncthreads();              // (the previous tile has been read by every thread)
    {
      i32x4 v[4];
      load_tile(tile0 + it, v);
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++) *(i32x4*)(tile + (threadIdx.x + 256 * c4) * 8) = v[c4];
    }
    __syncthreads();
    const int kt = (tile0 + it) * 2 + ks;
    if (kt >= nk) continue;   // (uniform per wave: a wave holds 64 features of ONE k-step)
    unsigned any[NP] = {};
    unsigned deep_dig[2][NP - ALWAYS_WRITTEN_PLANES][4];   // planes 4, 5 wait for the piece mask; planes 0 - 3 are stored as they are made
    // Balanced base-256 digits without a carry loop: N + 128 (256^0 + ... + 256^4) has the bytes d_i + 128 in its lower five
    // positions -- the addition's own carries are the digit carries -- and the top digit above them; d_i = byte ^ 0x80.  Four
    // elements at a time, byte k of each gathered into one dword by v_perm_b32: ~27 VALU operations per element where the
    // digit-by-digit loop in 64-bit arithmetic took ~60 (the pass was VALU-bound: 1.1 ms at the sigma_mlp shape for 2.8 GB).
#pragma unroll
    for (int h = 0; h < 2; h++) {
      unsigned dig[NP][4];
#pragma unroll
      for (int q4 = 0; q4 < 4; q4++) {
        unsigned lo[4], hi[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          int sig, ee;
          EL::parts(relu_bits<EL, RELU>(tile[(ks * 32 + h * 16 + q4 * 4 + e) * 128 + f]), sig, ee);
          q[NSTAT - 1] += (sig != 0);
          bool rounded;
          const long long N = fixed_point<EL>(sig, E - ee, rounded);
          if (rounded) q[NSTAT] += (sig != 0);      // rounded to an integer: the remainder term rho of the bound
          const unsigned long long biased = (unsigned long long)N + 0x0000008080808080ull;
          lo[e] = (unsigned)biased;
          hi[e] = (unsigned)(biased >> 32);
        }
#pragma unroll
        for (int s2 = 0; s2 < NP; s2++) {
          constexpr unsigned ZERO_HI = 0x0c0c0000u;            // v_perm_b32 selector 0x0c: constant 0x00
          const int byte = NP - 1 - s2;                        // plane s2 = byte 5 - s2 of the 48-bit integer
          const unsigned sel = ZERO_HI | (unsigned)(byte & 3) | ((4u + (unsigned)(byte & 3)) << 8);   // [byte of src1, byte of src0]
          const unsigned t01 = __builtin_amdgcn_perm(byte < 4 ? lo[1] : hi[1], byte < 4 ? lo[0] : hi[0], sel);
          const unsigned t23 = __builtin_amdgcn_perm(byte < 4 ? lo[3] : hi[3], byte < 4 ? lo[2] : hi[2], sel);
          unsigned w = t01 | (t23 << 16);
          if (s2 > 0) w ^= 0x80808080u;
          dig[s2][q4] = w;
          q[s2] = __builtin_amdgcn_sdot4((int)w, (int)w, q[s2], false);   // sum of the four digits' squares (v_dot4c_i32_i8)
        }
        q[STAT_D0D1] = __builtin_amdgcn_sdot4((int)dig[0][q4], (int)dig[1][q4], q[STAT_D0D1], false);
      }
#pragma unroll
      for (int s2 = 0; s2 < NP; s2++) {
        any[s2] |= dig[s2][0] | dig[s2][1] | dig[s2][2] | dig[s2][3];
        if (s2 < ALWAYS_WRITTEN_PLANES) {
          signed char* piece = planes + ((s2 * groups + G) * (int64_t)nk + kt) * 1024;
          *(i32x4*)(piece + h * 512 + r * 16) = (i32x4){(int)dig[s2][0], (int)dig[s2][1], (int)dig[s2][2], (int)dig[s2][3]};
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++) deep_dig[h][s2 - ALWAYS_WRITTEN_PLANES][i] = dig[s2][i];
        }
      }
    }
    const unsigned present = write_piece_mask(any, zmask, (int64_t)kt * groups + G);
#pragma unroll
    for (int s2 = ALWAYS_WRITTEN_PLANES; s2 < NP; s2++)
      if ((present >> s2) != 0) {   // some plane >= s2 holds a nonzero here: the product kernels load every plane below a
                                    // group's depth (uniform per half-wave = per piece)
        signed char* piece = planes + ((s2 * groups + G) * (int64_t)nk + kt) * 1024;
#pragma unroll
        for (int h = 0; h < 2; h++)
          *(i32x4*)(piece + h * 512 + r * 16) = (i32x4){(int)deep_dig[h][s2 - ALWAYS_WRITTEN_PLANES][0], (int)deep_dig[h][s2 - ALWAYS_WRITTEN_PLANES][1],
                                                        (int)deep_dig[h][s2 - ALWAYS_WRITTEN_PLANES][2], (int)deep_dig[h][s2 - ALWAYS_WRITTEN_PLANES][3]};
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i <= NSTAT; i++)
    if (q[i]) atomicAdd(&st_lds[i][f], q[i]);
  __syncthreads();
  if (threadIdx.x < 128) {
    unsigned long long* o = stats + f0 + threadIdx.x;
#pragma unroll
    for (int i = 0; i < STAT_COUNTS; i++) {   // (the sum of d_0 d_1 is signed: sign-extended, the 64-bit sum wraps correctly)
      const int val = st_lds[i][threadIdx.x];
      if (val) atomicAdd(o + (int64_t)i * n, (unsigned long long)(long long)val);
    }
    const unsigned long long counts = (unsigned long long)(unsigned)st_lds[NSTAT - 1][threadIdx.x] |
                                      ((unsigned long long)(unsigned)st_lds[NSTAT][threadIdx.x] << 32);
    if (counts) atomicAdd(o + (int64_t)STAT_COUNTS * n, counts);
  }
}

}  // namespace

// The column maxima of statistic i into its (zeroed) emax.  masked (MDG_I8_ROWS, the second pass): over the rows that stayed --
// every workgroup exits at once when no row left; the selection kernel zeroed emax again when one did.
int enqueue_colmax(const I8Call& c, int i, bool masked) {
  const I8Stat& s = c.stat[i];
  const int n = s.n;
  I8Call k = c;
  k.rows = masked;
  const unsigned* mask = masked ? s.rowmask : nullptr;
  const RowsOut* ro = masked ? s.rows_out : nullptr;
  if (s.vec()) {
    // (the maximum pass of a NARROW statistic: with 2048 tokens per workgroup 1024 columns are 128 workgroups walking 128 dependent
    //  16-byte loads each -- 82 us for 67 MB.  Token slabs sized for ~MDG_COLMAX_WGS workgroups in all, 64 tokens at least)
    const int64_t slabs = std::min(ceil_div(c.n_tokens, (int64_t)64), std::max((int64_t)1, (int64_t)MDG_COLMAX_WGS / (n / 128)));
    const int64_t rows_vec = ceil_div(ceil_div(c.n_tokens, slabs), (int64_t)16) * 16;
    MDG_I8_DISPATCH_ROWS(k, i8_colmax_vec_kernel, dim3((unsigned)(n / 128), (unsigned)ceil_div(c.n_tokens, rows_vec)), dim3(256), 0, c.st,
                         s.x, s.ld, c.n_tokens, rows_vec, s.emax, mask, ro);
  } else {
    const int64_t rows_per_block = 2048;
    MDG_I8_DISPATCH_ROWS(k, i8_colmax_kernel, dim3((unsigned)ceil_div(n, 64), (unsigned)ceil_div(c.n_tokens, rows_per_block)), dim3(256),
                         0, c.st, s.x, s.ld, c.n_tokens, n, rows_per_block, s.emax, mask, ro);
  }
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

int enqueue_split(const I8Call& c, int i) {
  const I8Stat& s = c.stat[i];
  const int n = s.n, nk = c.nk;
  MDG_HIP(hipMemsetAsync(s.emax, 0, ints_bytes(n), c.st));
  MDG_TRY(enqueue_colmax(c, i, false));
  if (c.rows) {     // which rows leave is decided against the maxima over ALL rows; the split then runs against those of the rest
    MDG_TRY(enqueue_row_selection(c, i));
    MDG_TRY(enqueue_colmax(c, i, true));
  }
  if (s.vec()) {
    MDG_I8_DISPATCH_ROWS(c, i8_split_vec_kernel, dim3((unsigned)(n / 128), (unsigned)ceil_div(nk, 2 * SPLIT_TILES)), dim3(256), 0, c.st, s.x,
                         s.ld, c.n_tokens, n, nk, s.emax, s.planes, s.stats(), s.zmask, (const unsigned*)s.rowmask);
  } else {
    MDG_I8_DISPATCH_ROWS(c, i8_split_kernel, dim3((unsigned)(n / 32), (unsigned)ceil_div(nk, SPLIT_STEPS)), dim3(256), 0, c.st, s.x, s.ld,
                         c.n_tokens, n, nk, s.emax, s.planes, s.stats(), s.zmask, (const unsigned*)s.rowmask);
  }
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg
