// int8 covariance, the products (the map of the units is at the head of cov_i8.hip): the plane-pair product kernel in its three
// instantiations, the tail combine of the persistent launch's k-split last round, the tile schedule and its cache, and the host
// half of the two diagnostic builds.
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "cov_i8.hpp"

namespace mdg {
namespace {

typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr int PA = TI * KS;      // bytes of one plane of the I operand in a k-step

// One statistic of a launch (block: see I8Stat).
struct SyrkProblem {
  const signed char* planes;
  const int* emax;
  const unsigned char* zmask;          // [nk][n / 32] piece masks written by the split pass (write_piece_mask)
  double* sigma;
  int64_t ld_sigma;
  int n, block;
};
constexpr int CODE_PROB = 28, CODE_BI = 14;   // tile code = problem << 28 | bi << 14 | bj

struct SyrkArgs {
  SyrkProblem prob[MAX_PROBLEMS];
  int nprob, nk;
  unsigned long long* mfma_count;      // += v_mfma instructions this launch executed (the dense count is known on the host)
  const int* route_flag;               // [nprob] per statistic, written by i8_route_kernel: bit 0 -> needs six planes, bit 1 -> the fp64 kernel;
                                       // see launch_route()
  int* route_counts;                   // optional device counters [five planes, six planes, fp64 fallback], += 1 by the launch that runs
  const int2* sched;                   // persistent launch: [ngroups][32] entries {tile code (-1 = none), k-chunk code
                                       // (0 = all k-steps; else slot << 10 | Q << 5 | q: chunk q of Q, folded into partial tile `slot`)};
                                       // nullptr = one tile per workgroup
  int ngroups;
  double* partial;                     // [slot][128][TJ] fp64 partial tiles of the k-split last round (zeroed per call; i8_tail_combine_kernel)
  const int4* tail;                    // [n_tail] {tile code, Q, first slot, 0}: the tiles of the split round
  int* xcd_arrive;                     // [8] arrival counters of the round barrier (zeroed per call)
  const int* exact_state;              // nullptr: the exact route is not on offer for this call; else {overflow, ran} written by i8_extract_lo_kernel
#ifdef MDG_I8_STAMPS
  unsigned long long* stamps;          // diagnostic build only: per (workgroup, wave) cycle sums of the k-step phases
#endif
#ifdef MDG_I8_WGTIMES
  unsigned long long* wgtimes;         // diagnostic build only: [256][2 + 32] wall clock (100 MHz) at workgroup start / end / after each tile
#endif
};
// The route of a launch from the per-statistic flags: a statistic with bit 1 set leaves the int8 path ALONE (its tiles are
// skipped here, a gated mdg_cov_accum launch does it); the others share the launch on six planes if any of them asks for six,
// else on five.  Returns 0 / 1 (five / six planes), or -1 when no statistic is left on the int8 path; `fallbacks` = how many left.
__device__ __forceinline__ int launch_route(const SyrkArgs& a, int& live, int& fallbacks) {
  int six = 0;
  live = fallbacks = 0;
  for (int p = 0; p < a.nprob; p++) {
    const int f = a.route_flag[p];
    if (f & 2) fallbacks++;
    else {
      live++;
      six |= f & 1;
    }
  }
  return live ? six : -1;
}

// The EXACT route (cov_i8_exact.hip): the three top digit planes through i8_syrk_kernel<3> -- all nine plane pairs of the 24-bit
// part, nothing truncated -- and the remainder of the elements that have one through the fp64 remainder kernels.  On offer when the
// remainder lists were built and none overflowed; it then serves the statistics of BOTH legacy classes (five and six planes) of
// the launch.
__device__ __forceinline__ bool exact_route(const SyrkArgs& a) {
  return a.exact_state && a.exact_state[1] == 1 && a.exact_state[0] == 0;
}
// Does the P-plane product launch of this call do the work?  (0: no; 1: the truncated product of P planes; 2: the exact route --
// P = 3: the launch of the three top planes, all nine pairs)
template <int P>
__device__ __forceinline__ int product_launch_runs(const SyrkArgs& a, int& live, int& fallbacks) {
  const int route = launch_route(a, live, fallbacks);
  if (route < 0) return 0;
  if (exact_route(a)) return P == 3 ? 2 : 0;
  if (P == 3) return 0;
  return route == (P == 5 ? 0 : 1) ? 1 : 0;
}

#ifdef MDG_I8_STAMPS
#define MDG_STAMP(x) x = __builtin_amdgcn_s_memtime()
constexpr int STAMP_WGS = 1024;
#else
#define MDG_STAMP(x)
#endif

// Shape and LDS ring per route.  One workgroup of 8 waves per CU (two waves per SIMD, <= 256 registers each).
//   P = 5: 128 x 128 tile, wave tile 64 x 32 (160 accumulators), stages of 40 KB -- 40 KB of L2 -> LDS traffic per k-step for
//          16384 outputs where two 128 x 64 tiles move 60 KB.  Ring of 3 stages, filled two k-steps ahead.
//   P = 6: 128 x 64 tile, wave tile 32 x 32 (96 accumulators), stages of 36 KB.  Ring of 4 stages, filled three k-steps ahead;
//          a stage is therefore complete one barrier before it is multiplied, and a wave reads the next step's fragments right
//          after its last MFMA of this one (their latency runs under its load issue / the barrier).
// What a k-step costs besides its MFMAs, by s_memtime stamps (diagnostic build -DMDG_I8_STAMPS; five planes, Gaussian
// columns, 18.8 MFMAs per wave and step = 1203 matrix-pipe cycles per SIMD): in the first versions (2-stage ring, every wave:
// barrier -> its 5 stage loads -> fragment reads -> MFMAs) a step took ~2500 cycles -- ~700-800 of them spent by all eight
// waves side by side on ~100 instructions of mask decoding (clz / med3 on the VALU), 64-bit address updates and LDS-DMA
// issue while no wave multiplied, then ~1360 on the MFMAs (the younger wave of each SIMD loses the arbitration and finishes
// last; the older one idles ~700 at the next barrier).  Two changes:
//   * the stage loads are driven by per-wave piece descriptors held in SGPRs (base address, LDS offset, mask byte position,
//     plane bits), ~9 scalar instructions per piece, the address an SGPR base + one VGPR offset shared by all pieces
//     (issue_stage): ~420-540 cycles for the 5 loads -- what is left is the LDS-DMA instruction itself, which holds its wave
//     ~85-100 cycles at issue;
//   * the two waves of a SIMD take OPPOSITE orders inside a k-step (roles by wave number >= 4, MI355X_MICROARCH.md "Two waves
//     per SIMD" item 9): waves 4-7 issue their share of the stage loads right after the barrier and multiply afterwards;
//     waves 0-3 multiply first and issue their loads at the end of the step -- one wave's load issue runs under its partner's
//     MFMAs.  A wave waits for its own loads (vmcnt(0)) right before it issues the next ones, a whole k-step after they went
//     out, so the wait is free and needs no load count (the number of pieces a wave loads varies with the zero-plane skipping).
// Five planes 26.7 -> 24.2 ms per sigma_mlp call (~1970 cycles per step), six planes 46.4 -> 37.9 ms.  Measured and dropped on
// the way: a ping-pong with a second barrier per step (one wave of a SIMD only loads while the other only multiplies: 50.8 ms
// -- an LDS-DMA issue beside a partner that issues MFMAs back to back takes 380 cycles instead of 85, s_setprio changes
// nothing); the loads dealt out between a wave's own MFMAs (EXEC = 0 for skipped pieces, the accumulators as asm operands
// to pin the order: 27.0 / 41.6 ms -- in lock-step both waves of a SIMD stall in their load issue together); fragment reads
// ahead of the load issue; static s_setprio 1 for waves 4-7 (26.4 ms); four stages + fragment prefetch for five planes too
// (24.7 ms); super-blocks of 1 / 4 x 4 tiles for six planes (39.4 / 39.0 ms).
// Build-time variants that were measured and dropped (lock-step round barrier, fixed tile lists, returnless atomic fold, the
// narrow five-plane tile, every-wave-loads-first order, deferred MFMAs on six planes, whole tiles in the last round, the
// timing experiments) live in scripts/probes/cov_i8_variants.patch with their numbers; what is compiled here is the shipped
// path.  Two diagnostic builds remain: -DMDG_I8_STAMPS (s_memtime phases of a k-step) and -DMDG_I8_WGTIMES (per-workgroup
// wall clock).
constexpr int SB5 = 2, SB6 = 2;       // one-tile-per-workgroup launches (n < 2048): super-blocks of 2 x 2 (2 x 4) tiles per XCD
constexpr int PERSISTENT_MIN_ROWS = 16;   // statistics of at least this many 128-row blocks (n >= 2048) run as the persistent launch
constexpr int DEFER5 = 4;             // MFMAs a loads-first wave of the five-plane kernel holds back across the barrier (0: 25.3, 2: 26.0, 3: 24.9, 4: 24.6, 5: 25.0, 6: 27.8 ms per call)
constexpr int NW = 8;                 // waves per workgroup
constexpr int RING5 = 3;              // LDS stages of the five-plane kernel (six planes: 4)
// (measured at the sigma_mlp shape, Gaussian / SiLU-gated columns, product launch alone: three stages without fragment prefetch
//  19.5 / 20.3 ms; four stages 19.6 / 20.4; fragment prefetch with four, five or six stages 39 - 40 ms -- hipcc then keeps two sets
//  of fragments beside the 160 accumulators and spills inside the loop.  The five-plane kernel with the deeper planes masked off,
//  which this instantiation replaced: 20.6 / 21.5 ms; the truncated five- / six-plane products: 21.4 / 35.5 ms.)
#ifndef MDG_I8_RING3
#define MDG_I8_RING3 3
#endif
constexpr int RING3 = MDG_I8_RING3;   // LDS stages of the three-plane (exact route) kernel: 24 KB per k-step each
// k-steps per LDS stage, i.e. per workgroup barrier (three planes only: nothing in that k-step is conditional).  The loads of a stage
// are the same 1 KB pieces, twice as many per issue; what halves is the number of barriers and role switches per MFMA.
// Measured at the sigma_mlp shape, Gaussian columns, product launch alone, one box (scripts/probes/p3_variants.sh,
// profiles/r04_p3_variants.log): one k-step per stage (ring of 3, 4 deferred MFMAs) 19.37 ms; two k-steps (ring of 3 x 48 KB) with
// 0 / 2 / 4 / 6 / 8 / 10 / 12 / 14+ deferred 19.47 / 19.21 / 18.98 / 18.73 / 18.56 / 20.2 / 21.3 / 23.2; three k-steps in a ring of
// two 20.04.
#ifndef MDG_I8_KSS3
#define MDG_I8_KSS3 2
#endif
// MFMA shape of the three-plane kernel.  32: v_mfma_i32_32x32x32_i8, one per k-step, plane pair and 32 x 32 block of the wave tile
// (18 per wave and k-step).  16: v_mfma_i32_16x16x64_i8, whose K = 64 is the TWO k-steps of a stage: one per stage, plane pair and
// 16 x 16 block (72 per wave and stage, half the cycles each) -- the same int32 class sums, so not a bit of sigma changes.  Cycles
// per op are equal; what differs is the clock the chip holds under its power cap (mdg_probe_mfma_i8_shape; DESIGN.md section 7,
// "The 16x16x64 MFMA shape").
#ifndef MDG_I8_SHAPE3
#define MDG_I8_SHAPE3 16
#endif
static_assert(MDG_I8_SHAPE3 == 16 || MDG_I8_SHAPE3 == 32, "MDG_I8_SHAPE3: 16 (v_mfma_i32_16x16x64_i8) or 32 (v_mfma_i32_32x32x32_i8)");
static_assert(MDG_I8_SHAPE3 == 32 || MDG_I8_KSS3 == 2, "one 16x16x64 MFMA takes the two k-steps of a stage");
#ifndef MDG_I8_DEFER3
// MFMAs a loads-first wave of the three-plane kernel holds back across the barrier (see DEFER5), in MFMAs of the shape built (72
// per wave and stage on the 16-wide shape, 36 on the 32-wide).  Measured at the sigma_mlp shape, Gaussian columns, product launch
// alone, one box (profiles/i8_shape3_defer_sweep.json): 32-wide, 8 deferred 19.31 ms; 16-wide with 0 / 4 / 8 / 12 / 16 / 20 / 24
// deferred 18.00 / 17.92 / 17.95 / 17.86 / 17.67-18.28 / 20.65 / 21.74 -- flat up to 16 within the run-to-run spread, a cliff above.
#define MDG_I8_DEFER3 (MDG_I8_SHAPE3 == 16 ? 12 : 8)
#endif
constexpr bool shape16(int planes) { return planes == 3 && MDG_I8_SHAPE3 == 16; }
constexpr int steps_per_stage(int planes) { return planes == 3 ? MDG_I8_KSS3 : 1; }
constexpr bool wide_tile(int planes) { return planes != 6; }   // 128 x 128 tiles (six planes: 128 x 64)
constexpr int ring_depth(int planes) { return planes == 3 ? RING3 : wide_tile(planes) ? RING5 : 4; }
// fragments of the next k-step read right behind this step's MFMAs (needs a stage that is complete a barrier early: RING >= 4;
// with the 160 accumulators of a wide tile hipcc spills inside the loop, see RING5)
constexpr bool prefetch_frags(int planes) { return !wide_tile(planes); }
// P = 3 is the product of the EXACT route: planes 0 .. 2 only, ALL nine plane pairs (classes 0 .. 4), no piece masks -- the same tile
// code with nothing conditional left in the k-step (24 KB stages, 36 fragment registers beside the 160 accumulators; 40 on the
// 16x16x64 shape, MDG_I8_SHAPE3)
constexpr int classes_of(int planes) { return planes == 3 ? 5 : planes; }
// tile shape per route, for the kernels and the host's LDS-size and grid arithmetic
template <int P> struct TileShape {
  static constexpr int WB = wide_tile(P) ? 2 : 1;         // 32-row blocks of a wave tile: 64 x 32, or 32 x 32 (96 accumulators at P = 6)
  static constexpr int TJ = WB == 2 ? 128 : 64;           // tile columns (rows of the J operand); waves are laid out (128 / 32 WB) x (TJ / 32)
  static constexpr int PB = TJ * KS;                      // bytes of one plane of the J operand in a k-step
  static constexpr int GA = TI / 32, GB = TJ / 32;        // 32-row groups (1 KB pieces per plane and stage) of the two operands
  static constexpr int WCOLS = TJ / 32;
  static constexpr int STEP_BYTES = P * (PA + PB);        // 40 KB (P = 5, 128 x 128) / 36 KB (P = 6, 128 x 64) / 24 KB (P = 3)
  static constexpr int STAGE_BYTES = steps_per_stage(P) * STEP_BYTES;
  static constexpr int LDS_BYTES = ring_depth(P) * STAGE_BYTES;
};

// One output tile (bi, bj) of the lower region: bi = 128-row block, bj = TJ-row block (bj <= bi for 128 x 128 tiles, bj <= 2 bi + 1
// for 128 x 64); the k-steps [kb, ke), then the fold: element (row, col) of the statistic goes to
// fold[(row - fold_row0) * fold_ld + col - fold_col0] (sigma itself, or a partial tile of the k-split last round).
// `executed` += the MFMAs this wave issued.
template <int P>
__device__ __forceinline__ void i8_syrk_tile(const SyrkArgs& a, const SyrkProblem& pr, const int bi, const int bj, const int kb, const int ke, double* const fold,
                                             const int64_t fold_ld, const int fold_row0, const int fold_col0, unsigned char* lds,
                                             unsigned& executed) {
  using S = TileShape<P>;
  constexpr int WB = S::WB, TJ = S::TJ, PB = S::PB, GA = S::GA, GB = S::GB, WCOLS = S::WCOLS;
  constexpr int KSS = steps_per_stage(P);          // k-steps per stage (per barrier)
  constexpr int STEP_BYTES = S::STEP_BYTES, STAGE_BYTES = S::STAGE_BYTES;
  constexpr int PIECES = (GA + GB) * P;            // 1 KB pieces per k-step
  constexpr int RING = ring_depth(P);              // LDS stages
  constexpr bool PREFETCH = prefetch_frags(P);     // the next step's fragments are read before the barrier (needs RING >= 4)
  static_assert(KSS == 1 || (P == 3 && !PREFETCH), "several k-steps per stage: the unconditional three-plane k-step only");
  constexpr int NCLS = classes_of(P);              // digit classes s + t kept: 0 .. NCLS - 1
  // the 16x16x64 shape (three planes): the 64 x 32 wave tile is 4 x 2 blocks of 16 x 16, one MFMA per block, plane pair and STAGE
  constexpr bool S16 = shape16(P);
  static_assert(!S16 || (KSS == 2 && WB == 2), "the 16x16x64 shape: stages of two k-steps, 64 x 32 wave tiles");
  // the wave index through readfirstlane: hipcc then knows it is wave-uniform and the staging code becomes scalar (SGPR piece
  // addresses, s_cbranch on the piece tests, M0 from SGPRs) instead of exec-masked branches with a v_readfirstlane per piece
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const bool loads_first = wave >= NW / 2;
  const int wr = wave / WCOLS, wc = wave % WCOLS;
  const int64_t groups = pr.n / 32;
  const int nk = a.nk;

  // staging: (GA + GB) P pieces of 1 KB per stage (A: P planes x 4 row groups, B: P planes x 2 or 4); wave w issues pieces w, w + NW, ...
  // mA / mB: piece masks of the stage's A and B row groups, one byte per 32-row group; planes at or beyond a group's depth
  // (group_depth below) are all-zero there in this k-step and are neither loaded nor multiplied
  constexpr int MIN_DEPTH = P == 3 ? 3 : P - 2;   // planes below this are always staged and multiplied (3 of five, 4 of six; all three of three)
  static_assert(MIN_DEPTH <= ALWAYS_WRITTEN_PLANES, "the split pass leaves all-zero pieces of the deeper planes unwritten");
  auto group_depth = [&](unsigned m, int g) {   // 1 + deepest plane with a nonzero in group g, but at least MIN_DEPTH
    const unsigned byte = (m >> (8 * g)) & 0xFFu;
    return max(MIN_DEPTH, min(P, 32 - __builtin_clz(byte | 1u)));
  };
  // Per-wave piece descriptors, all wave-uniform (SGPRs), set up once: the k-step loop then spends ~8 scalar instructions per
  // piece on the test "does this piece hold a nonzero" + M0 + one LDS-DMA load whose address is SGPR base + one VGPR offset
  // (lane * 16 + k-step * 1024) shared by all pieces.  (First version: a running 64-bit address per piece, depth through
  // clz / med3 on the VALU, exec-masked branches -- ~100 instructions per k-step and wave, 700-800 cycles by s_memtime stamps,
  // during which no wave of the workgroup multiplied.)
  constexpr int NQ = (PIECES + NW - 1) / NW;
  unsigned long long pc_base[NQ];
  unsigned pc_loff[NQ], pc_shift[NQ], pc_cmask[NQ], pc_force[NQ];
  bool pc_valid[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int p = wave + NW * q;
    pc_valid[q] = (PIECES % NW == 0 && q < PIECES / NW) || p < PIECES;
    const bool isA = p < GA * P;
    const int pp = isA ? p : p - GA * P;
    const int s = isA ? pp / GA : pp / GB, g = isA ? pp % GA : pp % GB;
    const int64_t G = (isA ? bi * (TI / 32) : bj * (TJ / 32)) + g;
    const unsigned long long base = (unsigned long long)(uintptr_t)pr.planes + (unsigned long long)((s * groups + G) * (int64_t)nk) * 1024ull;
    pc_base[q] = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(base >> 32)) << 32) |
                 (unsigned)__builtin_amdgcn_readfirstlane((unsigned)base);
    pc_loff[q] = (isA ? s * PA : P * PA + s * PB) + g * 1024;
    pc_shift[q] = (isA ? 0 : 32) + 8 * g;
    pc_cmask[q] = (0xFFu << s) & 0xFFu;          // bits s .. 7 of the group's mask byte: some plane >= s holds a nonzero
    pc_force[q] = s < MIN_DEPTH ? 1u : 0u;   // planes below MIN_DEPTH are always staged (the unconditional MFMA block reads them)
  }
  const unsigned lds_base = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)lds);
  const unsigned lane16 = lane * 16;
  auto issue_stage = [&](int kt, int buf, unsigned mA, unsigned mB) {
    const unsigned long long m64 = ((unsigned long long)mB << 32) | mA;
    const unsigned lbase = __builtin_amdgcn_readfirstlane(lds_base + buf * STAGE_BYTES);   // (wave-uniform; says so to the compiler)
#pragma unroll
    for (int kk = 0; kk < KSS; kk++) {
      if (KSS > 1 && kt + kk >= ke) break;   // (the last stage of a tile or k-chunk may hold fewer k-steps)
      const unsigned voff = lane16 + (unsigned)(kt + kk) * 1024u;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        if (!pc_valid[q]) continue;
        const unsigned present = ((unsigned)(m64 >> pc_shift[q]) & pc_cmask[q]) | pc_force[q];
        if (present)   // (an all-zero piece is not loaded: nothing will read it)
          asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lbase + kk * STEP_BYTES + pc_loff[q]), "v"(voff), "s"(pc_base[q])
                       : "memory");   // (M0 is written; nothing the compiler emits in this kernel reads it)
      }
    }
  };

  i32x16 acc[NCLS][WB];                  // [class][32-row block]: 32 x 32 blocks (unused, and gone, with S16)
  i32x4 acc16[S16 ? NCLS : 1][4][2];     // [class][16-row block][16-column block]: 16 x 16 blocks (S16 only)
#pragma unroll
  for (int k = 0; k < NCLS; k++)
#pragma unroll
    for (int b = 0; b < WB; b++) acc[k][b] = (i32x16)0;
#pragma unroll
  for (int k = 0; k < (S16 ? NCLS : 1); k++)
#pragma unroll
    for (int ab = 0; ab < 4; ab++)
#pragma unroll
      for (int bb = 0; bb < 2; bb++) acc16[k][ab][bb] = (i32x4)0;

  // The same fold from 16 x 16 blocks: lane l, register v of block (ab, bb) is row 16 ab + 4 (l / 16) + v, column 16 bb + l % 16 of
  // the wave tile.  Two 16-row blocks at a time, the same 16 loads in flight per lane, the same expression per element.
  auto flush16 = [&]() {
    const int col = bj * TJ + wc * 32 + (lane & 15);   // (of column block 0; block 1: + 16)
    int row0 = bi * TI + wr * 64 + 4 * (lane >> 4);
    asm volatile("" : "+v"(row0));                      // (see flush)
    int e_col[2];
    double sc_j[2];
#pragma unroll
    for (int bb = 0; bb < 2; bb++) {
      e_col[bb] = pr.emax[col + 16 * bb];
      sc_j[bb] = ldexp(1.0, (e_col[bb] & 255) - 172);
    }
#pragma unroll
    for (int b = 0; b < 2; b++) {
      double* const p = fold + (int64_t)(row0 + b * 32 - fold_row0) * fold_ld + (col - fold_col0);
      const int* const e = pr.emax + row0 + b * 32;
      int er[8];
      double old[16];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int off = (i & 3) + 16 * (i >> 2);
        er[i] = e[off];
#pragma unroll
        for (int bb = 0; bb < 2; bb++) old[2 * i + bb] = p[(int64_t)off * fold_ld + 16 * bb];
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int off = (i & 3) + 16 * (i >> 2);
#pragma unroll
        for (int bb = 0; bb < 2; bb++) {
          double v = 0.;
#pragma unroll
          for (int k = NCLS - 1; k >= 0; k--) v += ldexp((double)acc16[S16 ? k : 0][2 * b + (i >> 2)][bb][i & 3], 80 - 8 * k);
          if (col + 16 * bb <= row0 + b * 32 + off && !((e_col[bb] | er[i]) & EMAX_COLUMN_OUT))
            p[(int64_t)off * fold_ld + 16 * bb] = old[2 * i + bb] + v * sc_j[bb] * ldexp(1.0, (er[i] & 255) - 172);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < (S16 ? NCLS : 1); k++)
#pragma unroll
      for (int ab = 0; ab < 4; ab++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) acc16[k][ab][bb] = (i32x4)0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  // sigma[i][j] += 2^(E_i + E_j - 344) * sum_k acc_k 256^(10 - k)  =  (sum_k acc_k 2^(80 - 8k)) * 2^(E_i - 172) * 2^(E_j - 172)
  auto flush = [&]() {
    const int col = bj * TJ + wc * 32 + (lane & 31);
    int row0 = bi * TI + wr * 32 * WB + 4 * (lane >> 5);
    // opaque to the optimiser: otherwise the 32 element addresses are computed once, ahead of the MFMA loop, spilled (the
    // accumulators fill the register file there), and reloaded here behind one s_waitcnt vmcnt(0) each -- which turns the 16
    // sigma loads of a block into 16 serialised memory round trips (26 us per flush and tile, 2 x 0.65 ms per launch)
    asm volatile("" : "+v"(row0));
    const int e_col = pr.emax[col];      // bits 0-7: the column's maximum exponent; EMAX_COLUMN_OUT: the fp64 column kernel computes this column
    const double sc_j = ldexp(1.0, (e_col & 255) - 172);
    // all read-modify-writes of a lane: loads first (independent, in flight together), then the arithmetic and the stores;
    // written as `*p += v` one by one the compiler must keep them in order and every element pays a full memory round trip
#pragma unroll
    for (int b = 0; b < WB; b++) {  // one 32-row block at a time: 16 loads in flight per lane
      double* const p = fold + (int64_t)(row0 + b * 32 - fold_row0) * fold_ld + (col - fold_col0);
      const int* const e = pr.emax + row0 + b * 32;
      int er[16];
      double old[16];
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int off = (reg & 3) + 8 * (reg >> 2);
        old[reg] = p[(int64_t)off * fold_ld];
        er[reg] = e[off];
      }
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int off = (reg & 3) + 8 * (reg >> 2);
        double v = 0.;
#pragma unroll
        for (int k = NCLS - 1; k >= 0; k--) v += ldexp((double)acc[k][b][reg], 80 - 8 * k);
        // rows and columns the route handed to the fp64 column kernel are not ours: their digit products are computed and dropped
        if (col <= row0 + b * 32 + off && !((e_col | er[reg]) & EMAX_COLUMN_OUT))
          p[(int64_t)off * fold_ld] = old[reg] + v * sc_j * ldexp(1.0, (er[reg] & 255) - 172);
      }
    }
#pragma unroll
    for (int k = 0; k < NCLS; k++)
#pragma unroll
      for (int b = 0; b < WB; b++) acc[k][b] = (i32x16)0;
    // the stores above share the VM counter with the LDS-DMA loads: drain, so that the loop's waits see stage loads only
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  // piece masks: uniform-address loads; issued together with a stage's loads, for the stage after it
  const int64_t mgroups = pr.n / 32;
  auto load_masks = [&](int kt, unsigned& va, unsigned& vb) {
    if (P == 3) return;                      // (every piece of the three planes is staged: no masks)
    const unsigned* z = (const unsigned*)(pr.zmask + (int64_t)kt * mgroups);   // n / 32 is a multiple of 4: dword-aligned rows
    va = z[bi];                                                               // groups 4 bi .. 4 bi + 3
    vb = TJ == 128 ? z[bj] : z[bj >> 1];   // groups 4 bj .. + 3; or 2 bj, 2 bj + 1 in one half of the dword (see b_half)
  };
  // 128 x 64 tiles: the B panel's two mask bytes are one half of the loaded dword
  auto b_half = [&](unsigned m) { return TJ == 128 ? m : (m >> ((bj & 1) * 16)) & 0xFFFFu; };
  auto wait_loads = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  // masks of the stages kt (being multiplied) .. kt + D (the one this step issues) -- SGPRs; vA / vB: the loaded dwords of the
  // stage after those, in flight
  constexpr int D = RING - 1;
  unsigned mA[D + 1], mB[D + 1], vA = ~0u, vB = ~0u;
#pragma unroll
  for (int i = 0; i <= D; i++) mA[i] = mB[i] = ~0u;
#pragma unroll
  for (int i = 0; i < D; i++)
    if (KSS == 1 && kb + i < ke) {
      unsigned t0, t1;
      load_masks(kb + i, t0, t1);
      mA[i] = __builtin_amdgcn_readfirstlane(t0);
      mB[i] = b_half(__builtin_amdgcn_readfirstlane(t1));
    }
  if (KSS == 1 && ke - kb > D) load_masks(kb + D, vA, vB);
#pragma unroll
  for (int i = 0; i < D; i++)
    if (kb + i * KSS < ke) issue_stage(kb + i * KSS, i, mA[i], mB[i]);
  wait_loads();
  int buf = 0;                 // (kt - kb) % RING
#ifdef MDG_I8_STAMPS
  unsigned long long ta = 0, tb = 0, tc = 0, td = 0, te = 0, s_wait = 0, s_issue = 0, s_comp = 0, s_tail = 0, t_begin;
  const unsigned executed_before = executed;
  const unsigned long long w_begin = wall_clock64();   // 100 MHz: with t_begin, the clock this tile ran at
  MDG_STAMP(t_begin);
#endif
  const int r = lane & 31, h = lane >> 5;
  // fragments of the planes below MIN_DEPTH (always staged, always multiplied): ONE set of reads feeds all their pairs
  i32x4 fa[MIN_DEPTH][WB], fb[MIN_DEPTH];
  auto load_frags = [&](int stage_buf, int kk = 0) {
    const unsigned char* base = lds + stage_buf * STAGE_BYTES + kk * STEP_BYTES;
#pragma unroll
    for (int s = 0; s < MIN_DEPTH; s++) {
#pragma unroll
      for (int b = 0; b < WB; b++) fa[s][b] = *(const i32x4*)(base + s * PA + (wr * WB + b) * 1024 + h * 512 + r * 16);
      fb[s] = *(const i32x4*)(base + P * PA + s * PB + wc * 1024 + h * 512 + r * 16);
    }
  };
  // S16: an operand of v_mfma_i32_16x16x64_i8 is 16 rows x 64 k-bytes, lane l holding 16 bytes of row l % 16 -- lane group l / 16 =
  // g takes them from k-step g >> 1 of the stage, half g & 1 of the row's 32 bytes (both operands alike, so the order of the k
  // bytes inside the instruction does not matter to the sum).  The rows come from the same 1 KB pieces (2 halves x 32 rows x 16 B):
  // 16-row block x of a panel is rows 16 (x & 1) .. of piece x >> 1.  B's three planes stay in registers for the stage (24), A's
  // are read one plane at a time (16): all nine would be 72 beside the 160 accumulators.
  i32x4 fa16[4], fb16[MIN_DEPTH][2];
  const unsigned frag16 = ((lane >> 4) >> 1) * STEP_BYTES + ((lane >> 4) & 1) * 512 + (lane & 15) * 16;
  // one_step: the stage holds ONE k-step (the odd end of a tile segment or k-chunk) -- lane groups 2 and 3 multiply zeros
  auto load_fb16 = [&](int stage_buf, bool one_step) {
    const unsigned char* base = lds + stage_buf * STAGE_BYTES + frag16 + P * PA + wc * 1024;
#pragma unroll
    for (int t = 0; t < MIN_DEPTH; t++)
#pragma unroll
      for (int bb = 0; bb < 2; bb++) fb16[t][bb] = *(const i32x4*)(base + t * PB + bb * 256);
    if (one_step && lane >= 32) {
#pragma unroll
      for (int t = 0; t < MIN_DEPTH; t++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) fb16[t][bb] = (i32x4)0;
    }
  };
  auto load_fa16 = [&](int stage_buf, int s) {
    const unsigned char* base = lds + stage_buf * STAGE_BYTES + frag16 + s * PA + wr * WB * 1024;
#pragma unroll
    for (int ab = 0; ab < 4; ab++) fa16[ab] = *(const i32x4*)(base + (ab >> 1) * 1024 + (ab & 1) * 256);
  };
  constexpr int N16 = 9 * 4 * 2, N16_PLANE = 3 * 4 * 2;   // MFMAs per wave and stage; of them with one plane of A
  // the MFMAs of A's plane s in (t, row block, column block) order, those with stage index in [lo, hi)
  auto mfma16_plane = [&](int s, int lo, int hi) {
    int idx = s * N16_PLANE;
#pragma unroll
    for (int t = 0; t < MIN_DEPTH; t++)
#pragma unroll
      for (int ab = 0; ab < 4; ab++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) {
          if (idx >= lo && idx < hi)
            acc16[S16 ? s + t : 0][ab][bb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa16[ab], fb16[t][bb], acc16[S16 ? s + t : 0][ab][bb], 0, 0, 0);
          idx++;
        }
  };
  // the deeper planes of a step, each present one a block of its own (fragment read + its pairs).  A deep plane only pairs with
  // planes 0 (and 1) of the other panel (s + t < P), so the blocks are independent and simply add:
  //   P = 5: 9 pairs + 2 [dA > 3] + 2 [dB > 3] + [dA > 4] + [dB > 4];   P = 6: 15 + 2 [dA > 4] + 2 [dB > 4] + [dA > 5] + [dB > 5]
  // (branching around single MFMAs / fragment reads instead makes hipcc put an lgkmcnt(0) in front of every LDS read; nine
  // straight-line variants behind a switch make it spill the 160 accumulators at the merges)
  auto deep_planes = [&](int stage_buf, unsigned mAk, unsigned mBk) {
    const unsigned char* base = lds + stage_buf * STAGE_BYTES;
    int dAb[WB];
#pragma unroll
    for (int b = 0; b < WB; b++) dAb[b] = group_depth(mAk, wr * WB + b);
    const int dBw = group_depth(mBk, wc);
    int deep_mfmas = 0;
#pragma unroll
    for (int d = MIN_DEPTH; d < P; d++) {
#pragma unroll
      for (int b = 0; b < WB; b++)
        if (dAb[b] > d) {   // plane d of A block b with planes t < P - d of B (all below MIN_DEPTH: already in registers)
          const i32x4 fd = *(const i32x4*)(base + d * PA + (wr * WB + b) * 1024 + h * 512 + r * 16);
#pragma unroll
          for (int t = 0; t < P - d; t++) acc[d + t][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fd, fb[t], acc[d + t][b], 0, 0, 0);
          deep_mfmas += P - d;
        }
      if (dBw > d) {        // plane d of the B block with planes s < P - d of both A blocks
        const i32x4 fd = *(const i32x4*)(base + P * PA + d * PB + wc * 1024 + h * 512 + r * 16);
#pragma unroll
        for (int s2 = 0; s2 < P - d; s2++)
#pragma unroll
          for (int b = 0; b < WB; b++)
            acc[s2 + d][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[s2][b], fd, acc[s2 + d][b], 0, 0, 0);
        deep_mfmas += (P - d) * WB;
      }
    }
    executed += deep_mfmas;
  };
  constexpr int UNCOND_PAIRS = P == 6 ? 15 : 9;   // pairs (s, t), s, t < MIN_DEPTH, s + t < NCLS
  constexpr int N_UNCOND = UNCOND_PAIRS * WB;                               // unconditional MFMAs per wave and k-step
  // of them, held back across the barrier by the loads-first waves (six planes: none -- 37.2 ms per call without, 55 ms with 3 - 5
  // deferred: the loads-first waves then lose their fragment prefetch)
  constexpr int DEFER = PREFETCH ? 0 : P == 3 ? MDG_I8_DEFER3 : DEFER5;
  static_assert(!S16 || DEFER <= N16_PLANE, "the deferred MFMAs are of A's last plane: its fragments and B's stay in registers");
  auto rotate = [&]() {
#pragma unroll
    for (int i = 0; i < D; i++) {
      mA[i] = mA[i + 1];
      mB[i] = mB[i + 1];
    }
    buf = buf == RING - 1 ? 0 : buf + 1;
  };
  const auto ahead = [&](int d) { int x = buf + d; return x >= RING ? x - RING : x; };   // (kt + d) % RING
  if (PREFETCH) {
    __builtin_amdgcn_s_barrier();   // stages 0 .. D - 1 complete (every wave waited for its share)
    if (!(DEFER && loads_first)) load_frags(0);
  }
  // two loops: the int32 classes are folded into sigma between runs of FLUSH_STEPS k-steps, outside the MFMA loop (a
  // conditional flush inside it makes the compiler shuttle all 160 accumulators between AGPRs and VGPRs every step)
  constexpr int FOLD_STEPS = FLUSH_STEPS - FLUSH_STEPS % KSS;   // (a fold falls between two stages)
  for (int k0 = kb; k0 < ke; k0 += FOLD_STEPS) {
    const int k1 = min(ke, k0 + FOLD_STEPS);
    // Roles: the two waves of a SIMD take opposite orders inside a k-step.  Waves 4-7 issue their share of stage kt + D right
    // after the barrier and multiply afterwards; waves 0-3 multiply first and issue at the end of the step (after waiting for
    // their previous loads, a whole k-step old by then) -- one wave's ~450 cycles of LDS-DMA issue run under its partner's MFMAs.
    for (int kt = k0; kt < k1; kt += KSS) {
      MDG_STAMP(ta);
      if (loads_first) wait_loads();  // this wave's loads of the previous step
      __builtin_amdgcn_s_barrier();   // stage kt (PREFETCH: kt + 1 too) complete in LDS, stage kt - 1 no longer read
      auto refill = [&]() {           // stage kt + D into the buffer stage kt - 1 just left; masks of the stage after it behind it
        mA[D] = __builtin_amdgcn_readfirstlane(vA);
        mB[D] = b_half(__builtin_amdgcn_readfirstlane(vB));
        if (kt + D * KSS < ke) issue_stage(kt + D * KSS, ahead(D), mA[D], mB[D]);
        if (KSS == 1 && kt + D + 1 < ke) load_masks(kt + D + 1, vA, vB);
      };
      MDG_STAMP(tb);
      // the unconditional MFMAs of a step, in (s, t, block) order; [lo, hi) selects a run of them
      auto mfma_run = [&](int lo, int hi) {
        int idx = 0;
#pragma unroll
        for (int s = 0; s < MIN_DEPTH; s++)
#pragma unroll
          for (int t = 0; t < MIN_DEPTH; t++)
            if (s + t < NCLS) {
#pragma unroll
              for (int b = 0; b < WB; b++) {
                if (idx >= lo && idx < hi) acc[s + t][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[s][b], fb[t], acc[s + t][b], 0, 0, 0);
                idx++;
              }
            }
      };
      if (loads_first) {
        // the loads-first waves keep the last DEFER MFMAs of the previous step back until here: they run while their SIMD
        // partner, which multiplies first, is still waiting for its fragment reads -- the matrix pipe would idle ~150 cycles
        // at every step boundary otherwise (fragments of the previous step are still in this wave's registers: it re-reads
        // them only after its loads are out)
        if (DEFER && kt > k0) {
          if constexpr (S16) mfma16_plane(MIN_DEPTH - 1, N16 - DEFER, N16);
          else mfma_run(N_UNCOND - DEFER, N_UNCOND);
          __builtin_amdgcn_sched_barrier(0);
        }
        refill();
        __builtin_amdgcn_sched_barrier(0);
      }
      MDG_STAMP(tc);
      if constexpr (S16) {
        // the whole stage in one pass: B's planes, then A's one by one, each re-read into the same registers once the MFMAs of the
        // plane before are issued (the SIMD's other wave, half a stage out of phase, has the matrix pipe meanwhile)
        const bool one_step = kt + 1 >= k1;
        load_fb16(buf, one_step);
#pragma unroll
        for (int s = 0; s < MIN_DEPTH; s++) {
          load_fa16(buf, s);
          if (s < MIN_DEPTH - 1) {
            mfma16_plane(s, 0, N16);
            __builtin_amdgcn_sched_barrier(0);
          } else {
            mfma16_plane(s, 0, N16 - DEFER);
            if (DEFER == 0 || !loads_first) mfma16_plane(s, N16 - DEFER, N16);
          }
        }
        // (in 32x32x32 units, as the host's dense count: one 16x16x64 is half of one, and the zero half of an odd end is not work)
        executed += UNCOND_PAIRS * WB * (one_step ? 1 : KSS);
      } else {
      if (!PREFETCH || (DEFER && loads_first)) load_frags(buf);
      if (KSS > 1) {
        // the stage's k-steps but the last, whole: the fragment registers are re-read once their MFMAs are issued (the SIMD's other
        // wave, a stage's half out of phase, has the matrix pipe meanwhile)
#pragma unroll
        for (int kk = 1; kk < KSS; kk++)
          if (kt + kk < k1) {
            mfma_run(0, N_UNCOND);
            executed += UNCOND_PAIRS * WB;
            __builtin_amdgcn_sched_barrier(0);
            load_frags(buf, kk);
          }
      }
      mfma_run(0, N_UNCOND - DEFER);
      if (DEFER == 0 || !loads_first) mfma_run(N_UNCOND - DEFER, N_UNCOND);
      deep_planes(buf, mA[0], mB[0]);
      executed += UNCOND_PAIRS * WB;
      }
      if (PREFETCH) {
      // next step's fragments: stage kt + 1 has been complete since THIS step's barrier (its loads went out three steps ago
      // and every wave waited for its share before the barrier), so the read latency hides behind the refill / the barrier
      __builtin_amdgcn_sched_barrier(0);   // (not before the MFMAs above are issued: the fragment registers are theirs until then)
      if (kt + 1 < ke && !(DEFER && loads_first)) load_frags(ahead(1));
      }
      MDG_STAMP(td);
      if (!loads_first) {
        __builtin_amdgcn_sched_barrier(0);
        wait_loads();       // this wave's loads of the previous step
        refill();
      }
      MDG_STAMP(te);
#ifdef MDG_I8_STAMPS
      s_wait += tb - ta; s_issue += tc - tb; s_comp += td - tc; s_tail += te - td;
#endif
      rotate();
    }
    if constexpr (S16) {
      if (DEFER && loads_first) mfma16_plane(MIN_DEPTH - 1, N16 - DEFER, N16);   // (as below)
      flush16();
    } else {
    if (DEFER && loads_first) {   // the deferred MFMAs of the segment's last step (its fragments are still in registers)
#pragma unroll
      for (int s = 0, idx = 0; s < MIN_DEPTH; s++)
#pragma unroll
        for (int t = 0; t < MIN_DEPTH; t++)
          if (s + t < NCLS) {
#pragma unroll
            for (int b = 0; b < WB; b++) {
              if (idx >= N_UNCOND - DEFER) acc[s + t][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[s][b], fb[t], acc[s + t][b], 0, 0, 0);
              idx++;
            }
          }
    }
    flush();
    }
  }
#ifdef MDG_I8_STAMPS
  if (a.stamps && lane == 0 && blockIdx.x < STAMP_WGS) {
    unsigned long long t_end;
    MDG_STAMP(t_end);
    unsigned long long* o = a.stamps + ((size_t)blockIdx.x * NW + wave) * 8;
    o[0] = s_wait; o[1] = s_issue; o[2] = s_comp; o[3] = s_tail; o[4] = t_end - t_begin; o[5] = executed - executed_before; o[6] = ke - kb;   // (of the workgroup's LAST tile or k-chunk)
    o[7] = wall_clock64() - w_begin;
  }
#endif
}

// Persistent launch (large statistics): 8 x 32 workgroups, one per CU, pulling tiles from a host-built schedule
// (SyrkArgs::sched) instead of one tile per workgroup.  Workgroup b belongs to logical XCD b % 8 (what the dispatcher's
// round-robin gives -- if it ever does not, only locality is lost).  The tiles are dealt out in GROUPS of up to 32 that form
// a compact block of the lower region (4 tile rows x 8 tile columns: 12 distinct panels for 32 tiles instead of 64), one
// group per XCD and round.  Measured on one box, sigma_mlp 32768 x 14336, five / six planes per call:
//   one tile per workgroup, 2 x 2 super-blocks (round 1's launch)      25.3-25.5 / 38.9-39.0 ms   58 / -- GB of L2 misses
//   persistent, every workgroup through a fixed list of its own        24.5-24.6 / 38.2-38.3 ms   53 / 67 GB
//   persistent + a barrier of the XCD's 32 workgroups between rounds   25.4-25.6 / 40.4-40.6 ms   32 / 54 GB
//   persistent, tiles pulled from per-XCD queues (later in round 2, other kernel improvements included; fixed lists at that
//   point: 22.05 ms)                                                   21.3 / 35.5 ms             34 GB             <- shipped
// The lock-step variant halves the L2-miss traffic and is SLOWER: the misses are not what bounds the kernel (the power cap
// is: mdg_probe_mfma_i8), and 32 CUs folding into sigma and refilling their rings at the same instant
// cost more than the hits return.  (The fixed-list and barrier variants: scripts/probes/cov_i8_variants.patch.)
template <int P>  // planes used: 5 or 6
__global__ __launch_bounds__(64 * NW, 1) void i8_syrk_kernel(SyrkArgs a) {
  constexpr int TJ = TileShape<P>::TJ;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // The route is chosen on the DEVICE: mdg_cov_accum_i8 enqueues the three product launches and the fp64 kernel back to back,
  // and each exits at once unless the route of this call (i8_route_kernel, the exact route's state) selects it -- the host
  // never waits for the flag.  The six-plane launch also books the fp64 fallback in the route counters.
  {
    int live, fallbacks;
    const int runs = product_launch_runs<P>(a, live, fallbacks);
    if (P == 6 && fallbacks && a.route_counts && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.route_counts + 2, fallbacks);
    if (!runs) return;
    if (a.route_counts && blockIdx.x == 0 && threadIdx.x == 0) {
      if (runs == 2) {   // the exact route serves both legacy classes: book them as the route kernel classed them, and the exact count
        int six = 0;
        for (int p = 0; p < a.nprob; p++) six += (a.route_flag[p] & 3) == 1;
        if (live - six) atomicAdd(a.route_counts + 0, live - six);
        if (six) atomicAdd(a.route_counts + 1, six);
        atomicAdd(a.route_counts + 4, live);
      } else {
        atomicAdd(a.route_counts + (P == 5 ? 0 : 1), live);
      }
    }
  }
  unsigned executed = 0;
  const int lane = threadIdx.x & 63;
#ifdef MDG_I8_WGTIMES
  if (a.sched && threadIdx.x == 0) a.wgtimes[blockIdx.x * 64] = wall_clock64();
#endif
  if (a.sched) {
    const int xcd = blockIdx.x & 7;
    auto work = [&](const int2 entry) {
      const int code = __builtin_amdgcn_readfirstlane(entry.x), chunk = __builtin_amdgcn_readfirstlane(entry.y);
      if (code < 0 || (a.route_flag[code >> CODE_PROB] & 2)) return;   // (a statistic that went to the fp64 kernel: not ours)
      const SyrkProblem& pr = a.prob[code >> CODE_PROB];   // (uniform index into the kernel arguments: scalar loads)
      const int bi = (code >> CODE_BI) & ((1 << CODE_BI) - 1), bj = code & ((1 << CODE_BI) - 1);
      if (chunk == 0) {   // per-head statistics: the tile's columns start at the head's first feature
        i8_syrk_tile<P>(a, pr, bi, bj, 0, a.nk, pr.sigma, pr.ld_sigma, 0, pr.block ? bi * TI : 0, lds, executed);
      } else {   // the last round: k-chunk q of Q of this tile, folded into its own (zeroed) partial tile
        const int q = chunk & 31, Q = (chunk >> 5) & 31, pslot = chunk >> 10;
        const int kb = (int)((int64_t)a.nk * q / Q), ke = (int)((int64_t)a.nk * (q + 1) / Q);
        if (kb < ke) i8_syrk_tile<P>(a, pr, bi, bj, kb, ke, a.partial + (int64_t)pslot * TI * TJ, TJ, bi * TI, bj * TJ, lds, executed);
      }
    };
    // The schedule's groups are QUEUES, one per XCD (XCD x owns groups x, x + 8, ...): a workgroup pulls the next tile of its
    // XCD's queue with one atomic, and when that queue is empty helps the other XCDs with theirs.  The 32 tiles of a group
    // are still taken together by the 32 CUs of one XCD (same panels in the same L2), but a CU that runs a few percent faster
    // -- clocks differ from CU to CU and from board to board under the power cap -- simply takes more tiles, where fixed
    // lists made the whole launch wait for the slowest workgroup.  Which CU computes a tile does not change its result.
    __shared__ int next_entry;
#ifdef MDG_I8_WGTIMES
    int done = 0;
#endif
    for (int victim = 0; victim < 8; victim++) {
      const int x = (xcd + victim) & 7;
      const int entries = ((a.ngroups - x + 7) >> 3) * 32;     // of XCD x's groups
      for (;;) {
        __syncthreads();                                         // the previous tile is complete in every wave
        if (threadIdx.x == 0)
          next_entry = __hip_atomic_fetch_add(a.xcd_arrive + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(next_entry);
        if (t >= entries) break;
        work(a.sched[((t >> 5) * 8 + x) * 32 + (t & 31)]);
#ifdef MDG_I8_WGTIMES
        if (threadIdx.x == 0 && done < 60) a.wgtimes[blockIdx.x * 64 + 2 + done++] = wall_clock64();
#endif
      }
    }
  } else {
    // Tile (bi, bj): bi = 128-row block, bj = TJ-row block of the lower region (bj <= bi for 128 x 128 tiles, bj <= 2 bi + 1 for
    // 128 x 64).  XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2, so workgroup w belongs
    // to XCD w % 8 and is the (w / 8)-th one there.  The tiles are grouped into super-blocks that are square in features
    // (SI x SI tiles of 128 x 128, SI x 2 SI tiles of 128 x 64); a super-block lives on ONE XCD, so per k-step its tiles pull
    // each distinct panel row through that L2 once.  Super-blocks (R, C), C <= R, cover the lower region; tiles of a diagonal
    // super-block that lie above it exit at once.
    int bi, bj;
    constexpr int SI = P == 6 ? SB6 : SB5;   // super-block: SI x SI (or SI x 2 SI) tiles
    {
      constexpr int TPS = TJ == 128 ? SI * SI : SI * 2 * SI;   // tiles per super-block
      constexpr int SJ = TJ == 128 ? SI : 2 * SI;              // tile columns of a super-block
      const int w = blockIdx.x;
      const int q = w >> 3;
      const int sb = q / TPS * 8 + (w & 7), t_in = q % TPS;
      int R = (int)((sqrtf(8.f * sb + 1.f) - 1.f) * 0.5f);
      while ((R + 1) * (R + 2) / 2 <= sb) R++;
      while (R * (R + 1) / 2 > sb) R--;
      const int C = sb - R * (R + 1) / 2;
      bi = SI * R + t_in / SJ;
      bj = SJ * C + t_in % SJ;
    }
    if (bi >= a.prob[0].n / TI || bj * TJ > bi * TI + TI - 1) return;   // (one full-triangle statistic per launch on this path)
    i8_syrk_tile<P>(a, a.prob[0], bi, bj, 0, a.nk, a.prob[0].sigma, a.prob[0].ld_sigma, 0, 0, lds, executed);
  }
  if (a.mfma_count && lane == 0) atomicAdd(a.mfma_count, (unsigned long long)executed);
#ifdef MDG_I8_WGTIMES
  if (a.sched && threadIdx.x == 0) a.wgtimes[blockIdx.x * 64 + 1] = wall_clock64();
#endif
}

// The persistent launch's LAST round would keep R = (tiles mod 256) CUs busy for a whole tile while the others idle -- 16 of
// 256 at sigma_x's shape (528 tiles), 184 at sigma_mlp's (6328).  The schedule (schedule_for) therefore cuts each tile of that
// round into Q k-chunks -- R Q pieces worked by all CUs in ceil(R Q / 256) short rounds, 16 x 16 in one round resp. 184 x 4 in
// three -- each folding into its own fp64 partial tile; this kernel then adds a tile's partials to sigma in chunk order (a
// fixed order: the result stays run-to-run bit-identical).  One workgroup per 1024 elements of a split tile.
constexpr int COMBINE_ELEMS = 1024;   // tile elements per workgroup of the combine pass (4 per thread, all chunks' loads in flight together)
template <int P>
__global__ __launch_bounds__(256) void i8_tail_combine_kernel(SyrkArgs a, int n_tail) {
  constexpr int TJ = TileShape<P>::TJ;
  constexpr int PARTS = TI * TJ / COMBINE_ELEMS;
  int live, fallbacks;
  if (!product_launch_runs<P>(a, live, fallbacks)) return;     // the product launch of the other route produced the partials, or none did
  const int4 t = a.tail[blockIdx.x / PARTS];
  if (a.route_flag[t.x >> CODE_PROB] & 2) return;
  const SyrkProblem& pr = a.prob[t.x >> CODE_PROB];
  const int bi = (t.x >> CODE_BI) & ((1 << CODE_BI) - 1), bj = t.x & ((1 << CODE_BI) - 1), Q = t.y;
  const double* part = a.partial + (int64_t)t.z * TI * TJ;
#pragma unroll
  for (int i = 0; i < COMBINE_ELEMS / 256; i++) {
    const int e = (blockIdx.x % PARTS) * COMBINE_ELEMS + i * 256 + threadIdx.x;
    const int row = bi * TI + e / TJ, col = bj * TJ + e % TJ;
    if (col > row) continue;
    double* p = pr.sigma + (int64_t)row * pr.ld_sigma + col - (pr.block ? bi * TI : 0);
    double v = *p;
    for (int q = 0; q < Q; q++) v += part[(int64_t)q * TI * TJ + e];   // chunk order: fixed, so the sum is reproducible
    *p = v;
  }
}

// ---- tile schedule of the persistent launch (i8_syrk_kernel with SyrkArgs::sched)
// Groups of up to 32 tiles = one XCD's 32 CUs for one round.  The lower region is cut into macro-rows of 4 tile rows and those
// into chunks of 8 tile columns: a full group is a 4 x 8 block of tiles -- 4 A panels and 8 B panels shared by 32 tiles.  The
// ragged groups along the diagonal are then packed (tiles of the smallest ones fill up the largest), so that ceil(tiles / 32)
// groups -- and as few rounds as the tile count allows -- remain.  Built once per (device, tile-row count, tile shape) on the
// host and kept on the device: a few KB of immutable lookup data, the one allocation the library keeps across calls.
struct Schedule {
  int2* dev = nullptr;     // [ngroups][32] {tile code, k-chunk code}
  int4* tail = nullptr;    // [n_tail] {tile code, Q, first partial slot, 0}
  int ngroups = 0, n_tail = 0, pieces = 0;
};
constexpr int TAIL_MAX_Q = 16;         // k-chunks per tile of the split round(s) (a chunk should stay much longer than the 2-3 k-steps of ring fill)

// shapes: per statistic {row blocks of 128 features, block (0 = full lower triangle, 128 = per-head diagonal tiles)}
// The one thing the library keeps across calls: device copies of the schedules, a few KB each, keyed by (device, tile shape,
// statistic shapes).  Plain device memory -- no streams, no events (those are the caller's) -- released by mdg_shutdown(); the
// containers' destructors at process exit free host memory only and make no HIP call (the runtime may be gone by then).
std::mutex g_sched_mutex;
std::map<std::vector<int>, Schedule> g_sched_cache;

const Schedule* schedule_for(const std::vector<std::pair<int, int>>& shapes, int cw) {   // cw: tile columns per 128 features (1: 128 x 128 tiles, 2: 128 x 64)
  auto& cache = g_sched_cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_sched_mutex);
  std::vector<int> key = {dev, cw};
  for (auto& sh : shapes) {
    key.push_back(sh.first);
    key.push_back(sh.second);
  }
  auto it = cache.find(key);
  if (it != cache.end()) return &it->second;
  std::vector<std::vector<int>> full, ragged;
  for (size_t pi = 0; pi < shapes.size(); pi++) {
    const int rb = shapes[pi].first, pbits = (int)pi << CODE_PROB;
    if (shapes[pi].second) {   // per-head statistic: the diagonal tiles only
      std::vector<int> g;
      for (int h = 0; h < rb; h++)
        for (int c = 0; c < cw; c++) {
          g.push_back(pbits | (h << CODE_BI) | (h * cw + c));
          if (g.size() == 32) {
            full.push_back(g);
            g.clear();
          }
        }
      if (!g.empty()) ragged.push_back(g);
      continue;
    }
    for (int R = 0; R * 4 < rb; R++) {
      const int r1 = std::min(rb, R * 4 + 4);
      const int ncols = r1 * cw;                       // columns of the macro-row's last tile row
      for (int c0 = 0; c0 < ncols; c0 += 8) {
        std::vector<int> g;
        for (int bi = R * 4; bi < r1; bi++)
          for (int bj = c0; bj < c0 + 8; bj++)
            if (bj < (bi + 1) * cw) g.push_back(pbits | (bi << CODE_BI) | bj);
        if (g.size() == 32) full.push_back(g);
        else if (!g.empty()) ragged.push_back(g);
      }
    }
  }
  std::sort(ragged.begin(), ragged.end(), [](const std::vector<int>& x, const std::vector<int>& y) { return x.size() > y.size(); });
  size_t lo = 0, hi = ragged.size();
  while (lo + 1 < hi) {                               // fill the largest ragged group from the smallest one
    std::vector<int>& big = ragged[lo];
    std::vector<int>& small = ragged[hi - 1];
    while (big.size() < 32 && !small.empty()) {
      big.push_back(small.back());
      small.pop_back();
    }
    if (small.empty()) hi--;
    if (big.size() == 32) lo++;
  }
  std::vector<std::vector<int>> groups(full);        // all groups hold 32 tiles, except possibly the last one
  for (size_t i = 0; i < hi; i++)
    if (!ragged[i].empty()) groups.push_back(ragged[i]);
  size_t tiles = 0;
  for (auto& g : groups) tiles += g.size();
  std::vector<int2> table;
  std::vector<int4> tail;
  auto emit = [&](const std::vector<int>& g) {
    for (int i = 0; i < 32; i++) table.push_back(make_int2(i < (int)g.size() ? g[i] : -1, 0));
  };
  const size_t whole_groups = tiles / 256 * 8;        // the full rounds: 8 groups of 32 whole tiles each
  std::vector<int> rest;                              // tiles of the last, partly filled round
  for (size_t i = whole_groups; i < groups.size(); i++) rest.insert(rest.end(), groups[i].begin(), groups[i].end());
  // Q chunks per tile turn the R left-over tiles into R Q pieces worked in ceil(R Q / 256) short rounds of 1 / Q tile each
  // (+ ~4 % of a tile per round for the ring fill and the fold of a chunk): take the cheapest Q
  const int R = (int)rest.size();
  int Q = 1;
  double best = 1.0;
  for (int q = 2; q <= TAIL_MAX_Q && R > 0; q++) {
    if (R * q > TAIL_MAX_PIECES) break;
    const double cost = (double)((R * q + 255) / 256) * (1.0 / q + 0.04);
    if (cost < best - 0.02) { best = cost; Q = q; }
  }
  Schedule sch;
  if (Q >= 2) {
    for (size_t i = 0; i < whole_groups; i++) emit(groups[i]);
    // piece t Q + q = chunk q of tile t; piece p runs in tail round p / 256 on XCD p % 8; its partial tile is slot p
    const int pieces = R * Q, tail_rounds = (pieces + 255) / 256;
    std::vector<int2> last((size_t)tail_rounds * 256, make_int2(-1, 0));
    for (int t = 0; t < R; t++) {
      tail.push_back(make_int4(rest[t], Q, t * Q, 0));
      for (int q = 0; q < Q; q++) {
        const int piece = t * Q + q, idx = piece % 256;
        last[(size_t)(piece / 256) * 256 + (idx % 8) * 32 + idx / 8] = make_int2(rest[t], (piece << 10) | (Q << 5) | q);
      }
    }
    table.insert(table.end(), last.begin(), last.end());
    sch.n_tail = (int)tail.size();
    sch.pieces = pieces;
  } else {
    for (auto& g : groups) emit(g);
  }
  sch.ngroups = (int)(table.size() / 32);
  if (hipMalloc((void**)&sch.dev, table.size() * sizeof(int2)) != hipSuccess) return nullptr;
  if (hipMemcpy(sch.dev, table.data(), table.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  if (!tail.empty()) {
    if (hipMalloc((void**)&sch.tail, tail.size() * sizeof(int4)) != hipSuccess) return nullptr;
    if (hipMemcpy(sch.tail, tail.data(), tail.size() * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  }
  return &cache.emplace(key, sch).first->second;
}

// ---- host half of the two diagnostic builds: allocation before the product launches (diagnostics_begin), copy-back and printing
// after the call's last launch (report_product_diagnostics).  Both are empty in a normal build.
#ifdef MDG_I8_STAMPS
unsigned long long* g_stamps_dev = nullptr;
#endif
#ifdef MDG_I8_WGTIMES
unsigned long long* g_wgtimes_dev = nullptr;
#endif
int diagnostics_begin(SyrkArgs& a, hipStream_t st) {
#ifdef MDG_I8_STAMPS
  const size_t stamps_n = (size_t)STAMP_WGS * NW * 8;
  if (!g_stamps_dev) MDG_HIP(hipMalloc(&g_stamps_dev, stamps_n * 8));
  MDG_HIP(hipMemsetAsync(g_stamps_dev, 0, stamps_n * 8, st));
  a.stamps = g_stamps_dev;
#endif
#ifdef MDG_I8_WGTIMES
  if (!g_wgtimes_dev) MDG_HIP(hipMalloc(&g_wgtimes_dev, 256 * 64 * 8));
  MDG_HIP(hipMemsetAsync(g_wgtimes_dev, 0, 256 * 64 * 8, st));
  a.wgtimes = g_wgtimes_dev;
#endif
  (void)a;
  (void)st;
  return MDG_OK;
}

// One route's product: the LDS attribute, the launch -- persistent when there is a schedule, else one tile per workgroup -- and
// the tail combine of the schedule's k-split last round.
template <int P>
int launch_product(SyrkArgs& a, const Schedule* sch, hipStream_t st) {
  using S = TileShape<P>;
  constexpr int SI = P == 6 ? SB6 : SB5;                                     // super-block rows (see the kernel)
  constexpr int TPS = wide_tile(P) ? SI * SI : 2 * SI * SI;                  // tiles per super-block
  const int rb = a.prob[0].n / TI;
  const int sr = (rb + SI - 1) / SI, nsb = sr * (sr + 1) / 2;                // super-block rows, super-blocks
  dim3 grid((unsigned)((nsb + 7) / 8 * 8 * TPS));
  a.sched = nullptr;
  a.tail = nullptr;
  a.ngroups = 0;
  if (sch) {
    a.sched = sch->dev;
    a.tail = sch->tail;
    a.ngroups = sch->ngroups;
    grid = dim3(256);
  }
  MDG_HIP(hipFuncSetAttribute((const void*)i8_syrk_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS_BYTES));
  hipLaunchKernelGGL((i8_syrk_kernel<P>), grid, dim3(64 * NW), (size_t)S::LDS_BYTES, st, a);
  if (sch && sch->n_tail)
    hipLaunchKernelGGL((i8_tail_combine_kernel<P>), dim3(sch->n_tail * (TI * S::TJ / COMBINE_ELEMS)), dim3(256), 0, st, a, sch->n_tail);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace

// All three routes are enqueued; the flags the route kernel and the list kernels wrote decide on the device which one does the
// work (the other launches' workgroups exit on their first instruction: ~10 us each at the sigma_mlp grid).  No host round trip,
// graph-capturable.  ev_start / ev_stop bracket the product launches and their tail combines, nothing else.
int enqueue_products(const I8Call& c, bool offer_exact, void* ev_start, void* ev_stop) {
  SyrkArgs a;
  a.nprob = c.count;
  a.nk = c.nk;
  std::vector<std::pair<int, int>> shapes;
  for (int i = 0; i < c.count; i++) {
    const I8Stat& s = c.stat[i];
    a.prob[i] = SyrkProblem{s.planes, s.emax, s.zmask, s.sigma, s.ld_sigma, s.n, s.block};
    shapes.emplace_back(s.n / TI, s.block);
  }
  for (int i = c.count; i < MAX_PROBLEMS; i++) a.prob[i] = a.prob[0];
  a.mfma_count = &c.shared->mfma_count;
  a.route_flag = c.shared->route_flag;
  a.route_counts = c.route_counts;
  a.xcd_arrive = c.shared->xcd_queue;
  a.exact_state = offer_exact ? &c.shared->exact_overflow : nullptr;
  a.partial = c.partial;
  MDG_TRY(diagnostics_begin(a, c.st));
  // the persistent launch: one workgroup per CU, tiles of all statistics from one static schedule
  const Schedule* sched_of[2] = {nullptr, nullptr};       // [0]: 128 x 128 tiles, [1]: 128 x 64
  if (a.prob[0].n / TI >= PERSISTENT_MIN_ROWS || c.count > 1 || a.prob[0].block) {
    int dev = 0, n_cu = 0;
    MDG_HIP(hipGetDevice(&dev));
    MDG_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    if (n_cu == 256)   // 8 XCDs x 32 CUs is what the tables are cut for
      for (int i = 0; i < 2; i++) sched_of[i] = schedule_for(shapes, i + 1);
  }
  MDG_CHECK_ARG((c.count == 1 && !a.prob[0].block) || (sched_of[0] && sched_of[1]),
                "mdg_cov_accum_i8_multi: several statistics in one launch, and per-head statistics, need the persistent launch (a "
                "256-CU device); use mdg_cov_accum_i8 per full statistic and mdg_cov_accum for the per-head ones");
  {  // partial tiles of the k-split last round (only one of the three product launches runs: they share the region)
    size_t zero_bytes = 0;
    for (int i = 0; i < 2; i++)
      if (sched_of[i]) zero_bytes = std::max(zero_bytes, (size_t)sched_of[i]->pieces * TI * (i == 0 ? 128 : 64) * sizeof(double));
    if (zero_bytes) MDG_HIP(hipMemsetAsync(c.partial, 0, zero_bytes, c.st));
  }
  if (ev_start) MDG_HIP(hipEventRecord((hipEvent_t)ev_start, c.st));
  if (offer_exact) MDG_TRY(launch_product<3>(a, sched_of[0], c.st));      // the exact route's product: the three top planes, all nine pairs
  MDG_TRY(launch_product<5>(a, sched_of[0], c.st));
  MDG_TRY(launch_product<6>(a, sched_of[1], c.st));
  if (ev_stop) MDG_HIP(hipEventRecord((hipEvent_t)ev_stop, c.st));
  return MDG_OK;
}

int report_product_diagnostics(const I8Call& c) {
#if defined(MDG_I8_STAMPS) || defined(MDG_I8_WGTIMES)
  const int n = c.stat[0].n;
  hipStream_t st = c.st;
#endif
#ifdef MDG_I8_STAMPS
  {
    static unsigned long long host[STAMP_WGS * NW * 8];
    MDG_HIP(hipMemcpyAsync(host, g_stamps_dev, sizeof(host), hipMemcpyDeviceToHost, st));
    MDG_HIP(hipStreamSynchronize(st));
    double sum[2][6] = {};
    long cnt[2] = {};
    std::vector<double> ghz;   // in-kernel clock per wave: s_memtime cycles / 100 MHz wall ticks around its last tile
    for (int w = 0; w < STAMP_WGS * NW; w++) {
      const unsigned long long* o = host + (size_t)w * 8;
      if (!o[6]) continue;
      if (o[7]) ghz.push_back((double)o[4] / (double)o[7] * 0.1);
      const int role = (w % NW) >= NW / 2;
      for (int i = 0; i < 6; i++) sum[role][i] += (double)o[i] / (double)o[6];
      cnt[role]++;
    }
    for (int role = 0; role < 2; role++)
      if (cnt[role])
        fprintf(stderr, "[stamps n=%d] waves %s: per k-step cycles (s_memtime): wait+barrier %.0f  refill-first %.0f  reads+mfma-issue %.0f  "
                        "wait+refill-last %.0f  | whole tile / nk %.0f  mfma/step %.1f  (%ld waves)\n", n, role ? "4-7" : "0-3",
                sum[role][0] / cnt[role], sum[role][1] / cnt[role], sum[role][2] / cnt[role], sum[role][3] / cnt[role],
                sum[role][4] / cnt[role], sum[role][5] / cnt[role], cnt[role]);
    if (!ghz.empty()) {
      std::sort(ghz.begin(), ghz.end());
      fprintf(stderr, "[stamps n=%d] in-kernel clock (s_memtime / s_memrealtime x 100 MHz), median over %zu waves: %.3f GHz\n", n, ghz.size(),
              ghz[ghz.size() / 2]);
    }
  }
#endif
#ifdef MDG_I8_WGTIMES
  {
    static unsigned long long host[256 * 64];
    MDG_HIP(hipMemcpyAsync(host, g_wgtimes_dev, sizeof(host), hipMemcpyDeviceToHost, st));
    MDG_HIP(hipStreamSynchronize(st));
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int w = 0; w < 256; w++) if (host[w * 64]) { t0 = std::min(t0, host[w * 64]); t1 = std::max(t1, host[w * 64 + 1]); }
    if (t1) {
      std::vector<double> ends;
      double xcd_end[8] = {};
      for (int w = 0; w < 256; w++) { const double e = (host[w * 64 + 1] - t0) * 1e-5; ends.push_back(e); xcd_end[w & 7] = std::max(xcd_end[w & 7], e); }
      std::sort(ends.begin(), ends.end());
      fprintf(stderr, "[wgtimes n=%d] kernel %.3f ms; workgroup end times (ms): min %.3f  p10 %.3f  median %.3f  p90 %.3f  max %.3f; last end per XCD:", n,
              (t1 - t0) * 1e-5, ends[0], ends[25], ends[128], ends[230], ends[255]);
      for (int x = 0; x < 8; x++) fprintf(stderr, " %.3f", xcd_end[x]);
      // time of the last whole round's end and per-round durations of workgroup 0 and of the slowest workgroup
      int slow = 0;
      for (int w = 0; w < 256; w++) if (host[w * 64 + 1] > host[slow * 64 + 1]) slow = w;
      fprintf(stderr, "\n   slowest workgroup %d, its rounds end at (ms):", slow);
      for (int r = 0; r < 60 && host[slow * 64 + 2 + r]; r++) fprintf(stderr, " %.2f", (host[slow * 64 + 2 + r] - t0) * 1e-5);
      int fast = 0;
      for (int w = 0; w < 256; w++) if (host[w * 64 + 1] < host[fast * 64 + 1]) fast = w;
      fprintf(stderr, "\n   fastest workgroup %d, its rounds end at (ms):", fast);
      for (int r = 0; r < 60 && host[fast * 64 + 2 + r]; r++) fprintf(stderr, " %.2f", (host[fast * 64 + 2 + r] - t0) * 1e-5);
      fprintf(stderr, "\n");
    }
  }
#endif
  (void)c;
  return MDG_OK;
}

// mdg_shutdown(): give the cached schedules back.  The caller guarantees no int8 covariance call is in flight.
int release_i8_schedules() {
  std::lock_guard<std::mutex> lock(g_sched_mutex);
  int dev0 = 0;
  const bool have_dev = hipGetDevice(&dev0) == hipSuccess;
  int rc = MDG_OK;
  for (auto& kv : g_sched_cache) {
    if (hipSetDevice(kv.first[0]) != hipSuccess) { rc = MDG_ERR_HIP; continue; }
    if (kv.second.dev && hipFree(kv.second.dev) != hipSuccess) rc = MDG_ERR_HIP;
    if (kv.second.tail && hipFree(kv.second.tail) != hipSuccess) rc = MDG_ERR_HIP;
  }
  g_sched_cache.clear();
  if (have_dev) (void)hipSetDevice(dev0);
  (void)hipGetLastError();
  return rc;
}

}  // namespace mdg
