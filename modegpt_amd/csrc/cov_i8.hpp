// What the units of the int8 covariance (cov_i8*.hip; the map is at the head of cov_i8.hip) share: the constants more than one
// of them needs, the structs that cross a unit boundary -- all in namespace mdg: a struct in an anonymous namespace would be a
// different type in every unit -- and the host functions each unit exposes.  Kernels and unit-private helpers stay anonymous.
#pragma once
#include <cstddef>

#include "common.hpp"

namespace mdg {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int NP = 6;            // digit planes written by the split pass; the product kernel uses the top 3, the top 5 or all 6
constexpr int TI = 128;          // output tile rows (rows of the I operand); its width TJ is 64 or 128, see TileShape
constexpr int KS = 32;           // tokens per k-step (one v_mfma_i32_32x32x32_i8)
// k-steps between folds of the int32 classes into sigma.  A bf16 element is an 8-bit significand at some shift, so its balanced
// digits are two full digits and a carry digit at most, and a class sum grows by at most 32768 per token (enumerated over
// every digit vector the split pass can produce: scripts/probes/i8_int32_bound.py) -- 65535 tokens = 2047 k-steps stay below
// 2^31.  (First versions: 512, from the cruder bound 6 pairs x 128 x 128 per token; one fold per launch costs 0.65 ms at the
// sigma_mlp shape.)
constexpr int FLUSH_STEPS = 2047;
// The same enumeration for fp16 (scripts/probes/i8_int32_bound_f16.py): an 11-bit significand spreads over three digits, but where
// two of them are full the third holds at most 3 bits and a carry -- the worst pair is still (c, -128, -128) against itself,
// 2 x 128 x 128 = 32768 per token, so fp16 allows the same 2047 k-steps.  The product kernels read planes only and fold every
// FLUSH_STEPS k-steps whatever the element type: that interval must not exceed what either type allows.
constexpr int FLUSH_STEPS_F16 = 2047;
static_assert(FLUSH_STEPS <= FLUSH_STEPS_F16, "the product kernels' fold interval must hold for fp16 elements too");
constexpr int TOP_SHIFT = 8 * NP - 10;  // 38: the column maximum's significand sits below bit 46 of the 48-bit integer (bf16: 8 bits)
constexpr int TOP_SHIFT_F16 = 8 * NP - 13;  // 35: the same place for fp16's 11 bits

// ---- element traits of the kernels that interpret the bits of x (split, lists, remainder products, column kernel).  Both types
// are decoded to (signed significand, effective exponent ee) ON ONE EXPONENT SCALE -- the fp32 exponent field of the value's
// binade, 255 for Inf / NaN -- such that with the type's top shift the column's unit is 2^(E_j - 172) for both: everything behind
// the split (planes, emax, the route, the product kernels' fold, the lists' scale) is the same code for either type.
//   bf16: value = sig 2^(ee - 134), |sig| < 2^8;   N = sig << (38 - (E - ee))
//   fp16: value = sig 2^(ee - 137), |sig| < 2^11;  N = sig << (35 - (E - ee)),  ee = exponent field + 112 in 113 .. 142 (subnormals: 113)
// A finite fp16 column spans at most 29 binades (<= 35): every element is an exact integer, subnormals included; nothing is
// ever rounded and the bound's rho term is identically 0.
struct Bf16Elem {
  static constexpr int TOP = TOP_SHIFT, SIG_BITS = 8;
  static __device__ __forceinline__ void parts(unsigned b, int& sig, int& ee) {
    const int e = (b >> 7) & 0xFF, m = b & 0x7F;
    sig = e ? (128 | m) : m;
    ee = e ? e : 1;
    if (b & 0x8000) sig = -sig;
  }
  static __device__ __forceinline__ int ee_if_nonzero(unsigned b) {  // effective exponent of a nonzero value, 0 for +-0
    const int e = (b >> 7) & 0xFF;
    return (b & 0x7FFF) ? (e ? e : 1) : 0;
  }
  static __device__ __forceinline__ bool is_nan(unsigned b) { return (b & 0x7FFFu) > 0x7F80u; }
  static __device__ __forceinline__ double to_f64(unsigned b) { return (double)__uint_as_float(b << 16); }
  // the two elements of a dword, exactly
  static __device__ __forceinline__ double lo_f64(unsigned w) { return (double)__uint_as_float(w << 16); }
  static __device__ __forceinline__ double hi_f64(unsigned w) { return (double)__uint_as_float(w & 0xFFFF0000u); }
  static __device__ __forceinline__ unsigned from_f64(double v) { return __float_as_uint((float)v) >> 16; }   // v representable: exact
  // an element has a digit below plane 2 iff it lies more than 38 - 24 binades under E (and is not zero): 0 < |bits| < deep_limit(E)
  static __device__ __forceinline__ unsigned deep_limit(int E) { return (unsigned)max(E - 14, 1) << 7; }
};
struct F16Elem {
  static constexpr int TOP = TOP_SHIFT_F16, SIG_BITS = 11;
  static __device__ __forceinline__ void parts(unsigned b, int& sig, int& ee) {
    const int e = (b >> 10) & 0x1F, m = b & 0x3FF;
    sig = e ? (1024 | m) : m;
    ee = e == 31 ? 255 : (e ? e : 1) + 112;     // Inf / NaN: the exponent the route kernel takes a column out for
    if (b & 0x8000) sig = -sig;
  }
  static __device__ __forceinline__ int ee_if_nonzero(unsigned b) {
    const int e = (b >> 10) & 0x1F;
    return (b & 0x7FFF) ? (e == 31 ? 255 : (e ? e : 1) + 112) : 0;
  }
  static __device__ __forceinline__ bool is_nan(unsigned b) { return (b & 0x7FFFu) > 0x7C00u; }
  static __device__ __forceinline__ double to_f64(unsigned b) { return f16_to_f64((f16_t)b); }
  static __device__ __forceinline__ double lo_f64(unsigned w) { return f16_to_f64((f16_t)(w & 0xFFFFu)); }
  static __device__ __forceinline__ double hi_f64(unsigned w) { return f16_to_f64((f16_t)(w >> 16)); }
  static __device__ __forceinline__ unsigned from_f64(double v) { return __half_as_ushort(__float2half((float)v)); }   // v representable: exact
  // ... more than 35 - 24 = 11 binades under E: exponent field below (E - 112) - 11
  static __device__ __forceinline__ unsigned deep_limit(int E) { return (unsigned)max(E - 123, 1) << 10; }
};
// max(x, 0) on the bits of one element / of the two elements of a dword (MDG_I8_RELU): anything with the sign bit set becomes +0
// -- -0 and -Inf included -- except a NaN, which stays the NaN it is.
template <class EL, bool RELU>
__device__ __forceinline__ unsigned relu_bits(unsigned b) {
  return (RELU && (b & 0x8000u) && !EL::is_nan(b)) ? 0u : b;
}
template <class EL, bool RELU>
__device__ __forceinline__ unsigned relu_pair(unsigned w) {
  if (!RELU) return w;
  return relu_bits<EL, true>(w & 0xFFFFu) | (relu_bits<EL, true>(w >> 16) << 16);
}
// Host side: one launch statement for the four (element type, ReLU) instantiations of a kernel template.
#define MDG_I8_DISPATCH(c, KERNEL, ...)                                                   \
  do {                                                                                    \
    if ((c).f16) {                                                                        \
      if ((c).relu) hipLaunchKernelGGL((KERNEL<F16Elem, true>), __VA_ARGS__);             \
      else hipLaunchKernelGGL((KERNEL<F16Elem, false>), __VA_ARGS__);                     \
    } else {                                                                              \
      if ((c).relu) hipLaunchKernelGGL((KERNEL<Bf16Elem, true>), __VA_ARGS__);            \
      else hipLaunchKernelGGL((KERNEL<Bf16Elem, false>), __VA_ARGS__);                    \
    }                                                                                     \
  } while (0)

// The same for the kernels that also honour the row bitmask of MDG_I8_ROWS (template <EL, RELU, ROWS>): without the flag the
// ROWS = false instantiations run, which are the code the kernels had before the flag existed.
#define MDG_I8_DISPATCH_ROWS(c, KERNEL, ...)                                              \
  do {                                                                                    \
    if ((c).rows) {                                                                       \
      if ((c).f16) {                                                                      \
        if ((c).relu) hipLaunchKernelGGL((KERNEL<F16Elem, true, true>), __VA_ARGS__);     \
        else hipLaunchKernelGGL((KERNEL<F16Elem, false, true>), __VA_ARGS__);             \
      } else {                                                                            \
        if ((c).relu) hipLaunchKernelGGL((KERNEL<Bf16Elem, true, true>), __VA_ARGS__);    \
        else hipLaunchKernelGGL((KERNEL<Bf16Elem, false, true>), __VA_ARGS__);            \
      }                                                                                   \
    } else if ((c).f16) {                                                                 \
      if ((c).relu) hipLaunchKernelGGL((KERNEL<F16Elem, true, false>), __VA_ARGS__);      \
      else hipLaunchKernelGGL((KERNEL<F16Elem, false, false>), __VA_ARGS__);              \
    } else {                                                                              \
      if ((c).relu) hipLaunchKernelGGL((KERNEL<Bf16Elem, true, false>), __VA_ARGS__);     \
      else hipLaunchKernelGGL((KERNEL<Bf16Elem, false, false>), __VA_ARGS__);             \
    }                                                                                     \
  } while (0)
// MDG_I8_ROWS: is token t one of the rows that left the int8 path (cov_i8_rows.hip)?  Such a row reads as +0.
template <bool ROWS>
__device__ __forceinline__ bool row_left(const unsigned* rowmask, int64_t t) {
  return ROWS && ((rowmask[t >> 5] >> (t & 31)) & 1u);
}

// Per-column integers the split pass accumulates for the route (i8_route_kernel; host model: tests/i8_model.py), as [NSTAT][n]
// unsigned long long: q_s = sum over tokens of d_s^2 for the six planes, the signed sum of d_0 d_1 (so that the energy of the top
// two digits together, hence a lower bound on the column's norm, is an integer too), and two counters packed into one word.
constexpr int NSTAT = 8;
constexpr int STAT_D0D1 = 6, STAT_COUNTS = 7;     // [7]: (elements rounded to an integer: more than 38 binades down; fp16: never) << 32 | nonzero elements
constexpr int EMAX_COLUMN_OUT = 0x100;            // bit set in emax[j] by the route kernel: column j is computed by the fp64 column kernel

// Planes the product kernels may read even where the piece mask says "all zero": both load every plane below their MIN_DEPTH
// unconditionally (3 for five planes, 4 for six).  Pieces of the planes from here on are WRITTEN only when they hold a nonzero
// there or in a deeper plane of the same piece (a product kernel that finds plane 5 present loads plane 4 as well) -- on
// Gaussian / ReLU / SiLU-gated activations planes 4 and 5 practically never do: a third of the split pass's writes.
constexpr int ALWAYS_WRITTEN_PLANES = 4;

constexpr int MAX_PROBLEMS = 4;        // the four hooks of a layer: sigma_mlp, sigma_x, sigma_q, sigma_k
constexpr int ROUTE_JMAX = MDG_I8_MAX_COLUMNS;   // columns per statistic and call the fp64 column kernel takes (32)
constexpr int TAIL_MAX_PIECES = 1024;  // partial tiles of the persistent launch's k-split last round (chunks of all split tiles together)
constexpr size_t PARTIAL_BYTES = (size_t)TAIL_MAX_PIECES * TI * 128 * sizeof(double);   // partial tiles of at most 128 x 128

struct RouteOut {                           // per statistic, in the workspace (mdg_cov_accum_i8_route reads it back)
  int planes;                               // 5, 6, or 0: the whole statistic goes through the fp64 kernel
  int n_out;                                // columns handed to the fp64 column kernel
  int out[ROUTE_JMAX];                      // ... in the order they were taken
  double sq, x;                             // SQ_P, X_P of the columns that stay (the guaranteed bound is their sum)
  double rho;                               // 2 R + R^2 alone: what is left of the bound when no plane pair is dropped (the exact route)
};
constexpr int ROWS_MAX = MDG_I8_MAX_ROWS;   // token rows per statistic and call the fp64 row kernel takes (64)
struct RowsOut {                            // per statistic, in the workspace, with MDG_I8_ROWS (mdg_cov_accum_i8_rows reads it back)
  int n_rows;                               // rows that left the int8 path: 0, or 1 .. ROWS_MAX
  int n_dominant;                           // rows the vote found dominant (diagnostic: 0 or more than the limits -> nothing left)
  int rows[ROWS_MAX];                       // ... ascending
};
struct RouteScratch {            // behind the route statistics, zeroed with them before every call
  int ticket, forced;
};

// The first SHARED_BYTES of the workspace, zeroed at the start of every call.  The byte offsets are part of what the kernels
// were built against (LoArgs::state is the block's start, indexed in ints), hence pinned.
constexpr size_t SHARED_BYTES = 256;
struct SharedBlock {
  int reserved[2];
  unsigned long long mfma_count;     // += v_mfma instructions the product launch executed (mdg_cov_accum_i8_stats)
  int xcd_queue[8];                  // the persistent launch's per-XCD tile-queue counters
  int route_flag[MAX_PROBLEMS];      // per statistic, i8_route_kernel: bit 0 -> needs six planes, bit 1 -> the fp64 kernel
  int exact_overflow, exact_ran, exact_mode;   // the exact route: a list overflowed; lists were built; 1 sparse lists, 2 dense
  int rows_flag;                     // the call set MDG_I8_ROWS (read back by mdg_cov_accum_i8_route / _rows)
};
static_assert(offsetof(SharedBlock, mfma_count) == 8 && offsetof(SharedBlock, xcd_queue) == 16 && offsetof(SharedBlock, route_flag) == 48 &&
                  offsetof(SharedBlock, exact_overflow) == 64 && offsetof(SharedBlock, exact_ran) == 68 &&
                  offsetof(SharedBlock, exact_mode) == 72 && sizeof(SharedBlock) <= SHARED_BYTES,
              "the shared block's layout is fixed");

// One statistic of a call and its parts of the workspace.  block == 0: sigma is n x n, lower triangle; block == 128: sigma is
// [n / 128][128][128] (per-head Grams of a [tokens][heads x 128] activation): only the diagonal 128 x 128 tiles exist, element
// (row, col) of head row / 128 lives at sigma[row * ld_sigma + col - 128 (row / 128)] with ld_sigma = 128.
struct LoEntry;                  // cov_i8_exact.hip
struct I8Stat {
  const bf16_t* x;
  int64_t ld;
  double* sigma;
  int64_t ld_sigma;
  int n, block;                  // n: columns of the activation matrix
  int* route_flag;               // this statistic's word of SharedBlock::route_flag
  signed char* planes;           // digit planes, [plane][32-row group][k-step][k-half][row][16 tokens]
  int* emax;                     // column maxima (n ints, padded to 8 bytes), then the [NSTAT][n] route statistics and a RouteScratch
  unsigned char* zmask;          // [nk][n / 32] piece masks
  double* vals;                  // alpha_s / rho per column, then the route kernel's per-workgroup partial maxima
  RouteOut* route;
  double* colpart;               // chunk partials of the fp64 column kernel
  LoEntry *lo_entries, *lo_rentries;   // the exact route: event lists per column; sparse mode: merged (group, residue) lists
  int *lo_counts, *lo_rtotals;         // ... and their lengths
  bf16_t* lo_xd;                 // the x_d copy of the exact route: [tokens][n] of x's element type
  unsigned* rowmask;             // MDG_I8_ROWS: bit t of the mask = token t left for the fp64 row kernel; then the votes and the list,
  int* votes;                    // [tokens]                                                     (one region, zeroed per call when the
  RowsOut* rows_out;             //                                                               flag is set, untouched otherwise)
  bool vec() const { return (uintptr_t)x % 16 == 0 && ld % 8 == 0; }   // rows are 16-byte addressable
  unsigned long long* stats() const { return (unsigned long long*)(emax + (n + 1) / 2 * 2); }
};
struct I8Call {
  int count, nk;                 // statistics; k-steps of KS tokens
  int64_t n_tokens;
  I8Stat stat[MAX_PROBLEMS];
  bool f16, relu;                // MDG_I8_F16: x holds fp16 (else bf16); MDG_I8_RELU: max(x, 0) on load -- every statistic of the call
  bool rows;                     // MDG_I8_ROWS: outlier token rows may leave for the fp64 row kernel -- every statistic of the call
  SharedBlock* shared;
  double* partial;               // PARTIAL_BYTES behind the shared block
  int* route_counts;             // optional device counters [five planes, six planes, fp64 fallback, columns out, exact route] and,
                                 // with MDG_I8_ROWS, [5]: rows handed to the fp64 row kernel
  hipStream_t st;
};

// column maxima + the route statistics + the route kernel's ticket: zeroed together per call
inline size_t ints_bytes(int64_t n) { return (size_t)((n + 1) / 2 * 2) * sizeof(int) + (size_t)(NSTAT * n) * sizeof(unsigned long long) + sizeof(RouteScratch); }

// ---- what each unit exposes: workspace sizes of its own structures, and the functions that enqueue its stage.  All return MDG_OK
// or an error code with the message set.  (Hidden: the library's exported symbols stay what they were.)
#pragma GCC visibility push(hidden)
// cov_i8_split.hip: zero the statistic's integers, column maxima, digit planes + route statistics + piece masks; with MDG_I8_ROWS the
// row selection (enqueue_row_selection) and the second maximum pass run between the first maximum pass and the split
int enqueue_split(const I8Call& c, int i);
int enqueue_colmax(const I8Call& c, int i, bool masked);
// cov_i8_rows.hip (MDG_I8_ROWS only): the rows of statistic i that leave the int8 path -- votes, selection, row bitmask -- from the
// column maxima over all rows; after the products, sigma += X_R^T X_R of those rows in fp64
struct RowsWsBytes { size_t mask, votes, out; };
RowsWsBytes rows_ws_bytes(int64_t n_tokens);
int enqueue_row_selection(const I8Call& c, int i);
int enqueue_rows_product(const I8Call& c, int i);
// cov_i8_route.hip: the route of statistic i and the clearing of the columns it hands out; after the products, those columns in fp64
size_t route_vals_bytes(int64_t n);
size_t column_partials_bytes(int64_t n);
int enqueue_route(const I8Call& c, int i, double tolerance);
int enqueue_columns(const I8Call& c, int i);
// cov_i8_exact.hip: the remainder lists of every statistic (before the products), the remainder products (after them)
struct LoWsBytes { size_t entries, counts, xd, rentries, rtotals; };
LoWsBytes lo_ws_bytes(int64_t n_tokens, int64_t n);
int enqueue_lo_lists(const I8Call& c, bool always);
int enqueue_lo_products(const I8Call& c, bool always);
// cov_i8_product.hip: the three product launches (exact route's three planes if offered, five, six) with their tail combines,
// between ev_start and ev_stop; the host half of the two diagnostic builds, empty otherwise
int enqueue_products(const I8Call& c, bool offer_exact, void* ev_start, void* ev_stop);
int report_product_diagnostics(const I8Call& c);
#pragma GCC visibility pop

}  // namespace mdg
