// sigma += X^T X through the int8 matrix cores: an ERROR-FREE SPLIT of the bf16 (or fp16: flag MDG_I8_F16) activations into digit
// planes and a TRUNCATED plane-pair product whose error is bounded per call.  What follows is written for bf16; an fp16 value is a
// signed 11-bit significand, placed 35 instead of 38 bits up so that the column's unit is 2^(E_j - 172) for both (E_j on the fp32
// exponent scale: the element traits in cov_i8.hpp) -- every finite fp16 element is then an exact integer, and only the kernels
// that read x itself differ.  MDG_I8_RELU applies max(x, 0) wherever x is read.  MDG_I8_ROWS lets up to 64 outlier token rows per
// statistic leave the int8 path for an fp64 row kernel (cov_i8_rows.hip has the rule); without the flag none of that is launched.
//
// A bf16 value is a signed 8-bit significand times a power of two.  Against a per-column scale 2^(E_j - 172), E_j the largest
// exponent in column j of this call, it is a 48-bit fixed-point integer N = sig << (38 - (E_j - e)): six balanced base-256
// digits d_0..d_5 in [-128, 127] (|d_0| <= 64) -- exactly, for every element within 38 binades of its column maximum.  Then
//     x_ti x_tj = 2^(E_i + E_j - 344) * sum_{s,t} d_s(t,i) d_t(t,j) 256^(10 - s - t)
// and sum over tokens of d_s d_t is an int8 MFMA product with exact int32 accumulation.  The product keeps the plane pairs with
// s + t < P (P = 5: 15 pairs, P = 6: 21 pairs) and DROPS the others.  What the dropped pairs can amount to is bounded from integer
// plane energies the split pass accumulates per column (Cauchy-Schwarz over the tokens; i8_route_kernel below has the derivation):
//     |sigma_ij(P) - sigma_ij| <= (SQ_P + X_P) sqrt(sigma_ii sigma_jj),   entry-wise, for any input,
// and the route is the smallest P with SQ_P <= 1e-12 (the attained part) and X_P <= tau_x <= 1e-11 (cross terms), after at most 32
// columns have been handed to an fp64 column kernel: GUARANTEED <= 1.1e-11, MEASURED <= 1e-12 (scripts/probes/i8_error_bound.py,
// i8_fuzz.py; Gaussian / ReLU columns take five planes at 2e-14 .. 2e-13, SiLU- / GELU-gated products -- the MLP statistic of a
// real Llama -- six at 6e-14; a column whose bulk sits 10+ binades under a few massive activations leaves alone).  Otherwise the
// whole statistic goes through the fp64 kernel (mdg_cov_accum).
// fp64 reference semantics: src/adapters/LlamaAdapter.py:127-147 (sigma += X^T X with X upcast to fp64).
//
// The units, and the kernels of a call in launch order (all are enqueued for every call; the device picks: each workgroup of a
// launch whose route was not taken exits on its first instruction):
//   cov_i8.hpp           shared constants, the workspace's shared block (SharedBlock), I8Call / I8Stat, the units' host functions
//   cov_i8.hip           this file: workspace layout, argument checks, the six extern "C" entry points
//   cov_i8_split.hip     per statistic:
//     i8_colmax_kernel / i8_colmax_vec_kernel   E_j = max exponent per column (_vec: rows are 16-byte addressable, the usual case)
//   cov_i8_rows.hip      per statistic, with MDG_I8_ROWS only:
//     i8_row_votes_kernel, i8_row_select_kernel   which token rows leave (list + bitmask); then the maximum pass again, over the
//                        rows that stayed (exits at once when none left).  Every kernel below that reads x reads those rows as +0
//   cov_i8_split.hip     per statistic:
//     i8_split_kernel / i8_split_vec_kernel     six digit planes, written in the blocked layout the product kernel streams: [plane]
//                        [32-row group][k-step][k-half][row][16 tokens] -- each 1 KB piece is one contiguous global_load_lds_dwordx4
//                        per wave; accumulates the per-column integers of the route (sum of d_s^2 per plane, sum of d_0 d_1, nonzero /
//                        rounded counts) on the way, and writes one mask byte per (k-step, 32-row group) saying which planes hold a
//                        nonzero there (an element is two full digits and a carry digit, so whole pieces of the deeper planes are
//                        zero on real activations)
//   cov_i8_route.hip     per statistic:
//     i8_route_kernel    the route: bit 0 of the statistic's flag -> six planes, bit 1 -> the fp64 kernel for the whole statistic;
//                        bit 8 of emax[j] -> column j is computed by the fp64 column kernel (read by the launches below)
//     i8_clear_columns_kernel   zeroes the digits of such columns and refreshes their groups' piece masks
//   cov_i8_exact.hip     the exact route's event lists (elements with digits below plane 2), unless the caller declined it:
//     i8_extract_lo_kernel, i8_compact_lo_kernel   one list per column, in token order
//     i8_lo_mode_kernel  sparse or dense lists -> which remainder kernels run
//     i8_residue_lo_kernel                         sparse: merged lists per (32-column group, column mod 4)
//     i8_copy_xd_kernel, i8_patch_xd_kernel        dense: a bf16 copy of x with every listed element cut to its top three planes
//   cov_i8_product.hip   between ev_start and ev_stop:
//     i8_syrk_kernel<3>, i8_tail_combine_kernel<3>   the exact route's product: planes 0 .. 2, all nine plane pairs
//     i8_syrk_kernel<5>, i8_tail_combine_kernel<5>   the truncated products: 15 pairs of the top five planes,
//     i8_syrk_kernel<6>, i8_tail_combine_kernel<6>   21 pairs of all six
//                        output tiles of the lower triangle, two waves per SIMD inside one workgroup of 8 waves:
//                        P = 3, 5: 128 x 128 tile, wave tile 64 x 32 (160 int32 accumulators; a 64 x 64 wave tile's 320 would not
//                        fit); P = 6: 128 x 64 tile, wave tile 32 x 32 (96).  Per k-step of 32 tokens ONE set of fragment reads
//                        feeds all plane-pair products of the wave tile (3x less LDS traffic per MFMA than separate GEMMs, which
//                        is what lets it pass the library's int8 rate); 3- / 4-stage LDS ring filled by LDS-DMA from SGPR piece
//                        descriptors, the two waves of a SIMD in opposite load / multiply order, one raw barrier per stage; every
//                        2047 k-steps (65504 tokens, the int32 bound) the classes are folded into sigma in fp64.  Planes beyond a
//                        32-row group's depth in a k-step (piece masks) are neither written, nor loaded, nor read from LDS, nor
//                        multiplied: no bit of the result changes, and 28 - 37 % of the MFMAs go on SiLU-gated / Gaussian data.
//                        Statistics of 2048 features and more (everything ops.py sends here) run as a persistent launch: one
//                        workgroup per CU pulling tiles from per-XCD queues, the last, partly filled round cut into k-chunks that
//                        fold into fp64 partial tiles, which the tail combine adds to sigma in chunk order
//   cov_i8_exact.hip     the exact route's remainder products, in fp64:
//     i8_lo_product_kernel                         sparse lists: one workgroup per 128 x 128 tile
//     i8_lo_wide_kernel<false>, i8_lo_wide_kernel<true>   dense lists: X_lo^T X, then X_d^T X_lo
//   cov_i8_route.hip     per statistic:
//     i8_columns_kernel, i8_columns_reduce_kernel   rows / columns of sigma of the columns that left, in plain fp64
//   cov_i8_rows.hip      per statistic, with MDG_I8_ROWS only:
//     i8_rows_product_kernel                        sigma += X_R^T X_R of the rows that left, v_mfma_f64 (not for a statistic on the fallback)
//   cov.hip              per statistic: the gated fp64 kernel (cov_accum_gated), for a statistic whose flag has bit 1 set
// ev_start / ev_stop bracket the three int8 product launches and their tail combines -- not the split, the route or the list
// building before them, nor the remainder, column and fallback kernels after them.
// Where a comment in these units points at scripts/probes/*.patch: those patches apply to the single-file cov_i8.hip of the commit
// before the split into units.
#include <algorithm>

#include "cov_i8.hpp"

namespace mdg {
namespace {

// Workspace layout of a call: [shared block][partial tiles], then per statistic [digit planes][column maxima, route statistics]
// [alpha / rho][RouteOut][column-kernel partials][piece masks][the exact route's lists, counts, x_d copy, merged lists][MDG_I8_ROWS:
// row bitmask, votes, row list -- reserved always, zeroed and used only with the flag], then the fp64 fallback's split-K space.  Returns the bytes a call needs; with `out`, the call's pointers into `ws`.
size_t layout(int count, const mdg_cov_problem* pr, void* ws, I8Call* out, size_t* fallback_off) {
  size_t off = SHARED_BYTES + PARTIAL_BYTES, fb = 0;
  char* const base = (char*)ws;
  if (out) {
    out->count = count;
    out->n_tokens = pr[0].n_tokens;
    out->nk = (int)ceil_div(pr[0].n_tokens, KS);
    out->shared = (SharedBlock*)base;
    out->partial = (double*)(base + SHARED_BYTES);
  }
  for (int i = 0; i < count; i++) {
    const int64_t cols = pr[i].n_feat * pr[i].batch, T = pr[i].n_tokens;
    const LoWsBytes lo = lo_ws_bytes(T, cols);
    I8Stat s;
    s.x = (const bf16_t*)pr[i].x; s.ld = pr[i].ld;
    s.sigma = pr[i].sigma; s.ld_sigma = pr[i].ld_sigma;
    s.n = (int)cols; s.block = pr[i].batch > 1 ? TI : 0;
    s.route_flag = out ? out->shared->route_flag + i : nullptr;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += bytes; return p; };
    s.planes = (signed char*)take(align_up((size_t)NP * (size_t)cols * (size_t)ceil_div(T, KS) * KS, 256));
    s.emax = (int*)take(align_up(ints_bytes(cols), 256));
    s.vals = (double*)take(align_up(route_vals_bytes(cols), 256));
    s.route = (RouteOut*)take(align_up(sizeof(RouteOut), 256));
    s.colpart = (double*)take(align_up(column_partials_bytes(cols), 256));
    s.zmask = (unsigned char*)take(align_up((size_t)ceil_div(T, KS) * (size_t)(cols / 32), 256));
    s.lo_entries = (LoEntry*)take(lo.entries);
    s.lo_counts = (int*)take(align_up(lo.counts, 256));
    s.lo_xd = (bf16_t*)take(align_up(lo.xd, 256));
    s.lo_rentries = (LoEntry*)take(lo.rentries);
    s.lo_rtotals = (int*)take(align_up(lo.rtotals, 256));
    const RowsWsBytes rw = rows_ws_bytes(T);
    s.rowmask = (unsigned*)take(rw.mask);
    s.votes = (int*)take(rw.votes);
    s.rows_out = (RowsOut*)take(rw.out);
    if (out) out->stat[i] = s;
    fb = std::max(fb, mdg_cov_accum_ws_bytes(T, pr[i].n_feat, pr[i].batch));
  }
  if (fallback_off) *fallback_off = off;
  return off + fb + 256;
}

bool problems_ok(int count, const mdg_cov_problem* pr) {
  if (count < 1 || count > MAX_PROBLEMS || !pr) return false;
  for (int i = 0; i < count; i++) {
    if (pr[i].n_tokens != pr[0].n_tokens || pr[i].n_tokens < 0 || pr[i].n_tokens >= (1ll << 28) || pr[i].n_feat <= 0 || pr[i].batch < 1) return false;
    if (pr[i].batch == 1 ? pr[i].n_feat % TI != 0 : pr[i].n_feat != TI) return false;   // per-head statistics: head_dim 128 only
    if (pr[i].n_feat * pr[i].batch >= (1 << 21)) return false;
    if (pr[i].ld < pr[i].n_feat * pr[i].batch || pr[i].ld_sigma < pr[i].n_feat) return false;
    if (pr[i].batch > 1 && (pr[i].ld_sigma != TI || pr[i].sigma_batch_stride != (int64_t)TI * TI)) return false;
  }
  return true;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" size_t mdg_cov_accum_i8_multi_ws_bytes(int count, const mdg_cov_problem* problems) {
  if (!problems_ok(count, problems) || problems[0].n_tokens == 0) return 0;
  return layout(count, problems, nullptr, nullptr, nullptr);
}

extern "C" int mdg_cov_accum_i8_multi(int count, const mdg_cov_problem* problems, void* ws, size_t ws_bytes, double tolerance, int flags,
                                      int* used_i8, int* route_counts, void* ev_start, void* ev_stop, void* stream) {
  MDG_CLEAR();
  if (used_i8) *used_i8 = 0;
  MDG_CHECK_ARG(tolerance >= 1.0 && tolerance <= 1e6, "mdg_cov_accum_i8_multi: tolerance factor %g outside [1, 1e6] (1 = guaranteed <= 1.1e-11)",
                tolerance);
  MDG_CHECK_ARG((flags & ~(MDG_I8_NO_EXACT | MDG_I8_EXACT_ALWAYS | MDG_I8_F16 | MDG_I8_RELU | MDG_I8_ROWS)) == 0 &&
                    (flags & (MDG_I8_NO_EXACT | MDG_I8_EXACT_ALWAYS)) != (MDG_I8_NO_EXACT | MDG_I8_EXACT_ALWAYS),
                "mdg_cov_accum_i8_multi: bad flags 0x%x", flags);
  bool offer_exact = !(flags & MDG_I8_NO_EXACT);
  const bool exact_always = (flags & MDG_I8_EXACT_ALWAYS) != 0;
  for (int i = 0; i < count; i++)     // (the event lists address a token's row with a 32-bit byte offset)
    if ((uint64_t)problems[i].n_tokens * (uint64_t)problems[i].ld * 2ull >= (1ull << 32)) offer_exact = false;
  MDG_CHECK_ARG(problems_ok(count, problems),
                "mdg_cov_accum_i8_multi: 1..%d statistics of the same token count; full ones need n_feat %% 128 == 0, per-head ones "
                "head_dim 128 with contiguous [heads][128][128] sigma; leading dimensions at least the widths (use mdg_cov_accum)",
                MAX_PROBLEMS);
  if (problems[0].n_tokens == 0) return MDG_OK;
  for (int i = 0; i < count; i++) MDG_CHECK_ARG(problems[i].x && problems[i].sigma, "mdg_cov_accum_i8_multi: null pointer");
  I8Call c;
  size_t fb_off = 0;
  const size_t need = layout(count, problems, ws, &c, &fb_off);
  MDG_CHECK_ARG(ws && ws_bytes >= need, "mdg_cov_accum_i8_multi: workspace %zu < required %zu", ws_bytes, need);
  c.route_counts = route_counts;
  c.st = (hipStream_t)stream;
  c.f16 = (flags & MDG_I8_F16) != 0;
  c.relu = (flags & MDG_I8_RELU) != 0;
  c.rows = (flags & MDG_I8_ROWS) != 0;
  MDG_HIP(hipMemsetAsync(c.shared, 0, SHARED_BYTES, c.st));
  // (remembered for the read-backs: without the flag the rows' part of the workspace holds nothing of this call; one byte -> the int 1)
  if (c.rows) MDG_HIP(hipMemsetAsync(&c.shared->rows_flag, 1, 1, c.st));
  for (int i = 0; i < count; i++) {
    MDG_TRY(enqueue_split(c, i));
    MDG_TRY(enqueue_route(c, i, tolerance));
  }
  if (offer_exact) MDG_TRY(enqueue_lo_lists(c, exact_always));
  MDG_TRY(enqueue_products(c, offer_exact, ev_start, ev_stop));
  if (offer_exact) MDG_TRY(enqueue_lo_products(c, exact_always));
  for (int i = 0; i < count; i++) MDG_TRY(enqueue_columns(c, i));
  if (c.rows)
    for (int i = 0; i < count; i++) MDG_TRY(enqueue_rows_product(c, i));
  // a statistic the bound cannot certify on six planes even without its ROUTE_JMAX worst columns (its flag's bit 1) -- that
  // statistic, and only that one -- goes through the fp64 kernel
  for (int i = 0; i < count; i++) {
    const mdg_cov_problem& q = problems[i];
    MDG_TRY(cov_accum_gated(q.x, c.f16 ? MDG_F16 : MDG_BF16, c.n_tokens, q.n_feat, q.batch, q.ld, c.relu ? 1 : 0, q.sigma, q.ld_sigma, q.sigma_batch_stride, (char*)ws + fb_off,
                            ws_bytes - fb_off, c.stat[i].route_flag, 2, 2, stream));
  }
  MDG_TRY(report_product_diagnostics(c));
  if (used_i8) {   // measurement / test mode: report the route this call took (costs the host a round trip)
    int pf[MAX_PROBLEMS] = {};
    MDG_HIP(hipMemcpyAsync(pf, c.shared->route_flag, sizeof(pf), hipMemcpyDeviceToHost, c.st));
    MDG_HIP(hipStreamSynchronize(c.st));
    int live = 0, six = 0;
    for (int i = 0; i < count; i++)
      if (!(pf[i] & 2)) {
        live++;
        six |= pf[i] & 1;
      }
    *used_i8 = live ? (six ? 6 : 5) : 0;     // the route of the statistics that stayed on the int8 path; 0: all went to the fp64 kernel
  }
  return MDG_OK;
}

static mdg_cov_problem single_problem(const void* x, int64_t n_tokens, int64_t n_feat, int64_t ld, double* sigma, int64_t ld_sigma) {
  mdg_cov_problem q;
  q.x = x; q.n_tokens = n_tokens; q.n_feat = n_feat; q.batch = 1; q.ld = ld;
  q.sigma = sigma; q.ld_sigma = ld_sigma; q.sigma_batch_stride = 0;
  return q;
}

extern "C" size_t mdg_cov_accum_i8_ws_bytes(int64_t n_tokens, int64_t n_feat) {
  if (n_tokens <= 0 || n_feat <= 0) return 0;
  const mdg_cov_problem q = single_problem(nullptr, n_tokens, n_feat, n_feat, nullptr, n_feat);
  return mdg_cov_accum_i8_multi_ws_bytes(1, &q);
}

extern "C" int mdg_cov_accum_i8(const void* x, int64_t n_tokens, int64_t n_feat, int64_t ld, double* sigma, int64_t ld_sigma,
                                void* ws, size_t ws_bytes, double tolerance, int flags, int* used_i8, int* route_counts, void* ev_start,
                                void* ev_stop, void* stream) {
  MDG_CLEAR();
  if (used_i8) *used_i8 = 0;
  MDG_CHECK_ARG(n_tokens >= 0 && n_feat > 0, "mdg_cov_accum_i8: bad sizes (tokens=%lld feat=%lld)", (long long)n_tokens,
                (long long)n_feat);
  MDG_CHECK_ARG(n_feat % TI == 0, "mdg_cov_accum_i8: n_feat=%lld must be a multiple of %d (use mdg_cov_accum)",
                (long long)n_feat, TI);
  const mdg_cov_problem q = single_problem(x, n_tokens, n_feat, ld, sigma, ld_sigma);
  return mdg_cov_accum_i8_multi(1, &q, ws, ws_bytes, tolerance, flags, used_i8, route_counts, ev_start, ev_stop, stream);
}

extern "C" int mdg_cov_accum_i8_route(int count, const mdg_cov_problem* problems, int stat, const void* ws, int* planes, int* n_columns,
                                      int* columns, double* bound, int* exact, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(problems_ok(count, problems) && stat >= 0 && stat < count && ws, "mdg_cov_accum_i8_route: bad arguments");
  I8Call c;
  layout(count, problems, const_cast<void*>(ws), &c, nullptr);
  RouteOut r;
  SharedBlock shared;
  hipStream_t st = (hipStream_t)stream;
  MDG_HIP(hipMemcpyAsync(&r, c.stat[stat].route, sizeof(r), hipMemcpyDeviceToHost, st));
  MDG_HIP(hipMemcpyAsync(&shared, c.shared, sizeof(shared), hipMemcpyDeviceToHost, st));
  MDG_HIP(hipStreamSynchronize(st));
  const bool was_exact = r.planes != 0 && shared.exact_ran == 1 && shared.exact_overflow == 0;
  int rows_left = 0;
  if (shared.rows_flag && r.planes != 0) {
    RowsOut ro;
    MDG_HIP(hipMemcpyAsync(&ro, c.stat[stat].rows_out, sizeof(ro), hipMemcpyDeviceToHost, st));
    MDG_HIP(hipStreamSynchronize(st));
    rows_left = ro.n_rows;
  }
  if (exact) *exact = was_exact ? shared.exact_mode : 0;      // 1: the remainder ran on the tile kernel (sparse lists), 2: on the wide kernels
  if (planes) *planes = r.planes;
  if (n_columns) *n_columns = r.n_out;
  if (columns)
    for (int i = 0; i < MDG_I8_MAX_COLUMNS; i++) columns[i] = i < r.n_out ? r.out[i] : -1;
  if (bound) {   // the exact route drops no plane pair: the rounded-element term and fp64 rounding are what is left
    bound[0] = was_exact ? r.rho + MDG_I8_EXACT_ROUNDING : r.sq;
    bound[1] = was_exact ? 0.0 : r.x;
    if (rows_left) bound[0] += (double)(rows_left + 1) * 0x1p-53;     // the fp64 row update's rounding (cov_i8_rows.hip)
  }
  return MDG_OK;
}

// the rows statistic `stat` handed to the fp64 row kernel in the last call on `ws`; none when that call did not set MDG_I8_ROWS
// (the shared block remembers) or sent the statistic to the fp64 kernel as a whole
static int read_rows(const I8Call& c, int stat, RowsOut* out, hipStream_t st) {
  SharedBlock shared;
  MDG_HIP(hipMemcpyAsync(&shared, c.shared, sizeof(shared), hipMemcpyDeviceToHost, st));
  MDG_HIP(hipStreamSynchronize(st));
  out->n_rows = out->n_dominant = 0;
  if (!shared.rows_flag || (shared.route_flag[stat] & 2)) return MDG_OK;
  MDG_HIP(hipMemcpyAsync(out, c.stat[stat].rows_out, sizeof(*out), hipMemcpyDeviceToHost, st));
  MDG_HIP(hipStreamSynchronize(st));
  return MDG_OK;
}

extern "C" int mdg_cov_accum_i8_rows(int count, const mdg_cov_problem* problems, int stat, const void* ws, int* n_rows, int* rows,
                                     void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(problems_ok(count, problems) && stat >= 0 && stat < count && ws, "mdg_cov_accum_i8_rows: bad arguments");
  I8Call c;
  layout(count, problems, const_cast<void*>(ws), &c, nullptr);
  RowsOut r;
  MDG_TRY(read_rows(c, stat, &r, (hipStream_t)stream));
  if (n_rows) *n_rows = r.n_rows;
  if (rows)
    for (int i = 0; i < MDG_I8_MAX_ROWS; i++) rows[i] = i < r.n_rows ? r.rows[i] : -1;
  return MDG_OK;
}

extern "C" int mdg_cov_accum_i8_stats(const void* ws, int64_t n_tokens, int64_t n_feat, unsigned long long* executed_mfma,
                                      void* stream) {
  MDG_CLEAR();
  (void)n_tokens;
  (void)n_feat;
  MDG_CHECK_ARG(ws && executed_mfma, "mdg_cov_accum_i8_stats: bad arguments");
  const SharedBlock* shared = (const SharedBlock*)ws;   // at the start of every int8 workspace
  hipStream_t st = (hipStream_t)stream;
  MDG_HIP(hipMemcpyAsync(executed_mfma, &shared->mfma_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  MDG_HIP(hipStreamSynchronize(st));
  return MDG_OK;
}
