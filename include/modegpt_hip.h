/* modegpt_hip.h -- C ABI of libmodegpt_hip.so, the MI355X (gfx950) engine for MoDeGPT's per-layer
 * compression path: activation-covariance accumulation, Nystrom / CR / SVD factorisation of the MLP and
 * attention weights, and the compressed-weight build.
 *
 * The reference (cbacary/MoDeGPT) has no FFI: its seam is Python.  This ABI sits directly
 * beneath the reference's five hot-path functions; each entry point below names the reference lines it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the ctypes stubs a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the library borrows it for the call
 *     and owns no memory across calls (workspaces are passed in; query their size with the *_ws_bytes twin)
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work unless documented as
 *     synchronising
 *   - return value: MDG_OK or a negative MDG_ERR_* code; mdg_last_error() gives the message (thread-local)
 *   - re-entrant per device, no global lock, callable from any host thread
 */
#ifndef MODEGPT_HIP_H
#define MODEGPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDG_ABI_VERSION 10 /* 2: w_dtype on mdg_nystrom_down / mdg_vo_compress, mdg_rope_gather added; 3: mdg_cov_accum_i8_stats added;
                             4: mdg_cov_accum_i8 chooses its route on the device (route_counts argument, no host synchronisation);
                                mdg_comm_* / mdg_allgather_layers added;
                             5: mdg_potrs_lower takes a workspace (mdg_potrs_lower_ws_bytes);
                             6: mdg_cov_accum_i8_multi added (several statistics in one int8 launch); the int8 workspace layout changed;
                             7: the int8 route is derived from a per-call error bound, single columns can leave the int8 path for an fp64
                                column kernel (route_counts has 4 entries, mdg_cov_accum_i8_route added, workspace layout changed);
                                mdg_shutdown and mdg_deferred_status_* added;
                             8: mdg_cov_i8_set_tolerance / mdg_cov_i8_tolerance, mdg_nystrom_down_overlapped added;
                             9: the int8 route's tolerance factor is an ARGUMENT of mdg_cov_accum_i8 / mdg_cov_accum_i8_multi (the
                                process-wide setter / getter of ABI 8 are gone: no accuracy state in the library);
                                mdg_ridge_scores takes `sens`, mdg_select_margin added (certificate of the MLP rank selection);
                                the exact route of the int8 covariance (`flags`, route_counts[4], mdg_cov_accum_i8_route's `exact`);
                                added under 9: mdg_qk_select_margin, mdg_vo_spectrum; MDG_I8_ROWS / MDG_I8_MAX_ROWS (a flag bit of the int8
                                covariance, route_counts[5] with that bit), mdg_cov_accum_i8_rows;
                                added under 9: mdg_nystrom_rank_curve_ws_bytes, mdg_nystrom_rank_curve (the Nystrom refit's error at every rank);
                                added under 9: mdg_mlp_output_error_ws_bytes, mdg_mlp_output_error (the stored down projection's realised output error);
                                added under 9: mdg_vo_output_error_ws_bytes, mdg_vo_output_error, mdg_vo_rank_curve_ws_bytes, mdg_vo_rank_curve
                                (what the stored V/O factors lose of the attention output, and the truncation's cost at every rank);
                                changed under 9: mdg_nystrom_down_ws_bytes is larger (the compacted operands of the product over the
                                unselected columns, see mdg_nystrom_down); no signature changed;
                             10: mdg_rope_gather_plan added (the rotary kernel's dispatch as a device-free function);
                                added under 10: mdg_qk_rank_curve (what the Q/K pair selection costs the attention logits, per head and rank);
                                added under 10: mdg_vo_bias (the v_proj / o_proj biases through the V/O truncation);
                                added under 10: mdg_col_sum_ws_bytes, mdg_col_sum_accum, mdg_cov_center, mdg_nystrom_intercept_ws_bytes,
                                mdg_nystrom_intercept (first moments of the MLP statistic, the centred refit and its intercept);
                                added under 10: mdg_vo_intercept_ws_bytes, mdg_vo_intercept (the intercept of the mean-aware V/O truncation);
                                added under 10: mdg_rope_rows (the rotary embedding of a projection output in its own layout: post-RoPE statistics);
                                added under 10: mdg_qk_pair_ws_bytes, mdg_qk_pair_accum (the within-sequence, shift-invariant Q/K statistic);
                                added under 10: mdg_nystrom_greedy_ws_bytes, mdg_nystrom_greedy_select (MLP columns by block-greedy descent on the refit's objective);
                                added under 10: mdg_qk_causal_ws_bytes, mdg_qk_causal_accum (the causal Q/K statistic);
                                added under 10: mdg_attn_fwd (fused causal attention forward for compressed heads of unequal q/k and v width);
                                added under 10: mdg_attn_decode_ws_bytes, mdg_attn_decode_splits, mdg_attn_decode (the same product on a split-key decode schedule);
                                added under 10: mdg_attn_mask_summary_bytes, mdg_attn_mask_summary, mdg_attn_fwd_masked, mdg_attn_decode_masked (both products under a bool mask) */

enum mdg_status {
  MDG_OK = 0,
  MDG_ERR_BAD_ARG = -1,     /* shape / pointer / alignment / workspace-size problem */
  MDG_ERR_HIP = -2,         /* a HIP runtime call failed */
  MDG_ERR_NOT_PD = -3,      /* Cholesky met a non-positive pivot (torch.linalg.cholesky would raise) */
  MDG_ERR_NO_CONVERGE = -4, /* Jacobi eigensolver hit its sweep limit, or was given a NaN / Inf (the message says which) */
  MDG_ERR_NO_DEVICE = -5    /* no gfx950 device visible */
};

enum mdg_dtype { MDG_BF16 = 0, MDG_F16 = 1, MDG_F32 = 2, MDG_F64 = 3 };

/* QK scoring variants (compress_qk.py:244-285) */
enum mdg_qk_mode {
  MDG_QK_ROPE_GROUPED = 0, /* compress_head_llama_grouped, compress_qk.py:320-382 */
  MDG_QK_ROPE_MHA = 1,     /* compress_head_llama,         compress_qk.py:387-436 */
  MDG_QK_OPT = 2           /* compress_head_opt,           compress_qk.py:439-476 */
};

int mdg_abi_version(void);
const char* mdg_last_error(void);
/* Fills name (<= cap bytes) with the gcnArchName of `device`; MDG_ERR_NO_DEVICE if HIP sees no GPU. */
int mdg_device_info(int device, char* name, int cap, int* n_cu, int64_t* hbm_bytes);
/* Deferred status.  The decomposition entry points below that say "SYNCHRONISES" do so for one reason: a 4-byte device status
 * word (the Cholesky's not-positive-definite pivot, the Jacobi solver's convergence flag) has to reach the host before they can
 * return MDG_ERR_NOT_PD / MDG_ERR_NO_CONVERGE.  Between mdg_deferred_status_begin and mdg_deferred_status_end, on the calling
 * thread, they merge that word into `status_dev` (DEVICE int[2], zeroed by _begin on `stream`: {kind of the FIRST failure, its
 * detail}) with a one-thread kernel and return MDG_OK at once -- a whole layer's chain (ridge scores, Nystrom refit, QK selection,
 * VO factors) then enqueues without a host round trip, and the caller reads the two ints whenever it next has to wait for the
 * stream anyway.  mdg_deferred_status_decode turns the two ints (copied to the host by the caller) into the status code and
 * mdg_last_error() text the synchronising call would have produced: MDG_ERR_NOT_PD -> torch.linalg.LinAlgError upstream
 * (torch.linalg.cholesky, compress_mlp.py:20,56), MDG_ERR_NO_CONVERGE -> RuntimeError.  After a failure the remaining kernels of
 * the chain still run (on garbage, within their buffers); their outputs must be discarded. */
int mdg_deferred_status_begin(int* status_dev, void* stream);
int mdg_deferred_status_end(void);
int mdg_deferred_status_decode(const int* status_host);
/* Releases what the library keeps across calls: the device copies of the int8 product's tile schedules (a few KB per shape,
 * built at first use).  The library owns no HIP streams or events -- those are the caller's -- and makes no HIP call from a static
 * destructor; call this before the process tears the HIP runtime down (modegpt_amd/_lib.py registers it with atexit), with no
 * library call in flight.  Safe to call repeatedly; the next covariance call rebuilds what it needs. */
int mdg_shutdown(void);

/* ------------------------------------------------------------------ covariance (calibration hooks)
 * sigma[b] (lower triangle incl. diagonal tiles) += X_b^T X_b, products and sums in fp64 of the exactly
 * converted inputs.  X is [n_tokens, >= batch*n_feat] row-major (ld elements per token); problem b reads
 * columns [b*n_feat, (b+1)*n_feat).  batch=1: replaces `H.T @ H` (LlamaAdapter.py:127-136, model_adapter.py:546-554)
 * and `sum(X.mT @ X, 0)` (LlamaAdapter.py:138-147); batch=n_heads, n_feat=head_dim: replaces the permute + bmm of
 * LlamaAdapter.py:115-125 / model_adapter.py:556-567 without the permute copy.
 * Only the lower triangle of sigma is valid until mdg_cov_finalize mirrors it.  Above the diagonal, the 128 x 128 tiles on the
 * diagonal are accumulated whole (an entry above the diagonal inside one receives the same sum as its mirror image, added to
 * whatever it held), the tiles strictly above the diagonal are neither read nor written; the lower triangle depends on neither.
 * relu != 0 applies max(x, 0) on load (OPT fc1 hook) as v > 0 ? v : 0: -0.0, -Inf and NaN all count as +0.  Without it a
 * non-finite element reaches row and column j of sigma only (NaN, or +-Inf / NaN as the fp64 sum of products gives), nothing else.
 * n_tokens == 0 returns MDG_OK without touching sigma (x may be NULL).  ws may be NULL when mdg_cov_accum_ws_bytes says 0;
 * it holds split-K partials (reduced in fixed order -> run-to-run deterministic). */
size_t mdg_cov_accum_ws_bytes(int64_t n_tokens, int64_t n_feat, int64_t batch);
int mdg_cov_accum(const void* x, int dtype, int64_t n_tokens, int64_t n_feat, int64_t batch, int64_t ld,
                  int relu, double* sigma, int64_t ld_sigma, int64_t sigma_batch_stride, void* ws,
                  size_t ws_bytes, void* stream);
/* The same accumulate for up to 4 problems of one calibration batch in ONE launch (the four hooks of a layer:
 * sigma_mlp, sigma_x, sigma_q, sigma_k): the small problems' workgroups fill the slots the large one's last,
 * under-filled round leaves idle.  Put the largest problem first.  Every problem must have n_feat % 128 == 0 and
 * 16-byte aligned rows (otherwise call mdg_cov_accum per problem); no ReLU.  `problems` is a HOST array.  The problems may
 * differ in n_tokens (each is split over its own tokens; the same-token rule below is mdg_cov_accum_i8_multi's), every n_tokens
 * must be > 0, and ld_sigma / sigma_batch_stride may be padded as in mdg_cov_accum. */
typedef struct {
  const void* x;   /* [n_tokens, >= batch*n_feat], ld elements per token */
  int64_t n_tokens, n_feat, batch, ld;
  double* sigma;   /* [batch][n_feat][ld_sigma] */
  int64_t ld_sigma, sigma_batch_stride;
} mdg_cov_problem;
size_t mdg_cov_accum_multi_ws_bytes(int n, const mdg_cov_problem* problems, int dtype);
int mdg_cov_accum_multi(int n, const mdg_cov_problem* problems, int dtype, void* ws, size_t ws_bytes, void* stream);
/* The same accumulation for ONE bf16 (or, with MDG_I8_F16, fp16) matrix through the int8 matrix cores (csrc/cov_i8*.hip; the map of the units is at the head of cov_i8.hip): an ERROR-FREE SPLIT of every bf16 value
 * into six balanced base-256 digits against a per-column power-of-two scale, and a TRUNCATED PRODUCT -- the digit-plane products with
 * s + t < P are formed by v_mfma_i32_32x32x32_i8 with exact int32 accumulation and folded into sigma in fp64 every 65504 tokens (2047 k-steps of 32: the
 * exact int32 bound -- a class sum grows by at most 32768 per token for bf16 AND for fp16 elements, enumerated in
 * scripts/probes/i8_int32_bound.py and i8_int32_bound_f16.py); the pairs with s + t >= P are dropped.  What the dropped pairs can amount to is bounded per call from integer
 * plane energies the split pass accumulates (Cauchy-Schwarz over the tokens; derivation in csrc/cov_i8_route.hip at i8_route_kernel and
 * DESIGN.md section 7, host model tests/i8_model.py):
 *     |sigma_ij - exact| <= (SQ_P + X_P) sqrt(sigma_ii sigma_jj)   entry-wise, for any input,
 * and the route is the smallest P in {5, 6} with SQ_P <= 1e-12 (the part of the bound that is attained) and X_P <= 1e-11 (cross
 * terms; 20-50x above what uncorrelated columns produce).  GUARANTEED for any input: <= 1.1e-11 (times `tolerance`).  TYPICAL:
 * 1e-13 (an empirical figure, not a promise: <= 1e-12 on every distribution family of scripts/probes/i8_fuzz.py and at the
 * product's widths; data whose columns have proportional digit sequences can come arbitrarily close to the bound).  Columns that alone break the bound -- a bulk 10-15 binades under a
 * few massive activations, columns holding an Inf / NaN -- leave the int8 path one by one (at most MDG_I8_MAX_COLUMNS per statistic
 * and call): the fold skips their rows and columns of sigma and an fp64 column kernel (plain fp64 sums of products, the reference's
 * arithmetic, LlamaAdapter.py:127-147) computes them.  Only when that is not enough does the whole statistic run through
 * mdg_cov_accum.
 * The route is chosen ON THE DEVICE: the call enqueues the five-plane product, the six-plane product, the column kernel and the fp64
 * kernel back to back, and the launches the route does not select exit at once -- the call only enqueues and never waits for the host
 * (it can be captured in a hipGraph) when used_i8 is NULL.  Every decision is a function of integer sums: run-to-run bit-identical.
 * route_counts (DEVICE pointer to 5 ints -- 6 with MDG_I8_ROWS, see there --, optional): [0] += 1 when five planes ran, [1] six planes, [2] the fp64 kernel for the whole
 *   statistic, [3] += the number of columns handed to the fp64 column kernel, [4] += 1 when the exact route ran (see below; such a
 *   call is also booked under [0] or [1], the class the route kernel gave it); the caller keeps it across calls and reads it
 *   whenever it likes (calibration reads it once, at the end).
 * used_i8 (HOST pointer, optional; measurement and tests): receives the route of THIS call -- 5, 6, or 0 for the fp64 kernel --
 *   at the price of one stream synchronisation.
 * tolerance: the accuracy / speed dial of THIS call, one factor f in [1, 1e6] on both thresholds of the route (SQ_P <= f 1e-12,
 *   X_P <= f tau_x).  f = 1 is the guarantee stated above.  A caller who accepts f times that bound gets five planes where the default
 *   takes six -- SiLU-gated MLP activations have X_5 = 3.7e-10, so f >= 37 moves them to five planes: measured 3.8e-12 instead of
 *   8e-14, the sigma_mlp launch 29 instead of 37 ms -- and fewer columns on the fp64 column kernel.  The call still computes and
 *   reports its own bound (mdg_cov_accum_i8_route), so what was guaranteed for a given input is known, whatever f.  An argument,
 *   not process state: concurrent callers with different factors do not see each other.  Not in the reference (plain fp64 there).
 * n_feat must be a multiple of 128, n_tokens < 2^28.  ws: mdg_cov_accum_i8_ws_bytes (about 10 bytes per element of x: six digit planes, the
 * exact route's event lists and its copy of x in x's own element type).
 * ev_start / ev_stop: optional hipEvent_t recorded on `stream` right before / after the three int8 product launches and their tail
 * combines -- the split, the route and the exact route's list building come before ev_start, the remainder, column and fallback
 * kernels after ev_stop (bench.py times the dominant kernels alone with them); NULL otherwise. */
/* THE EXACT ROUTE (since ABI 9.  flags = 0: taken where it is the faster product -- launches the route kernel classes as six planes,
 * i.e. SiLU- / GELU-gated MLP activations, and five-plane launches whose first statistic has >= 4096 features; MDG_I8_EXACT_ALWAYS:
 * wherever the remainder lists fit; MDG_I8_NO_EXACT: never).  Planes 3 .. 5 are reached only by elements 17
 * binades and more below their column's maximum -- 3e-5 of the elements of a Gaussian column, 0.5 % of a SiLU-gated one -- so the
 * call lists those elements (token, column, low 24 bits) and, when every list fits (at most 6.2 % of any column x 2048 tokens),
 * replaces the truncated product by an exact one:  X^T X = X_d^T X_d + X_lo^T X + X_d^T X_lo  with X_d the top three digit planes --
 * all NINE of their plane pairs on the int8 matrix cores (a product launch of its own: three planes, no piece masks) -- and the two
 * remainder products as fp64 sums over the listed elements (i8_lo_product_kernel for sparse lists, i8_lo_wide_kernel for dense
 * ones; the device picks).  No plane pair is dropped: the error is fp64
 * rounding (<= MDG_I8_EXACT_ROUNDING of sqrt(sigma_ii sigma_jj)) plus the bound's rho term for elements more than 38 binades under
 * their column maximum, whatever `tolerance` says; 9 executed plane pairs instead of 9.4 (Gaussian) / 15.1 (SiLU-gated).  The route
 * kernel's decisions are unchanged -- which columns leave for the fp64 column kernel, whether the whole statistic goes to
 * mdg_cov_accum, five or six planes when a list does not fit -- and so is everything the call reports, plus: route_counts[4] += the
 * statistics that took the exact route (they are also booked under the five- / six-plane class the route kernel gave them), and
 * mdg_cov_accum_i8_route's `exact`. */
#define MDG_I8_MAX_COLUMNS 32
#define MDG_I8_NO_EXACT 1             /* flags: never the exact route (the truncated five- / six-plane product with its bound) */
#define MDG_I8_EXACT_ALWAYS 2         /* flags: the exact route wherever the remainder lists fit, also for launches of the five-plane class */
/* ELEMENT TYPE AND ReLU (flag bits of the same `flags` argument; each works alone, both together, and beside either bit above):
 * MDG_I8_F16: x holds IEEE fp16 instead of bf16, for EVERY statistic of the call.  An fp16 value is a signed 11-bit significand
 *   with an effective exponent in 1 .. 30; with the column maximum's significand below bit 46 every finite element of the column
 *   is an exact 48-bit integer, subnormals included -- nothing is rounded, the rho term is identically 0, and a call on the exact
 *   route reports exactly MDG_I8_EXACT_ROUNDING.  Elements reach below the top three planes from 12 binades under their column
 *   maximum (bf16: 15), so the exact route's lists are longer than for bf16 data of the same distribution; the device's choice
 *   between the exact route and the truncated product is the same code.  Exponent field 31 (Inf / NaN) sends the column to the
 *   fp64 column kernel as bf16's 255 does.  Workspace sizes are unchanged (2-byte elements; the x_d copy is an fp16 copy).
 * MDG_I8_RELU: max(x, 0) is applied wherever x is read, as `relu != 0` of mdg_cov_accum (OPT's fc1 statistic): anything with the
 *   sign bit set counts as +0, -0 and -Inf included; a NaN stays a NaN whatever its sign bit (its column leaves for the fp64
 *   column kernel and poisons its row and column of sigma as in torch.relu(x) followed by the fp64 product).  ONE
 *   DIFFERENCE: a statistic the bound cannot certify goes through mdg_cov_accum as a whole, whose ReLU (v > 0 ? v : 0) turns a NaN
 *   into 0 -- on that fallback route, and there only, a NaN column contributes zeros instead of NaNs. */
#define MDG_I8_F16 4                  /* flags: x is fp16 */
#define MDG_I8_RELU 8                 /* flags: max(x, 0) on load */
/* OUTLIER TOKEN ROWS (added under ABI 9; a flag bit of the same `flags` argument, combines with every bit above, applies to EVERY
 * statistic of the call; off by default, and without it every launch, every bit of sigma and every reported value is what it was).
 * MDG_I8_ROWS: up to MDG_I8_MAX_ROWS token rows per statistic leave the int8 path.  Why: the split measures every element against its
 *   COLUMN's maximum exponent, so a handful of tokens that are large across many columns raise every maximum at once, push the bulk of
 *   every column deeper under it, overflow the exact route's event lists and break the truncated product's bound in more columns than
 *   the fp64 column kernel takes -- the whole statistic then drops to mdg_cov_accum (about five times the time at the sigma_mlp shape).
 *   X^T X = sum_t x_t x_t^T is additive over tokens: X^T X = X_rest^T X_rest + X_R^T X_R for any row set R, without cross terms.  The
 *   int8 path (column maxima, split, route statistics, event lists, fp64 column kernel) reads the rows of R as +0, and an fp64 row
 *   kernel (v_mfma_f64_16x16x4_f64, one workgroup per 128 x 128 tile of the lower triangle, rows in ascending token order, no atomics)
 *   adds X_R^T X_R for all columns in the reference's arithmetic (LlamaAdapter.py:127-147).
 *   THE RULE, decided on the device from the exponent fields of x alone -- integers, no floating-point sum, no host round trip,
 *   bit-identical from run to run, the call still only enqueues (csrc/cov_i8_rows.hip; host model tests/i8_rows_model.py):
 *     1. E_j = the column maxima over all rows.  2. v_t = the number of columns j where x_tj != 0 and ee(x_tj) >= E_j - 4 (ee: the
 *     element's effective exponent; ReLU on load honoured).  3. row t is DOMINANT when v_t >= n / 8.  4. if 1 .. MDG_I8_MAX_ROWS rows
 *     are dominant and they are at most an eighth of the call's tokens, they leave (ascending token order; a row bitmask in the
 *     workspace).  5. otherwise nothing leaves and the call proceeds exactly as without the flag (on ordinary data most rows are
 *     dominant: far more than 64).  6. the column maxima are then recomputed over the rows that stayed.
 *   ONE ROUND: two tiers of outliers (rows x 2^16 and rows x 2^8 together) and a continuum of token scales (lognormal per-token
 *   scales, scripts/probes/i8_fuzz.py kind 7) are out of scope -- those statistics take the route they took without the flag.
 *   A statistic that goes to mdg_cov_accum as a whole even so is computed there from every row of x; the row kernel does not run for it.
 *   route_counts: with this bit set the array has 6 ints, [5] += the rows handed to the fp64 row kernel (callers that never set the bit
 *   keep passing 5).  mdg_cov_accum_i8_rows reads the rows of the last call back.
 *   BOUND: on a call where rows left mdg_cov_accum_i8_route's bound[0] additionally carries the rounding of the row update.  The product
 *   of two bf16 or two fp16 values is exact in fp64 (16 / 22 significand bits), so the update of entry (i, j) is a sum of |R| exact
 *   terms x_ti x_tj: each of the |R| additions (the last one into sigma) rounds once, by at most 2^-53 of a partial sum, and every
 *   partial sum obeys |sum_{t in S} x_ti x_tj| <= sqrt(sum_S x_ti^2 sum_S x_tj^2) <= sqrt(sigma_ii sigma_jj) (Cauchy-Schwarz; sigma of
 *   this call's tokens): at most |R| 2^-53 sqrt(sigma_ii sigma_jj), reported as (|R| + 1) 2^-53 -- one more for the sum of the two
 *   parts.  The bound of the int8 part holds relative to sigma of the rows that stayed, which is no larger than that of all rows. */
#define MDG_I8_ROWS 16                /* flags: outlier token rows may leave the int8 path for the fp64 row kernel */
#define MDG_I8_MAX_ROWS 64            /* rows per statistic and call the fp64 row kernel takes */
#define MDG_I8_EXACT_ROUNDING 5e-15   /* what mdg_cov_accum_i8_route reports beside the rho term for a call on the exact route */
size_t mdg_cov_accum_i8_ws_bytes(int64_t n_tokens, int64_t n_feat);
int mdg_cov_accum_i8(const void* x, int64_t n_tokens, int64_t n_feat, int64_t ld, double* sigma, int64_t ld_sigma, void* ws,
                     size_t ws_bytes, double tolerance, int flags, int* used_i8, int* route_counts, void* ev_start, void* ev_stop,
                     void* stream);
/* v_mfma instructions the product kernel of the LAST mdg_cov_accum_i8 call on workspace `ws` executed (0 after a call that
 * fell back to mdg_cov_accum).  The split pass records, per k-step and 32-row group, which digit planes hold a nonzero
 * there; the product kernel neither loads nor multiplies planes that are all-zero over a tile panel, so the count is at
 * most -- and on real activations well below -- the dense (tiles) x (k-steps) x (waves) x (MFMAs per step).  Copies 8 bytes
 * device -> host on `stream` and synchronises it.  bench.py prices the kernel with this count. */
int mdg_cov_accum_i8_stats(const void* ws, int64_t n_tokens, int64_t n_feat, unsigned long long* executed_mfma, void* stream);
/* The route the LAST mdg_cov_accum_i8 / mdg_cov_accum_i8_multi call on workspace `ws` took for statistic `stat` of `problems` (the
 * array that call was given): *planes = 5, 6, or 0 (whole statistic through mdg_cov_accum); *n_columns and columns[MDG_I8_MAX_COLUMNS]
 * (-1 padded) = the columns the fp64 column kernel computed, in the order the route took them; bound[0] = SQ_P, bound[1] = X_P of
 * the columns that stayed (their sum bounds the entry-wise error relative to sqrt(sigma_ii sigma_jj) of this call's tokens); *exact != 0
 * when the call ran the exact route -- 1: its remainder products on the tile kernel (sparse event lists), 2: on the wide kernels --
 * and then bound[0] = the rho term + MDG_I8_EXACT_ROUNDING, bound[1] = 0.  Any output pointer may be NULL.  Copies device -> host on `stream` and synchronises it: tests and measurements only. */
int mdg_cov_accum_i8_route(int count, const mdg_cov_problem* problems, int stat, const void* ws, int* planes, int* n_columns,
                           int* columns, double* bound, int* exact, void* stream);
/* The token rows statistic `stat` of the LAST call on workspace `ws` handed to the fp64 row kernel (MDG_I8_ROWS): *n_rows and
 * rows[MDG_I8_MAX_ROWS], ascending, -1 padded.  0 rows when that call did not set the flag, when nothing left, or when the statistic
 * went through mdg_cov_accum as a whole.  Either output pointer may be NULL.  Copies device -> host on `stream` and synchronises it:
 * tests and measurements only. */
int mdg_cov_accum_i8_rows(int count, const mdg_cov_problem* problems, int stat, const void* ws, int* n_rows, int* rows, void* stream);
/* Up to 4 statistics of ONE calibration batch (the four hooks of a layer) through the int8 digit-plane kernels with ONE
 * persistent product launch: the tiles of all statistics share one static tile schedule, so the small ones fill what the large
 * one's last round leaves idle instead of ending launches of their own, and one route -- the deepest any statistic on the int8 path
 * asks for (more planes never loosen a bound); every statistic has its own bound, its own columns for the fp64 column kernel, and
 * leaves the launch alone for mdg_cov_accum when its bound cannot be met (its tiles are skipped on the device).  `problems` is a HOST
 * array, largest statistic first, all with the same n_tokens, all bf16 (or all fp16 with MDG_I8_F16).  batch == 1: sigma [n_feat][ld_sigma], n_feat a multiple of 128.
 * batch > 1: per-head Grams of an activation [n_tokens][batch * 128] -- n_feat must be 128, sigma contiguous
 * [batch][128][128] (ld_sigma 128, sigma_batch_stride 16384); only the diagonal tiles are computed.  Several statistics need a
 * 256-CU device (the schedule is cut for 8 XCDs x 32 CUs); otherwise call mdg_cov_accum_i8 per statistic.
 * tolerance / flags / used_i8 / route_counts / ev_start / ev_stop as in mdg_cov_accum_i8 (route_counts += the number of statistics per route;
 * used_i8 = 5 or 6, the planes of the statistics that stayed on the int8 path, 0 when all of them went to the fp64 kernel);
 * mdg_cov_accum_i8_stats(ws, 0, 0, ...) reads the executed-MFMA count of the whole launch.  mdg_cov_accum_i8 is this call with
 * one statistic. */
size_t mdg_cov_accum_i8_multi_ws_bytes(int count, const mdg_cov_problem* problems);
int mdg_cov_accum_i8_multi(int count, const mdg_cov_problem* problems, void* ws, size_t ws_bytes, double tolerance, int flags,
                           int* used_i8, int* route_counts, void* ev_start, void* ev_stop, void* stream);
/* sigma[b] <- scale * sigma[b] on the lower triangle, mirrored into the upper.  scale = 1/(n_texts*2048)
 * reproduces calibration.py:141-146. */
int mdg_cov_finalize(double* sigma, int64_t n, int64_t batch, int64_t ld_sigma, int64_t sigma_batch_stride,
                     double scale, void* stream);
/* Packed storage of a finalized statistic -- what load_calibs' calibs_save_path / load_calibs_from (calibration.py:23-24; declared
 * and never read upstream) write and read.  packed holds `batch` matrices of n(n+1)/2 contiguous doubles each, the LOWER triangle
 * in row-major packed order: row i contributes its entries 0..i at offset i(i+1)/2, so a file of it reads with numpy alone
 * (full[np.tril_indices(n)] = np.fromfile(path, "<f8")).  full: `batch` matrices [n][ld], ld >= n, batch_stride elements apart.
 * mdg_sym_pack_lower reads nothing above the diagonal (a buffer mdg_cov_finalize has not mirrored yet packs the same).
 * mdg_sym_unpack_lower writes both triangles in one pass and leaves elements [n, ld) of every row, and whatever lies between two
 * matrices, untouched.  Both move raw 64-bit patterns: NaN payloads, +-Inf, -0.0 and subnormals survive bit for bit.  All offsets
 * are 64-bit (a packed matrix passes 4 GiB at n = 23 170).  full and packed must not overlap. */
int mdg_sym_pack_lower(const double* full, int64_t n, int64_t batch, int64_t ld, int64_t batch_stride, double* packed, void* stream);
int mdg_sym_unpack_lower(const double* packed, int64_t n, int64_t batch, double* full, int64_t ld, int64_t batch_stride, void* stream);
/* Block-Influence partial: *out += sum over tokens of (1 - cos(x_in[t], x_out[t])) in fp64
 * (calibration.py:118-124; the caller divides by T and n_texts).  ws: mdg_bi_ws_bytes(n_tokens). */
size_t mdg_bi_ws_bytes(int64_t n_tokens);
int mdg_bi_accum(const void* x_in, const void* x_out, int dtype, int64_t n_tokens, int64_t d, int64_t ld,
                 double* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ dense fp64 building blocks
 * C = alpha * op(A) * op(B) + beta * C on v_mfma_f64_16x16x4_f64.  Element (i,k) of op(A) is
 * A[i*sa_i + k*sa_k] (or A[a_rows[i]*sa_i + k*sa_k] when a_rows != NULL), element (k,j) of op(B) is
 * B[k*sb_k + j*sb_j]; C is row-major [M, N] with ldc, dtype f64 or bf16 (bf16: beta must be 0, rounding as
 * torch's .to(bfloat16)).  flags: MDG_GEMM_*.  Batched with element strides. */
/* The triangle flags clip the k-range per 128 x 128 tile of C: the entries of the zero triangle that lie inside the tile's diagonal
 * 128 x 128 block ARE read and must hold zeros; the entries beyond that block are never read (they may hold anything, NaN too).
 * a_rows may be unsorted and may repeat rows.  beta == 0 never reads C. */
#define MDG_GEMM_LOWER_ONLY 1   /* M==N: only tiles with row-block >= col-block are computed (SYRK update); a diagonal tile is
                                   written WHOLE (its part above the diagonal too), tiles above the diagonal are not touched */
#define MDG_GEMM_A_LOWER_TRI 2  /* op(A)[i,k] = 0 for k > i: k < i0 + 128 for the rows i0 .. i0+127 of a tile (k >= i0 + 128 not read) */
#define MDG_GEMM_B_LOWER_TRI 4  /* op(B)[k,j] = 0 for k < j: k >= j0 for the columns j0 .. j0+127 of a tile (k < j0 not read) */
#define MDG_GEMM_A_UPPER_TRI 8  /* op(A)[i,k] = 0 for k < i: k >= i0 for the rows i0 .. i0+127 of a tile (k < i0 not read) */
int mdg_gemm_f64(int64_t M, int64_t N, int64_t K, double alpha, const void* A, int a_dtype, int64_t sa_i,
                 int64_t sa_k, const int64_t* a_rows, const void* B, int b_dtype, int64_t sb_k,
                 int64_t sb_j, double beta, void* C, int c_dtype, int64_t ldc, int64_t batch,
                 int64_t a_batch_stride, int64_t b_batch_stride, int64_t c_batch_stride, int flags,
                 void* stream);

/* In-place lower Cholesky A = L L^T, blocked right-looking with 128-wide panels; inv_diag receives the inverses of
 * the 128x128 diagonal blocks of L ([ceil(n/128)][128][128], identity-padded).  Strictly above the diagonal: entries
 * outside the 128x128 diagonal blocks are neither read nor written (they may hold anything, NaN too); entries inside
 * the diagonal blocks are not read for the result either, but MAY BE OVERWRITTEN with unspecified values (the rank-128
 * and outer updates store a diagonal tile whole) -- factorise a copy if the upper
 * triangle matters, as mdg_ridge_scores and mdg_nystrom_down do in their workspace.  Nothing beyond column n of a row
 * (lda > n) or beyond row n is touched.  SYNCHRONISES the stream once at the end to read the pivot flag (the first
 * leading minor that is not positive definite; a zero or NaN pivot counts).
 * Replaces torch.linalg.cholesky at compress_mlp.py:20,56. */
size_t mdg_potrf_inv_diag_elems(int64_t n);
int mdg_potrf_lower(double* A, int64_t n, int64_t lda, double* inv_diag, void* stream);
/* X (n x nrhs, ldx, in place) <- (L L^T)^-1 X by blocks of 2048 rows: the diagonal blocks of L are inverted explicitly
 * (recursive doubling from inv_diag), a block's substitution is one triangular-aware GEMM with that inverse, one rank-2048
 * GEMM carries its solution on.  ws: mdg_potrs_lower_ws_bytes(n, nrhs) (the block inverses, the doubling's scratch and a second
 * right-hand-side buffer: potrs_layout in csrc/chol.hip).
 * Replaces torch.cholesky_solve at compress_mlp.py:57. */
size_t mdg_potrs_lower_ws_bytes(int64_t n, int64_t nrhs);
int mdg_potrs_lower(const double* L, int64_t n, int64_t ldl, const double* inv_diag, double* X, int64_t nrhs,
                    int64_t ldx, void* ws, size_t ws_bytes, void* stream);
/* out[j] = ((L L^T)^-1)_jj = || L^-1 e_j ||^2.  ws: mdg_chol_inverse_diag_ws_bytes(n) (inv_diag_layout in csrc/chol.hip).
 * Replaces torch.cholesky_inverse + torch.diag at compress_mlp.py:21-23. */
size_t mdg_chol_inverse_diag_ws_bytes(int64_t n);
int mdg_chol_inverse_diag(const double* L, int64_t n, int64_t ldl, const double* inv_diag, double* out,
                          void* ws, size_t ws_bytes, void* stream);

/* Batched symmetric eigensolver, n <= 128 and even: cyclic Jacobi in LDS, one workgroup per matrix.
 * A [batch][n][n] (symmetric, destroyed), evals [batch][n] DESCENDING, evecs [batch][n][n] with eigenvector j
 * in COLUMN j.  SYNCHRONISES to read the convergence flag.  (The reference reaches torch.linalg.eigh / svd
 * through sqrt_M, compression_utils.py:21, and compress_vo.py:130,187,194.)
 * Only the lower triangle of a matrix is read; what stands above the diagonal, NaN included, has no effect.
 * Order: descending, ties by index (-0.0 == 0.0 is a tie), a NaN eigenvalue before everything else -- a total order for every bit
 * pattern, so every element of evals and evecs is written whatever the input.
 * Non-finite input: a matrix with a NaN or Inf in its lower triangle is not iterated.  Its evals and evecs are all NaN, the other
 * matrices of the batch are solved as usual, and the call returns MDG_ERR_NO_CONVERGE with a message that names the non-finite
 * input (status detail 2; 1 is the limit of 40 sweeps; the larger one of a batch is reported).  In deferred-status mode the same
 * code and message come out of mdg_deferred_status_decode, and every later kernel of the chain stays within its buffers.
 * Scale: a pair is rotated while |a_pq| > 2^-52 sqrt|a_pp| sqrt|a_qq|, the two roots taken separately, so the test neither
 * overflows nor underflows and the results of A and 2^k A agree bit for bit (evals scaled by 2^k) as long as no entry of 2^k A
 * overflows or becomes subnormal: roughly ||A||_2 within [2^-900, 2^1000].  Because the test is relative to the pair's own diagonal,
 * a graded positive definite matrix D B D (D diagonal, B well conditioned) gets every eigenvalue, and the eigenvectors of its
 * small eigenvalues, to a relative accuracy of order cond(B) n 2^-52, independent of cond(D). */
int mdg_syevj_batched(double* A, int64_t n, int64_t batch, double* evals, double* evecs, void* stream);

/* ------------------------------------------------------------------ MLP: ridge-leverage + Nystrom
 * scores = diag((C + ridge I)^-1).  `ridge` is added as given: pass the fp32-rounded lambda to reproduce the
 * float32 eye of compress_mlp.py:18.  C is not modified.  ws: mdg_ridge_scores_ws_bytes(n).  SYNCHRONISES.
 * sens (optional, [n]; NULL = not wanted): the first-order sensitivity of every score to an ENTRY-WISE RELATIVE perturbation of C,
 * |E_ab| <= eps sqrt(c_aa c_bb) -- the form of the covariance routes' error bounds (mdg_cov_accum_i8: eps <= 1.1e-11 guaranteed;
 * fp64 accumulation: eps <= tokens 2^-53):  |delta scores[j]| <= eps sens[j] + O(eps^2),
 *     sens[j] = (sum_b |X_bj| sum_a |X_ba| sqrt(c_aa))^2 >= (sum_a sqrt(c_aa) |((C + ridge I)^-1)_aj|)^2,   X = inv(chol(C + ridge I)).
 * Two extra passes over the triangle of X the call holds anyway (1.6 GB of reads at n = 14336, < 1 ms); the scores are the same
 * bits with or without it. */
size_t mdg_ridge_scores_ws_bytes(int64_t n);
int mdg_ridge_scores(const double* C, int64_t n, int64_t ldc, double ridge, double* scores, double* sens, void* ws,
                     size_t ws_bytes, void* stream);
/* idx[0..k) = indices of the k smallest scores, ascending index order (topk(largest=False) + sort,
 * compress_mlp.py:45-47).  Ties: lower index first.  NaN ranks as largest.  k == 0: nothing is written, idx may be NULL. */
int mdg_select_smallest_sorted(const double* scores, int64_t n, int64_t k, int64_t* idx, void* stream);
/* The certificate of that selection ("rank selections bit-identical" made checkable): with every score known only up to
 * eps * sens[j] (mdg_ridge_scores), can the selected SET differ?  idx [k]: the selection (ascending); out8 (DEVICE, 8 doubles):
 *   [0] largest selected score s_(k)      [1] smallest unselected score s_(k+1)     -> margin = ([1] - [0]) / [0]
 *   [2] max over selected of s + eps sens [3] min over unselected of s - eps sens   -> certified iff [2] < [3]
 *   [4] / [5] largest sens among the selected / unselected   ([1] - [0]) / ([4] + [5]) <= the largest eps that still certifies
 *   [6] how many scores' intervals reach across the midpoint of [0] and [1]        [7] 1.0 if certified else 0.0
 * Only enqueues; the caller reads the 8 doubles when it next waits for the stream (modegpt_amd reads them with the chain's
 * status).  Not in the reference: there the selection is whatever torch.topk makes of the fp64 scores (compress_mlp.py:45-47). */
int mdg_select_margin(const double* scores, const double* sens, const int64_t* idx, int64_t n, int64_t k, double eps,
                      double* out8, void* stream);
/* out[i,:] = src[rows[i],:] for 2-byte elements (W_u[topk,:], W_g[topk,:], compress_mlp.py:49-50;
 * Q/K row gathers, compress_qk.py:375-376). */
int mdg_gather_rows_16(const void* src, int64_t ld_src, const int64_t* rows, int64_t n_rows, int64_t n_cols,
                       void* out, int64_t ld_out, void* stream);
/* down_out [d, r] (bf16, ld_out) = ((C[idx,idx] + eps I)^-1 C[idx,:] W_d^T)^T, W_d [d, n] (ld_wd) of dtype w_dtype:
 * MDG_BF16, or MDG_F64 for checkpoints in another precision (fp16 OPT: the caller widens exactly, as the reference's
 * .to(float64) does).
 * compress_mlp.py:52-62,97.  down_f64 (optional, [r, d] row-major) receives the fp64 solution before the
 * cast; down_out is the cast of exactly those values.
 * Evaluated as (k = idx, k' = its complement in 0 .. n-1 in ascending order, M = C_kk + eps I, so M^-1 C_kk = I - eps M^-1):
 *     W_d[:,k]^T + M^-1 ( C[k,k'] W_d[:,k']^T - eps_p W_d[:,k]^T ),      eps_p = fl(c_pp + eps) - c_pp  (what fp64 really added)
 * -- the selected columns' share of C[k,:] W_d^T is the weights themselves, exactly; only the n - r unselected columns of C are
 * multiplied (2 r (n - r) d flop instead of 2 r n d), in a fixed order: the result does not depend on the order of the launches
 * and is the same bits from call to call.  r == n: no product at all; eps == 0 then returns W_d^T entry for entry.
 * PRECONDITION: the entries of idx are distinct and in 0 .. n-1 (any order).  A repeated index makes C_kk singular up to eps
 * already; the result is then unspecified (nothing is written out of bounds: the complement list is cut at n - r entries, and
 * an entry outside 0 .. n-1 names no column of the complement).
 * ws: mdg_nystrom_down_ws_bytes(n, r, d), 8-byte aligned; nystrom_layout in csrc/mlp.hip states the blocks -- C_kk (rows r rounded
 * up to 16), its inverted diagonal blocks, the right-hand side and the substitution's workspace, then from a 16-byte address
 * C[k,k'] as fp64 [r][K'], W_d[:,k'] as [d][K'] in W_d's own dtype (sized for fp64), the complement list and its marks; K' = n - r
 * rounded up to 16, the padding columns written as zeros by the call (the workspace may hold anything).  SYNCHRONISES. */
size_t mdg_nystrom_down_ws_bytes(int64_t n, int64_t r, int64_t d);
int mdg_nystrom_down(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd,
                     int64_t d, int64_t ld_wd, int w_dtype, double eps, void* down_out, int64_t ld_out, double* down_f64,
                     void* ws, size_t ws_bytes, void* stream);
/* The same with the cross product C[k,k'] W_d[:,k']^T on `side_stream`, beside the factorisation of C_kk on `stream` (they do
 * not depend on each other; the factorisation's 128-column steps leave most of the chip idle between their GEMMs); the complement
 * list, the compaction of both operands and the -eps W right-hand side run on `side_stream` in front of the product.  Streams and the
 * two events are the CALLER'S (any two hipEvent_t, timing disabled is fine): ev_fork is recorded on `stream` and waited for by
 * `side_stream` before the product, ev_join is recorded behind the product and waited for by `stream` before the solve; when the
 * call returns everything later on `stream` is ordered behind both.  Results are bit-identical to mdg_nystrom_down. */
int mdg_nystrom_down_overlapped(const double* C, int64_t n, int64_t ldc, const int64_t* idx, int64_t r, const void* Wd,
                                int64_t d, int64_t ld_wd, int w_dtype, double eps, void* down_out, int64_t ld_out,
                                double* down_f64, void* ws, size_t ws_bytes, void* side_stream, void* ev_fork, void* ev_join,
                                void* stream);
/* The mean-aware refit (added under ABI 10; not in the reference, whose refit is linear against the uncentred second moment).  With
 * mu = E[h] over the calibration tokens (normalised as mdg_cov_finalize normalises C) and S = C - mu mu^T, minimising
 * E|| W_d h + b_d - D h_k - b' ||^2 over (D, b') with the ridge on D alone gives
 *     D  = W_d S[:,k] (S_kk + eps I)^-1        -- mdg_nystrom_down[_overlapped] called with S in place of C, nothing else
 *     b' = b_d + W_d mu - D^ mu_k              -- D^ = the bf16 tensor that is STORED: the optimal intercept for exactly that tensor
 * which is the least-squares fit on the augmented feature [h_k; 1] (Sherman-Morrison).  Three entry points supply what that needs.
 *
 * mdg_col_sum_accum:  sum[j] += sum_t f(x[t, j]), j < n, in fp64; x [n_tokens, n] of `dtype` (any MDG_* element type) with leading
 * dimension ld >= n, f = identity or, with relu != 0, max(., 0) on load (OPT's fc1 statistic; a NaN stays a NaN).  One pass over x:
 * a workgroup owns 128 tokens and 256 column slots, a slot being a 16-byte load of the row (8 / 4 / 2 columns) wherever the rows
 * allow aligned ones -- ld a multiple of the vector; the columns in front of x's first 16-byte boundary and behind the last whole
 * vector are single-column slots, as is every column when ld is no multiple of the vector -- so x need only be aligned to its
 * element.  A thread adds its tokens in ascending order; the partial row of every 128-token chunk goes to the workspace, and a second
 * kernel adds the partials in ascending chunk order and the total to sum[j].  No atomics: the same bits from run to run.  A column
 * is only ever added to itself: a NaN or Inf stays in its column.  Nothing beyond column n of a row is read.
 * ws: mdg_col_sum_ws_bytes(n_tokens, n) bytes (one partial row per chunk: col_sum_layout in csrc/colsum.hip), 8-byte aligned.  Only enqueues.  MDG_ERR_BAD_ARG for a null
 * pointer, an unknown dtype, n_tokens or n < 1, ld < n, a misaligned pointer or a workspace that is too small. */
size_t mdg_col_sum_ws_bytes(int64_t n_tokens, int64_t n);
int mdg_col_sum_accum(const void* x, int dtype, int64_t n_tokens, int64_t n, int64_t ld, int relu, double* sum, void* ws,
                      size_t ws_bytes, void* stream);
/* S[i, j] = fma(-mu[i], mu[j], C[i, j]): one rounding per entry.  C [n, n] (ldc) is read at and below the diagonal only, S [n, n]
 * (lds) is written in both triangles from the one value, so S equals its transpose bit for bit; the columns from n to ldc / lds are
 * neither read nor written, and n need not be a multiple of the 64 x 64 tile.  C is not modified; C and S must not overlap.
 * Only enqueues.  MDG_ERR_BAD_ARG for a null pointer, n < 1, ldc or lds < n. */
int mdg_cov_center(const double* C, int64_t n, int64_t ldc, const double* mu, double* S, int64_t lds, void* stream);
/* delta_i = sum_j W_d[i, j] mu[j] - sum_p D^[i, p] mu[idx[p]], i < d, in fp64, every product exact (fma).  W_d [d, n] (ld_wd) of
 * w_dtype MDG_BF16 or MDG_F64, as mdg_nystrom_down takes it; down_hat = D^ [d, r] bf16 (ld_down), the tensor mdg_nystrom_down stored;
 * idx [r] the selection it was called with; mu [n] fp64.
 *     bias_f64[i] = b_d[i] + delta_i             (b_d [d] of b_dtype, any MDG_* element type; NULL: 0)
 *     bias_out[i] = bias_f64[i] rounded once to out_dtype (the way torch's .to() rounds: through fp32 for the 16-bit types); may be NULL
 *     norms[0] = sum_i delta_i^2 ,  norms[1] = sum_i (W_d mu)_i^2     (thread t adds rows t, t + 256, ... ascending, then a fixed tree)
 * One read of both operands: a wave owns four rows, lanes go along the row (16-byte loads of eight bf16 where the pointer and the
 * leading dimension allow), mu and mu[idx] are staged in LDS per 2048 columns; a lane adds its columns in ascending order, the wave
 * reduces by butterfly.  No atomics: the same bits from run to run.  A NaN in row i of W_d or D^ reaches bias entry i alone (and
 * both norms); an entry of idx outside 0 .. n-1 reads no memory and contributes NaN.
 * ws: mdg_nystrom_intercept_ws_bytes(d) bytes (delta and W_d mu per row: intercept_layout in csrc/colsum.hip), 8-byte aligned.  Only enqueues.  MDG_ERR_BAD_ARG
 * for a null pointer, an unsupported dtype, d, n or r < 1, r > n, ld_wd < n, ld_down < r, or a workspace that is too small. */
size_t mdg_nystrom_intercept_ws_bytes(int64_t d);
int mdg_nystrom_intercept(const void* Wd, int64_t d, int64_t n, int64_t ld_wd, int w_dtype, const void* down_hat, int64_t r,
                          int64_t ld_down, const int64_t* idx, const double* mu, const void* b_d, int b_dtype, void* bias_out,
                          int out_dtype, double* bias_f64, double* norms, void* ws, size_t ws_bytes, void* stream);
/* What that refit costs, at EVERY rank, from one factorisation (added under ABI 9; not in the reference, which reports nothing
 * about the objective compress_mlp.py:52-62 minimises).  With M = C + eps I, `order` = the columns in ascending ridge-score order
 * (ties: lower index first, NaN last -- torch.argsort(scores, stable=True) -- so that order[:r], sorted, is what
 * mdg_select_smallest_sorted(scores, r) returns, for every r), M[order, order] = L L^T, Z = W_d[:, order] L and c_j = ||Z[:, j]||^2:
 *     curve[r] = sum_{j >= r} c_j = tr(W_d (M - M[:, S] M_SS^-1 M[S, :]) W_d^T),   S = order[:r],   r = 0 .. n
 * -- the Nystrom residual energy of keeping the columns S, summed over the d output channels: the minimum over ALL refits of
 * sum_k u_k^T M u_k, u_k = row k of W_d minus row k of the refit at the columns S.  curve[0] = tr(W_d M W_d^T), curve[n] = +0.0
 * exactly, and the curve is non-increasing entry by entry (a suffix sum of squares, accumulated from the tail).  Against the
 * refit D = down_f64 of mdg_nystrom_down (which solves with C[S, :], not M[S, :]), with E_D its output error under C and U the
 * residual weights:  E_D + eps ||U||_F^2 - eps ||W_d[:, S]||_F^2 <= curve[r] <= E_D + eps ||U||_F^2  ("The error-versus-rank curve").
 * C [n, n] fp64 (ldc; only the lower triangle is read, C is not modified), n <= 2^31 - 1 (beyond: MDG_ERR_BAD_ARG); order: DEVICE int64 [n], a permutation of 0 .. n-1 --
 * out-of-range entries are clamped (memory safety only, as mdg_rope_gather clamps its mask) and an index that occurs twice makes
 * the matrix singular: MDG_ERR_NOT_PD, reported at the first position of a repeated index.  W_d [d, n] (ld_wd) of dtype w_dtype,
 * MDG_BF16 or MDG_F64 as in mdg_nystrom_down; a NaN in W_d gives NaN in curve[0 .. p] (p: at least the NaN column's position in
 * `order`) and MDG_OK.  eps is added in fp64 with one rounding per diagonal entry, as mdg_nystrom_down adds it.  curve: [n + 1].
 * No atomics, every sum in a fixed order: bit-identical from run to run.
 * ws: mdg_nystrom_rank_curve_ws_bytes(n, d) bytes (rank_curve_layout in csrc/rank_curve.hip: the gathered matrix / its factor,
 * W_d[:, order] and Z in fp64 with rows of n rounded up to 16, the inverted diagonal blocks of the factorisation, the column norms,
 * the clamped order and its marks): 2.6 GB at n = 14336, d = 4096 -- per call in flight.
 * Status: follows the deferred-status convention.  Between mdg_deferred_status_begin / _end the call only enqueues and merges the
 * factorisation's pivot word into the device status; outside, it SYNCHRONISES once, behind the factorisation, to return
 * MDG_ERR_NOT_PD (curve is then not written), and enqueues the rest. */
size_t mdg_nystrom_rank_curve_ws_bytes(int64_t n, int64_t d);
int mdg_nystrom_rank_curve(const double* C, int64_t n, int64_t ldc, const int64_t* order, const void* Wd, int64_t d,
                           int64_t ld_wd, int w_dtype, double eps, double* curve /* [n + 1] */, void* ws,
                           size_t ws_bytes, void* stream);

/* MLP column selection by block-greedy descent on the objective the Nystrom refit minimises (added under ABI 10; not in the
 * reference, whose ridge-leverage rule never looks at W_d; DESIGN.md section 7, "Greedy MLP selection").
 * Inputs: C [n, n] fp64 (ldc; only the lower triangle is read -- NaN above the diagonal is harmless -- and C is not modified);
 * W = W_d [d, n] (ld_wd), MDG_BF16 or MDG_F64 as in mdg_nystrom_down; eps; the rank r, 0 <= r <= n; rounds = T >= 1 (T > r counts as r).
 * State: M = C + eps I (eps added in fp64, one rounding per diagonal entry, as mdg_nystrom_down adds it); S = {}, R = M, B = W R
 * [d, n]; J = sum_ij B_ij W_ij = tr(W R W^T), the value mdg_nystrom_rank_curve reports.
 * Round t = 0 .. T-1 takes m_t = floor(r (t + 1) / T) - floor(r t / T) columns:
 *   gain         g_j = (sum_i B_ij^2) / R_jj -- the exact drop of J if j alone joined S;
 *   eligibility  j not in S, R_jj > n 2^-52 M_jj (the accumulated rounding of at most n non-negative downdates of a diagonal
 *                entry: a condition, not a knob) and g_j finite;
 *   pick         the m_t eligible columns of largest gain, ties to the lower index; if fewer are eligible, the round is filled with
 *                unselected ineligible columns in ascending index order -- "dead picks", which join S with no downdate and are counted;
 *   downdate     with the eligible picks P: K = R[P, P], X = K^-1 R[P, :] by Cholesky of K, R <- R - R[:, P] X, B <- B - B[:, P] X;
 *   record       objective[t + 1] = sum B o W.
 * Outputs (DEVICE): order int64 [r], round by round and ascending index within a round (dead picks included); objective fp64
 * [rounds + 1], objective[0] = tr(W M W^T) -- a round that takes nothing (t >= r) repeats the previous entry; cut fp64
 * [rounds][2] (optional), per round the smallest picked gain and the largest eligible gain not picked, NaN where there is none
 * (both NaN for a round that takes nothing); n_dead int64 [1] (optional), the number of dead picks.  T = r is exact forward greedy
 * selection (orthogonal least squares), T = 1 a one-shot weighted score.
 * R is never formed: Yt [|S|, n] with R = M - Yt^T Yt, diag(R) as a vector, one panel R[P, :] per round (its product split over K
 * and summed in split order where a round's picks are few), B downdated right-looking -- about n r^2 + 2 d n r + 2 d n^2 flops in the fp64 GEMM.  Every round is ordinary launches on one stream; no
 * atomics, every sum in a fixed order: bit-identical from run to run.
 * r == 0 writes objective[0 .. rounds] = J_0 and nothing else (order may then be NULL).  Non-finite input: order is still r
 * distinct indices in 0 .. n-1, objectives may be NaN, the status may be MDG_ERR_NOT_PD, nothing is written out of bounds.
 * ws: mdg_nystrom_greedy_ws_bytes(n, d, r, rounds) bytes, 16-byte aligned (greedy_layout in csrc/greedy.hip): about 8 n' (d + r + max(m, min(n, 2048))) for B, Yt and
 * the panel, 8 m' (2.25 m + 2 d + r) for K, its inverse and the picked columns (m = ceil(r / T); n', m' rounded up to 16) and
 * 8 n' (38 + ceil(n / 1024) / 2) for the vectors and the pick's counts, and for T > 1 min(8 m n', 2^24) doubles for the K-split
 * partial panels: 2.0 GB at n = 14336, d = 4096, r = 10035, T = 32.  0 for arguments the call refuses.
 * Status: follows the deferred-status convention.  Between mdg_deferred_status_begin / _end the call only enqueues and merges each
 * round's pivot word into the device status; outside, it SYNCHRONISES once per round and returns MDG_ERR_NOT_PD after the last
 * round if a pivot of some K failed.  MDG_ERR_BAD_ARG, with a message and before any device work: a null required pointer,
 * n < 1, d < 1, r < 0, r > n, rounds < 1, ldc < n, ld_wd < n, an unsupported dtype, a workspace that is too small. */
size_t mdg_nystrom_greedy_ws_bytes(int64_t n, int64_t d, int64_t r, int64_t rounds);
int mdg_nystrom_greedy_select(const double* C, int64_t n, int64_t ldc, const void* Wd, int64_t d, int64_t ld_wd, int w_dtype,
                              double eps, int64_t r, int64_t rounds, int64_t* order /* [r] */, double* objective /* [rounds + 1] */,
                              double* cut /* [rounds][2], optional */, int64_t* n_dead /* device, optional */, void* ws,
                              size_t ws_bytes, void* stream);

/* What a STORED down projection lost, per output channel, on the calibration statistic (added under ABI 9; not in the reference:
 * compress_mlp.py:52-62 computes the refit and reports nothing about it).  The rank curve above belongs to the fp64 minimiser under
 * C + eps I; this call takes the tensor that goes into the checkpoint -- or any other `down`.  With U [d, n] the residual weights,
 * column j of U = W_d[:, j] where j is not in idx and W_d[:, j] - down[:, p] where j = idx[p], and u_k = row k of U:
 *     e[k] = u_k C u_k^T = sum_i C_ii u_ki^2 + 2 sum_{i > j} C_ij u_ki u_kj ,        unorm2[k] = ||u_k||^2   (optional, may be NULL)
 * sum_k e[k] is the E_D and sum_k unorm2[k] the ||U||_F^2 of the sandwich  E_D + eps ||U||^2 - eps ||W_S||^2 <= curve[r] <= E_D + eps ||U||^2
 * (DESIGN.md section 7); with down == NULL or r == 0 nothing is subtracted and e[k] = q_k = w_k C w_k^T, the channel's output energy.
 * C [n, n] fp64 (ldc >= n; only the LOWER triangle is read -- NaN above the diagonal is harmless -- and C is not modified),
 * n <= 2^31 - 1.  W_d [d, n] (ld_wd) of dtype w_dtype, MDG_BF16 or MDG_F64 as in mdg_nystrom_down.  down is addressed as
 * down[k sd_row + p sd_col], k < d, p < r, of dtype down_dtype, MDG_BF16 or MDG_F64: the stored [d, r] bf16 artefact is
 * (sd_row = ld_out, sd_col = 1), mdg_nystrom_down's down_f64 [r, d] is (sd_row = 1, sd_col = d).  The subtraction is done in fp64 on
 * the exactly widened operands (a bf16 - bf16 difference is exact there).  idx: DEVICE int64 [r] (what mdg_select_smallest_sorted
 * wrote; need not be sorted); entries outside 0 .. n-1 are clamped (memory safety only) and where an index occurs more than once
 * its HIGHEST position is the one subtracted.  A NaN in row k of W_d or down gives NaN in e[k] and leaves the other rows alone; a
 * NaN in the lower triangle of C may reach every row; MDG_OK either way.
 * One 128-row block of U against the lower-triangle tiles of C on v_mfma_f64_16x16x4_f64, U formed while staging, the row dot
 * product folded into the epilogue: d n (n + 1) flop, the product U C is never written.  No atomics, every sum in a fixed order:
 * bit-identical from run to run.
 * ws: mdg_mlp_output_error_ws_bytes(n, d) bytes (out_err_layout in csrc/out_err.hip: the inverse index map, then from a 16-byte
 * boundary the per-tile-column partial sums of e and unorm2): 7.4 MB at n = 14336, d = 4096.
 * Status: there is no factorisation -- the call only enqueues, never synchronises, and is the same inside and outside
 * mdg_deferred_status_begin / _end.  MDG_ERR_BAD_ARG for n <= 0, d <= 0, r < 0, r > n, ldc < n, ld_wd < n, an unsupported dtype,
 * a workspace that is too small, or r > 0 without down / idx. */
size_t mdg_mlp_output_error_ws_bytes(int64_t n, int64_t d);
int mdg_mlp_output_error(const double* C, int64_t n, int64_t ldc, const void* Wd, int64_t d, int64_t ld_wd, int w_dtype,
                         const int64_t* idx, int64_t r, const void* down, int64_t sd_row, int64_t sd_col, int down_dtype,
                         double* e /* [d] */, double* unorm2 /* [d], optional */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ QK: CR selection
 * mask [n_kv, rank] (int64, score-descending, NOT sorted: compress_qk.py:366-367,418-419,464),
 * q_rows [n_heads*rank] / k_rows [n_kv*rank]: absolute row indices into W_q / W_k for mdg_gather_rows_16.
 * cov_q [n_heads, hd, hd], cov_k [n_kv, hd, hd] fp64.  Scores use ||col_j(sqrt(C + rho I))||^2 = C_jj + rho
 * (exact for symmetric PSD C; DESIGN.md section "Identities"), clamped at 0; a NaN diagonal entry stays NaN, and a NaN score ranks
 * first (torch.topk).  Ties: lower index first.  ROPE modes need even rank. */
int mdg_qk_select(const double* cov_q, const double* cov_k, int n_heads, int n_kv, int hd, double ridge_q,
                  double ridge_k, int rank, int mode, int64_t* mask, int64_t* q_rows, int64_t* k_rows,
                  void* stream);
/* The certificate of that selection: can the selected SET (and its ORDER -- the reference does not sort the mask) differ for any
 * sigma_q / sigma_k within the error bound of the covariance route, or under the rounding of the reference's own route to the same
 * score?  The reference reaches ||col_j(sqrt(C + rho I))||^2 through eigh -> sqrt -> V diag V^T -> column norm
 * (compression_utils.py:15-55, compress_qk.py:355-367, 403-419, 452-464); mdg_qk_select uses the identity C_jj + rho.  The two agree
 * in exact arithmetic only: the eigh route carries rounding of the order u * lambda_max, however small C_jj is.  Model: a diagonal
 * entry c = C_jj of any head matrix is known to within
 *     delta_j = eps_rel * |c| + eps_abs * (||C||_inf + rho)
 * eps_rel: the covariance route's entry-wise bound (relative to c itself on the diagonal); eps_abs: the eigh route's rounding
 * relative to ||C||_inf (largest absolute row sum, an upper bound on lambda_max that needs no eigensolve; the kernel computes it from
 * the hd x hd matrices it reads).  Every score of the three modes is monotone non-decreasing in every diagonal entry, so the bound
 * is INTERVAL ARITHMETIC, not first order: s_lo / s_hi = the score formula with every factor max(c - delta + rho, 0) /
 * max(c + delta + rho, 0).  Same shapes, modes and argument checks as mdg_qk_select; mask [n_kv, rank] is what that call wrote
 * (it is read, not recomputed).  out (DEVICE, [n_kv][8] doubles), per kv head:
 *   [0] smallest selected score             [1] largest unselected score           -> margin = ([0] - [1]) / [0]
 *   [2] min over selected of s_lo           [3] max over unselected of s_hi        -> the set is certified iff [2] > [3]
 *   [4] max over units of (s_hi - s_lo) / (2 s): the relative half-width a score can move
 *   [5] number of units whose interval reaches across the midpoint of [0] and [1]
 *   [6] number of neighbouring positions in the selected (score-descending) order whose intervals overlap; 0: the order is certified too
 *   [7] 1.0 if the set is certified else 0.0
 * rank == number of units: nothing to separate, certified, [1] = -inf.  NaN scores rank as in mdg_qk_select (largest) and make the
 * head uncertified.  Only enqueues; one workgroup per kv head.  Not in the reference. */
int mdg_qk_select_margin(const double* cov_q, const double* cov_k, int n_heads, int n_kv, int hd, double ridge_q,
                         double ridge_k, int rank, int mode, const int64_t* mask, double eps_rel, double eps_abs,
                         double* out, void* stream);

/* What the Q/K selection costs the attention LOGITS on the calibration statistic, per query head and at EVERY rank (added under ABI
 * 10; not in the reference, whose scores -- compress_qk.py:355-367, 403-419, 452-464 -- read four diagonal entries of sigma_q / sigma_k
 * and report nothing about what the selection loses).  mdg_qk_select_margin says whether the selection is DETERMINED; this says what
 * it LOSES.  Drop the column set D of q and k of one query head: the logit of token pair (i, j) changes by sum_{c in D} q_ic k_jc, and
 * its mean square over all token pairs of the calibration set is
 *     E(D) = <C_q[D, D], C_k[D, D]>_F = sum_{a, b in D} P[a][b] ,      P_h = (sigma_q,h + rho_q I) (.) (sigma_k,kv(h) + rho_k I)
 * (entry-wise product; sigma normalised as mdg_cov_finalize leaves it) -- the CR objective || C_q^1/2 (I - S S^T) C_k^1/2 ||_F^2 that
 * the reference's scores approximate by its diagonal.  The stored q_proj / k_proj are row gathers (bit copies), so with rho = 0 this
 * IS the realised error of the artefact on the statistic.  P is PSD (Schur product theorem), so E >= 0 in exact arithmetic; E is NOT
 * monotone in D (P = [[1, -.81], [-.81, 1]]: 1 with one column dropped, 0.38 with both), and nothing here is clamped or made monotone.
 * Shapes, modes and argument checks as mdg_qk_select (no rank): cov_q [n_heads, hd, hd], cov_k [n_kv, hd, hd] fp64 contiguous, both
 * triangles are read; RoPE modes: unit u < ns = hd / 2 is the column pair {u, u + hd / 2}; OPT: unit u < ns = hd is column u.
 * order (DEVICE, int64 [n_kv][ns]): the units of every kv head, keep-first -- the first ns mask entries per head of mdg_qk_select at
 * rank = hd (all units, score-descending); nothing is ranked here.  Entries outside 0 .. ns-1 are clamped when read (memory safety
 * only); for a head whose order is not a permutation the values of that head alone are unspecified.
 * With g = n_heads / n_kv and D_m = {order[i] : i >= m}, outputs (DEVICE, fp64 unless stated):
 *   curve_h [n_heads][ns + 1]   curve_h[h][m] = sum_{a, b in cols(D_m)} P_h[a][b]: the error of query head h when the first m units are
 *                               kept.  [ns] = +0.0 exactly; [0] = the head's whole logit energy <C_q,h, C_k>.
 *   curve [n_kv][ns + 1]        the group's: curve_h of its heads added in ascending h, ((c_0 + c_1) + c_2) + ..., to the bit.
 *   terms [n_kv][ns]            (optional) the diagonal share of unit order[i],
 *                               sum_{h in group} sum_{a in cols(u)} max(Cq_aa + tau_q, 0) max(Ck_aa + tau_k, 0), tau = terms_ridge_q /
 *                               terms_ridge_k, by the expression and in the order of mdg_qk_select's score (whose GROUPED / OPT score is
 *                               its square root, the MHA score the number itself; fmax drops a NaN, as there).  Its suffix sums are
 *                               what the reference's rule believes the cost is.  The ridges of the terms are arguments of their own
 *                               so that one call gives the error on the raw statistic (rho = 0) and the terms of the real scores.
 *   scale [n_kv]                (optional) sum_{h in group} sum_{a, b} |P_h[a][b]| = sum_h A_h[0] below: what a reader multiplies the
 *                               unit roundoff by to get the floor under which a value of this head says nothing.
 *   greedy_curve [n_kv][ns + 1], greedy_order [n_kv][ns] (int64)   (optional, given together) a comparison order built on the FULL
 *                               objective: start from nothing dropped and repeatedly drop the unit whose move into D raises the
 *                               group's E least, Delta_u = B[u][u] + 2 sum_{v in D} B[u][v], B the group's unit-block sums of
 *                               sum_h P_h (2 B[u][v] is taken as B[u][v] + B[v][u]).  Compared with <, ties to the lower unit index, a
 *                               NaN increment never wins while another exists.  greedy_order is keep-first (the first unit dropped
 *                               is last); greedy_curve[m] is E of the group with the first m units of greedy_order kept, evaluated
 *                               from B along that order as curve is, [ns] = +0.0.  It is an UPPER BOUND on the best selection of
 *                               each size, NOT the optimum (the problem is a quadratic subset selection).
 * Accuracy: the sums have mixed sign, so a value is accurate relative to A_h[m] = sum_{a, b in cols(D_m)} |P_h[a][b]|, not to itself:
 *     |curve_h - exact| <= (hd^2 + 2) 2^-53 A_h ,      group (curve, greedy_curve):  <= (g hd^2 + 2) 2^-53 sum_h A_h
 * (one rounding per ridge addition, per product and per addition, in any order); terms: (2 g |cols| + 2) 2^-53 relative to itself.
 * Non-finite input: an entry [a][b] of one query head's sigma_q reaches curve_h of THAT head at every m <= min(position of a's unit,
 * position of b's unit), and the same entries of its group's curve, that group's scale and greedy outputs; a diagonal Inf also that
 * unit's term (a diagonal NaN counts as 0 there).  An entry of one kv head's sigma_k does the same for every head of that group.
 * Nothing of another kv head changes by a bit.  greedy_order stays a permutation.  MDG_OK in every case.
 * One workgroup per kv head; the head's packed unit-block sums (and the group's, with the greedy outputs) live in LDS, up to 137 KB;
 * no atomics, every sum in a fixed order: bit-identical from run to run.  Only enqueues, no workspace.  MDG_ERR_BAD_ARG for a null
 * required pointer, a head layout / mode / hd that mdg_qk_select rejects, or only one of the greedy pair. */
int mdg_qk_rank_curve(const double* cov_q, const double* cov_k, int n_heads, int n_kv, int hd, double ridge_q, double ridge_k,
                      int mode, const int64_t* order, double terms_ridge_q, double terms_ridge_k,
                      double* curve_h /* [n_heads][ns + 1] */, double* curve /* [n_kv][ns + 1] */, double* terms /* [n_kv][ns], optional */,
                      double* scale /* [n_kv], optional */, double* greedy_curve /* [n_kv][ns + 1], optional */,
                      int64_t* greedy_order /* [n_kv][ns], optional */, void* stream);

/* ------------------------------------------------------------------ VO: SVD of sqrt(C) W_v^T
 * v_out [n_kv*rank, d] bf16, o_out [d, n_heads*rank] bf16 (compress_vo.py:89-90).  W_v [n_kv*hd, d],
 * W_o [d, n_heads*hd], both of dtype w_dtype (MDG_BF16 or MDG_F64).  n_kv == n_heads selects the two-SVD MHA variant (compress_vo.py:162-223), else the
 * grouped one (:112-159).  Works on the Gram matrix W_v (C + rho I) W_v^T (DESIGN.md "Identities"), so the
 * d x d eigensolve and inverse of compress_vo.py:43-45 never happen.  v_f64 / o_f64 optional fp64 copies of
 * the factors.  ws: mdg_vo_compress_ws_bytes.  SYNCHRONISES.
 * A NaN or Inf in cov_x (a poisoned statistic: one bad column is a NaN row and column) or in the weights reaches the Gram
 * matrices, whose eigensolves report it: MDG_ERR_NO_CONVERGE with the non-finite-input message of mdg_syevj_batched, at once or,
 * in deferred-status mode, from mdg_deferred_status_decode; the outputs are then to be discarded (all accesses stay in bounds).
 * Scale: as mdg_syevj_batched, on W_v (C + rho I) W_v^T. */
size_t mdg_vo_compress_ws_bytes(int64_t d, int n_heads, int n_kv, int hd);
int mdg_vo_compress(const double* cov_x, int64_t d, int64_t ldc, const void* Wv, int64_t ld_wv, const void* Wo,
                    int64_t ld_wo, int w_dtype, int n_heads, int n_kv, int hd, int rank, double ridge, void* v_out,
                    int64_t ld_v, void* o_out, int64_t ld_o, double* v_f64, double* o_f64, void* ws,
                    size_t ws_bytes, void* stream);
/* What the truncation at `rank` did to the spectrum (compress_vo.py:130-131,145-146 / :187-223 cut U, S, Vh at `rank` and report
 * nothing about sigma_r against sigma_r+1; when they nearly coincide the kept subspace is not determined by the data).  Reads the
 * eigenvalues the LAST mdg_vo_compress call left in workspace `ws` (same shapes): the spectrum that call truncated -- the Gram
 * matrix's for the grouped variant, the second SVD's for the two-SVD MHA variant (lambda = sigma^2 of the reference's SVD).
 * out (DEVICE, [n_kv][8] doubles), per kv head:
 *   [0], [1] lambda_r, lambda_r+1 ([1] = 0 when rank == hd)
 *   [2] relative gap (sigma_r - sigma_r+1) / sigma_r, sigma = sqrt(max(lambda, 0))
 *   [3] retained energy sum_{i<r} lambda_i / sum_i lambda_i
 *   [4] grouped: the Weyl bound b = eps * || |W_v,h| s ||_2^2, s_a = sqrt(c_aa) of sigma_x; NaN for the MHA variant
 *   [5] 1.0 if lambda_r - lambda_r+1 > 2 b (the kept subspace is separated from the dropped one for every sigma_x within the
 *       bound), 0.0 if not; NaN for the MHA variant
 *   [6], [7] lambda_1, lambda_hd
 * [4]: an entry-wise error |E_ab| <= eps s_a s_b of sigma_x gives ||W E W^T||_2 <= || |W| |E| |W|^T ||_2 <= eps || |W| s ||_2^2, and the
 * matrix diagonalised is W_v,h (sigma_x + rho I) W_v,h^T, so by Weyl no eigenvalue moves by more than b.  One pass over the head's
 * hd x d slice of W_v and the diagonal of sigma_x.  The MHA variant's second spectrum also depends on W_o; no bound is given for
 * it, the gap alone is reported.  Only enqueues; one workgroup per kv head. */
int mdg_vo_spectrum(const void* ws, size_t ws_bytes, const double* cov_x, int64_t d, int64_t ldc, const void* Wv, int64_t ld_wv,
                    int w_dtype, int n_heads, int n_kv, int hd, int rank, double ridge, double eps, double* out, void* stream);
/* The v_proj / o_proj biases through the truncation (added under ABI 10).  The reference's save_layer -> convert_model route rebuilds
 * both projections bias-free (model_adapter.py:199-208) and compress_vo.py:112-223 never looks at a bias; its in-place route keeps
 * b_o and drops b_v.  Softmax rows sum to one, so a v bias passes through attention unchanged and query head h adds the constant
 * W_o,h b_v,kv(h) to the output.  With P_g [rank, hd] (W_v,g' = P_g W_v,g) and Q_g [hd, rank] (W_o,h' = W_o,h Q_g) the factors the
 * LAST mdg_vo_compress call left in workspace `ws` (same shapes and rank; grouped and two-SVD MHA variant alike), Pi_g = Q_g P_g:
 *   b_o given  (o_proj has a bias):  o_bias[i] = b_o[i] + sum_h W_o,h[i, :] b_v,kv(h)   -- exact at every rank; v_bias is not written
 *   b_o NULL   (o_proj has none):    v_bias[g rank + a] = (P_g b_v,g)[a]                  -- o_bias is not written
 *   resid[0] = ||rho||^2, rho = sum_h W_o,h (I - Pi_g) b_v,kv(h): what the second form cannot represent (0 at rank == hd up to rounding);
 *   resid[1] = ||sum_h W_o,h b_v,kv(h)||^2.  Both are written in either form.
 * Wo: the ORIGINAL o_proj weight [d, n_heads hd] (ld_wo), w_dtype MDG_BF16, MDG_F16 or MDG_F64; b_v [n_kv hd] and b_o [d] of b_dtype
 * (any MDG_* element type).  o_bias [d], v_bias [n_kv rank], resid [2]: fp64 on the device; the caller rounds once to the model's
 * dtype.  One read of W_o: lanes along a row (16-byte loads of 16-bit weights when Wo and ld_wo allow), a wave per group of rows,
 * b_v and (I - Pi) b_v staged in LDS; every sum in a fixed order, no atomics: the same bits from run to run.  A NaN in one kv
 * head's b_v reaches that head's v_bias entries only (and every o_bias entry, resid).
 * Uses the T block of the workspace as scratch (dead after mdg_vo_compress; mdg_vo_spectrum / mdg_vo_rank_curve do not read it), so
 * the calls on one workspace belong on one stream.  Only enqueues.  MDG_ERR_BAD_ARG for a null pointer, an unsupported dtype, head
 * layout or rank, ld_wo < n_heads hd, a workspace smaller than mdg_vo_compress_ws_bytes, b_o without o_bias / no b_o without v_bias,
 * or 2 (n_kv hd + d) > n_kv hd d (no room for the scratch). */
int mdg_vo_bias(void* ws, size_t ws_bytes, const void* Wo, int64_t ld_wo, int w_dtype, int64_t d, const void* b_v, const void* b_o,
                int b_dtype, int n_heads, int n_kv, int hd, int rank, double* o_bias, double* v_bias, double* resid, void* stream);
/* The intercept of the mean-aware V/O truncation (added under ABI 10; not in the reference: compress_vo.py:112-223 looks at no first
 * moment and truncates the spectrum of the UNCENTRED second moment).  Softmax rows sum to one, so with mu = E[x] (x the post-norm
 * hidden state, normalised as mdg_cov_finalize normalises sigma_x) the mean reaches the attention output as the constant
 * sum_h W_o,h (W_v,kv(h) mu + b_v,kv(h)), whatever the attention weights are; the truncation then runs on S = sigma_x - mu mu^T
 * (mdg_cov_center, then mdg_vo_compress unchanged) and this call computes the optimal intercept for exactly the tensors that are STORED:
 *     a_g  = W_v,g mu + b_v,g   [hd]    per kv head   (b_v NULL: 0)
 *     a'_g = v^_g mu            [rank]  per kv head   (v^_g = rows g rank .. of v_new)
 *     delta_i = sum_h ( W_o,h[i, :] a_kv(h) - o^_h[i, :] a'_kv(h) )        i < d   (o^_h = columns h rank .. of o_new)
 *     bias_f64[i] = b_o[i] + delta_i             (b_o NULL: 0)
 *     bias_out[i] = bias_f64[i] rounded once to out_dtype (the way torch's .to() rounds: through fp32 for the 16-bit types); may be NULL
 *     norms[0] = sum_i delta_i^2 ,  norms[1] = sum_i (sum_h W_o,h[i, :] a_kv(h))^2    (the constant the uncompressed attention adds)
 * Wv [n_kv hd, d] (ld_wv) and Wo [d, n_heads hd] (ld_wo) of w_dtype, v_new [n_kv rank, d] (ld_v) and o_new [d, n_heads rank] (ld_o) of
 * new_dtype, each MDG_BF16 or MDG_F64 as mdg_vo_output_error takes them (the stored bf16 tensors or mdg_vo_compress's v_f64 / o_f64);
 * mu [d] fp64; b_v [n_kv hd] and b_o [d] of b_dtype (any MDG_* element type).  Head layouts as mdg_vo_compress (grouped, and MHA with
 * n_kv == n_heads); 0 <= rank <= hd, and at rank 0 the factors are not read (they may be NULL) and delta is the whole constant.
 * Two launches and the norm tree.  Head stage: the n_kv (hd + rank) rows of W_v and v^ against mu; row stage: the d rows of
 * [W_o | o^] against a and a', expanded to the query heads' columns in LDS.  In both a wave owns four rows, lanes go along the row
 * (16-byte loads of eight bf16 where the pointer and the leading dimension allow, single elements otherwise), the vector is staged in
 * LDS per 2048 columns; every product enters through fma, a lane adds its columns in ascending order, the wave reduces by butterfly;
 * norms: thread t adds rows t, t + 256, ... ascending, then a fixed tree.  One read of each operand, no atomics: the same bits from
 * run to run.  A NaN in row i of W_o or o_new reaches bias entry i alone (and the norms); a NaN in one kv head's W_v, v_new or b_v
 * reaches every bias entry (every row sums over all heads) and the norms.
 * ws: mdg_vo_intercept_ws_bytes(d, n_kv, hd, rank) bytes (vo_intercept_layout in csrc/vo_mean.hip: a, a', delta and the constant
 * per row), 8-byte aligned, its own (not mdg_vo_compress's: the call also serves factors from elsewhere).  Only enqueues.  MDG_ERR_BAD_ARG for a null
 * required pointer, an unsupported dtype or head layout, a rank outside the range, ld_wv or ld_v < d, ld_wo < n_heads hd,
 * ld_o < n_heads rank, a workspace that is too small, or rank > 0 without v_new / o_new. */
size_t mdg_vo_intercept_ws_bytes(int64_t d, int n_kv, int hd, int rank);
int mdg_vo_intercept(const void* Wv, int64_t ld_wv, const void* Wo, int64_t ld_wo, int w_dtype, const void* v_new, int64_t ld_v,
                     const void* o_new, int64_t ld_o, int new_dtype, int64_t d, int n_heads, int n_kv, int hd, int rank,
                     const double* mu, const void* b_v, const void* b_o, int b_dtype, void* bias_out, int out_dtype, double* bias_f64,
                     double* norms, void* ws, size_t ws_bytes, void* stream);

/* What the STORED V/O factors lose of the attention output on the calibration statistic, per query head and output channel (added
 * under ABI 9; not in the reference: compress_vo.py:112-223 cuts its SVD at `rank` and reports nothing about the product).  Field [3]
 * of mdg_vo_spectrum is the retained energy of the VALUE stream of the fp64 factors (grouped: W_o is not in it); this call takes the
 * tensors that go into the checkpoint -- or any other factors -- and weighs what they lose by W_o.  The objective is the one
 * compress_vo works on, the map x -> W_o,h W_v,g x per query head h of kv group g (no token mixing by the attention weights).
 * C = cov_x, the finalised sigma_x [d, d]; W_v,g = rows g hd .. of W_v; W_o,h = columns h hd .. of W_o; the factors
 * v'_g = rows g rank .. of v_new [n_kv rank, d] (ld_v), o'_h = columns h rank .. of o_new [d, n_heads rank] (ld_o).  With
 *     delta_{h,k} = W_o,h[k, :] W_v,g - o'_h[k, :] v'_g                              (a row of length d; never formed)
 *     e[h][k] = delta C delta^T ,      dnorm2[h][k] = ||delta||^2   (optional, may be NULL)
 * e + rho dnorm2 is the channel's objective under M = C + rho I, rho the ridge mdg_vo_compress was called with.  rank == 0 (v_new and
 * o_new are then not read and may be NULL): nothing is subtracted and e[h][k] = q[h][k], the channel's output energy.
 * Route: the stacked Gram.  V_g = [W_v,g ; -v'_g] [(hd + rank), d], y_{h,k} = [W_o,h[k, :], o'_h[k, :]]:
 *     e[h][k] = y (V_g C V_g^T) y^T ,   dnorm2[h][k] = y (V_g V_g^T) y^T
 * -- T = V_g C and the two Grams through the fp64 GEMM core (bf16 operands read directly, batched over the kv heads), then one
 * fused kernel on v_mfma_f64_16x16x4_f64: a workgroup owns 128 output channels of one head, y is stitched from W_o and o_new while
 * staging (both widened exactly), the LOWER triangle of the head's Gram is read with the factor 2 on its strict part, and the row dot
 * product sits in the epilogue; y G is never written.  About 2 (hd + rank) d (n_kv d + n_heads (hd + rank)) flop: 0.07 TFLOP at
 * d = 4096, 32 / 8 heads, hd = 128, rank = 88, where forming delta C would take 4.4.
 * Accuracy: the result is a difference of Gram entries, so it is accurate relative to the scale
 *     a[h][k] = (|y| |V_g|) |C| (|y| |V_g|)^T ,
 * NOT relative to itself: where the factors reproduce W_o,h W_v,g (rank == hd, fp64 factors) e is rounding noise of EITHER SIGN.  It
 * is returned raw; a reader takes 64 (d + hd + rank) 2^-53 a as the floor below which a value says nothing.
 * w_dtype (W_v, W_o) and new_dtype (v_new, o_new): MDG_BF16 or MDG_F64, so mdg_vo_compress's v_out / o_out and its v_f64 / o_f64
 * (ld_v = d, ld_o = n_heads rank) go in unchanged.  cov_x is read in full (both triangles), as mdg_vo_compress reads it; nothing
 * is modified.  Head layout as mdg_vo_compress, 0 <= rank <= hd.
 * A NaN in row k of one head's W_o or o' gives NaN in e[h][k] (and dnorm2[h][k]) of that head alone; a NaN in one kv head's W_v or
 * v' reaches every channel of that group's heads and no other group; a NaN in cov_x reaches everything; MDG_OK in every case.
 * No atomics, every sum in a fixed order: bit-identical from run to run, and e is the same bits with and without dnorm2.
 * ws: mdg_vo_output_error_ws_bytes(d, n_heads, n_kv, hd, rank) bytes (vo_err_layout in csrc/vo_err.hip: with n = hd + rank, T
 * [n_kv][n][d], the two Grams, the tile-column partials).
 * Status: there is no factorisation -- the call only enqueues, never synchronises, and is the same inside and outside
 * mdg_deferred_status_begin / _end.  MDG_ERR_BAD_ARG for a null pointer, an unsupported head layout or rank, a leading dimension
 * that is too small (ldc, ld_wv, ld_v < d; ld_wo < n_heads hd; ld_o < n_heads rank), an unsupported dtype, a workspace that is too
 * small, or rank > 0 without v_new / o_new. */
size_t mdg_vo_output_error_ws_bytes(int64_t d, int n_heads, int n_kv, int hd, int rank);
int mdg_vo_output_error(const double* cov_x, int64_t d, int64_t ldc, const void* Wv, int64_t ld_wv, const void* Wo, int64_t ld_wo,
                        int w_dtype, int n_heads, int n_kv, int hd, int rank, const void* v_new, int64_t ld_v, const void* o_new,
                        int64_t ld_o, int new_dtype, double* e /* [n_heads][d] */, double* dnorm2 /* [n_heads][d], optional */,
                        void* ws, size_t ws_bytes, void* stream);
/* What the V/O truncation costs the attention output at EVERY rank (added under ABI 9).  Reads the eigen-decomposition the LAST
 * mdg_vo_compress call left in its workspace vo_ws (same shapes), as mdg_vo_spectrum does.  Per kv head g, r = 0 .. hd:
 *     grouped:  c_i = max(lambda_i, 0) sum_{h in g} ||W_o,h v_i||^2 ,  (lambda_i, v_i) of G = W_v,g (C + rho I) W_v,g^T, descending
 *     MHA (n_kv == n_heads):  c_i = max(lambda2_i, 0), the second SVD's spectrum (W_o is then not read)
 *     curve[g][r] = sum_{i >= r} c_i
 * accumulated from the tail, so the curve is non-increasing entry by entry and curve[g][hd] = +0.0 exactly.  For the fp64 factors of
 * rank r, sum over the group's heads and channels of (e + rho dnorm2) of mdg_vo_output_error equals curve[g][r] in exact
 * arithmetic.  Grouped: it is the error of the REFERENCE'S choice of subspace (which ignores W_o), not the minimum over all
 * rank-r factorisations.  ||W_o,h v_i||^2 as the column norms of W_o,h V_g (fp64 GEMM): accurate to (hd + d) 2^-53 relative to
 * itself.  ws: mdg_vo_rank_curve_ws_bytes bytes (grouped; vo_curve_layout in csrc/vo_err.hip), 0 (MHA; ws may then be NULL).
 * A NaN eigenvalue stays a NaN.  Only enqueues.  MDG_ERR_BAD_ARG for a null pointer, an unsupported head layout or dtype,
 * ld_wo < n_heads hd, or a workspace that is too small. */
size_t mdg_vo_rank_curve_ws_bytes(int64_t d, int n_heads, int n_kv, int hd);
int mdg_vo_rank_curve(const void* vo_ws, size_t vo_ws_bytes, const void* Wo, int64_t ld_wo, int w_dtype, int64_t d, int n_heads,
                      int n_kv, int hd, double* curve /* [n_kv][hd + 1] */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ sqrt_M (compression_utils.py:15-55)
 * root = V diag(sqrt(max(lambda + ridge*scale, 0))) V^T, inv_root (optional) with the 1e-12 clamp;
 * scale = max eigenvalue if scaled else 1.  n <= 128 and even, batched.  evals_out optional [batch][n]
 * (pre-ridge, descending) for the caller's diagnostics.  SYNCHRONISES.
 * Only the lower triangle of M is read.  A matrix with a NaN or Inf there: MDG_ERR_NO_CONVERGE with the non-finite-input message
 * of mdg_syevj_batched (deferred-status mode: from mdg_deferred_status_decode), its root, inv_root and evals_out all NaN, the
 * batch's other matrices computed as usual.  Scale: as mdg_syevj_batched; `ridge` and the 1e-12 clamp are absolute unless scaled. */
int mdg_sqrt_psd_small(const double* M, int64_t n, int64_t batch, double ridge, int scaled, double* root,
                       double* inv_root, double* evals_out, void* ws, size_t ws_bytes, void* stream);
size_t mdg_sqrt_psd_small_ws_bytes(int64_t n, int64_t batch);
/* The same function for one n x n matrix of any size (the d_model-sized call of compress_vo.py:44).
 * evals_out == NULL and scaled == 0 (the plain sqrt_M(M, ridge) call): sqrt(M + ridge I) and its inverse by the coupled
 * Newton-Schulz iteration -- three n^3 fp64-MFMA GEMMs per step, ~25 steps at n = 4096 -- valid because the reference's
 * clamps never bind on a PSD input; an input it cannot certify (indefinite) falls through to the eigen route.
 * Otherwise: two-sided block Jacobi on 64-wide blocks -- 128x128 pair sub-problems through the LDS Jacobi kernel,
 * rotations applied by batched fp64-MFMA GEMMs, blocks rotated round-robin; evals_out [n], UNSORTED (pre-ridge).
 * Once ||off||_F <= 1e-13 ||A||_F the accumulated V takes one Newton-Schulz step towards its polar factor,
 * V (3 I - V^T V) / 2 (orthogonality defect delta -> delta^2), V^T M V is formed afresh and the sweeps go on until the threshold
 * is met a second time -- the one confirming sweep -- so the result does not carry the drift of the earlier sweeps.  If that
 * does not happen within 30 sweeps in all: MDG_ERR_NO_CONVERGE.
 * Not used by this engine's own VO stage (DESIGN.md "Identities").  SYNCHRONISES once per step / sweep.
 * Only the lower triangle of M is read (ld >= n, any alignment); M is not written; ws may hold anything.  Calls are
 * bit-reproducible: every sum that steers a route (||A||_F^2, the Newton-Schulz residual, the off-norm) is formed in a fixed
 * order, no floating-point atomics -- the same input gives the same bits of root, inv_root and evals_out on every call and stream.
 * A NaN or Inf in the lower triangle is found by the load pass of either route: MDG_ERR_NO_CONVERGE with the message
 * "mdg_sqrt_psd_large: the input holds non-finite values (NaN or Inf)" (as mdg_sqrt_psd_small's), root, inv_root and evals_out
 * all NaN.  Block Jacobi then runs no sweep; the Newton-Schulz route reads the flag with its first residual, after one GEMM
 * and one shift pass, and does not go on to the eigen route.  MDG_ERR_BAD_ARG (nothing launched, outputs untouched) for a null M / root / ws, n <= 0, ld < n,
 * or ws_bytes < mdg_sqrt_psd_large_ws_bytes(n) -- the larger of the two routes' layouts (newton_layout, jacobi_layout in csrc/eigh.hip).
 * Accuracy (tests/test_gpu_sqrt_large.py, against long double): both routes within max(4 e_ref, n 2^-52) of the truth in the
 * relative Frobenius norm, e_ref the larger fp64 CPU error of LAPACK's eigh formula and of the route's own algorithm.
 * That is what was measured.  The CONTRACT of the eigen route is what its stopping rule implies: it returns the function of a
 * matrix B with ||A - B||_F <= 4 tau ||A||_F, tau = 1e-13 (the off-norm at the stop, and a factor 4 for the rounding of the
 * rebuild), and for PSD A, B  ||A^1/2 - B^1/2||_F <= ||A - B||_F / (lambda_min(A)^1/2 + lambda_min(B)^1/2), hence
 *     ||root - truth||_F <= 4 tau ||A||_F / (2 sqrt(max(lambda_min, 0) + ridge))      (ridge times lambda_max if scaled),
 * also asserted by that test on every eigen-route case (largest share seen: DESIGN.md "Eigensolver accuracy"). */
size_t mdg_sqrt_psd_large_ws_bytes(int64_t n);
int mdg_sqrt_psd_large(const double* M, int64_t n, int64_t ld, double ridge, int scaled, double* root,
                       double* inv_root, double* evals_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ compressed-model attention
 * Rotary embedding of a compressed layer's q or k projection, fused with the gather of cos/sin by the layer's rotary
 * mask, the optional Qwen3 masked RMSNorm, and the transpose into the layout attention consumes.  Replaces the eager
 * chains apply_rotary_pos_emb(..., rotary_mask) (src/patchers/LlamaRebuild.py:153-176) and _masked_rms_norm
 * (src/patchers/DenseQwenRebuild.py:262-286).
 *   x    [B*T, n_heads*r] rows of pitch ld_x elements (the projection output, token-major), dtype bf16 / f16 / f32
 *   out  [B, n_heads, T, r] contiguous, same dtype
 *   cos, sin  [Bc, T, hd] same dtype; cs_batch_stride elements between batches, 0 = one table shared by every batch
 *   mask int64 [n_kv, r] -- kept column j of (kv) head g is original column mask[g, j] in [0, hd); query heads use the
 *        row of their kv head (h / (n_heads / n_kv)); the two halves [0, r/2) and [r/2, r) are the rotate_half partners.
 *        NULL = identity (then r must equal hd).  Out-of-range entries are clamped (memory safety only).
 *   norm_w  [hd] same dtype or NULL: y = dtype(norm_w[mask] * (float(x) * rsqrt(mean(float(x)^2 over the r kept columns)
 *        + eps))) is applied before the rotation.
 * Every product and the sum are rounded to the element dtype one op at a time, as torch's eager expression does: the
 * rotation is bit-identical to it; the fp32 sum of squares of the norm is taken in a fixed (16-lane tree) order. */
int mdg_rope_gather(const void* x, int dtype, int64_t ld_x, int64_t B, int64_t T, int n_heads, int n_kv, int r, int hd,
                    const void* cos, const void* sin, int64_t cs_batch_stride, const int64_t* mask,
                    const void* norm_w, double eps, void* out, void* stream);

/* What mdg_rope_gather would launch for the same arguments: its whole dispatch, computed from the shapes, the dtype and the
 * operands' ADDRESSES taken as integers.  Nothing is dereferenced and no device is needed, so the pointers may be synthetic
 * (only their alignment and, for mask / norm_w, whether they are NULL matter).  mdg_rope_gather calls the same function and
 * launches exactly this plan.  Refuses what mdg_rope_gather refuses (except NULL operands); B == 0 or T == 0 gives all zeros.
 * plan[MDG_ROPE_PLAN_LEN]:
 *    [0] route      0 = direct kernel (rope_gather_kernel<DT, VEC, NORM, HPT>), 1 = LDS tile kernel (rope_tile_kernel<DT, NORM, HALF_EVEN>)
 *    [1] hpt        query heads of one kv head per thread group: 4, 2 or 1 (the tile kernel's CH)
 *    [2] vec        elements per pack of the direct kernel, 4 or 2; 1 on the tile route
 *    [3] norm       1 when norm_w is given
 *    [4] half_even  tile route: r / 2 is even (HALF_EVEN); 0 on the direct route
 *    [5] iters      direct route: passes over a row, ceil(r / 2 / (16 * vec)); > 1 with norm = the sum-of-squares pre-pass; 0 on the tile route
 *    [6] one_shot   direct route: a cos / sin row is one 16-byte load per lane and is staged through registers
 *    [7] cs_vec16   cos / sin rows are 16-byte aligned and a multiple of 16 bytes long
 *    [8] nw_vec16   norm_w is given and 16-byte aligned
 *    [9] tt         tokens per workgroup: 64 / hpt on the direct route; on the tile route halved from there until the tile fits 64 KB of LDS
 *   [10] wi  [11] wo  tile route: chunk bytes of the copies in / out (16, 8, 4 or 2, never below the element size); 0 on the direct route
 *   [12] hp1        tile route: ceil(r / 4) == 1, the row index is the item index (no magic division)
 *   [13] lds        dynamic LDS bytes of the launch   [14] lds_attr  1 when they exceed 64 KB (the launch raises the kernel's limit first)
 *   [15..17] grid x, y, z = (8 * n_kv, ceil(n_tiles / 8), (n_heads / n_kv) / hpt); 256 threads per workgroup
 *   [18] t_tiles    token tiles per batch, ceil(T / tt)   [19] n_tiles = B * t_tiles */
#define MDG_ROPE_PLAN_LEN 20
int mdg_rope_gather_plan(const void* x, int dtype, int64_t ld_x, int64_t B, int64_t T, int n_heads, int n_kv, int r, int hd,
                         const void* cos, const void* sin, int64_t cs_batch_stride, const int64_t* mask,
                         const void* norm_w, double eps, void* out, void* stream, int64_t* plan);

/* ------------------------------------------------------------------ post-RoPE rows for the calibration statistics
 * Rotary embedding of a projection output in its own layout: the rows q', k' the model's attention really multiplies
 * (apply_rotary_pos_emb), for sigma_q' / sigma_k'.  Stands for the post-RoPE hook variant the reference carries but disabled:
 * src/adapters/LlamaAdapter.py:46-69 (patched_attn_forward) and 305-325 (_attn_hook).  Additive entry, ABI version unchanged.
 *   x    [B*T, n_heads*hd] rows of pitch ld_x elements, last dimension contiguous, dtype bf16 / f16 / f32
 *   cos, sin  [Bc, T, hd] same dtype, FULL width (the two halves need not be equal); cs_batch_stride elements between batches,
 *        0 = one table shared by every batch
 *   out  [B*T, n_heads*hd] rows of pitch ld_out elements, same dtype; elements of a row beyond n_heads*hd are not written
 *   out[t, h, c] = dt( dt(x[t, h, c] * cos[t, c]) + dt(r[t, h, c] * sin[t, c]) ),  r[c] = -x[c + hd/2] for c < hd/2, x[c - hd/2] otherwise
 * Every product and the sum are formed in fp32 and rounded to the element dtype one op at a time, without FMA contraction, as
 * torch's eager expression does: the result is bit-identical to it.  Each element of x is read once and each element of out
 * written once; 16-byte loads and stores when x, out, cos, sin are 16-byte aligned, ld_x, ld_out and cs_batch_stride are
 * multiples of 16 bytes of elements and hd/2 is one too, element-wise otherwise.  No atomics, no dependence on launch order.
 * MDG_ERR_BAD_ARG (with a message, before any device work): unknown dtype, negative extent, n_heads <= 0, hd odd, < 2 or > 256,
 * ld_x or ld_out < n_heads*hd, a batch stride in (0, T*hd), a NULL operand of a non-empty call, and an out whose byte range
 * (pitch included) intersects that of x -- the model still needs x.  B == 0 or T == 0 launches nothing. */
int mdg_rope_rows(const void* x, int dtype, int64_t ld_x, int64_t B, int64_t T, int n_heads, int hd, const void* cos,
                  const void* sin, int64_t cs_batch_stride, void* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------ within-sequence, shift-invariant Q/K statistic
 * Softmax ignores any part of a logit that depends on the query alone.  Dropping the columns D of a head changes logit (i, j)
 * by e_ij = q'_iD . k'_jD; what the attention probabilities of query i see is the VARIANCE of e_ij over the keys j of i's own
 * sequence, and summed over the queries of the calibration set that is 1^T P_h[D,D] 1 with, per query head h,
 *   P_h = sum over sequences s of  G^q_{s,h} (.) ( G^k_{s,kv} - m m^T / T ),   G^q = Q'^T Q', G^k = K'^T K', m = K'^T 1
 * ((.): entry-wise product; kv = h / (n_heads / n_kv)).  P_h is positive semidefinite.  Additive entries, ABI version unchanged.
 *   q  [B*T, n_heads*hd] rows of pitch ld_q elements, k [B*T, n_kv*hd] rows of pitch ld_k, last dimension contiguous, dtype
 *      bf16 / f16 / f32 (widened to fp64 exactly on load): the layouts mdg_rope_rows writes.  Rows b*T .. b*T+T-1 are sequence b.
 *   pair, pair_raw  [n_heads, hd, hd] fp64 contiguous, ACCUMULATED INTO; pair_raw may be NULL.  For b = 0 .. B-1 in ascending
 *      order   pair[h] += G^q_{b,h} (.) (G^k_{b,kv} - m m^T / T),   pair_raw[h] += G^q_{b,h} (.) G^k_{b,kv};  nothing is normalised.
 *   ws  mdg_qk_pair_ws_bytes(B, n_heads, hd, pair_raw != NULL) bytes, 8-byte aligned (seq_layout in csrc/qk_seq.hpp: one slot per
 *       sequence and head, a second set with pair_raw).
 * hd <= 128: one workgroup per (sequence, query head) holds both 128x128 Grams in accumulator registers, on
 * v_mfma_f64_16x16x4_f64; a second kernel adds the per-sequence products onto pair, one addition per sequence in ascending b.
 * So one call over B sequences gives the bits of B single-sequence calls in that order, and every run gives the same bits: no
 * atomics, every sum in a fixed order.  Both triangles of every output matrix are written and are equal to the bit.  16-byte
 * loads when q (k) is 16-byte aligned and ld_q (ld_k) and hd are multiples of 16 bytes of elements, element-wise otherwise.
 * A non-finite element of q in head h reaches pair[h] and pair_raw[h] only; one of k in kv head v reaches the heads of group v only.
 * At T == 1 the centred term is exactly zero, so pair receives +0.
 * Accuracy (u = 2^-53; no overflow or underflow).  Products of two bf16, f16 or f32 values are exact in fp64, so per sequence:
 * a Gram entry is a chain of T additions, |err G_ab| <= T u sqrt(G_aa G_bb); a column sum m_a is a chain of at most T additions,
 * and with |m_a| <= sqrt(T G^k_aa) the product, the division by T and the chain errors give |err (m_a m_b / T)| <= (2T + 2) u K_ab,
 * K_ab = sqrt(G^k_aa G^k_bb); the subtraction adds u K_ab (|S_ab| <= K_ab), so |err S_ab| <= (3T + 3) u K_ab; the Hadamard
 * product adds the query Gram's T u and one rounding: (4T + 4) u sqrt(G^q_aa G^q_bb) K_ab per sequence.  The fold onto a pair
 * that held zero rounds B - 1 times a running sum of at most sum_s sqrt(G^q_aa G^q_bb) K_ab.  With the second-order terms,
 *   | pair[h][a,b] - exact | <= (4T + B + 8) u  sum_s sqrt(G^q_{s,aa} G^q_{s,bb}) sqrt(G^k_{s,aa} G^k_{s,bb}),
 * and the same bound holds for pair_raw.  A pair that held p on entry adds B u |p[a,b]|.
 * Only enqueues.  MDG_ERR_BAD_ARG (with a message, before any device work): unknown dtype, hd < 1 or > 128, n_heads <= 0,
 * n_kv <= 0 or n_heads % n_kv != 0, negative extent, ld_q < n_heads*hd or ld_k < n_kv*hd, a NULL q, k, pair or ws of a non-empty
 * call, ws_bytes below mdg_qk_pair_ws_bytes.  B == 0 or T == 0 launches nothing and returns MDG_OK. */
size_t mdg_qk_pair_ws_bytes(int64_t B, int n_heads, int hd, int want_raw);
int mdg_qk_pair_accum(const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T, int n_heads,
                      int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ causal Q/K statistic
 * In a causal decoder query i of a sequence multiplies the keys j <= i only, and its softmax normalises over n_i = i + 1 of them.
 * Dropping the columns D of a head changes logit (i, j) by e_ij = q'_iD . k'_jD; what the attention probabilities of query i see is
 * the variance of e_ij over the keys j <= i.  Summed over the queries that is 1^T P^c_h[D,D] 1 with, per query head h,
 *   K_i = sum_{j<=i} k'_j k'_j^T,   m_i = sum_{j<=i} k'_j,   C_i = K_i / n_i - m_i m_i^T / n_i^2,
 *   P^c_h     = sum over sequences s, tokens i of  (q'_i q'_i^T) (.) C_i          1^T P^c_h[D,D] 1     = sum_s sum_i Var_{j<=i}(e_ij)
 *   P^c_raw,h = sum over sequences s, tokens i of  (q'_i q'_i^T) (.) K_i / n_i    1^T P^c_raw,h[D,D] 1 = sum_s sum_i mean_{j<=i}(e_ij^2)
 * ((.): entry-wise product; k' of kv head h / (n_heads / n_kv)).  P^c_h is positive semidefinite.  Additive entries, ABI version
 * unchanged.  Arguments as mdg_qk_pair_accum:
 *   q  [B*T, n_heads*hd] rows of pitch ld_q elements, k [B*T, n_kv*hd] rows of pitch ld_k, last dimension contiguous, dtype
 *      bf16 / f16 / f32 (widened to fp64 exactly on load): the layouts mdg_rope_rows writes.  Rows b*T .. b*T+T-1 are sequence b,
 *      row b*T its position 0.
 *   pair, pair_raw  [n_heads, hd, hd] fp64 contiguous, ACCUMULATED INTO; pair_raw may be NULL.  For b = 0 .. B-1 in ascending order
 *      pair[h] += (sequence b's sum over i of the first expression), pair_raw[h] += (the second); nothing is normalised.
 *   ws  mdg_qk_causal_ws_bytes(B, n_heads, hd, pair_raw != NULL) bytes, 8-byte aligned (seq_layout in csrc/qk_seq.hpp: one slot per
 *       sequence and head, a second set with pair_raw).
 * The expression evaluated, per sequence, for i = 0 .. T-1 in ascending order, per entry (a, b), in fp64 (fma: one rounding):
 *   m_i[a] = m_{i-1}[a] + k_i[a]           r = 1.0 / (double)n_i  (correctly rounded)
 *   K = fma(k_i[a], k_i[b], K)             w = (q_i[a] * q_i[b]) * r                      t = fma(-(m_i[a] * m_i[b]), r, K)
 *   S = fma(w, t, S)                       S_raw = fma(w, K, S_raw)
 * from K = S = S_raw = 0, m_{-1} = 0: S accumulates q_a q_b (K - m_a m_b r) r.  Then pair[h][a,b] += S, pair_raw[h][a,b] += S_raw.
 * hd <= 128: one workgroup per (sequence, query head) keeps K, S and S_raw in registers on the vector ALU (the recurrence is
 * serial in the token and element-wise in the entry); a second kernel adds the per-sequence sums onto pair, one addition per
 * sequence in ascending b.  So one call over B sequences gives the bits of B single-sequence calls in that order, and every run
 * gives the same bits: no atomics, every sum in a fixed order.  Every operation above is symmetric in (a, b), so both triangles
 * of every output matrix are written and are equal to the bit.  16-byte loads when q (k) is 16-byte aligned and ld_q (ld_k) and hd
 * are multiples of 16 bytes of elements, element-wise otherwise.  A non-finite element of q in head h reaches pair[h] and
 * pair_raw[h] only; one of k in kv head v reaches the heads of group v only.  At T == 1, t = fma(-k_a k_b, 1, k_a k_b) = 0, so
 * pair receives +0.
 * Accuracy (u = 2^-53; no overflow or underflow; (4T + B + 8) u < 2^-20).  Write kappa_i = sqrt(K_i[a,a] K_i[b,b]) for the exact
 * prefix Gram, and   A_h[a,b] = sum_s sum_i |q'_ia q'_ib| kappa_i / n_i.   Products of two bf16, f16 or f32 values are exact in
 * fp64.  To first order in u, at token i with n = n_i:
 *   K       a chain of n fused additions of exact products, sum_j |k_ja k_jb| <= kappa_i:        |err K|  <=  n u kappa_i
 *   m_a     a chain of n additions, |m_a| <= sum_j |k_ja| <= sqrt(n K_i[a,a]):                   |err m_a| <= n u sqrt(n K_i[a,a])
 *   mm      two such factors and one rounding:                                                    |err mm| <= (2n + 1) u n kappa_i
 *   t       exact value K - m_a m_b / n = n C_i[a,b], |n C_i[a,b]| <= kappa_i (C_i is a covariance with n C_i[a,a] <= K_i[a,a]);
 *           err K, err mm / n, r's rounding on |m_a m_b| / n <= kappa_i, and the fma's own:      |err t|  <= (3n + 3) u kappa_i
 *   w       q_a q_b exact, r and the product round:                                               |err w|  <= 2 u |q_a q_b| / n
 *   w t     |err| <= (3n + 5) u |q_a q_b| kappa_i / n;      w K:  |err| <= (n + 2) u |q_a q_b| kappa_i / n
 * Summed over the T tokens of a sequence these give (3T + 5) u A_s; each of the T fused accumulations rounds a partial sum of
 * magnitude <= A_s, T u A_s more: (4T + 5) u A_s per sequence for pair, (2T + 2) u A_s for pair_raw.  The fold onto a pair that
 * held zero rounds B - 1 times a running sum of at most A.  With the second-order terms (a factor 1 + 2^-19 under the condition
 * above, inside the constant),
 *   | pair[h][a,b] - exact |  <=  (4T + B + 8) u A_h[a,b],        c = 4, c' = 8,
 * and the same bound holds for pair_raw.  The scale is sqrt(K_aa K_bb), not |C_ab|: the centring cancels.  A pair that held p on
 * entry adds B u |p[a,b]|.
 * Only enqueues.  MDG_ERR_BAD_ARG (with a message, before any device work): unknown dtype, hd < 1 or > 128, n_heads <= 0,
 * n_kv <= 0 or n_heads % n_kv != 0, negative extent, ld_q < n_heads*hd or ld_k < n_kv*hd, a NULL q, k, pair or ws of a non-empty
 * call, ws_bytes below mdg_qk_causal_ws_bytes.  B == 0 or T == 0 launches nothing and returns MDG_OK. */
size_t mdg_qk_causal_ws_bytes(int64_t B, int n_heads, int hd, int want_raw);
int mdg_qk_causal_accum(const void* q, int64_t ld_q, const void* k, int64_t ld_k, int dtype, int64_t B, int64_t T, int n_heads,
                        int n_kv, int hd, double* pair, double* pair_raw, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ fused attention forward for compressed heads
 * The attention product of a compressed layer: q/k heads of width r_qk and v/o heads of width r_vo, each arbitrary per layer,
 * flash-style in one kernel (csrc/attn.hip); nothing of size T x S touches HBM.  Additive entry, ABI version unchanged.
 *   q    [B, n_heads, T, r_qk] contiguous: what mdg_rope_gather writes
 *   k    [B, n_kv, S, r_qk], v [B, n_kv, S, r_vo]: last dimension contiguous, batch / head / token strides in elements (a cache
 *        may hand back views of longer buffers)
 *   out  [B*T, n_heads*r_vo] rows of pitch ld_out elements: the token-major rows o_proj reads; elements of a row beyond
 *        n_heads*r_vo are not written
 *   dtype  MDG_BF16 or MDG_F16, of all four
 *   out[b, i, h, :] = softmax_j( scale * q[b, h, i, :] . k[b, g, j, :] ) v[b, g, :, :],   g = h / (n_heads / n_kv)
 * over the keys query i sees: with causal != 0 the keys j <= i + (S - T) (prefill S == T, chunked prefill, decode T == 1), every
 * key otherwise.  A query that sees no key (S == 0) gets zeros.
 * Arithmetic: logits in fp32 from exact element products on v_mfma_f32_32x32x16_{bf16,f16}; online softmax with running maximum
 * and sum in fp32, scale * log2(e) folded into one multiply, exp2; the probabilities rounded to the element dtype for the second
 * product; the output accumulated in fp32, divided by the fp32 sum and rounded once.  With u the element type's unit roundoff
 * (2^-9 bf16, 2^-11 f16) and |scale * logit| <= 20:   |out - exact| <= 4 u max_j |v[b, g, j, c]|   entry-wise (u max|v| from
 * rounding the probabilities, u |out| from rounding the output, fp32 accumulation and exp2 below u together; the 4 is twice that).
 * Widths that are no multiple of the MFMA k-step or tile are zero-padded in LDS and registers; the caller pads nothing.  Aligned
 * 16-byte loads of an operand whose base and strides are multiples of 16 bytes; otherwise a narrower path (16-byte loads at the
 * elements' 2-byte alignment, a row's last partial chunk element by element), chosen per operand on the host.  No atomics; every
 * run gives the same bits.  Only enqueues.
 * Decode (T * n_heads / n_kv <= 32) has a schedule of its own: mdg_attn_decode below; here it is correct, not fast.
 * Bool masks (padded batches): mdg_attn_fwd_masked / mdg_attn_decode_masked below.
 * Out of scope: sliding windows, additive float masks, dropout, returning attention weights, a backward pass, fp32 inputs.
 * MDG_ERR_BAD_ARG (with a message, before any device work): a dtype other than bf16 / f16, negative extent, n_heads % n_kv != 0,
 * r_qk odd or outside 2..256, r_vo outside 1..256, causal with S < T, a token stride below the row width, ld_out < n_heads*r_vo,
 * a scale that is not finite and positive, a NULL operand of a non-empty call, an out whose byte range (pitch included)
 * intersects that of q, k or v.  B == 0 or T == 0 launches nothing and returns MDG_OK. */
int mdg_attn_fwd(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads, int n_kv,
                 int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                 int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, double scale, int causal, void* out,
                 int64_t ld_out, void* stream);

/* ------------------------------------------------------------------ split-key (flash-decoding) attention for compressed heads
 * mdg_attn_fwd's product on a decode schedule (csrc/attn_decode.hip), for T * G <= 32 with G = n_heads / n_kv: every query row of a
 * kv head fits the 32 query columns of one MFMA tile (column c = query c / G, head of the group c % G), so one read of a kv head's K
 * and V serves the whole group.  T == 1 at any group up to 32, short speculative or chunked steps, MHA up to T == 32.  Operands,
 * dtype, widths, strides, causal rule (query i sees keys j <= i + S - T), out layout and error bound are mdg_attn_fwd's.  Additive
 * entries, ABI version unchanged.
 * The keys are cut into `splits` contiguous chunks of L = 64 * ceil(ceil(S / 64) / splits) keys; one workgroup per (batch, kv head,
 * chunk) runs the online softmax over its chunk and writes an unnormalised fp32 partial to the caller's workspace
 *   ws [B][n_heads][T][splits][RP + 4] floats, RP = r_vo rounded up to 4: O_s at [0, RP), m_s (log2 domain) at [RP], l_s at [RP + 1];
 * a second kernel on the same stream forms  M = max_s m_s,  out = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s  in fp32 and rounds
 * once.  A chunk with no admitted key for a query (an empty range: splits may exceed the key tiles; or one wholly beyond the causal
 * limit) has m_s = -inf, l_s = 0, O_s = 0 and contributes exactly nothing; a row with no admitted key at all (S == 0) gets zeros.
 * Two launches ordered by the stream; no counters, flags or atomics; every run gives the same bits.  The workspace holds nothing
 * between calls and need not be initialised.  Bound, with |scale * logit| <= 20:  |out - exact| <= 4 u max_j |v[b, g, j, c]|
 * entry-wise, as for mdg_attn_fwd: the partials and the combine are fp32, the only roundings to the element type are the
 * probabilities and the final store.
 *   mdg_attn_decode_ws_bytes  the workspace size: B * T * n_heads * splits * (RP + 4) * 4 (0 when an argument is not positive)
 *   mdg_attn_decode_splits    the default split count, a pure host function: enough workgroups to give each of n_cu compute units
 *                             one, but no chunk under 4 key tiles (one for each wave of the workgroup):
 *                             clamp(n_cu / (B * n_kv), 1, min(ceil(ceil(S / 64) / 4), 256)); 1 for arguments that are not positive
 * MDG_ERR_BAD_ARG (with a message, before any device work): what mdg_attn_fwd refuses, and T * G > 32, splits outside 1..256, a
 * NULL, short (ws_bytes < mdg_attn_decode_ws_bytes) or not 16-byte aligned workspace, a workspace that overlaps q, k, v or out.
 * B == 0 or T == 0 launches nothing and returns MDG_OK. */
int64_t mdg_attn_decode_ws_bytes(int64_t B, int64_t T, int n_heads, int r_vo, int splits);
int mdg_attn_decode_splits(int64_t B, int n_kv, int64_t S, int n_cu);
int mdg_attn_decode(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads, int n_kv,
                    int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, double scale, int causal, int splits,
                    void* ws, int64_t ws_bytes, void* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------ bool masks on both attention kernels (padded batches)
 * mdg_attn_fwd / mdg_attn_decode with a bool mask tensor, taken as a framework hands it over (Transformers' sdpa_mask: the causal
 * rule ANDed with the padding columns, expanded): nothing is inspected on the host, nothing synchronises, no form is assumed.
 * Additive entries, ABI version unchanged; the unmasked entries and their kernels are as they were.
 *   mask  logical [B, Hm, T, S], Hm == 1 (one mask for every head) or Hm == n_heads; ONE BYTE per element, non-zero admits; batch,
 *         head and query strides in BYTES, any of them may be 0 (an expanded axis); the key stride is 1
 * Key j is admitted for query (b, h, i) iff mask[b, Hm == 1 ? 0 : h, i, j] != 0 and, with causal != 0, also j <= i + S - T.  A
 * query with no admitted key gets zeros (the rule of S == 0; -inf - -inf is never formed).  A masked logit is set to -inf before
 * the running maximum, where the causal rule sets it, so its probability is exactly 0 and a masked key's k row is never seen (it may
 * hold Inf or NaN); v at masked keys must be FINITE (0 x NaN, as for torch's sdpa).  Everything else -- operands, widths, strides,
 * out rows, arithmetic, determinism, no atomics -- is the unmasked entry's, and |out - exact| <= 4 u max_j |v[b, g, j, c]| holds
 * with the maximum over the admitted keys.
 * Prefill reads a tile summary first:
 *   mdg_attn_mask_summary_bytes  B * Hm * ceil(T / 32) * ceil(S / 64) (0 when an argument is not positive): a pure host function
 *   mdg_attn_mask_summary        one pass over the mask writes summary[B][Hm][ceil(T/32)][ceil(S/64)] bytes: 0 = no element of the
 *                                32-query x 64-key tile admitted, 1 = every element, 2 = mixed; positions beyond T or S are
 *                                ignored.  4-byte loads when the mask's base and strides are multiples of 4, byte loads otherwise.
 *   mdg_attn_fwd_masked          mdg_attn_fwd's arguments, then the mask and its summary.  Enqueue mdg_attn_mask_summary on the same
 *                                stream first: two launches ordered by the stream, no counters, no flags.  A key tile that admits
 *                                nothing for all units of a workgroup is not staged (left padding; the causal triangle when
 *                                causal == 0 and the rule lives in the mask); a wave skips a tile that admits nothing for its unit,
 *                                runs the unmasked code on a tile that admits everything, and reads the mask (4-byte loads when
 *                                base and strides allow, chosen on the host) only for a mixed tile.
 *   mdg_attn_decode_masked       mdg_attn_decode's arguments, then the mask: column c reads the mask row of query c / G (head
 *                                c % G of the group when Hm == n_heads) directly, S bytes per row; no summary, no extra
 *                                workspace; every key tile is still loaded.  The combine kernel is mdg_attn_decode's.
 * MDG_ERR_BAD_ARG (with a message, before any device work): what the unmasked entry refuses, and Hm not in {1, n_heads}, a negative
 * mask stride, a NULL mask or summary of a non-empty call, a summary shorter than mdg_attn_mask_summary_bytes, a mask or summary
 * (decode: a mask or workspace) whose byte span -- computed with the strides, an axis of stride 0 counting extent 1 -- intersects
 * out's.  mdg_attn_mask_summary refuses a negative extent or stride, Hm < 1, a NULL or short summary, a summary inside the mask.
 * Out of scope: additive float masks, sliding windows, one summary for all layers of a forward, skipping whole cache chunks in
 * decode, varlen / packed layouts without a mask tensor, a backward pass. */
int64_t mdg_attn_mask_summary_bytes(int64_t B, int Hm, int64_t T, int64_t S);
int mdg_attn_mask_summary(const void* mask, int64_t B, int Hm, int64_t T, int64_t S, int64_t mask_batch_stride,
                          int64_t mask_head_stride, int64_t mask_query_stride, void* summary, int64_t summary_bytes, void* stream);
int mdg_attn_fwd_masked(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads,
                        int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                        int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, double scale, int causal, void* out,
                        int64_t ld_out, void* stream, const void* mask, int Hm, int64_t mask_batch_stride,
                        int64_t mask_head_stride, int64_t mask_query_stride, const void* summary, int64_t summary_bytes);
int mdg_attn_decode_masked(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads,
                           int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                           int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, double scale, int causal,
                           int splits, void* ws, int64_t ws_bytes, void* out, int64_t ld_out, void* stream, const void* mask,
                           int Hm, int64_t mask_batch_stride, int64_t mask_head_stride, int64_t mask_query_stride);

/* ------------------------------------------------------------------ multi-GPU (the reference is single-process,
 * its unit of independent work is the layer loop of src/run_modegpt.py:107-156)
 * Layers shard over the GPUs of a node, one process per GPU, no data-path exchange until the end: ONE all-gather of the
 * ranks' packed per-layer records (modegpt_amd/sharding.py documents the record: header with shapes, rotary mask, bf16
 * payload; every rank pads to the same bytes_per_rank).  This engine's driver runs that step through torch.distributed
 * (backend "nccl" = RCCL over xGMI); the entry points below are the same step for a host without torch.  RCCL is resolved
 * with dlopen("librccl.so.1") on first use -- no link-time dependency.
 *   mdg_comm_unique_id   rank 0 fills id128 (128 bytes) and hands it to the other ranks by the host's own means (file, env, MPI)
 *   mdg_comm_init        every rank, after hipSetDevice(its GPU): *comm receives the communicator
 *   mdg_allgather_layers recv[r * bytes_per_rank ...] = rank r's send buffer, for every r; device pointers; enqueued on `stream`
 *   mdg_comm_destroy     releases the communicator (NULL is accepted) */
int mdg_comm_unique_id(void* id128);
int mdg_comm_init(void** comm, int world, int rank, const void* id128);
int mdg_allgather_layers(const void* send, void* recv, size_t bytes_per_rank, void* comm, void* stream);
int mdg_comm_destroy(void* comm);

/* ------------------------------------------------------------------ utilities
 * out_bf16[j, i] = bf16(in_f64[i, j])  (transpose + cast with torch's double->float->bf16 rounding) */
int mdg_cast_transpose_f64_bf16(const double* in, int64_t rows, int64_t cols, int64_t ld_in, void* out,
                                int64_t ld_out, void* stream);
/* Raw fp64 MFMA issue-rate probe used by bench.py to state the measured peak next to the spec:
 * returns TFLOP/s over `iters` back-to-back v_mfma_f64_16x16x4_f64 per wave on every CU.  SYNCHRONISES. */
int mdg_probe_mfma_f64(int iters, double* tflops, void* stream);
/* The same for the int8 pipe: TOP/s of back-to-back v_mfma_i32_32x32x32_i8 from registers, two waves per SIMD on every CU, the
 * operands changing from one MFMA to the next -- all zero (random_operands = 0: nothing toggles, the pipe runs at full clock,
 * ~0.97 of the 5 POP/s nominal peak) or random bytes (random_operands = 1: the board sits at its power cap and the clock
 * gives way, ~0.68 of nominal on an MI355X -- the ceiling of ANY int8 kernel on random data, before a single byte is loaded).
 * bench.py states both next to the kernel's achieved rate.  SYNCHRONISES. */
int mdg_probe_mfma_i8(int iters, int random_operands, double* tops, void* stream);
/* The same register-only loop on either int8 MFMA shape, to compare them on one device: shape = 32 runs the kernel of
 * mdg_probe_mfma_i8 (8 x v_mfma_i32_32x32x32_i8 per iteration), shape = 16 runs 16 x v_mfma_i32_16x16x64_i8 per iteration on
 * sixteen independent accumulators -- the same operands in the same rotation and the same int8 op count per wave.
 * waves_per_simd = 1 or 2 (the product kernels run two).  The chip may hold a different clock on the two shapes under its
 * power cap, so the ratio on random operands, not cycles per op, says which is faster.  SYNCHRONISES. */
int mdg_probe_mfma_i8_shape(int shape, int waves_per_simd, int iters, int random_operands, double* tops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEGPT_HIP_H */
