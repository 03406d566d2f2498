// One launch from a layer's three projection outputs to the fp8 KV cache: the rotary embedding (+ Qwen3's masked RMSNorm) of q and k,
// q written in the [B, n_heads, T, r_qk] layout attention reads, and the rotated K row and the V row quantised in place into the
// cache -- contiguous planes (mdg_kv8_append's layout) or pages behind a block table (mdg_kv8_paged_append's).  It stands for
//   src/patchers/LlamaRebuild.py:153-176      cos/sin gathered by the layer's rotary mask, rotate_half over the KEPT columns
//   src/patchers/DenseQwenRebuild.py:262-286  RMSNorm over the kept columns with the norm weight gathered by the same mask
// followed by the cache update, and replaces mdg_rope_gather (q) + mdg_rope_gather (k) + the append launch(es): on a decode step the
// rotated k never exists in memory as bf16 (k_out == NULL).
//
// Work.  The unit is a BUNDLE: one (batch, token, kv head) = the G = n_heads / n_kv query rows, the K row and the V row that share one
// token's cos / sin gathered by one mask row.  A 256-thread workgroup is 16 lane groups of 16; a row belongs to one lane group and
// lane c owns its elements [16 c, 16 c + 16), so a K or V lane ends in one aligned 16-byte fp8 store.  With G + 2 <= 16 a workgroup
// takes NB = 16 / (G + 2) bundles -- consecutive tokens of one kv head, which share the mask row and the norm weights; with G + 2 > 16
// it takes one bundle and loops over chunks of 16 rows.  blockIdx -> (token tile, kv head) as in rope.hip: workgroups are dealt
// round-robin to the 8 XCDs, the low 3 bits of blockIdx.x pick the XCD and every kv head of a token tile lands on the same one.
// Data.  Thread j of the workgroup loads mask[j] and gathers cos[mask[j]], sin[mask[j]] of each of the NB tokens and the two norm
// weights; every lane loads its 16 row elements (attn_tile.hpp's load8: any alignment, columns beyond the width read as zero).  All
// of these loads are issued before the first LDS write; addresses of dead rows / tokens / columns are clamped and only stores are
// predicated.  Then the gathered tables and the RAW rows go to LDS, one barrier, and each lane reads its own table entries as two
// 16-byte LDS reads each and its rotate_half partners -- elements j +- r_qk / 2, which lie in another lane's chunk and straddle
// chunks when r_qk / 2 is no multiple of 16 -- element by element from the row in LDS; nothing is read from memory twice.  With a
// norm a lane normalises its own elements and its partners' (the same two roundings on the same inputs: the same bits the partner's
// lane gets), so one barrier serves.  The fp32 sum of squares is the lane's 16 terms, then a DPP sum over the 16 lanes; the amax is
// 4 xor-shuffles over the lane group.
// Arithmetic.  rope.hip's, op by op (rope_round.hpp: mul_r / add_r, no contraction): without a norm weight q_out and k_out have the
// bits of mdg_rope_gather; with one only the order of the sum of squares differs, as between rope.hip's own routes.  The K row is
// rounded to the element type and then quantised by kv8.hpp's row_scale / pack16, the V row is quantised as it was read: the bytes
// and scales mdg_kv8_append / mdg_kv8_paged_append write for those rows.  A paged position outside the table is not written; table
// entries are clamped for memory safety only (kv8_paged.hip's rule).
// row16_sum is rope.hip's (file-local there): copied, not shared.
#include "kv8.hpp"
#include "rope_round.hpp"
#pragma STDC FP_CONTRACT OFF

namespace mdg {
namespace {

using namespace attn;

template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_sum(float s) {
  s = s + dpp_f32<0xB1>(s);   // quad_perm [1,0,3,2]
  s = s + dpp_f32<0x4E>(s);   // quad_perm [2,3,0,1]
  s = s + dpp_f32<0x141>(s);  // row_half_mirror
  s = s + dpp_f32<0x140>(s);  // row_mirror
  return s;
}

constexpr int THREADS = 256;
constexpr int GROUP = 16;     // lanes of a row
constexpr int GROUPS = 16;    // rows in flight per workgroup
constexpr int MAX_R = 256;    // widest row: 16 lanes x 16 elements
constexpr int MAX_NB = 5;     // bundles per workgroup at G = 1
constexpr int N_XCD = 8;

struct StepArgs {
  const void* q;
  const void* k;
  const void* v;
  int64_t ld_q, ld_k, vbs, vhs, vts;
  int64_t B, T;
  int n_heads, n_kv, group, r_qk, r_vo, hd;
  const void* cos;
  const void* sin;
  int64_t cs_bstride;
  const int64_t* mask;
  const void* qw;
  const void* kw;
  float eps;
  void* q_out;
  void* k_out;  // or nullptr
  unsigned char* k_data;
  unsigned char* v_data;
  float* k_scale;
  float* v_scale;
  int64_t k_pitch, v_pitch;
  int64_t cap, pos;                 // contiguous planes
  const int* table;                 // pages
  const int* dpos;
  int64_t table_len, limit;         // limit = table_len * page: positions at or beyond it are not written
  int page, n_pages;
  unsigned n_tiles;                 // B * t_tiles
  int t_tiles, nb, rows_pb, passes; // token tiles per batch; bundles and lane groups per bundle of a workgroup; row chunks of a bundle
  int q_vec, k_vec, v_vec;          // every row of the source starts 16-byte aligned
  int qo_w, ko_w;                   // bytes of the widest store q_out / k_out rows allow: 16, 4 or 2
};

// the lane's 16 rotated elements (two quads of packed pairs) to elements [16 c, 16 c + 16) of a row of r elements
template <typename E> __device__ __forceinline__ void store_row16(E* orow, int c, int r, int w, u32x4 o0, u32x4 o1) {
  const int c0 = GROUP * c;
  if (w == 16) {  // r is a multiple of 8: a half chunk is whole or absent
    if (c0 + 8 <= r) *(u32x4*)(orow + c0) = o0;
    if (c0 + 16 <= r) *(u32x4*)(orow + c0 + 8) = o1;
  } else if (w == 4) {  // r is even: so is a pair
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (c0 + 2 * i < r) *(unsigned*)(orow + c0 + 2 * i) = i < 4 ? o0[i & 3] : o1[i & 3];
  } else {
#pragma unroll
    for (int e = 0; e < 16; e++)
      if (c0 + e < r) orow[c0 + e] = (E)half_of(e < 8 ? o0[(e >> 1) & 3] : o1[(e >> 1) & 3], e & 1);
  }
}

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int DT, bool NORM, bool PAGED> __global__ __launch_bounds__(THREADS) void rope_kv8_step_kernel(StepArgs a) {
  typedef typename Lp<DT>::T E;
  __shared__ __attribute__((aligned(16))) E rows[GROUPS][MAX_R];    // the raw rows in flight
  __shared__ __attribute__((aligned(16))) E cg[MAX_NB][MAX_R];      // cos[mask] of each bundle's token
  __shared__ __attribute__((aligned(16))) E sg[MAX_NB][MAX_R];      // sin[mask]
  __shared__ __attribute__((aligned(16))) E wg[2][MAX_R];           // q_norm_w[mask], k_norm_w[mask]
  // grid = (8 * n_kv, ceil(n_tiles / 8)): the low 3 bits of blockIdx.x are the XCD the workgroup lands on
  const unsigned tile = blockIdx.y * N_XCD + (blockIdx.x & (N_XCD - 1));
  if (tile >= a.n_tiles) return;
  const int hk = blockIdx.x >> 3;
  const unsigned bu = tile / (unsigned)a.t_tiles;
  const int64_t b = bu;
  const int64_t t0 = (int64_t)(tile - bu * (unsigned)a.t_tiles) * a.nb;
  const int lg = threadIdx.x / GROUP, c = threadIdx.x % GROUP;
  const int half = a.r_qk >> 1;
  const int last = a.group + 1;  // rows of a bundle: 0 .. G - 1 the query heads, G the K row, G + 1 the V row
  const int slot_ = a.passes == 1 ? lg / a.rows_pb : 0;
  const int slot = min(slot_, a.nb - 1);
  const bool tok_live = slot_ < a.nb && t0 + slot_ < a.T;
  const int64_t t = min(t0 + slot, a.T - 1);

  // where the token's K and V rows land
  int64_t kv_slot;
  bool kv_live = tok_live;
  if (PAGED) {
    const int64_t at = (int64_t)a.dpos[b] + t;
    kv_live = kv_live && at >= 0 && at < a.limit;
    const int64_t pi = at < 0 ? 0 : at >= a.limit ? a.table_len - 1 : at / a.page;
    int pid = a.table[b * a.table_len + pi];
    pid = clamp_int(pid, 0, a.n_pages - 1);
    kv_slot = ((int64_t)pid * a.n_kv + hk) * a.page + (at - pi * a.page);
  } else {
    kv_slot = (b * a.n_kv + hk) * a.cap + a.pos + t;
  }

  for (int p = 0; p < a.passes; p++) {
    const int rho_ = a.passes == 1 ? lg - slot_ * a.rows_pb : p * GROUPS + lg;
    const bool live = tok_live && rho_ <= last;
    const int rho = min(rho_, last);
    const bool is_k = rho == a.group, is_v = rho == last;
    // 1. the lane's 16 elements of its row
    const E* src;
    int width, vec;
    if (is_v) {
      src = (const E*)a.v + b * a.vbs + hk * a.vhs + t * a.vts;
      width = a.r_vo;
      vec = a.v_vec;
    } else if (is_k) {
      src = (const E*)a.k + (b * a.T + t) * a.ld_k + (int64_t)hk * a.r_qk;
      width = a.r_qk;
      vec = a.k_vec;
    } else {
      src = (const E*)a.q + (b * a.T + t) * a.ld_q + (int64_t)(hk * a.group + rho) * a.r_qk;
      width = a.r_qk;
      vec = a.q_vec;
    }
    u32x4 x[2];
#pragma unroll
    for (int h = 0; h < 2; h++) x[h] = load8(src, GROUP * c + 8 * h, width, vec != 0);
    // 2. once a workgroup: column j's mask entry and what it gathers, for every bundle
    if (p == 0) {
      const int j = min((int)threadIdx.x, a.r_qk - 1);
      int m = j;
      if (a.mask) m = clamp_int((int)a.mask[(int64_t)hk * a.r_qk + j], 0, a.hd - 1);  // memory safety only; the binding validates masks
      E cv[MAX_NB], sv[MAX_NB], wq = 0, wk = 0;
#pragma unroll
      for (int s = 0; s < MAX_NB; s++) {
        const int64_t ts = min(t0 + min(s, a.nb - 1), a.T - 1);
        cv[s] = ((const E*)a.cos)[b * a.cs_bstride + ts * a.hd + m];
        sv[s] = ((const E*)a.sin)[b * a.cs_bstride + ts * a.hd + m];
      }
      if (NORM) {
        wq = ((const E*)(a.qw ? a.qw : a.kw))[m];
        wk = ((const E*)(a.kw ? a.kw : a.qw))[m];
      }
      if ((int)threadIdx.x < a.r_qk) {
#pragma unroll
        for (int s = 0; s < MAX_NB; s++) {
          cg[s][j] = cv[s];
          sg[s][j] = sv[s];
        }
        if (NORM) {
          wg[0][j] = wq;
          wg[1][j] = wk;
        }
      }
    }
    *(u32x4*)(&rows[lg][GROUP * c]) = x[0];
    *(u32x4*)(&rows[lg][GROUP * c + 8]) = x[1];
    __syncthreads();

    float f[16];
#pragma unroll
    for (int e = 0; e < 16; e++) f[e] = Lp<DT>::up((E)half_of(x[e >> 3][(e >> 1) & 3], e & 1));
    float ss = 0.f;
    if (NORM) {
#pragma unroll
      for (int e = 0; e < 16; e++) ss = add_r(ss, mul_r(f[e], f[e]));
      ss = row16_sum(ss);
    }
    if (!is_v) {
      // 3. q and k rows: (norm,) rotate, round; the partners come from the row in LDS
      const bool nrm = NORM && (is_k ? a.kw : a.qw) != nullptr;
      const float inv = nrm ? 1.f / sqrtf(add_r(ss / (float)a.r_qk, a.eps)) : 1.f;
      const E* xr = rows[lg];
      const E* wt = wg[is_k ? 1 : 0];
      u32x4 cw[2], sw[2], ww[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        cw[h] = *(const u32x4*)(&cg[slot][GROUP * c + 8 * h]);
        sw[h] = *(const u32x4*)(&sg[slot][GROUP * c + 8 * h]);
        if (NORM) ww[h] = *(const u32x4*)(&wt[GROUP * c + 8 * h]);
      }
      unsigned ob[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int j_ = GROUP * c + e;
        const bool on = j_ < a.r_qk;
        const int j = on ? j_ : 0;
        const bool lo = j < half;
        const int pj = lo ? j + half : j - half;
        float a1 = f[e], a2 = Lp<DT>::up(xr[pj]);
        if (nrm) {  // (gathered_weight * (x_float * rsqrt(var + eps))).to(dtype)
          const float w1 = Lp<DT>::up((E)half_of(ww[e >> 3][(e >> 1) & 3], e & 1)), w2 = Lp<DT>::up(wt[pj]);
          a1 = Lp<DT>::up(Lp<DT>::down(mul_r(w1, mul_r(a1, inv))));
          a2 = Lp<DT>::up(Lp<DT>::down(mul_r(w2, mul_r(a2, inv))));
        }
        const float cj = Lp<DT>::up((E)half_of(cw[e >> 3][(e >> 1) & 3], e & 1));
        const float sj = Lp<DT>::up((E)half_of(sw[e >> 3][(e >> 1) & 3], e & 1));
        // q * cos + rotate_half(q) * sin, rotate_half(q) = cat(-q[half:], q[:half])
        const float u = Lp<DT>::up(Lp<DT>::down(mul_r(a1, cj)));
        const float w = Lp<DT>::up(Lp<DT>::down(mul_r(lo ? -a2 : a2, sj)));
        ob[e] = on ? (unsigned)Lp<DT>::down(add_r(u, w)) : 0u;
      }
      u32x4 o[2];
#pragma unroll
      for (int i = 0; i < 8; i++) o[i >> 2][i & 3] = ob[2 * i] | (ob[2 * i + 1] << 16);
      if (is_k) {
        if (live && a.k_out) store_row16((E*)a.k_out + ((b * a.n_kv + hk) * a.T + t) * a.r_qk, c, a.r_qk, a.ko_w, o[0], o[1]);
#pragma unroll
        for (int e = 0; e < 16; e++) f[e] = Lp<DT>::up((E)ob[e]);  // the cache holds the ROUNDED row, quantised
      } else if (live) {
        store_row16((E*)a.q_out + ((b * a.n_heads + hk * a.group + rho) * a.T + t) * a.r_qk, c, a.r_qk, a.qo_w, o[0], o[1]);
      }
    }
    if (rho >= a.group) {
      // 4. K and V rows: kv8.hip's quantiser, one aligned 16-byte store a lane, lane 0 stores the scale
      float amax = 0.f;
#pragma unroll
      for (int e = 0; e < 16; e++) amax = fmaxf(amax, fabsf(f[e]));
      for (int d = GROUP >> 1; d; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
      float sc, qinv;
      kv8::row_scale(amax, sc, qinv);
      const u32x4 pk = kv8::pack16(f, qinv);
      if (live && kv_live) {
        const int64_t pitch = is_v ? a.v_pitch : a.k_pitch;
        const int chunks = (int)(pitch / kv8::CHUNK);
        unsigned char* drow = (is_v ? a.v_data : a.k_data) + kv_slot * pitch;
        if (c < chunks) *(u32x4*)(drow + kv8::CHUNK * c) = pk;  // elements >= r were read as zero: the padding goes with the data
        // a pitch beyond 256 bytes (the caller's choice): zero bytes too
        for (int cc = c + GROUP; cc < chunks; cc += GROUP) *(u32x4*)(drow + kv8::CHUNK * cc) = (u32x4){0u, 0u, 0u, 0u};
        if (c == 0) (is_v ? a.v_scale : a.k_scale)[kv_slot] = sc;
      }
    }
  }
}

template <int DT, bool PAGED> void launch_step(const StepArgs& a, dim3 grid, hipStream_t st) {
  if (a.qw || a.kw) hipLaunchKernelGGL((rope_kv8_step_kernel<DT, true, PAGED>), grid, dim3(THREADS), 0, st, a);
  else hipLaunchKernelGGL((rope_kv8_step_kernel<DT, false, PAGED>), grid, dim3(THREADS), 0, st, a);
}

// what the two entries share: everything but where the K and V rows land
struct StepCall {
  const void* q; int64_t ld_q;
  const void* k; int64_t ld_k;
  const void* v; int64_t vbs, vhs, vts;
  int dtype;
  int64_t B, T;
  int n_heads, n_kv, r_qk, r_vo, hd;
  const void* cos; const void* sin; int64_t cs_bstride;
  const int64_t* mask;
  const void* qw; const void* kw; double eps;
  void* q_out; void* k_out;
  void* k_data; void* k_scale; void* v_data; void* v_scale;
  int64_t k_pitch, v_pitch;
};

// the refusals that need no device and no pointer, under the caller's name
int check_shapes(const char* fn, const StepCall& p) {
  MDG_CHECK_ARG(p.dtype == MDG_BF16 || p.dtype == MDG_F16, "%s: dtype %d (bf16 or f16)", fn, p.dtype);
  MDG_CHECK_ARG(p.B >= 0 && p.T >= 0, "%s: negative extent", fn);
  MDG_CHECK_ARG(p.n_heads > 0 && p.n_kv > 0 && p.n_heads % p.n_kv == 0, "%s: n_heads %d must be a multiple of n_kv %d", fn, p.n_heads,
                p.n_kv);
  MDG_CHECK_ARG(p.hd >= 2 && p.hd <= MAX_R, "%s: head_dim=%d must be in 2..%d", fn, p.hd, MAX_R);
  MDG_CHECK_ARG(p.r_qk >= 2 && p.r_qk % 2 == 0 && p.r_qk <= p.hd, "%s: kept width r_qk=%d must be even, >= 2 and <= head_dim=%d", fn,
                p.r_qk, p.hd);
  MDG_CHECK_ARG(p.r_vo >= 1 && p.r_vo <= MAX_R, "%s: r_vo=%d must be in 1..%d", fn, p.r_vo, MAX_R);
  MDG_CHECK_ARG(p.mask || p.r_qk == p.hd, "%s: no mask given but r_qk=%d != head_dim=%d", fn, p.r_qk, p.hd);
  MDG_CHECK_ARG(p.ld_q >= (int64_t)p.n_heads * p.r_qk && p.ld_k >= (int64_t)p.n_kv * p.r_qk, "%s: ld_q=%lld / ld_k=%lld below a row",
                fn, (long long)p.ld_q, (long long)p.ld_k);
  MDG_CHECK_ARG(p.cs_bstride == 0 || p.cs_bstride >= p.T * p.hd, "%s: cos/sin batch stride %lld", fn, (long long)p.cs_bstride);
  const int r[2] = {p.r_qk, p.r_vo};
  const int64_t pitch[2] = {p.k_pitch, p.v_pitch};
  for (int i = 0; i < 2; i++)
    MDG_CHECK_ARG(pitch[i] >= kv8::pitch_of(r[i]) && pitch[i] % kv8::CHUNK == 0,
                  "%s: pitch=%lld must be a multiple of 16 and >= mdg_kv8_pitch(%d) = %lld", fn, (long long)pitch[i], r[i],
                  (long long)kv8::pitch_of(r[i]));
  return MDG_OK;
}

// pointers, alignments and overlaps (B, T > 0); `target` holds the nt cache spans and gets q_out (and k_out) appended
int check_operands(const char* fn, const StepCall& p, Span* target, int nt, const Span* extra, int n_extra) {
  MDG_CHECK_ARG(p.q && p.k && p.v && p.cos && p.sin && p.q_out, "%s: null pointer", fn);
  MDG_CHECK_ARG(p.k_data && p.k_scale && p.v_data && p.v_scale, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)p.k_data % 16 == 0 && (uintptr_t)p.v_data % 16 == 0 && (uintptr_t)p.k_scale % 4 == 0 &&
                    (uintptr_t)p.v_scale % 4 == 0, "%s: data must be 16-byte and scales 4-byte aligned", fn);
  const uintptr_t two = (uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.cos | (uintptr_t)p.sin | (uintptr_t)p.qw |
                        (uintptr_t)p.kw | (uintptr_t)p.q_out | (uintptr_t)p.k_out;
  MDG_CHECK_ARG(two % 2 == 0 && (uintptr_t)p.mask % 8 == 0, "%s: element pointers must be 2-byte, the mask 8-byte aligned", fn);
  MDG_CHECK_ARG(p.B <= INT64_MAX / p.T / 1024 / (p.n_heads + 2), "%s: B*T*n_heads overflows", fn);
  MDG_CHECK_ARG(p.B * p.T <= INT64_MAX / 4 / (p.ld_q > p.ld_k ? p.ld_q : p.ld_k), "%s: B*T*ld overflows", fn);
  const size_t es = dtype_size(p.dtype);
  target[nt++] = span_of("q_out", p.q_out, 1, 0, 1, 0, p.B * p.n_heads * p.T, p.r_qk, p.r_qk, es);
  if (p.k_out) target[nt++] = span_of("k_out", p.k_out, 1, 0, 1, 0, p.B * p.n_kv * p.T, p.r_qk, p.r_qk, es);
  const int64_t csb = p.cs_bstride ? p.B : 1;
  const Span in[8] = {span_of("q", p.q, 1, 0, 1, 0, p.B * p.T, p.ld_q, (int64_t)p.n_heads * p.r_qk, es),
                      span_of("k", p.k, 1, 0, 1, 0, p.B * p.T, p.ld_k, (int64_t)p.n_kv * p.r_qk, es),
                      span_of("v", p.v, p.B, p.vbs, p.n_kv, p.vhs, p.T, p.vts, p.r_vo, es),
                      span_of("cos", p.cos, csb, p.cs_bstride, 1, 0, p.T, p.hd, p.hd, es),
                      span_of("sin", p.sin, csb, p.cs_bstride, 1, 0, p.T, p.hd, p.hd, es),
                      span_of("mask", p.mask, 1, 0, 1, 0, p.mask ? p.n_kv : 0, p.r_qk, p.r_qk, 8),
                      span_of("q_norm_w", p.qw, 1, 0, 1, 0, p.qw ? 1 : 0, p.hd, p.hd, es),
                      span_of("k_norm_w", p.kw, 1, 0, 1, 0, p.kw ? 1 : 0, p.hd, p.hd, es)};
  for (int i = 0; i < 8; i++) MDG_TRY(apart(fn, target, nt, in[i]));
  for (int i = 0; i < n_extra; i++) MDG_TRY(apart(fn, target, nt, extra[i]));
  for (int i = 1; i < nt; i++) MDG_TRY(apart(fn, target, i, target[i]));
  return MDG_OK;
}

// the split of the work and the widths of the accesses; then the launch
int plan_and_launch(const char* fn, const StepCall& p, StepArgs& a, bool paged, void* stream) {
  a.q = p.q; a.k = p.k; a.v = p.v;
  a.ld_q = p.ld_q; a.ld_k = p.ld_k; a.vbs = p.vbs; a.vhs = p.vhs; a.vts = p.vts;
  a.B = p.B; a.T = p.T;
  a.n_heads = p.n_heads; a.n_kv = p.n_kv; a.group = p.n_heads / p.n_kv; a.r_qk = p.r_qk; a.r_vo = p.r_vo; a.hd = p.hd;
  a.cos = p.cos; a.sin = p.sin; a.cs_bstride = p.cs_bstride; a.mask = p.mask;
  a.qw = p.qw; a.kw = p.kw; a.eps = (float)p.eps;
  a.q_out = p.q_out; a.k_out = p.k_out;
  a.k_data = (unsigned char*)p.k_data; a.v_data = (unsigned char*)p.v_data;
  a.k_scale = (float*)p.k_scale; a.v_scale = (float*)p.v_scale;
  a.k_pitch = p.k_pitch; a.v_pitch = p.v_pitch;
  const int rows = a.group + 2;
  if (rows <= GROUPS) {
    a.rows_pb = rows;
    a.nb = (int)(p.T < GROUPS / rows ? p.T : GROUPS / rows);
    a.passes = 1;
  } else {
    a.rows_pb = GROUPS;
    a.nb = 1;
    a.passes = (int)ceil_div(rows, GROUPS);
  }
  a.t_tiles = (int)ceil_div(p.T, a.nb);
  const int64_t n_tiles = p.B * a.t_tiles, tiles8 = ceil_div(n_tiles, N_XCD);
  MDG_CHECK_ARG(ceil_div(p.T, a.nb) <= 0x7fffffff && n_tiles <= 0xffffffffll && tiles8 <= 65535 && (int64_t)p.n_kv * N_XCD <= 0x7fffffff,
                "%s: B*T = %lld tokens exceed one launch (%d tokens per workgroup, 65535 * 8 workgroups a kv head)", fn,
                (long long)(p.B * p.T), a.nb);
  a.n_tiles = (unsigned)n_tiles;
  a.q_vec = (uintptr_t)p.q % 16 == 0 && p.ld_q % 8 == 0 && p.r_qk % 8 == 0;
  a.k_vec = (uintptr_t)p.k % 16 == 0 && p.ld_k % 8 == 0 && p.r_qk % 8 == 0;
  a.v_vec = (uintptr_t)p.v % 16 == 0 && p.vbs % 8 == 0 && p.vhs % 8 == 0 && p.vts % 8 == 0;
  auto widest = [&](const void* out) { return p.r_qk % 8 == 0 && (uintptr_t)out % 16 == 0 ? 16 : (uintptr_t)out % 4 == 0 ? 4 : 2; };
  a.qo_w = widest(p.q_out);
  a.ko_w = widest(p.k_out);
  const dim3 grid((unsigned)(N_XCD * p.n_kv), (unsigned)tiles8);
  hipStream_t st = (hipStream_t)stream;
  if (paged) {
    if (p.dtype == MDG_BF16) launch_step<MDG_BF16, true>(a, grid, st);
    else launch_step<MDG_F16, true>(a, grid, st);
  } else {
    if (p.dtype == MDG_BF16) launch_step<MDG_BF16, false>(a, grid, st);
    else launch_step<MDG_F16, false>(a, grid, st);
  }
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_rope_kv8_step(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t v_batch_stride,
                                 int64_t v_head_stride, int64_t v_token_stride, int dtype, int64_t B, int64_t T, int n_heads, int n_kv,
                                 int r_qk, int r_vo, int hd, const void* cos, const void* sin, int64_t cs_batch_stride,
                                 const int64_t* mask, const void* q_norm_w, const void* k_norm_w, double eps, void* q_out, void* k_out,
                                 void* k_data, void* k_scale, void* v_data, void* v_scale, int64_t cap, int64_t k_pitch, int64_t v_pitch,
                                 int64_t pos, void* stream) {
  const char* fn = "mdg_rope_kv8_step";
  MDG_CLEAR();
  const StepCall p = {q, ld_q, k, ld_k, v, v_batch_stride, v_head_stride, v_token_stride, dtype, B, T, n_heads, n_kv, r_qk, r_vo, hd,
                      cos, sin, cs_batch_stride, mask, q_norm_w, k_norm_w, eps, q_out, k_out, k_data, k_scale, v_data, v_scale,
                      k_pitch, v_pitch};
  MDG_TRY(check_shapes(fn, p));
  MDG_CHECK_ARG(cap >= 0 && pos >= 0 && T <= cap && pos <= cap - T, "%s: pos=%lld + T=%lld rows exceed cap=%lld", fn, (long long)pos,
                (long long)T, (long long)cap);
  if (B == 0 || T == 0) return MDG_OK;
  const int64_t wide = k_pitch > v_pitch ? k_pitch : v_pitch;
  MDG_CHECK_ARG(B <= INT64_MAX / n_kv / cap / wide, "%s: B*n_kv*cap*pitch overflows", fn);
  const int64_t rows = B * n_kv * cap;
  Span target[6] = {Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                    Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                    Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                    Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)}};
  MDG_TRY(check_operands(fn, p, target, 4, nullptr, 0));
  StepArgs a = StepArgs();
  a.cap = cap; a.pos = pos;
  return plan_and_launch(fn, p, a, false, stream);
}

extern "C" int mdg_rope_kv8_paged_step(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t v_batch_stride,
                                       int64_t v_head_stride, int64_t v_token_stride, int dtype, int64_t B, int64_t T, int n_heads,
                                       int n_kv, int r_qk, int r_vo, int hd, const void* cos, const void* sin, int64_t cs_batch_stride,
                                       const int64_t* mask, const void* q_norm_w, const void* k_norm_w, double eps, void* q_out,
                                       void* k_out, void* k_data, void* k_scale, void* v_data, void* v_scale, int64_t n_pages,
                                       int64_t page, int64_t k_pitch, int64_t v_pitch, const void* block_table, int64_t table_len,
                                       const void* pos, void* stream) {
  const char* fn = "mdg_rope_kv8_paged_step";
  MDG_CLEAR();
  const StepCall p = {q, ld_q, k, ld_k, v, v_batch_stride, v_head_stride, v_token_stride, dtype, B, T, n_heads, n_kv, r_qk, r_vo, hd,
                      cos, sin, cs_batch_stride, mask, q_norm_w, k_norm_w, eps, q_out, k_out, k_data, k_scale, v_data, v_scale,
                      k_pitch, v_pitch};
  MDG_TRY(check_shapes(fn, p));
  MDG_CHECK_ARG(page > 0 && page % KT == 0, "%s: page=%lld must be a positive multiple of %d", fn, (long long)page, KT);
  MDG_CHECK_ARG(n_pages > 0 && table_len > 0, "%s: n_pages=%lld and table_len=%lld must be positive", fn, (long long)n_pages,
                (long long)table_len);
  MDG_CHECK_ARG(page <= 0x7fffffff && n_pages <= 0x7fffffff && table_len <= INT64_MAX / page, "%s: table_len*page overflows", fn);
  if (B == 0 || T == 0) return MDG_OK;
  const int64_t wide = k_pitch > v_pitch ? k_pitch : v_pitch;
  MDG_CHECK_ARG(n_pages <= INT64_MAX / n_kv / page / wide, "%s: n_pages*n_kv*page*pitch overflows", fn);
  MDG_CHECK_ARG(B <= INT64_MAX / 4 / table_len, "%s: B*table_len overflows", fn);
  MDG_CHECK_ARG(block_table && pos, "%s: null pointer", fn);
  MDG_CHECK_ARG((uintptr_t)block_table % 4 == 0 && (uintptr_t)pos % 4 == 0, "%s: block_table and pos must be 4-byte aligned", fn);
  const int64_t rows = n_pages * n_kv * page;
  Span target[6] = {Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                    Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                    Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                    Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)}};
  const Span extra[2] = {Span{"block_table", (uintptr_t)block_table, (uintptr_t)block_table + (uintptr_t)(B * table_len * 4)},
                         Span{"pos", (uintptr_t)pos, (uintptr_t)pos + (uintptr_t)(B * 4)}};
  MDG_TRY(check_operands(fn, p, target, 4, extra, 2));
  StepArgs a = StepArgs();
  a.table = (const int*)block_table; a.dpos = (const int*)pos;
  a.table_len = table_len; a.limit = table_len * page;
  a.page = (int)page; a.n_pages = (int)n_pages;
  return plan_and_launch(fn, p, a, true, stream);
}
