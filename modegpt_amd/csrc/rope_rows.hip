// Rotary embedding of a projection output IN ITS OWN LAYOUT -- the post-RoPE rows q', k' of a calibration batch, as the model
// itself computes them (reference: src/adapters/LlamaAdapter.py:46-69 patched_attn_forward, 305-325 _attn_hook: the variant
// upstream disabled).  x [B*T, n_heads*hd] -> out [B*T, n_heads*hd], so the result goes straight into the covariance kernels
// (sigma_q', sigma_k': the statistics for which mdg_qk_rank_curve's logit error is exact on a rotary model).
//
// HBM-bound: algorithmic bytes = 2 * B*T*n_heads*hd * sizeof(elt).  The rotate_half partner of column c is column c +- hd/2 of
// the same head and row.  Partner exchange chosen: NONE IS NEEDED -- a lane owns the PAIR of packs (c .. c+VEC) and
// (c + hd/2 .. c + hd/2 + VEC) of a row, loads both (its "second load" is the only load of those bytes, not a re-read) and
// writes both results.  Every element of x is read by exactly one lane, once; every element of out is written once; no lane
// exchange, no LDS, no barrier.  The same lane does this for HPT heads of its token (4, 2 or 1: what divides n_heads), which
// share the token's cos / sin packs: the tables (n_heads times smaller than x) are read once per HPT heads and stay in L2.
// Full-width tables: cos[c] and cos[c + hd/2] (sin likewise) are loaded separately, the halves are not assumed equal.
//
// Two paths, one kernel template: VEC = 16 bytes of elements (8 bf16 / f16, 4 f32) when x, out, cos, sin are 16-byte
// aligned, both pitches and the table batch stride are multiples of VEC and hd/2 is one too; VEC = 1 (element-wise)
// otherwise -- unaligned views, odd pitches, head_dim too small for a pack per half.
//
// Arithmetic: rope_round.hpp -- torch's eager expression op by op, out = dt(dt(x cos) + dt(rotate_half(x) sin)), every product
// and the sum rounded to the element type, no FMA contraction.  No atomics; nothing depends on launch order.
#include "common.hpp"
#include "rope_round.hpp"
#pragma STDC FP_CONTRACT OFF

namespace mdg {
namespace {

constexpr int THREADS = 256;
constexpr int MAX_HD = 256;

struct RowsArgs {
  const void* x;
  const void* cos;
  const void* sin;
  void* out;
  int64_t ld_x, ld_out, N, T, cs_bstride;
  int hd, half;
  unsigned jn;   // packs per half row: half / VEC
  unsigned per;  // work items per token: (n_heads / HPT) * jn
  int tok;       // tokens per workgroup
};

template <typename E, int VEC> struct alignas(sizeof(E) * VEC) RowPack { E v[VEC]; };

// Work item = (token, chunk of HPT heads, pack j of the first half).  A workgroup owns `tok` consecutive tokens (tok * per is
// 256 items where per divides 256; a wider row makes the loop below run more than once).  Consecutive lanes take consecutive
// packs of one head: a wave's load instruction covers whole 128-byte lines of x.
template <int DT, int VEC, int HPT>
__global__ __launch_bounds__(THREADS) void rope_rows_kernel(RowsArgs a) {
  typedef typename Lp<DT>::T E;
  typedef RowPack<E, VEC> P;
  const int64_t t0 = (int64_t)blockIdx.x * a.tok;
  const int64_t left = a.N - t0;
  const unsigned ntok = (unsigned)(left < (int64_t)a.tok ? left : (int64_t)a.tok);
  const int64_t b0 = t0 / a.T, tt0 = t0 - b0 * a.T;  // uniform: once per wave
  const unsigned items = ntok * a.per;
  for (unsigned i = threadIdx.x; i < items; i += THREADS) {
    const unsigned lt = i / a.per, rem = i - lt * a.per;
    const unsigned hc = rem / a.jn, j = rem - hc * a.jn;
    int64_t tt = tt0 + lt, b = b0;
    while (tt >= a.T) {  // at most once unless T < tok
      tt -= a.T;
      b++;
    }
    const int c = (int)j * VEC;
    const E* crow = (const E*)a.cos + b * a.cs_bstride + tt * a.hd + c;
    const E* srow = (const E*)a.sin + b * a.cs_bstride + tt * a.hd + c;
    const int64_t col = (int64_t)hc * HPT * a.hd + c;
    const E* xr = (const E*)a.x + (t0 + lt) * a.ld_x + col;
    E* orow = (E*)a.out + (t0 + lt) * a.ld_out + col;
    // every load of the item in flight before the first use
    P p1[HPT], p2[HPT];
#pragma unroll
    for (int hh = 0; hh < HPT; hh++) {
      p1[hh] = *(const P*)(xr + hh * a.hd);
      p2[hh] = *(const P*)(xr + hh * a.hd + a.half);
    }
    const P c1 = *(const P*)crow, c2 = *(const P*)(crow + a.half);
    const P s1 = *(const P*)srow, s2 = *(const P*)(srow + a.half);
#pragma unroll
    for (int hh = 0; hh < HPT; hh++) {
      P o1, o2;
#pragma unroll
      for (int v = 0; v < VEC; v++) {
        const float a1 = Lp<DT>::up(p1[hh].v[v]), a2 = Lp<DT>::up(p2[hh].v[v]);
        // x * cos + rotate_half(x) * sin, rotate_half(x) = cat(-x[half:], x[:half])
        const float u1 = Lp<DT>::up(Lp<DT>::down(mul_r(a1, Lp<DT>::up(c1.v[v]))));
        const float v1 = Lp<DT>::up(Lp<DT>::down(mul_r(-a2, Lp<DT>::up(s1.v[v]))));
        const float u2 = Lp<DT>::up(Lp<DT>::down(mul_r(a2, Lp<DT>::up(c2.v[v]))));
        const float v2 = Lp<DT>::up(Lp<DT>::down(mul_r(a1, Lp<DT>::up(s2.v[v]))));
        o1.v[v] = Lp<DT>::down(add_r(u1, v1));
        o2.v[v] = Lp<DT>::down(add_r(u2, v2));
      }
      *(P*)(orow + hh * a.hd) = o1;
      *(P*)(orow + hh * a.hd + a.half) = o2;
    }
  }
}

template <int DT, int VEC> void launch_rows_hpt(const RowsArgs& a, int hpt, dim3 grid, hipStream_t st) {
  if (hpt == 4) hipLaunchKernelGGL((rope_rows_kernel<DT, VEC, 4>), grid, dim3(THREADS), 0, st, a);
  else if (hpt == 2) hipLaunchKernelGGL((rope_rows_kernel<DT, VEC, 2>), grid, dim3(THREADS), 0, st, a);
  else hipLaunchKernelGGL((rope_rows_kernel<DT, VEC, 1>), grid, dim3(THREADS), 0, st, a);
}

template <int DT> void launch_rows(const RowsArgs& a, bool vec, int hpt, dim3 grid, hipStream_t st) {
  constexpr int PER16 = 16 / (int)sizeof(typename Lp<DT>::T);
  if (vec) launch_rows_hpt<DT, PER16>(a, hpt, grid, st);
  else launch_rows_hpt<DT, 1>(a, hpt, grid, st);
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_rope_rows(const void* x, int dtype, int64_t ld_x, int64_t B, int64_t T, int n_heads, int hd, const void* cos,
                             const void* sin, int64_t cs_batch_stride, void* out, int64_t ld_out, void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(dtype == MDG_BF16 || dtype == MDG_F16 || dtype == MDG_F32, "mdg_rope_rows: dtype %d (bf16, f16 or f32)", dtype);
  MDG_CHECK_ARG(B >= 0 && T >= 0, "mdg_rope_rows: negative extent");
  MDG_CHECK_ARG(n_heads > 0, "mdg_rope_rows: n_heads %d", n_heads);
  MDG_CHECK_ARG(hd >= 2 && hd % 2 == 0 && hd <= MAX_HD, "mdg_rope_rows: head_dim=%d must be even, >= 2 and <= %d", hd, MAX_HD);
  const int64_t width = (int64_t)n_heads * hd;
  MDG_CHECK_ARG(width <= 0x7fffffff, "mdg_rope_rows: row width n_heads*head_dim=%lld exceeds 2^31 - 1", (long long)width);
  MDG_CHECK_ARG(ld_x >= width, "mdg_rope_rows: ld_x=%lld < n_heads*head_dim=%lld", (long long)ld_x, (long long)width);
  MDG_CHECK_ARG(ld_out >= width, "mdg_rope_rows: ld_out=%lld < n_heads*head_dim=%lld", (long long)ld_out, (long long)width);
  MDG_CHECK_ARG(cs_batch_stride == 0 || cs_batch_stride >= T * hd, "mdg_rope_rows: cos/sin batch stride %lld",
                (long long)cs_batch_stride);
  MDG_CHECK_ARG(T == 0 || B <= INT64_MAX / T, "mdg_rope_rows: B*T overflows");
  const int64_t N = B * T;
  if (N == 0) return MDG_OK;
  MDG_CHECK_ARG(x && cos && sin && out, "mdg_rope_rows: null pointer");
  const size_t es = dtype_size(dtype);
  // the byte ranges the two operands span, pitches included: the model still needs x, so a call that could write into it
  // (in place, or interleaved views of one buffer) is refused
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  const uintptr_t xe = xa + (uintptr_t)((N - 1) * ld_x + width) * es, oe = oa + (uintptr_t)((N - 1) * ld_out + width) * es;
  MDG_CHECK_ARG(xe <= oa || oe <= xa, "mdg_rope_rows: out overlaps x (the rotation is not done in place)");

  const int hpt = n_heads % 4 == 0 ? 4 : n_heads % 2 == 0 ? 2 : 1;
  const int half = hd / 2, per16 = 16 / (int)es;
  const bool vec = half % per16 == 0 && xa % 16 == 0 && oa % 16 == 0 && (uintptr_t)cos % 16 == 0 && (uintptr_t)sin % 16 == 0 &&
                   ld_x % per16 == 0 && ld_out % per16 == 0 && cs_batch_stride % per16 == 0;
  RowsArgs a;
  a.x = x; a.cos = cos; a.sin = sin; a.out = out;
  a.ld_x = ld_x; a.ld_out = ld_out; a.N = N; a.T = T; a.cs_bstride = cs_batch_stride;
  a.hd = hd; a.half = half;
  a.jn = (unsigned)(half / (vec ? per16 : 1));
  a.per = (unsigned)(n_heads / hpt) * a.jn;  // <= width / 2 < 2^30
  a.tok = a.per >= (unsigned)THREADS ? 1 : THREADS / (int)a.per;
  const int64_t blocks = ceil_div(N, a.tok);
  MDG_CHECK_ARG(blocks <= 0x7fffffff, "mdg_rope_rows: B*T = %lld tokens exceed one launch (%d tokens per workgroup)",
                (long long)N, a.tok);
  const dim3 grid((unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDG_BF16) launch_rows<MDG_BF16>(a, vec, hpt, grid, st);
  else if (dtype == MDG_F16) launch_rows<MDG_F16>(a, vec, hpt, grid, st);
  else launch_rows<MDG_F32>(a, vec, hpt, grid, st);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
