// mdg_attn_decode_kv8's product from a PAGED fp8 KV cache (layout: include/modegpt_hip.h; written by kv8_paged.hip): the same domain
// T * G <= 32, column map, workspace, combine kernel, lane maps and arithmetic as attn_decode_kv8.hip -- and everything about WHERE the
// keys are decided on the device, so that the launch arguments of a decode step do not change from step to step:
//
// Chunks.  Workgroup (b, g, split) loads S_b = seq_lens[b] (clamped to 0 .. table_len * page) and cuts its own chunk
//     L_b = 64 ceil(ceil(S_b / 64) / splits), keys [split L_b, min(S_b, (split + 1) L_b)): attn_decode_kv8.hip's host rule per
//     sequence.  A chunk at or beyond S_b (a short or an empty sequence) enters no tile and writes the empty partial (m = -inf, l = 0)
//     the combine kernel already merges at splits = 256; a sequence without keys gets zeros.  The grid is B * n_kv * splits as before,
//     and a ragged batch reads the keys that exist, not max(S) of them.
// Causal.  Query i of sequence b admits keys j <= i + S_b - T; with S_b < T the first queries admit none and get zeros.
// Tiles.  A wave's tile t0 is a multiple of 64 and a page a multiple of 64 rows, so a tile lies in ONE page: its page id
//     block_table[b][t0 / page] is one 4-byte load per tile, made wave-uniform (readfirstlane), and gives four uniform 64-bit bases --
//     K bytes, K scales, V bytes, V scales of row (t0 % page) of kv head g in that page -- from which the lanes address rows
//     0 .. 63 exactly as attn_decode_kv8.hip addresses rows t0 .. t0 + 63 of its contiguous plane.  Rows beyond the chunk's end are
//     read as the chunk's last row, which lies in the tile being read, hence in the same page.  Where the template prefetches
//     (<= 128 / 128) the next tile's table entry is loaded with the next tile's bytes.  A page id is clamped to 0 .. n_pages - 1 for
//     memory safety only: the caller's table holds valid pages wherever it may be read.
// K, V, the online softmax, the merge of the four waves and the partial row: attn_decode_kv8.hip's text, copied (that unit and
//     attn_fwd_kv8.hip keep theirs), so for every sequence the result is bit-identical to mdg_attn_decode_kv8 on that sequence alone
//     (B = 1, S = S_b, the same rows laid contiguously, the same splits).
// mask: mdg_attn_decode_masked's bool mask with last extent max_S; keys at or beyond max_S are not admitted.
#include <math.h>

#include "kv8.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = DECODE_THREADS;
constexpr int WAVES = DECODE_WAVES;

struct PagedArgs {
  const void* q;
  const unsigned char *kd, *vd;  // the pools [n_pages, n_kv, page, pitch]
  const float *ks, *vs;          //           [n_pages, n_kv, page]
  const int* table;              // [B, table_len]
  const int* seq_lens;           // [B]
  float* ws;
  int64_t T, max_S, limit, table_len, kp, vp;  // limit = table_len * page; pitches in bytes
  int page, n_pages;
  int n_heads, n_kv, G, r_qk, r_vo, causal, splits;
  int cols;            // T * G live columns
  int rp;              // r_vo rounded up to 4; a workspace row has rp + 4 floats
  int kbytes, vbytes;  // mdg_kv8_pitch(r_qk), mdg_kv8_pitch(r_vo): the bytes of a row that hold elements or their zero padding
  int vec_q;
  float c;  // scale * log2(e)
};

// attn_decode.hip's arithmetic after the logits, as two functions (that kernel keeps its own text: moving it changed its code).
// One 64-key tile of a wave, after the logits t (log2 domain) are masked: running maximum and sum, the probabilities rounded to the
// element type, o += V^T P from the wave's Vs tile.  Lane (r, hh); nv column tiles are live.
template <int DT, int NV>
__device__ __forceinline__ void softmax_pv(float (&t)[2][16], float& m, float& l, f32x16 (&o)[NV], const typename Mma<DT>::E* Vs,
                                           int r, int hh, int nv) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  float mx = t[0][0];
#pragma unroll
  for (int sub = 0; sub < 2; sub++)
#pragma unroll
    for (int i = 0; i < 16; i++) mx = fmaxf(mx, t[sub][i]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_new = fmaxf(m, mx);
  const float m_use = m_new == -INFINITY ? 0.f : m_new;  // a column with no admitted key yet: every p is exp2(-inf) = 0
  const float alpha = __builtin_amdgcn_exp2f(m - m_use);
  m = m_new;
  float sum = 0.f;
  frag pf[2][2];
#pragma unroll
  for (int sub = 0; sub < 2; sub++)
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float p = __builtin_amdgcn_exp2f(t[sub][i] - m_use);
      sum += p;
      pf[sub][i >> 3][i & 7] = (E)p;
    }
  l = l * alpha + sum;
#pragma unroll
  for (int ct = 0; ct < NV; ct++) {
    if (ct >= nv) continue;
#pragma unroll
    for (int i = 0; i < 16; i++) o[ct][i] *= alpha;
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const frag va = *(const frag*)(Vs + (ct * 32 + r) * VP + sub * 32 + s * 16 + hh * 8);
        o[ct] = Mma<DT>::mfma(va, pf[sub][s], o[ct]);
      }
  }
}

// The end of a decode workgroup: the WAVES waves' (o, m, l) meet in LDS (each wave's own Vs region, reused), are merged with weights
// 2^(m_w - M), and the workgroup writes one unnormalised fp32 partial row [O at 0 .. rp), m at [rp], l at [rp + 1]] of a live column.
template <int DT, int NV, int WAVES>
__device__ __forceinline__ void merge_store(unsigned char* smem, typename Mma<DT>::E* Vs, const f32x16 (&o)[NV], float m, float l, int lane,
                                            int wave, int hh, bool live, float* row, int rp, int nv) {
  typedef typename Mma<DT>::E E;
  constexpr int VS_ELEMS = NV * 32 * VP;
  // the waves' states meet in LDS: wave w's image [NV * 16 registers][64 lanes] of o, then m, then l (both lane halves summed)
  const float lt = l + __shfl_xor(l, 32);
  __builtin_amdgcn_wave_barrier();
  {
    float* img = (float*)Vs;
#pragma unroll
    for (int ct = 0; ct < NV; ct++)
#pragma unroll
      for (int i = 0; i < 16; i++) img[(ct * 16 + i) * 64 + lane] = o[ct][i];
    img[NV * 1024 + lane] = m;
    img[NV * 1024 + 64 + lane] = lt;
  }
  __syncthreads();
  float wgt[WAVES], M = -INFINITY, lsum = 0.f;
#pragma unroll
  for (int x = 0; x < WAVES; x++) {
    wgt[x] = ((const float*)((const E*)smem + (size_t)x * VS_ELEMS))[NV * 1024 + lane];
    M = fmaxf(M, wgt[x]);
  }
#pragma unroll
  for (int x = 0; x < WAVES; x++) {
    wgt[x] = wgt[x] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(wgt[x] - M);  // M >= that wave's m > -inf here
    lsum += wgt[x] * ((const float*)((const E*)smem + (size_t)x * VS_ELEMS))[NV * 1024 + 64 + lane];
  }
  if (!live) return;
  if (wave == 0 && hh == 0) {
    row[rp] = M;
    row[rp + 1] = lsum;
  }
  // column tiles over the waves: wave w merges and stores tiles w, w + 4
#pragma unroll
  for (int c4 = 0; c4 < (NV + WAVES - 1) / WAVES; c4++) {
    const int ct = wave + c4 * WAVES;
    if (ct >= nv) continue;
#pragma unroll
    for (int q4 = 0; q4 < 4; q4++) {
      const int c = ct * 32 + 8 * q4 + 4 * hh;  // registers 4 q4 .. 4 q4 + 3 are columns c .. c + 3
      typedef float f4 __attribute__((ext_vector_type(4)));
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int x = 0; x < WAVES; x++) {
        const float* img = (const float*)((const E*)smem + (size_t)x * VS_ELEMS);
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] += wgt[x] * img[(ct * 16 + 4 * q4 + i) * 64 + lane];
      }
      if (c < rp) *(f4*)(row + c) = acc;  // rp is a multiple of 4 and the rows are 16-byte aligned
    }
  }
}

// Two workgroups a CU (two waves a SIMD) where 256 registers a lane hold the template: <= 64 / 128 and 128 / 64.  128 / 128 has one,
// masked or not: the table lookup's bases put the unmasked template, at 255 registers in attn_decode_kv8.hip, over the limit.
template <int DT, int NQ, int NV, bool MASKED>
__global__ __launch_bounds__(THREADS, (NQ <= 8 && NV <= 4 && !(NQ == 8 && NV == 4)) ? 2 : 1) void attn_decode_paged8_kernel(PagedArgs a, MaskArgs mk) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  constexpr int NP = NQ / 2;              // 16-byte loads of a lane per key row: pairs of k-steps
  constexpr int VS_ELEMS = NV * 32 * VP;  // one wave's Vs tile; as floats it also holds the wave's (o, m, l) for the merge
  static_assert((size_t)VS_ELEMS * 2 >= ((size_t)NV * 16 * 64 + 128) * 4, "the merge image must fit the wave's Vs region");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  E* Vs = (E*)smem + (size_t)wave * VS_ELEMS;
  const int64_t bg = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - bg * a.splits);
  const int64_t b = bg / a.n_kv;
  const int g = (int)(bg - b * a.n_kv);
  const int np = (a.kbytes + 31) >> 5, nv = (a.r_vo + 31) >> 5;

  // column r of the tile: query tq, head g * G + hg
  const bool live = r < a.cols;
  const int tq = live ? r / a.G : 0;
  const int head = g * a.G + (live ? r - tq * a.G : 0);
  // the sequence's own key count and chunk: the host rule of attn_decode_kv8.hip, per sequence
  int64_t S = a.seq_lens[b];
  S = S < 0 ? 0 : S > a.limit ? a.limit : S;
  const int64_t tiles = (S + KT - 1) / KT;
  const int64_t L = KT * ((tiles + a.splits - 1) / a.splits);
  const int64_t shift = S - a.T;
  int64_t lim = S - 1;  // the last key this column admits
  if (a.causal && live && tq + shift < lim) lim = tq + shift;
  const int64_t first_lim = a.causal ? shift : S - 1;  // query 0's: the smallest of the tile

  // Q^T fragments under K's column map: B[k = 8 hh + j][col r] of k-step 2 p + e is q[query tq, head][32 p + 16 hh + 8 e + j]
  frag qf[NQ];
  {
    const E* qrow = (const E*)a.q + ((b * a.n_heads + head) * a.T + tq) * a.r_qk;
#pragma unroll
    for (int s = 0; s < NQ; s++) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (live) w = load8(qrow, 32 * (s >> 1) + 16 * hh + 8 * (s & 1), a.r_qk, a.vec_q != 0);
      qf[s] = __builtin_bit_cast(frag, w);
    }
  }

  f32x16 o[NV];
#pragma unroll
  for (int ct = 0; ct < NV; ct++)
#pragma unroll
    for (int i = 0; i < 16; i++) o[ct][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  const int64_t k0 = (int64_t)split * L;
  const int64_t kend = k0 + L < S ? k0 + L : S;
  // Rows beyond the chunk's end are read as its last row (every tile the loop visits has kend > t0 >= 0, so that row exists): their
  // logits are masked to -inf and their probabilities are exactly 0, so no load needs a predicate of its own.
  const int64_t klast = kend - 1;

  // The tile at t0 (a multiple of KT, < kend <= limit): one table load, then the uniform bases of its first row in the four planes.
  const int* trow = a.table + b * a.table_len;
  const int tiles_per_page = a.page / KT;
  // The bases are those of key 0 of a contiguous plane that has the tile's rows where the page holds them (the page's base minus
  // the tile's first key), so the lanes index them by key as attn_decode_kv8.hip does; only rows of the tile are ever addressed.
  const unsigned char *kbase, *vbase;  // of the tile fetch_k / fetch_v were last pointed at
  const float *ksb, *vsb;
  auto point_at = [&](int64_t t0) {
    const int tile = __builtin_amdgcn_readfirstlane((int)(t0 / KT));
    const int pi = tile / tiles_per_page;
    int pid = __builtin_amdgcn_readfirstlane(trow[pi]);
    pid = pid < 0 ? 0 : pid >= a.n_pages ? a.n_pages - 1 : pid;
    const int64_t slot = ((int64_t)pid * a.n_kv + g) * a.page - (int64_t)pi * a.page;  // + key: the key's row in the pool
    kbase = a.kd + slot * a.kp;
    vbase = a.vd + slot * a.vp;
    ksb = a.ks + slot;
    vsb = a.vs + slot;
  };

  constexpr bool PREFETCH = NQ <= 8 && NV <= 4;
  constexpr int VIT = NV / 2;  // V items of a lane per tile at the template's widest r_vo
  constexpr int VR = PREFETCH ? VIT : 1;
  u32x4 kreg[2][NP], vreg[VR][4];
  float ksc[2], vsc[4];
  // (written out per use, as in attn_decode.hip: a helper that takes kreg[sub] put kreg into scratch memory there)
#define MDG_FETCH_K_SUB(t0_, sub_)                                                                     \
  {                                                                                                    \
    const int64_t key_ = (t0_) + (sub_) * 32 + r;                                                      \
    const int64_t row_ = (key_ < klast ? key_ : klast);                                                \
    const unsigned char* krow_ = kbase + row_ * a.kp + 16 * hh;                                        \
    ksc[sub_] = ksb[row_];                                                                             \
    _Pragma("unroll") for (int p = 0; p < NP; p++) {                                                   \
      kreg[sub_][p] = (u32x4){0u, 0u, 0u, 0u};                                                         \
      if (p < np && 32 * p + 16 * hh < a.kbytes) kreg[sub_][p] = *(const u32x4*)(krow_ + 32 * p);      \
    }                                                                                                  \
  }
  auto fetch_k = [&](int64_t t0) {
#pragma unroll
    for (int sub = 0; sub < 2; sub++) MDG_FETCH_K_SUB(t0, sub)
  };
  const int mq = lane & 15;  // the lane's key quad: keys 4 mq .. 4 mq + 3 of the tile, in every item
  auto fetch_vscale = [&](int64_t t0) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t key = t0 + 4 * mq + i;
      vsc[i] = vsb[key < klast ? key : klast];
    }
  };
  auto fetch_item = [&](int64_t t0, int it, u32x4 (&w)[4]) {
    const int c0 = ((lane >> 4) + 4 * it) * 16;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t key = t0 + 4 * mq + i;
      w[i] = (u32x4){0u, 0u, 0u, 0u};
      if (c0 < a.vbytes) w[i] = *(const u32x4*)(vbase + (key < klast ? key : klast) * a.vp + c0);
    }
  };
  auto commit_item = [&](int it, const u32x4 (&w)[4]) {
    const int c0 = ((lane >> 4) + 4 * it) * 16;
    const int pos = v_quad_pos(mq);
#pragma unroll
    for (int h = 0; h < 2; h++) {  // columns c0 + 8 h .. + 8 of the 4 keys
      u32x4 d[4];
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = kv8::dequant8<DT>(w[i][2 * h], w[i][2 * h + 1], vsc[i]);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        u32x2 p;
        p.x = half_of(d[0][j >> 1], j & 1) | (half_of(d[1][j >> 1], j & 1) << 16);
        p.y = half_of(d[2][j >> 1], j & 1) | (half_of(d[3][j >> 1], j & 1) << 16);
        *(u32x2*)(Vs + (c0 + 8 * h + j) * VP + pos) = p;
      }
    }
  };
  auto fetch_v = [&](int64_t t0) {
    fetch_vscale(t0);
#pragma unroll
    for (int it = 0; it < VR; it++)
      if (2 * it < nv) fetch_item(t0, it, vreg[it]);  // wave-uniform
  };

  const unsigned char* mrow = nullptr;  // the column's mask row (a dead column reads query 0's of the group's first head)
  if constexpr (MASKED) mrow = mk.mask + b * mk.mbs + (mk.per_head ? head : 0) * mk.mhs + tq * mk.mqs;

  const int64_t t_first = k0 + (int64_t)wave * KT;
  if (PREFETCH && t_first < kend) {
    point_at(t_first);
    fetch_k(t_first);
    fetch_v(t_first);
  }
  for (int64_t t0 = t_first; t0 < kend; t0 += (int64_t)WAVES * KT) {
    if constexpr (!PREFETCH) point_at(t0);
    unsigned mb[2] = {0u, 0u};
    if constexpr (MASKED) {  // issued before the first product, used after it
#pragma unroll
      for (int sub = 0; sub < 2; sub++) mb[sub] = mask_bits16(mrow, t0 + 32 * sub + 4 * hh, a.max_S, mk.vec != 0);
    }
    float t[2][16];
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      if constexpr (!PREFETCH) {
        MDG_FETCH_K_SUB(t0, sub)
      }
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; i++) st[i] = 0.f;
#pragma unroll
      for (int p = 0; p < NP; p++) {
        if (p >= np) continue;  // wave-uniform
        const u32x4 w = kreg[sub][p];
        st = Mma<DT>::mfma(__builtin_bit_cast(frag, kv8::dequant8<DT>(w.x, w.y, ksc[sub])), qf[2 * p], st);
        st = Mma<DT>::mfma(__builtin_bit_cast(frag, kv8::dequant8<DT>(w.z, w.w, ksc[sub])), qf[2 * p + 1], st);
      }
#pragma unroll
      for (int i = 0; i < 16; i++) t[sub][i] = st[i] * a.c;
    }
    __builtin_amdgcn_wave_barrier();  // the wave's reads of the previous tile are issued before these writes: LDS runs a wave in order
    if constexpr (PREFETCH) {
#pragma unroll
      for (int it = 0; it < VR; it++)
        if (2 * it < nv) commit_item(it, vreg[it]);
      if (t0 + WAVES * KT < kend) {
        point_at(t0 + WAVES * KT);
        fetch_k(t0 + WAVES * KT);
        fetch_v(t0 + WAVES * KT);
      }
    } else {
      fetch_vscale(t0);
#pragma nounroll
      for (int it = 0; 2 * it < nv; it++) {
        fetch_item(t0, it, vreg[0]);
        commit_item(it, vreg[0]);
      }
    }
    __builtin_amdgcn_wave_barrier();

    const bool need_mask = t0 + KT > kend || t0 + KT - 1 > first_lim;
    if (need_mask) {
      const int64_t top = lim < kend - 1 ? lim : kend - 1;
      const int64_t d = top - t0;  // keys of this tile beyond d are not admitted
      const int rel = d < -1 ? -1 : d > KT ? KT : (int)d;
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh > rel) t[sub][i] = -INFINITY;
    }
    if constexpr (MASKED) {
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (!((mb[sub] >> i) & 1)) t[sub][i] = -INFINITY;
    }
    softmax_pv<DT, NV>(t, m, l, o, Vs, r, hh, nv);
  }

#undef MDG_FETCH_K_SUB

  float* row = a.ws + (((b * a.n_heads + head) * a.T + tq) * a.splits + split) * (int64_t)(a.rp + 4);
  merge_store<DT, NV, WAVES>(smem, Vs, o, m, l, lane, wave, hh, live, row, a.rp, nv);
}

template <int DT> int launch_paged8(const PagedArgs& a, const MaskArgs* mk, dim3 grid, hipStream_t st) {
  MDG_TRY(with_template(a.r_qk, a.r_vo, [&](auto nq, auto nv) {
    constexpr int NQ = decltype(nq)::value, NV = decltype(nv)::value;
    const size_t lds = (size_t)WAVES * NV * 32 * VP * 2;
    if (mk) return launch(attn_decode_paged8_kernel<DT, NQ, NV, true>, grid, THREADS, lds, st, a, *mk);
    return launch(attn_decode_paged8_kernel<DT, NQ, NV, false>, grid, THREADS, lds, st, a, MaskArgs{});
  }));
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_attn_decode_paged8(const void* q, const void* k_data, const void* k_scale, const void* v_data, const void* v_scale,
                                      int dtype, int64_t B, int64_t T, int64_t max_S, int n_heads, int n_kv, int r_qk, int r_vo,
                                      int64_t n_pages, int64_t page, int64_t k_pitch, int64_t v_pitch, const void* block_table,
                                      int64_t table_len, const void* seq_lens, double scale, int causal, int splits, void* ws,
                                      int64_t ws_bytes, void* out, int64_t ld_out, void* stream, const void* mask, int Hm,
                                      int64_t mask_batch_stride, int64_t mask_head_stride, int64_t mask_query_stride) {
  const char* fn = "mdg_attn_decode_paged8";
  // what the shared checks read of a call; k and v stand for the data pools, their token strides for the pitches in bytes, S for max_S
  const Call p = {q, k_data, v_data, dtype, B, T, max_S, n_heads, n_kv, r_qk, r_vo, 0, 0, k_pitch, 0, 0, v_pitch, scale, causal, out, ld_out,
                  stream};
  MDG_CLEAR();
  MDG_TRY(check_widths(fn, p));
  const int G = n_heads / n_kv;
  MDG_CHECK_ARG(T * G <= DECODE_COLS, "%s: T=%lld queries x group of %d heads exceed the tile of %d columns", fn, (long long)T, G,
                DECODE_COLS);
  MDG_CHECK_ARG(splits >= 1 && splits <= DECODE_MAX_SPLITS, "%s: splits=%d must be in 1..%d", fn, splits, DECODE_MAX_SPLITS);
  MDG_CHECK_ARG(page > 0 && page % KT == 0, "%s: page=%lld must be a positive multiple of %d", fn, (long long)page, KT);
  MDG_CHECK_ARG(n_pages >= 0 && table_len >= 0, "%s: negative n_pages or table_len", fn);
  MDG_CHECK_ARG(page <= 0x7fffffff && n_pages <= 0x7fffffff && table_len <= INT64_MAX / page, "%s: table_len*page overflows", fn);
  MDG_CHECK_ARG(max_S <= table_len * page, "%s: max_S=%lld keys exceed table_len*page=%lld", fn, (long long)max_S, (long long)(table_len * page));
  MDG_CHECK_ARG(k_pitch >= kv8::pitch_of(r_qk) && k_pitch % kv8::CHUNK == 0 && v_pitch >= kv8::pitch_of(r_vo) && v_pitch % kv8::CHUNK == 0,
                "%s: pitches (%lld, %lld) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d", fn, (long long)k_pitch,
                (long long)v_pitch, r_qk, r_vo);
  {  // the causal rule is per sequence and decided on the device (S_b < T gives zeros): max_S takes no part in it
    Call lay = p;
    lay.causal = 0;
    MDG_TRY(check_layout(fn, lay));
  }
  MDG_CHECK_ARG(T == 0 || B <= INT64_MAX / T / n_heads / DECODE_MAX_SPLITS / 1040, "%s: B*T overflows", fn);
  MDG_CHECK_ARG(n_pages == 0 || n_pages <= INT64_MAX / n_kv / page / (k_pitch > v_pitch ? k_pitch : v_pitch),
                "%s: n_pages*n_kv*page*pitch overflows", fn);
  MDG_CHECK_ARG(table_len == 0 || B <= INT64_MAX / 4 / table_len, "%s: B*table_len overflows", fn);
  if (B == 0 || T == 0) return MDG_OK;
  const bool keys = n_pages > 0 && table_len > 0;  // otherwise every sequence is empty and nothing of the pools or the table is read
  MDG_CHECK_ARG(q && out && seq_lens && (!keys || (k_data && k_scale && v_data && v_scale && block_table)), "%s: null pointer", fn);
  MDG_CHECK_ARG(!keys || ((uintptr_t)k_data % 16 == 0 && (uintptr_t)v_data % 16 == 0 && (uintptr_t)k_scale % 4 == 0 &&
                          (uintptr_t)v_scale % 4 == 0),
                "%s: data must be 16-byte and scales 4-byte aligned", fn);
  MDG_CHECK_ARG((uintptr_t)seq_lens % 4 == 0 && (!keys || (uintptr_t)block_table % 4 == 0),
                "%s: block_table and seq_lens must be 4-byte aligned", fn);
  const int64_t need = mdg_attn_decode_ws_bytes(B, T, n_heads, r_vo, splits);
  MDG_CHECK_ARG(ws != nullptr, "%s: null workspace", fn);
  MDG_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes is short of mdg_attn_decode_ws_bytes = %lld", fn, (long long)ws_bytes,
                (long long)need);
  MDG_CHECK_ARG((uintptr_t)ws % 16 == 0, "%s: workspace must be 16-byte aligned", fn);
  const size_t es = dtype_size(dtype);
  const Span target[2] = {span_of("out", out, 1, 0, 1, 0, B * T, ld_out, (int64_t)n_heads * r_vo, es),
                          Span{"workspace", (uintptr_t)ws, (uintptr_t)ws + (uintptr_t)need}};
  MDG_TRY(apart(fn, target + 1, 1, target[0]));
  MaskArgs mk{};
  if (mask) {
    const MaskCall m = {mask, Hm, mask_batch_stride, mask_head_stride, mask_query_stride};
    Span s;
    MDG_TRY(mask_args(fn, p, m, mk, s));
    MDG_TRY(apart(fn, target, 2, s));
  }
  const int64_t rows = keys ? n_pages * n_kv * page : 0;  // the pools' extents
  const Span in[7] = {span_of("q", q, 1, 0, 1, 0, B * n_heads * T, r_qk, r_qk, es),
                      Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                      Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                      Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                      Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)},
                      Span{"block_table", (uintptr_t)block_table, (uintptr_t)block_table + (uintptr_t)(keys ? B * table_len * 4 : 0)},
                      Span{"seq_lens", (uintptr_t)seq_lens, (uintptr_t)seq_lens + (uintptr_t)(B * 4)}};
  for (int i = 0; i < 7; i++) MDG_TRY(apart(fn, target, 2, in[i]));

  PagedArgs a;
  a.q = q; a.kd = (const unsigned char*)k_data; a.vd = (const unsigned char*)v_data;
  a.ks = (const float*)k_scale; a.vs = (const float*)v_scale; a.ws = (float*)ws;
  a.table = (const int*)block_table; a.seq_lens = (const int*)seq_lens;
  a.T = T; a.max_S = max_S; a.limit = keys ? table_len * page : 0; a.table_len = table_len; a.kp = k_pitch; a.vp = v_pitch;
  a.page = (int)page; a.n_pages = (int)n_pages;
  a.n_heads = n_heads; a.n_kv = n_kv; a.G = G; a.r_qk = r_qk; a.r_vo = r_vo; a.causal = causal != 0; a.splits = splits;
  a.cols = (int)T * G;
  a.rp = (r_vo + 3) / 4 * 4;
  a.kbytes = (int)kv8::pitch_of(r_qk); a.vbytes = (int)kv8::pitch_of(r_vo);
  a.vec_q = (uintptr_t)q % 16 == 0 && r_qk % 8 == 0;
  a.c = (float)(scale * 1.4426950408889634);
  MDG_CHECK_ARG(B * n_kv <= 0x7fffffff / splits && B * n_heads * T <= 0x7fffffff, "%s: B=%lld exceeds one launch", fn, (long long)B);
  const dim3 grid((unsigned)(B * n_kv * splits));
  const MaskArgs* pm = mask ? &mk : nullptr;
  if (dtype == MDG_BF16) MDG_TRY(launch_paged8<MDG_BF16>(a, pm, grid, (hipStream_t)stream));
  else MDG_TRY(launch_paged8<MDG_F16>(a, pm, grid, (hipStream_t)stream));
  return decode_combine(dtype, (const float*)ws, out, B, T, n_heads, r_vo, splits, ld_out, (hipStream_t)stream);
}
