// Split-key (flash-decoding) attention for compressed heads: the decode schedule beside attn.hip's prefill schedule, same operands
// (q [B, n_heads, T, r_qk] contiguous, k / v strided with a contiguous last dimension, out token-major rows of pitch ld_out), same
// widths (r_qk even <= 256, r_vo <= 256), same arithmetic.  Domain: T * G <= 32 with G = n_heads / n_kv -- every query row that
// shares one kv head fits the 32 query columns of ONE MFMA tile, so one read of a kv head's K and V serves the whole group.
//
// Column map.  Column c of the tile is (query c / G, head of the group c % G): the heads of one query are adjacent.  Columns
// >= T * G carry zero queries and are never stored.
//
// Split.  The keys are cut into `splits` contiguous chunks of L = 64 * ceil(ceil(S / 64) / splits) keys; a workgroup (256 threads =
// 4 waves) takes one (batch, kv head, chunk) and its wave w the 64-key tiles w, w + 4, ... of the chunk, each wave with its own
// online softmax (fp32 running maximum and sum, scale * log2(e) folded in, exp2, probabilities rounded to the element type for the
// second product: attn.hip's).  No barrier inside the key loop: nothing is shared between the waves until the end.
//   K  goes from HBM straight into the A fragments of  S^T = K Q^T:  lane (r, h) of k-step s needs k[key r][16 s + 8 h .. + 8], 16
//      contiguous bytes of a row, so there is nothing for LDS to reorder.  Every K byte is requested once.
//   V  needs the transposition and key permutation of attn.hip's Vs tile (attn_tile.hpp), through a wave-private LDS tile
//      Vs [NV * 32 columns][64 + 8]; items of 4 keys x 8 columns as there.  Every V byte is requested once.
// Where the registers allow (the templates up to 128 / 128: every width a compressed model has) the next tile's loads are issued
// before the softmax and the second product of the current one; the wider templates stage K per tile and V item by item.  A wave
// stages whole tiles alone, four times the staging registers of attn.hip's shared tiles, so only the 64 / 64 template is built for
// two workgroups per CU.
// At the end the four waves' (o, m, l) meet in LDS (each wave's own Vs region, reused), are merged with weights 2^(m_w - M), and the
// workgroup writes ONE unnormalised fp32 partial per (batch, head, query, split) to the caller's workspace:
//   ws [B][n_heads][T][splits][RP + 4] floats, RP = r_vo rounded up to 4:  O_s at [0, RP) (columns >= r_vo are zero), m_s at [RP],
//   l_s at [RP + 1], two unused floats (the rows stay 16-byte aligned).  m_s is in the log2 domain (scale * log2 e folded in).
// A chunk with no admitted key for a query -- an empty range, since splits may exceed the key tiles, or one wholly beyond the
// query's causal limit -- writes m_s = -inf, l_s = 0, O_s = 0.
//
// Combine.  A second kernel on the same stream, one workgroup per (batch, head, query):  M = max_s m_s,  w_s = 2^(m_s - M) where
// m_s > -inf and exactly 0 otherwise (-inf - -inf is never evaluated, and a split of weight 0 is not read at all),
// out = sum_s w_s O_s / sum_s w_s l_s in fp32 in split order, rounded once.  No admitted key at all: zeros.
// Two launches, no hand-off between workgroups inside one: no counters, flags or grid barriers; every run gives the same bits.
//
// Bool masks (padded batches): the MASKED variant below, behind mdg_attn_decode_masked.
// Out of scope: T * G > 32 (mdg_attn_fwd), an in-launch reduction, paged or quantised caches, sliding windows, additive float masks,
// skipping whole chunks a mask excludes, a backward pass.
#include <math.h>

#include "attn_tile.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;
constexpr int WAVES = 4;
constexpr int COLS = 32;         // query columns of the tile
constexpr int MAX_SPLITS = 256;  // also the combine kernel's workgroup size

// Position in a Vs row of the first of the 4 consecutive keys 4 mq .. 4 mq + 3 of a 64-key tile (attn.hip's permutation): inside
// k-step s of the second product element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3) of the 32-key half, so key kappa
// sits at 16 s + 8 h + 4 ((kappa >> 3) & 1) + (kappa & 3) and a lane's A fragment is one 16-byte read.
__device__ __forceinline__ int v_quad_pos(int mq) {
  const int kap = (4 * mq) & 31;
  return ((4 * mq) & 32) + (kap & 16) + ((kap >> 2) & 1) * 8 + ((kap >> 3) & 1) * 4;
}

struct DecodeArgs {
  const void* q;
  const void* k;
  const void* v;
  float* ws;
  void* out;
  int64_t T, S, L, ld_out;
  int64_t kbs, khs, kts, vbs, vhs, vts;
  int n_heads, n_kv, G, r_qk, r_vo, causal, splits;
  int cols;  // T * G live columns
  int rp;    // r_vo rounded up to 4; a workspace row has rp + 4 floats
  int vec_q, vec_k, vec_v;
  float c;  // scale * log2(e)
};

// MASKED (mdg_attn_decode_masked; `mk` is unused otherwise): column c also reads the mask row of its query (and head, when
// the mask has one per head) -- S bytes against the S (r_qk + r_vo) 2 bytes of cache the workgroups of a kv head read -- and a
// key the mask does not admit gets the logit -inf where the causal rule sets it.  No summary: every tile is loaded and multiplied.
template <int DT, int NQ, int NV, bool MASKED>
__global__ __launch_bounds__(THREADS, (NQ <= 4 && NV <= 2) ? 2 : 1) void attn_decode_kernel(DecodeArgs a, MaskArgs mk) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  constexpr int VS_ELEMS = NV * 32 * VP;  // one wave's Vs tile; as floats it also holds the wave's (o, m, l) for the merge
  static_assert((size_t)VS_ELEMS * 2 >= ((size_t)NV * 16 * 64 + 128) * 4, "the merge image must fit the wave's Vs region");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  E* Vs = (E*)smem + (size_t)wave * VS_ELEMS;
  const int64_t bg = (int64_t)blockIdx.x / a.splits;
  const int split = (int)((int64_t)blockIdx.x - bg * a.splits);
  const int64_t b = bg / a.n_kv;
  const int g = (int)(bg - b * a.n_kv);
  const int nq = (a.r_qk + 15) >> 4, nv = (a.r_vo + 31) >> 5;

  // column r of the tile: query tq, head g * G + hg
  const bool live = r < a.cols;
  const int tq = live ? r / a.G : 0;
  const int head = g * a.G + (live ? r - tq * a.G : 0);
  const int64_t shift = a.S - a.T;
  int64_t lim = a.S - 1;  // the last key this column admits
  if (a.causal && live && tq + shift < lim) lim = tq + shift;
  const int64_t first_lim = a.causal ? shift : a.S - 1;  // query 0's: the smallest of the tile

  // Q^T fragments: B[k = 8h + j][col r] of k-step s is q[query tq, head][16 s + 8 h + j]
  frag qf[NQ];
  {
    const E* qrow = (const E*)a.q + ((b * a.n_heads + head) * a.T + tq) * a.r_qk;
#pragma unroll
    for (int s = 0; s < NQ; s++) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (live) w = load8(qrow, 16 * s + 8 * hh, a.r_qk, a.vec_q != 0);
      qf[s] = __builtin_bit_cast(frag, w);
    }
  }

  f32x16 o[NV];
#pragma unroll
  for (int ct = 0; ct < NV; ct++)
#pragma unroll
    for (int i = 0; i < 16; i++) o[ct][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  const E* kbase = (const E*)a.k + b * a.kbs + (int64_t)g * a.khs;
  const E* vbase = (const E*)a.v + b * a.vbs + (int64_t)g * a.vhs;
  const int64_t k0 = (int64_t)split * a.L;
  const int64_t kend = k0 + a.L < a.S ? k0 + a.L : a.S;
  // Rows beyond the chunk's end are read as its last row (every tile the loop visits has kend > t0 >= 0, so that row exists): their
  // logits are masked to -inf and their probabilities are exactly 0, so no load needs a predicate of its own.
  const int64_t klast = kend - 1;

  // A second tile in flight where the registers allow it: the widths a compressed model has (<= 128 / 128).  The wider templates
  // stage K per 32-key half and V item by item.
  constexpr bool PREFETCH = NQ <= 8 && NV <= 4;
  constexpr int VR = PREFETCH ? NV : 1;
  u32x4 kreg[2][NQ], vreg[VR][4];
  // (written out per use, not through a helper that takes kreg[sub]: with one the compiler put kreg into scratch memory)
#define MDG_FETCH_K_SUB(t0_, sub_)                                                                          \
  {                                                                                                         \
    const int64_t key_ = (t0_) + (sub_) * 32 + r;                                                           \
    const E* krow_ = kbase + (key_ < klast ? key_ : klast) * a.kts;                                         \
    _Pragma("unroll") for (int s = 0; s < NQ; s++) {                                                        \
      kreg[sub_][s] = (u32x4){0u, 0u, 0u, 0u};                                                              \
      if (s < nq) kreg[sub_][s] = load8(krow_, 16 * s + 8 * hh, a.r_qk, a.vec_k != 0); /* wave-uniform */   \
    }                                                                                                       \
  }
  auto fetch_k = [&](int64_t t0) {
#pragma unroll
    for (int sub = 0; sub < 2; sub++) MDG_FETCH_K_SUB(t0, sub)
  };
  // V items of 4 consecutive keys x 8 columns: item idx = lane + 64 it has key quad idx & 15 and column chunk idx >> 4; its 8
  // transposed 8-byte packs land at the keys' permuted position
  auto fetch_item = [&](int64_t t0, int it, u32x4 (&w)[4]) {
    const int idx = lane + it * 64;
    const int mq = idx & 15, c0 = (idx >> 4) * 8;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t key = t0 + 4 * mq + i;
      w[i] = load8(vbase + (key < klast ? key : klast) * a.vts, c0, a.r_vo, a.vec_v != 0);
    }
  };
  auto commit_item = [&](int it, const u32x4 (&w)[4]) {
    const int idx = lane + it * 64;
    const int mq = idx & 15, c0 = (idx >> 4) * 8;
    const int pos = v_quad_pos(mq);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      u32x2 p;
      p.x = half_of(w[0][j >> 1], j & 1) | (half_of(w[1][j >> 1], j & 1) << 16);
      p.y = half_of(w[2][j >> 1], j & 1) | (half_of(w[3][j >> 1], j & 1) << 16);
      *(u32x2*)(Vs + (c0 + j) * VP + pos) = p;
    }
  };
  auto fetch_v = [&](int64_t t0) {
#pragma unroll
    for (int it = 0; it < VR; it++)
      if (it < nv) fetch_item(t0, it, vreg[it]);  // wave-uniform
  };

  const unsigned char* mrow = nullptr;  // the column's mask row (a dead column reads query 0's of the group's first head)
  if constexpr (MASKED) mrow = mk.mask + b * mk.mbs + (mk.per_head ? head : 0) * mk.mhs + tq * mk.mqs;

  const int64_t t_first = k0 + (int64_t)wave * KT;
  if (PREFETCH && t_first < kend) {
    fetch_k(t_first);
    fetch_v(t_first);
  }
  for (int64_t t0 = t_first; t0 < kend; t0 += (int64_t)WAVES * KT) {
    unsigned mb[2] = {0u, 0u};
    if constexpr (MASKED) {  // issued before the first product, used after it
#pragma unroll
      for (int sub = 0; sub < 2; sub++) mb[sub] = mask_bits16(mrow, t0 + 32 * sub + 4 * hh, a.S, mk.vec != 0);
    }
    float t[2][16];
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      if constexpr (!PREFETCH) MDG_FETCH_K_SUB(t0, sub)
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; i++) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NQ; s++) {
        if (s < nq) st = Mma<DT>::mfma(__builtin_bit_cast(frag, kreg[sub][s]), qf[s], st);  // wave-uniform
      }
#pragma unroll
      for (int i = 0; i < 16; i++) t[sub][i] = st[i] * a.c;
    }
    __builtin_amdgcn_wave_barrier();  // the wave's reads of the previous tile are issued before these writes: LDS runs a wave in order
    if constexpr (PREFETCH) {
#pragma unroll
      for (int it = 0; it < VR; it++)
        if (it < nv) commit_item(it, vreg[it]);
      if (t0 + WAVES * KT < kend) {
        fetch_k(t0 + WAVES * KT);
        fetch_v(t0 + WAVES * KT);
      }
    } else {
#pragma nounroll
      for (int it = 0; it < nv; it++) {
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

#undef MDG_FETCH_K_SUB

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
  float* row = a.ws + (((b * a.n_heads + head) * a.T + tq) * a.splits + split) * (int64_t)(a.rp + 4);
  if (wave == 0 && hh == 0) {
    row[a.rp] = M;
    row[a.rp + 1] = lsum;
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
      if (c < a.rp) *(f4*)(row + c) = acc;  // rp is a multiple of 4 and the rows are 16-byte aligned
    }
  }
}

// One workgroup of MAX_SPLITS threads per (batch, head, query): thread s owns split s's weight, then thread c owns output column c.
template <int DT> __global__ __launch_bounds__(MAX_SPLITS) void attn_combine_kernel(DecodeArgs a) {
  typedef typename Mma<DT>::E E;
  __shared__ float wsh[MAX_SPLITS], lsh[MAX_SPLITS], red[MAX_SPLITS / 64];
  const int tid = threadIdx.x;
  const int64_t rowi = blockIdx.x;  // (b * n_heads + head) * T + tq
  const int64_t bh = rowi / a.T;
  const int64_t tq = rowi - bh * a.T;
  const int64_t b = bh / a.n_heads;
  const int head = (int)(bh - b * a.n_heads);
  const int rw = a.rp + 4;
  const float* part = a.ws + rowi * a.splits * rw;
  float ms = -INFINITY, ls = 0.f;
  if (tid < a.splits) {
    ms = part[(int64_t)tid * rw + a.rp];
    ls = part[(int64_t)tid * rw + a.rp + 1];
  }
  float M = ms;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) M = fmaxf(M, __shfl_xor(M, d));
  if ((tid & 63) == 0) red[tid >> 6] = M;
  __syncthreads();
  M = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // a split with no admitted key weighs exactly 0 and -inf - -inf is never formed; M == -inf only when every split is such
  const float w = ms == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(ms - M);
  wsh[tid] = w;
  lsh[tid] = w == 0.f ? 0.f : w * ls;
  __syncthreads();
  if (tid >= a.r_vo) return;
  float den = 0.f, acc = 0.f;
  for (int s = 0; s < a.splits; s++) {
    const float ws_ = wsh[s];
    if (ws_ == 0.f) continue;  // contributes exactly nothing, and its partial is not read
    den += lsh[s];
    acc += ws_ * part[(int64_t)s * rw + tid];
  }
  const float inv = den > 0.f ? 1.0f / den : 0.f;
  E* orow = (E*)a.out + (b * a.T + tq) * a.ld_out + (int64_t)head * a.r_vo;
  orow[tid] = (E)(acc * inv);
}

template <int DT> int launch_decode(const DecodeArgs& a, const MaskArgs* mk, dim3 grid, dim3 rows, hipStream_t st) {
  MDG_TRY(with_template(a.r_qk, a.r_vo, [&](auto nq, auto nv) {
    constexpr int NQ = decltype(nq)::value, NV = decltype(nv)::value;
    const size_t lds = (size_t)WAVES * NV * 32 * VP * 2;
    if (mk) return launch(attn_decode_kernel<DT, NQ, NV, true>, grid, THREADS, lds, st, a, *mk);
    return launch(attn_decode_kernel<DT, NQ, NV, false>, grid, THREADS, lds, st, a, MaskArgs{});
  }));
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL((attn_combine_kernel<DT>), rows, dim3(MAX_SPLITS), 0, st, a);
  return MDG_OK;
}

int64_t ws_row_floats(int r_vo) { return (int64_t)((r_vo + 3) / 4 * 4 + 4); }

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int64_t mdg_attn_decode_ws_bytes(int64_t B, int64_t T, int n_heads, int r_vo, int splits) {
  if (B <= 0 || T <= 0 || n_heads <= 0 || r_vo <= 0 || splits <= 0) return 0;
  return B * T * n_heads * splits * ws_row_floats(r_vo) * (int64_t)sizeof(float);
}

extern "C" int mdg_attn_decode_splits(int64_t B, int n_kv, int64_t S, int n_cu) {
  if (B <= 0 || n_kv <= 0 || S <= 0 || n_cu <= 0) return 1;
  // enough workgroups to give every CU one, but no chunk under 4 key tiles, one for each wave (the sweep)
  const int64_t tiles = ceil_div(S, KT);
  const int64_t quads = ceil_div(tiles, WAVES);
  const int64_t cap = quads < MAX_SPLITS ? quads : MAX_SPLITS;
  const int64_t want = (int64_t)n_cu / (B * n_kv);
  return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

// Both entries: `fn` names the caller in the messages; `m` is mdg_attn_decode_masked's (null otherwise).
static int attn_decode_entry(const char* fn, const Call& p, const MaskCall* m, int splits, void* ws, int64_t ws_bytes) {
  MDG_CLEAR();
  MDG_TRY(check_widths(fn, p));
  const int G = p.n_heads / p.n_kv;
  MDG_CHECK_ARG(p.T * G <= COLS, "%s: T=%lld queries x group of %d heads exceed the tile of %d columns (use mdg_attn_fwd)", fn,
                (long long)p.T, G, COLS);
  MDG_CHECK_ARG(splits >= 1 && splits <= MAX_SPLITS, "%s: splits=%d must be in 1..%d", fn, splits, MAX_SPLITS);
  MDG_TRY(check_layout(fn, p));
  MDG_CHECK_ARG(p.T == 0 || p.B <= INT64_MAX / p.T / p.n_heads / MAX_SPLITS / 1040, "%s: B*T overflows", fn);
  if (p.B == 0 || p.T == 0) return MDG_OK;
  MDG_TRY(check_pointers(fn, p));
  const int64_t need = mdg_attn_decode_ws_bytes(p.B, p.T, p.n_heads, p.r_vo, splits);
  MDG_CHECK_ARG(ws != nullptr, "%s: null workspace", fn);
  MDG_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes is short of mdg_attn_decode_ws_bytes = %lld", fn,
                (long long)ws_bytes, (long long)need);
  MDG_CHECK_ARG((uintptr_t)ws % 16 == 0, "%s: workspace must be 16-byte aligned", fn);
  Span sp[4];  // out, q, k, v
  operand_spans(p, sp);
  const Span target[2] = {sp[0], Span{"workspace", (uintptr_t)ws, (uintptr_t)ws + (uintptr_t)need}};
  MDG_TRY(apart(fn, target + 1, 1, sp[0]));
  MaskArgs mk{};
  if (m) {  // the mask's own checks and its span come before q, k and v
    Span s;
    MDG_TRY(mask_args(fn, p, *m, mk, s));
    MDG_TRY(apart(fn, target, 2, s));
  }
  for (int i = 1; i < 4; i++) MDG_TRY(apart(fn, target, 2, sp[i]));

  DecodeArgs a;
  fill_args(a, p);
  a.ws = (float*)ws;
  a.L = KT * ceil_div(ceil_div(p.S, KT), splits);
  a.splits = splits;
  a.cols = (int)p.T * G;
  a.rp = (p.r_vo + 3) / 4 * 4;
  MDG_CHECK_ARG(p.B * p.n_kv <= 0x7fffffff / splits && p.B * p.n_heads * p.T <= 0x7fffffff, "%s: B=%lld exceeds one launch", fn,
                (long long)p.B);
  const dim3 grid((unsigned)(p.B * p.n_kv * splits)), rows((unsigned)(p.B * p.n_heads * p.T));
  const MaskArgs* pm = m ? &mk : nullptr;
  if (p.dtype == MDG_BF16) MDG_TRY(launch_decode<MDG_BF16>(a, pm, grid, rows, (hipStream_t)p.stream));
  else MDG_TRY(launch_decode<MDG_F16>(a, pm, grid, rows, (hipStream_t)p.stream));
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" int mdg_attn_decode(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads,
                               int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride,
                               int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
                               double scale, int causal, int splits, void* ws, int64_t ws_bytes, void* out, int64_t ld_out,
                               void* stream) {
  const Call p = {q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, k_batch_stride, k_head_stride, k_token_stride,
                  v_batch_stride, v_head_stride, v_token_stride, scale, causal, out, ld_out, stream};
  return attn_decode_entry("mdg_attn_decode", p, nullptr, splits, ws, ws_bytes);
}

extern "C" int mdg_attn_decode_masked(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S,
                                      int n_heads, int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride,
                                      int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride,
                                      int64_t v_token_stride, double scale, int causal, int splits, void* ws, int64_t ws_bytes,
                                      void* out, int64_t ld_out, void* stream, const void* mask, int Hm, int64_t mask_batch_stride,
                                      int64_t mask_head_stride, int64_t mask_query_stride) {
  const Call p = {q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, k_batch_stride, k_head_stride, k_token_stride,
                  v_batch_stride, v_head_stride, v_token_stride, scale, causal, out, ld_out, stream};
  const MaskCall m = {mask, Hm, mask_batch_stride, mask_head_stride, mask_query_stride};
  return attn_decode_entry("mdg_attn_decode_masked", p, &m, splits, ws, ws_bytes);
}
