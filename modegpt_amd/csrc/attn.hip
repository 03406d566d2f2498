// Fused causal attention forward for compressed heads: q/k head width r_qk (even, <= 256) and v/o head width r_vo (any, <= 256)
// are independent and arbitrary -- the shapes a compressed layer has (patchers/compressed_attention.py), which the fused back
// ends behind torch's sdpa (one width for q, k and v) are not written for.  Flash-style: nothing of size T x S touches HBM.
//   q [B, n_heads, T, r_qk] contiguous (what mdg_rope_gather writes), k [B, n_kv, S, r_qk], v [B, n_kv, S, r_vo] strided with a
//   contiguous last dimension (a cache's view), out [B*T, n_heads*r_vo] rows of pitch ld_out: the token-major rows o_proj reads.
//
// Tiling.  256 threads = 4 waves; a wave owns one UNIT = 32 consecutive queries of one query head and keeps its whole state in
// registers.  Units of a (batch, kv head) are ordered (query tile, head of the group), a workgroup takes 4 consecutive units, so
// the 4 waves share every K/V tile the workgroup stages: with a group of 4 heads a kv head is read once per query tile of the
// group; with 8 heads twice, with 1 head once per 128 queries.  Key tiles of 64 are staged in LDS by all 256 threads:
//   Ks [64 keys][DQ + 8]   row-major, columns >= r_qk and keys >= S zero-filled (the padding lives in LDS only)
//   Vs [DV cols][64 + 8]   TRANSPOSED, and the keys of each 32-key half in the permuted order the second product needs (below)
// First product  S^T = K Q^T  on v_mfma_f32_32x32x16: A = K rows from LDS (one 16-byte read per k-step), B = the wave's Q
// fragments, loaded once from HBM into registers.  The result has the QUERY on the lane (col = lane & 31) and 16 keys in the
// lane's registers (key = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so the row maximum and sum are in-lane reductions plus one
// exchange between the lane halves, and the rescale of the output accumulator is a per-lane scalar.
// Second product  O^T = V^T P^T: P^T is the first product's accumulator, rounded to the element type in registers and used as the
// B operand with no lane movement (cdna_hip_programming.md section 3, "an accumulator tile as the next MFMA's operand").  Inside
// k-step s element j of lane half h is then key 16 s + 8 (j >> 2) + 4 h + (j & 3) of the 32-key half, not key 16 s + 8 h + j; Vs
// stores key kappa at position 16 s + 8 h + 4 ((kappa >> 3) & 1) + (kappa & 3) so that a lane's A fragment is again one 16-byte read.
// Online softmax over 64 keys at a time: running maximum and sum in fp32, scale * log2(e) folded into one multiply, exp2.
// Staging is split into fetch (HBM -> registers) and commit (registers -> LDS): the next tile's fetch is issued before the current
// tile's products, and the templates up to 128 / 128 are built for two waves per SIMD, so loads overlap matrix work.
// Causal: query i sees keys j <= i + (S - T).  Key tiles above a wave's last query are skipped; only tiles that cross the limit of
// one of the wave's queries (or the end of the keys) apply the mask.
//
// Load paths, chosen on the host per operand from its address and strides: aligned 16-byte loads when base and every stride are
// multiples of 16 bytes; otherwise (r_vo = 77 in bf16 has 154-byte rows) 16-byte loads at 2-byte alignment; a row's tail chunk of
// fewer than 8 elements is always read element by element.  The output is stored 8 bytes at a time when out, ld_out and r_vo
// allow it, element-wise otherwise.
//
// Decode (T * group <= 32) has a schedule of its own, split over the keys: attn_decode.hip.  Here it is correct, a wave then carries
// one query.  Bool masks (padded batches): the MASKED variant below, behind mdg_attn_fwd_masked, with attn_mask.hip's tile summary.
// Out of scope: sliding windows, additive float masks, dropout, returning attention weights, a backward pass, fp32 inputs.
#include <math.h>

#include "attn_tile.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;
constexpr int WAVES = 4;
constexpr int QT = 32;   // queries per wave

struct AttnArgs {
  const void* q;
  const void* k;
  const void* v;
  void* out;
  int64_t T, S, ld_out, units;
  int64_t kbs, khs, kts, vbs, vhs, vts;
  int n_heads, n_kv, G, r_qk, r_vo, causal;
  int wg_per_bg;  // workgroups per (batch, kv head)
  int vec_q, vec_k, vec_v, vec_o;
  float c;  // scale * log2(e)
};

// MASKED (mdg_attn_fwd_masked; `mk` is unused otherwise and the unmasked instantiations compile to the instructions they had before
// the flag existed): every tile is first looked up in the caller's tile summary.  Tiles
// that admit nothing for all of the workgroup's units are neither staged nor visited -- every thread derives that from the same
// summary bytes (lane x of every wave reads the bytes of tile 64 grp + x and a ballot makes a 64-tile word), so the decision is
// workgroup-uniform and the two barriers are skipped together; a wave skips the products of a tile that admits nothing for its own
// unit, runs the unmasked code on a tile that admits everything, and reads the mask only for a mixed tile.
template <int DT, int NQ, int NV, bool MASKED>
__global__ __launch_bounds__(THREADS, (NQ <= 8 && NV <= 4) ? 2 : 1) void attn_fwd_kernel(AttnArgs a, MaskArgs mk) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  constexpr int KP = NQ * 16 + 8;  // Ks pitch in elements
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  E* Ks = (E*)smem;       // [KT][KP]
  E* Vs = Ks + KT * KP;   // [NV * 32][VP]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int64_t bg = (int64_t)blockIdx.x / a.wg_per_bg;
  const int wgi = a.wg_per_bg - 1 - (int)((int64_t)blockIdx.x - bg * a.wg_per_bg);  // the longest key ranges start first
  const int64_t b = bg / a.n_kv;
  const int g = (int)(bg - b * a.n_kv);
  const int64_t u0 = (int64_t)wgi * WAVES, u = u0 + wave;
  const bool live = u < a.units;
  const int64_t qt = u / a.G;
  const int head = g * a.G + (int)(u - qt * a.G);
  const int64_t q0 = qt * QT, qi = q0 + r;
  const int64_t shift = a.S - a.T;
  const int nq = (a.r_qk + 15) >> 4, nv = (a.r_vo + 31) >> 5;

  // key range of this wave and of the workgroup (its last live unit sees the most keys)
  int64_t wave_end = 0;
  if (live) {
    const int64_t qlast = q0 + QT - 1 < a.T - 1 ? q0 + QT - 1 : a.T - 1;
    wave_end = a.causal && qlast + shift + 1 < a.S ? qlast + shift + 1 : a.S;
  }
  int64_t wg_end;
  {
    const int64_t ul = u0 + WAVES - 1 < a.units - 1 ? u0 + WAVES - 1 : a.units - 1;
    const int64_t ql0 = (ul / a.G) * QT;
    const int64_t ql = ql0 + QT - 1 < a.T - 1 ? ql0 + QT - 1 : a.T - 1;
    wg_end = a.causal && ql + shift + 1 < a.S ? ql + shift + 1 : a.S;
  }

  // the wave's Q^T fragments: B[k = 8h + j][col = query r] of k-step s is q[query r][16 s + 8 h + j]
  const bool qok = live && qi < a.T;
  frag qf[NQ];
  {
    const E* qrow = (const E*)a.q + ((b * a.n_heads + head) * a.T + (qok ? qi : 0)) * a.r_qk;
#pragma unroll
    for (int s = 0; s < NQ; s++) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (qok) w = load8(qrow, 16 * s + 8 * hh, a.r_qk, a.vec_q != 0);
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
  const int kcpr = nq * 2;   // 8-element chunks per K row
  const int vcpr = nv * 4;   // 8-element chunks per V row

  // Staging in two halves: fetch (HBM -> registers) and commit (registers -> LDS).  With PREFETCH the next tile's fetch is issued
  // before the products of the current one, so its latency hides under them; the widest template has no registers to spare.
  constexpr bool PREFETCH = !(NQ == 16 && NV == 8);
  constexpr int KIT = (KT * NQ * 2 + THREADS - 1) / THREADS;  // K chunks per thread at the template's widest r_qk
  constexpr int VIT = (16 * NV * 4 + THREADS - 1) / THREADS;  // V items (4 keys x 8 columns) per thread
  u32x4 kreg[KIT], vreg[VIT][4];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int it = 0; it < KIT; it++) {
      const int idx = tid + it * THREADS;
      kreg[it] = (u32x4){0u, 0u, 0u, 0u};
      if (idx < KT * kcpr) {
        const int row = idx / kcpr, c0 = (idx - row * kcpr) * 8;
        const int64_t key = t0 + row;
        if (key < a.S) kreg[it] = load8(kbase + key * a.kts, c0, a.r_qk, a.vec_k != 0);
      }
    }
#pragma unroll
    for (int it = 0; it < VIT; it++) {
      const int idx = tid + it * THREADS;
      const int mq = idx & 15, c0 = (idx >> 4) * 8;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int64_t key = t0 + 4 * mq + i;
        vreg[it][i] = (u32x4){0u, 0u, 0u, 0u};
        if (idx < 16 * vcpr && key < a.S) vreg[it][i] = load8(vbase + key * a.vts, c0, a.r_vo, a.vec_v != 0);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < KIT; it++) {
      const int idx = tid + it * THREADS;
      if (idx < KT * kcpr) {
        const int row = idx / kcpr, c0 = (idx - row * kcpr) * 8;
        *(u32x4*)(Ks + row * KP + c0) = kreg[it];
      }
    }
    // V: an item is 4 consecutive keys x 8 columns; its 8 transposed 8-byte packs land at the keys' permuted position
#pragma unroll
    for (int it = 0; it < VIT; it++) {
      const int idx = tid + it * THREADS;
      if (idx < 16 * vcpr) {
        const int mq = idx & 15, c0 = (idx >> 4) * 8;
        const int kap = (4 * mq) & 31;
        const int pos = ((4 * mq) & 32) + (kap & 16) + ((kap >> 2) & 1) * 8 + ((kap >> 3) & 1) * 4;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          u32x2 p;
          p.x = half_of(vreg[it][0][j >> 1], j & 1) | (half_of(vreg[it][1][j >> 1], j & 1) << 16);
          p.y = half_of(vreg[it][2][j >> 1], j & 1) | (half_of(vreg[it][3][j >> 1], j & 1) << 16);
          *(u32x2*)(Vs + (c0 + j) * VP + pos) = p;
        }
      }
    }
  };

  // MASKED: the summary words of the 64 key tiles [64 grp, 64 grp + 64): bit x of wg_any = tile 64 grp + x admits something for one
  // of the workgroup's units, of my_any / my_mix = for this wave's unit / only part of it.  All wave-uniform.
  int64_t grp = -1;
  unsigned long long wg_any = 0, my_any = 0, my_mix = 0;
  const unsigned char* mrow = nullptr;  // the lane's mask row
  auto next_live = [&](int64_t tile) -> int64_t {  // the first key tile >= tile the workgroup has to stage; ktiles when none
    while (tile < mk.ktiles) {
      const int64_t gq = tile >> 6;
      if (gq != grp) {
        grp = gq;
        const int64_t kt = gq * 64 + lane;
        unsigned any = 0, mine = 0;
        if (kt < mk.ktiles) {
#pragma unroll
          for (int w = 0; w < WAVES; w++) {
            const int64_t uw = u0 + w;
            if (uw < a.units) {
              const int64_t qtw = uw / a.G;
              const int64_t hw = mk.per_head ? g * a.G + (uw - qtw * a.G) : 0;
              const int64_t mh = mk.per_head ? a.n_heads : 1;
              const unsigned s = mk.summary[((b * mh + hw) * mk.qtiles + qtw) * mk.ktiles + kt];
              any |= s;
              if (w == wave) mine = s;
            }
          }
        }
        wg_any = __ballot(any != 0);
        my_any = __ballot(mine != 0);
        my_mix = __ballot(mine == MASK_MIXED);
      }
      const unsigned long long rest = wg_any >> (tile & 63);
      if (rest) return tile + __builtin_ctzll(rest);
      tile = (gq + 1) << 6;
    }
    return mk.ktiles;
  };
  int64_t first = 0, tn = 0;  // MASKED: the first live tile's key, the next one's
  if constexpr (MASKED) {
    const int64_t hm = mk.per_head ? head : 0;
    mrow = mk.mask + b * mk.mbs + hm * mk.mhs + (qi < a.T ? qi : a.T - 1) * mk.mqs;
    first = next_live(0) * KT;
  }
  if (PREFETCH && wg_end > first) fetch(first);
  for (int64_t t0 = first; t0 < wg_end; t0 = MASKED ? tn : t0 + KT) {
    bool none = false, mixed = false;
    if constexpr (MASKED) {  // this tile's state for the wave's unit, taken before next_live moves the words on
      const int x = (int)(t0 / KT) & 63;
      none = !((my_any >> x) & 1);
      mixed = (my_mix >> x) & 1;
    }
    __syncthreads();  // every wave is done with the previous tile
    if constexpr (PREFETCH) {
      commit();
    } else {  // item by item: nothing of the tile stays in registers (written out: through shared per-item helpers the compiler put
              // kreg / vreg into scratch memory)
      for (int idx = tid; idx < KT * kcpr; idx += THREADS) {
        const int row = idx / kcpr, c0 = (idx - row * kcpr) * 8;
        const int64_t key = t0 + row;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (key < a.S) w = load8(kbase + key * a.kts, c0, a.r_qk, a.vec_k != 0);
        *(u32x4*)(Ks + row * KP + c0) = w;
      }
      // V: an item is 4 consecutive keys x 8 columns; its 8 transposed 8-byte packs land at the keys' permuted position
      for (int idx = tid; idx < 16 * vcpr; idx += THREADS) {
        const int mq = idx & 15, c0 = (idx >> 4) * 8;
        u32x4 w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int64_t key = t0 + 4 * mq + i;
          w[i] = (u32x4){0u, 0u, 0u, 0u};
          if (key < a.S) w[i] = load8(vbase + key * a.vts, c0, a.r_vo, a.vec_v != 0);
        }
        const int kap = (4 * mq) & 31;
        const int pos = ((4 * mq) & 32) + (kap & 16) + ((kap >> 2) & 1) * 8 + ((kap >> 3) & 1) * 4;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          u32x2 p;
          p.x = half_of(w[0][j >> 1], j & 1) | (half_of(w[1][j >> 1], j & 1) << 16);
          p.y = half_of(w[2][j >> 1], j & 1) | (half_of(w[3][j >> 1], j & 1) << 16);
          *(u32x2*)(Vs + (c0 + j) * VP + pos) = p;
        }
      }
    }
    __syncthreads();
    if constexpr (MASKED) {  // the prefetch targets the next LIVE tile
      tn = next_live(t0 / KT + 1) * KT;
      if (PREFETCH && tn < wg_end) fetch(tn);
    } else {
      if (PREFETCH && t0 + KT < wg_end) fetch(t0 + KT);
    }
    if (!live || t0 >= wave_end) continue;  // wave-uniform; the barriers above are outside
    unsigned mb[2] = {0u, 0u};
    if constexpr (MASKED) {
      if (none) continue;  // wave-uniform as well
      if (mixed) {         // issued before the first product, used after it
#pragma unroll
        for (int sub = 0; sub < 2; sub++) mb[sub] = mask_bits16(mrow, t0 + 32 * sub + 4 * hh, a.S, mk.vec != 0);
      }
    }

    float t[2][16];
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; i++) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NQ; s++) {
        if (s < nq) {  // wave-uniform; a break would keep the loop rolled and qf in scratch
          const frag ka = *(const frag*)(Ks + (sub * 32 + r) * KP + 16 * s + 8 * hh);
          st = Mma<DT>::mfma(ka, qf[s], st);
        }
      }
#pragma unroll
      for (int i = 0; i < 16; i++) t[sub][i] = st[i] * a.c;
    }
    const bool need_mask = t0 + KT > a.S || (a.causal && t0 + KT - 1 > q0 + shift);
    if (need_mask) {
      int64_t lim = a.S - 1;
      if (a.causal && qi + shift < lim) lim = qi + shift;
      const int64_t d = lim - t0;  // keys of this tile beyond d are not admitted
      const int rel = d < -1 ? -1 : d > KT ? KT : (int)d;
#pragma unroll
      for (int sub = 0; sub < 2; sub++)
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh > rel) t[sub][i] = -INFINITY;
    }
    if constexpr (MASKED) {
      if (mixed) {
#pragma unroll
        for (int sub = 0; sub < 2; sub++)
#pragma unroll
          for (int i = 0; i < 16; i++)
            if (!((mb[sub] >> i) & 1)) t[sub][i] = -INFINITY;
      }
    }
    float mx = t[0][0];
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int i = 0; i < 16; i++) mx = fmaxf(mx, t[sub][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;  // a query with no admitted key yet: every p is exp2(-inf) = 0
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

  const float lt = l + __shfl_xor(l, 32);  // the two lane halves of a query hold the sums of their own keys
  if (!qok) return;
  const float inv = lt > 0.f ? 1.0f / lt : 0.f;
  E* orow = (E*)a.out + (b * a.T + qi) * a.ld_out + (int64_t)head * a.r_vo;
#pragma unroll
  for (int ct = 0; ct < NV; ct++) {
    if (ct >= nv) continue;
#pragma unroll
    for (int q4 = 0; q4 < 4; q4++) {
      const int c = ct * 32 + 8 * q4 + 4 * hh;  // registers 4 q4 .. 4 q4 + 3 are columns c .. c + 3
      typedef E e4 __attribute__((ext_vector_type(4)));
      e4 e;
#pragma unroll
      for (int i = 0; i < 4; i++) e[i] = (E)(o[ct][4 * q4 + i] * inv);
      if (a.vec_o && c + 4 <= a.r_vo) {
        *(e4*)(orow + c) = e;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (c + i < a.r_vo) orow[c + i] = e[i];
      }
    }
  }
}

template <int DT> int launch_attn(const AttnArgs& a, const MaskArgs* mk, dim3 grid, hipStream_t st) {
  return with_template(a.r_qk, a.r_vo, [&](auto nq, auto nv) {
    constexpr int NQ = decltype(nq)::value, NV = decltype(nv)::value;
    const size_t lds = ((size_t)KT * (NQ * 16 + 8) + (size_t)NV * 32 * VP) * 2;
    if (mk) return launch(attn_fwd_kernel<DT, NQ, NV, true>, grid, THREADS, lds, st, a, *mk);
    return launch(attn_fwd_kernel<DT, NQ, NV, false>, grid, THREADS, lds, st, a, MaskArgs{});
  });
}

// Both entries: `fn` names the caller in the messages; `m`, `summary` and `summary_bytes` are mdg_attn_fwd_masked's (m null otherwise).
int attn_fwd_entry(const char* fn, const Call& p, const MaskCall* m, const void* summary, int64_t summary_bytes) {
  MDG_CLEAR();
  MDG_TRY(check_widths(fn, p));
  MDG_TRY(check_layout(fn, p));
  MDG_CHECK_ARG(p.T == 0 || p.B <= INT64_MAX / p.T / p.n_heads / 256, "%s: B*T overflows", fn);
  if (p.B == 0 || p.T == 0) return MDG_OK;
  MDG_TRY(check_pointers(fn, p));
  Span sp[4];  // out, q, k, v
  operand_spans(p, sp);
  for (int i = 1; i < 4; i++) MDG_TRY(apart(fn, sp, 1, sp[i]));
  MaskArgs mk{};
  if (m) {  // the mask's own checks come before its span, the summary's before the summary's
    Span s;
    MDG_TRY(mask_args(fn, p, *m, mk, s));
    MDG_TRY(apart(fn, sp, 1, s));
    const int64_t need = mdg_attn_mask_summary_bytes(p.B, m->Hm, p.T, p.S);
    MDG_CHECK_ARG(summary != nullptr || need == 0, "%s: null summary", fn);
    MDG_CHECK_ARG(summary_bytes >= need, "%s: summary of %lld bytes is short of mdg_attn_mask_summary_bytes = %lld", fn,
                  (long long)summary_bytes, (long long)need);
    MDG_TRY(apart(fn, sp, 1, Span{"summary", (uintptr_t)summary, (uintptr_t)summary + (uintptr_t)need}));
    mk.summary = (const unsigned char*)summary;
  }

  AttnArgs a;
  fill_args(a, p);
  a.units = ceil_div(p.T, QT) * a.G;
  const int64_t wg = ceil_div(a.units, WAVES);
  MDG_CHECK_ARG(wg <= 0x7fffffff && p.B * p.n_kv <= 0x7fffffff / wg, "%s: B=%lld, T=%lld exceed one launch", fn, (long long)p.B,
                (long long)p.T);
  a.wg_per_bg = (int)wg;
  a.vec_o = (uintptr_t)p.out % 8 == 0 && p.ld_out % 4 == 0 && p.r_vo % 4 == 0;
  const dim3 grid((unsigned)(p.B * p.n_kv * wg));
  const MaskArgs* pm = m ? &mk : nullptr;
  if (p.dtype == MDG_BF16) MDG_TRY(launch_attn<MDG_BF16>(a, pm, grid, (hipStream_t)p.stream));
  else MDG_TRY(launch_attn<MDG_F16>(a, pm, grid, (hipStream_t)p.stream));
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_attn_fwd(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S, int n_heads,
                            int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                            int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, double scale, int causal,
                            void* out, int64_t ld_out, void* stream) {
  const Call p = {q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, k_batch_stride, k_head_stride, k_token_stride,
                  v_batch_stride, v_head_stride, v_token_stride, scale, causal, out, ld_out, stream};
  return attn_fwd_entry("mdg_attn_fwd", p, nullptr, nullptr, 0);
}

extern "C" int mdg_attn_fwd_masked(const void* q, const void* k, const void* v, int dtype, int64_t B, int64_t T, int64_t S,
                                   int n_heads, int n_kv, int r_qk, int r_vo, int64_t k_batch_stride, int64_t k_head_stride,
                                   int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
                                   double scale, int causal, void* out, int64_t ld_out, void* stream, const void* mask, int Hm,
                                   int64_t mask_batch_stride, int64_t mask_head_stride, int64_t mask_query_stride,
                                   const void* summary, int64_t summary_bytes) {
  const Call p = {q, k, v, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, k_batch_stride, k_head_stride, k_token_stride,
                  v_batch_stride, v_head_stride, v_token_stride, scale, causal, out, ld_out, stream};
  const MaskCall m = {mask, Hm, mask_batch_stride, mask_head_stride, mask_query_stride};
  return attn_fwd_entry("mdg_attn_fwd_masked", p, &m, summary, summary_bytes);
}
