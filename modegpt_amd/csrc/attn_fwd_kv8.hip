// mdg_attn_fwd's product from an fp8 KV cache (layout: include/modegpt_hip.h; written by kv8.hip): any T, the causal rule
// j <= i + S - T or every key, GQA, an optional bool mask with attn_mask.hip's tile summary -- attn.hip's schedule behind a front end
// of its own.  A cache row is `pitch` bytes of e4m3, 16-byte aligned and zero-padded to a multiple of 16, with one power-of-two fp32
// scale: every load is an aligned 16-byte load, there is no vec_k / vec_v choice and no element-wise tail.
//
// Work split (attn.hip's, unchanged: it is what shares every staged tile among the heads of a group).  256 threads = 4 waves; a wave
// owns one UNIT = 32 consecutive queries of one query head, with its Q fragments, the O^T accumulator, running maximum and sum in
// registers; a workgroup takes 4 consecutive units of one (batch, kv head) in the order (query tile, head of the group); key tiles
// of 64; the workgroups with the longest key ranges start first.
//
// Fetch (HBM -> registers), all 256 threads, raw bytes:
//   K   chunk idx = tid + 256 it, it < NQ / 4:  key row = idx / nq, 16-byte chunk ch = idx % nq  (nq = ceil(r_qk / 16) = pitch_of(r_qk) / 16
//       chunks a row, 64 nq a tile); one 16-byte load and the row's scale as one 4-byte load.
//   V   item tid (one per thread: 16 key quads x 2 NV chunks <= 256): key quad mq = tid & 15 -> keys 4 mq .. 4 mq + 3, 16-byte chunk
//       tid >> 4 -> columns 16 (tid >> 4) .. + 15; four 16-byte loads and the quad's four row scales.
//   A key >= S is not requested: its bytes are zero in registers and its scale is 1 (rows beyond S hold anything).  A V chunk at or
//   beyond pitch_of(r_vo) is not requested either (those bytes are the next row's): zero in registers.
//   The raw bytes wait in registers across the current tile's products: 4 dwords per 16 elements, half of attn.hip's kreg / vreg.
// Commit (registers -> LDS): kv8::dequant8 with the row's scale (v_cvt_scalef32_pk_{bf16,f16}_fp8), into the images attn.hip stages:
//   Ks [64 keys][16 NQ + 8]  row-major, natural column order: a chunk is two 16-byte writes at columns 16 ch and 16 ch + 8.  Columns
//                            r_qk .. 16 nq - 1 are the row's zero padding bytes; the k-steps read nothing beyond 16 nq.
//   Vs [32 NV cols][64 + 8]  transposed: an item's 16 columns are 16 eight-byte packs of its 4 keys at v_quad_pos(mq).  The items of
//                            the chunks pitch_of(r_vo) / 16 .. 2 nv - 1 (r_vo = 77: pitch 80, the third column tile reads to 95) write
//                            zeros every tile, so every row the column tiles read holds dequantised values or zero.
// From there the kernel is attn.hip's, statement for statement (copied, not shared: moving them into attn_tile.hpp would have to
// leave attn.hip's code unchanged, which was not tried): the fragment reads, both v_mfma_f32_32x32x16_{bf16,f16} products, the
// online softmax, the causal / mask handling with the tile summary, the output store.  LDS holds exactly the dequantised values, so
// the result is mdg_attn_fwd's on mdg_kv8_dequant's output.  No permuted contraction order (attn_decode_kv8.hip needs one because its
// K fragments come straight from registers; here they pass through LDS).
#include <math.h>

#include "kv8.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;
constexpr int WAVES = 4;
constexpr int QT = 32;   // queries per wave

// The fields fill_args writes keep attn.hip's names: k / v are the data planes, kts / vts their pitches in bytes; the batch and
// head strides and vec_k / vec_v are not read (a kv head's rows start at (b n_kv + g) cap).
struct Fwd8Args {
  const void* q;
  const void* k;
  const void* v;
  void* out;
  const float *ks, *vs;
  int64_t T, S, ld_out, units, cap;
  int64_t kbs, khs, kts, vbs, vhs, vts;
  int n_heads, n_kv, G, r_qk, r_vo, causal;
  int wg_per_bg;  // workgroups per (batch, kv head)
  int vbytes;     // mdg_kv8_pitch(r_vo): the bytes of a V row that hold elements or their zero padding
  int vec_q, vec_k, vec_v, vec_o;
  float c;  // scale * log2(e)
};

template <int DT, int NQ, int NV, bool MASKED>
__global__ __launch_bounds__(THREADS, (NQ <= 8 && NV <= 4) ? 2 : 1) void attn_fwd_kv8_kernel(Fwd8Args a, MaskArgs mk) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  constexpr int KP = NQ * 16 + 8;  // Ks pitch in elements
  static_assert(32 * NV <= THREADS, "one V item per thread");
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

  const int64_t slot0 = (b * a.n_kv + g) * a.cap;  // the kv head's first row in data (x pitch) and in scale
  const unsigned char* kbase = (const unsigned char*)a.k + slot0 * a.kts;
  const unsigned char* vbase = (const unsigned char*)a.v + slot0 * a.vts;
  const float* ksb = a.ks + slot0;
  const float* vsb = a.vs + slot0;

  // Staging in two halves: fetch (HBM -> registers, raw bytes and row scales) and commit (convert, registers -> LDS).  The next
  // tile's fetch is issued before the products of the current one, in every template.
  constexpr int KIT = NQ / 4;  // K chunks per thread at the template's widest r_qk: 64 NQ / 256
  const int mq = tid & 15;     // the thread's key quad: keys 4 mq .. 4 mq + 3 of the tile
  const int vc0 = (tid >> 4) * 16;  // its V chunk's first column (= byte of the row)
  const bool vitem = vc0 < 32 * nv;  // the chunk lies in a column tile the second product reads
  u32x4 kreg[KIT], vreg[4];
  float ksc[KIT], vsc[4];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int it = 0; it < KIT; it++) {
      const int idx = tid + it * THREADS;
      kreg[it] = (u32x4){0u, 0u, 0u, 0u};
      ksc[it] = 1.f;
      if (idx < KT * nq) {
        const int row = idx / nq, ch = idx - row * nq;
        const int64_t key = t0 + row;
        if (key < a.S) {
          kreg[it] = *(const u32x4*)(kbase + key * a.kts + 16 * ch);
          ksc[it] = ksb[key];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t key = t0 + 4 * mq + i;
      vreg[i] = (u32x4){0u, 0u, 0u, 0u};
      vsc[i] = 1.f;
      if (vitem && vc0 < a.vbytes && key < a.S) {
        vreg[i] = *(const u32x4*)(vbase + key * a.vts + vc0);
        vsc[i] = vsb[key];
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int it = 0; it < KIT; it++) {
      const int idx = tid + it * THREADS;
      if (idx < KT * nq) {
        const int row = idx / nq, ch = idx - row * nq;
        const u32x4 w = kreg[it];
        *(u32x4*)(Ks + row * KP + 16 * ch) = kv8::dequant8<DT>(w.x, w.y, ksc[it]);
        *(u32x4*)(Ks + row * KP + 16 * ch + 8) = kv8::dequant8<DT>(w.z, w.w, ksc[it]);
      }
    }
    // V: the item's 16 transposed 8-byte packs land at the keys' permuted position
    if (vitem) {
      const int pos = v_quad_pos(mq);
#pragma unroll
      for (int h = 0; h < 2; h++) {  // columns vc0 + 8 h .. + 8 of the 4 keys
        u32x4 d[4];
#pragma unroll
        for (int i = 0; i < 4; i++) d[i] = kv8::dequant8<DT>(vreg[i][2 * h], vreg[i][2 * h + 1], vsc[i]);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          u32x2 p;
          p.x = half_of(d[0][j >> 1], j & 1) | (half_of(d[1][j >> 1], j & 1) << 16);
          p.y = half_of(d[2][j >> 1], j & 1) | (half_of(d[3][j >> 1], j & 1) << 16);
          *(u32x2*)(Vs + (vc0 + 8 * h + j) * VP + pos) = p;
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
  if (wg_end > first) fetch(first);
  for (int64_t t0 = first; t0 < wg_end; t0 = MASKED ? tn : t0 + KT) {
    bool none = false, mixed = false;
    if constexpr (MASKED) {  // this tile's state for the wave's unit, taken before next_live moves the words on
      const int x = (int)(t0 / KT) & 63;
      none = !((my_any >> x) & 1);
      mixed = (my_mix >> x) & 1;
    }
    __syncthreads();  // every wave is done with the previous tile
    commit();
    __syncthreads();
    if constexpr (MASKED) {  // the prefetch targets the next LIVE tile
      tn = next_live(t0 / KT + 1) * KT;
      if (tn < wg_end) fetch(tn);
    } else {
      if (t0 + KT < wg_end) fetch(t0 + KT);
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

template <int DT> int launch_fwd8(const Fwd8Args& a, const MaskArgs* mk, dim3 grid, hipStream_t st) {
  return with_template(a.r_qk, a.r_vo, [&](auto nq, auto nv) {
    constexpr int NQ = decltype(nq)::value, NV = decltype(nv)::value;
    const size_t lds = ((size_t)KT * (NQ * 16 + 8) + (size_t)NV * 32 * VP) * 2;
    if (mk) return launch(attn_fwd_kv8_kernel<DT, NQ, NV, true>, grid, THREADS, lds, st, a, *mk);
    return launch(attn_fwd_kv8_kernel<DT, NQ, NV, false>, grid, THREADS, lds, st, a, MaskArgs{});
  });
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_attn_fwd_kv8(const void* q, const void* k_data, const void* k_scale, const void* v_data, const void* v_scale, int dtype,
                                int64_t B, int64_t T, int64_t S, int n_heads, int n_kv, int r_qk, int r_vo, int64_t cap, int64_t k_pitch,
                                int64_t v_pitch, double scale, int causal, void* out, int64_t ld_out, void* stream, const void* mask,
                                int Hm, int64_t mask_batch_stride, int64_t mask_head_stride, int64_t mask_query_stride,
                                const void* summary, int64_t summary_bytes) {
  const char* fn = "mdg_attn_fwd_kv8";
  // what the shared checks read of a call; k and v stand for the data planes, their token strides for the pitches in bytes
  const Call p = {q, k_data, v_data, dtype, B, T, S, n_heads, n_kv, r_qk, r_vo, 0, 0, k_pitch, 0, 0, v_pitch, scale, causal, out, ld_out,
                  stream};
  MDG_CLEAR();
  MDG_TRY(check_widths(fn, p));
  MDG_CHECK_ARG(cap >= 0 && S <= cap, "%s: S=%lld keys exceed cap=%lld", fn, (long long)S, (long long)cap);
  MDG_CHECK_ARG(k_pitch >= kv8::pitch_of(r_qk) && k_pitch % kv8::CHUNK == 0 && v_pitch >= kv8::pitch_of(r_vo) && v_pitch % kv8::CHUNK == 0,
                "%s: pitches (%lld, %lld) must be multiples of 16 and >= mdg_kv8_pitch of r_qk=%d, r_vo=%d", fn, (long long)k_pitch,
                (long long)v_pitch, r_qk, r_vo);
  MDG_TRY(check_layout(fn, p));
  MDG_CHECK_ARG(T == 0 || B <= INT64_MAX / T / n_heads / 256, "%s: B*T overflows", fn);
  MDG_CHECK_ARG(cap == 0 || B <= INT64_MAX / n_kv / cap / (k_pitch > v_pitch ? k_pitch : v_pitch), "%s: B*n_kv*cap*pitch overflows", fn);
  if (B == 0 || T == 0) return MDG_OK;
  MDG_CHECK_ARG(q && out && (S == 0 || (k_data && k_scale && v_data && v_scale)), "%s: null pointer", fn);
  MDG_CHECK_ARG(S == 0 || ((uintptr_t)k_data % 16 == 0 && (uintptr_t)v_data % 16 == 0 && (uintptr_t)k_scale % 4 == 0 &&
                           (uintptr_t)v_scale % 4 == 0),
                "%s: data must be 16-byte and scales 4-byte aligned", fn);
  // the targets every input lies apart from: out, and with a mask the summary (another launch wrote it)
  const size_t es = dtype_size(dtype);
  Span target[2] = {span_of("out", out, 1, 0, 1, 0, B * T, ld_out, (int64_t)n_heads * r_vo, es), Span{"summary", 0, 0}};
  MaskArgs mk{};
  Span ms{"mask", 0, 0};
  if (mask) {  // the mask's own checks come before its span, the summary's before the summary's
    const MaskCall m = {mask, Hm, mask_batch_stride, mask_head_stride, mask_query_stride};
    MDG_TRY(mask_args(fn, p, m, mk, ms));
    const int64_t need = mdg_attn_mask_summary_bytes(B, Hm, T, S);
    MDG_CHECK_ARG(summary != nullptr || need == 0, "%s: null summary", fn);
    MDG_CHECK_ARG(summary_bytes >= need, "%s: summary of %lld bytes is short of mdg_attn_mask_summary_bytes = %lld", fn,
                  (long long)summary_bytes, (long long)need);
    target[1] = Span{"summary", (uintptr_t)summary, (uintptr_t)summary + (uintptr_t)need};
    MDG_TRY(apart(fn, target, 1, target[1]));
    mk.summary = (const unsigned char*)summary;
  }
  const int64_t rows = S == 0 ? 0 : B * n_kv * cap;  // the planes' extents; without keys nothing of them is read
  const Span in[6] = {span_of("q", q, 1, 0, 1, 0, B * n_heads * T, r_qk, r_qk, es),
                      Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                      Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                      Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                      Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)},
                      ms};
  for (int i = 0; i < 6; i++) MDG_TRY(apart(fn, target, 2, in[i]));

  Fwd8Args a;
  fill_args(a, p);
  a.ks = (const float*)k_scale; a.vs = (const float*)v_scale;
  a.cap = cap;
  a.vbytes = (int)kv8::pitch_of(r_vo);
  a.units = ceil_div(T, QT) * a.G;
  const int64_t wg = ceil_div(a.units, WAVES);
  MDG_CHECK_ARG(wg <= 0x7fffffff && B * n_kv <= 0x7fffffff / wg, "%s: B=%lld, T=%lld exceed one launch", fn, (long long)B, (long long)T);
  a.wg_per_bg = (int)wg;
  a.vec_o = (uintptr_t)out % 8 == 0 && ld_out % 4 == 0 && r_vo % 4 == 0;
  const dim3 grid((unsigned)(B * n_kv * wg));
  const MaskArgs* pm = mask ? &mk : nullptr;
  if (dtype == MDG_BF16) MDG_TRY(launch_fwd8<MDG_BF16>(a, pm, grid, (hipStream_t)stream));
  else MDG_TRY(launch_fwd8<MDG_F16>(a, pm, grid, (hipStream_t)stream));
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
