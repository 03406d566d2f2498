// mdg_attn_fwd_kv8's product from a PAGED fp8 KV cache (layout: include/modegpt_hip.h; written by kv8_paged.hip): any T, GQA, an optional
// bool mask with attn_mask.hip's tile summary -- attn_fwd_kv8.hip's work split and LDS images behind a front end that finds its rows
// through the block table, with everything about WHERE the keys are decided on the device (as attn_decode_paged8.hip does).
//
// Work split (attn_fwd_kv8.hip's): 256 threads = 4 waves; a wave owns one UNIT = 32 consecutive queries of one query head; a workgroup
// takes 4 consecutive units of one (batch, kv head) in the order (query tile, head of the group); key tiles of 64 staged in LDS are
// shared by the units; the workgroups with the longest key ranges start first.  The grid depends on B, n_kv and T only.
// Per sequence.  A workgroup loads S_b = seq_lens[b] (clamped to 0 .. table_len * page); shift = S_b - T; wave_end and wg_end come from
//     S_b (under a mask from min(S_b, max_S): keys at or beyond it are not admitted).  Causal: query i admits keys j <= i + S_b - T; with
//     S_b < T the first queries admit none and get zeros.  A workgroup whose range is empty enters no barrier and stores zeros.
// Table front end.  A tile's t0 is a multiple of 64 and a page a multiple of 64 rows, so a tile lies in ONE page.  Before the key loop
//     all 256 threads stage a WINDOW of W = 256 consecutive table entries of the sequence (one 4-byte load a thread, clamped to
//     0 .. n_pages - 1, entries at or beyond ceil(wg_end / page) not read) in LDS behind the Ks / Vs images; windows are aligned
//     (window w holds entries [w W, w W + W)).  The fetch of a tile reads its page id from LDS -- one broadcast ds_read, made
//     wave-uniform -- so NO ADDRESS OF A FETCH WAITS ON A TABLE LOAD FROM MEMORY: the id gives one uniform row number (the page's first row of kv head
//     g, minus the page's first key) from which the threads index the four planes by key as attn_fwd_kv8.hip does.  When the next tile to fetch (MASKED: the next LIVE tile, which may lie any number of windows ahead) falls outside the
//     window, the new window is loaded and stored between the two barriers the iteration already has: every read of the old window
//     precedes the first, every read of the new one follows a barrier of its own.  That load is waited for, once per 16384 keys at
//     page 64.  In every other iteration the next tile's entry is read from LDS BEFORE the first barrier (see slot_of below).
// Fetch (HBM -> registers), commit (kv8::dequant8, registers -> LDS): attn_fwd_kv8.hip's chunk and item maps; a key >= S_b is not
//     requested (zero bytes, scale 1).  The raw bytes wait in registers across the current tile's products.
// From there the kernel is attn_fwd_kv8.hip's, statement for statement (copied, not shared, as that file did): fragment reads, both
//     v_mfma_f32_32x32x16 products, the online softmax, the causal / mask handling with the tile summary, the output store.  LDS holds
//     the same images, so for every sequence the result is bit-identical to mdg_attn_fwd_kv8 on that sequence alone (B = 1, S = S_b).
// mask: mdg_attn_fwd_masked's bool mask with last extent max_S and its summary over max_S keys.
#include <math.h>

#include "kv8.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;
constexpr int WAVES = 4;
constexpr int QT = 32;        // queries per wave
constexpr int WINDOW = 256;   // table entries staged in LDS: one per thread

struct FwdPagedArgs {
  const void* q;
  const unsigned char *kd, *vd;  // the pools [n_pages, n_kv, page, pitch]
  const float *ks, *vs;          //           [n_pages, n_kv, page]
  const int* table;              // [B, table_len]
  const int* seq_lens;           // [B]
  void* out;
  int64_t T, max_S, limit, table_len, kp, vp, ld_out, units;  // limit = table_len * page; pitches in bytes
  int page, n_pages;
  int n_heads, n_kv, G, r_qk, r_vo, causal;
  int wg_per_bg;  // workgroups per (batch, kv head)
  int vbytes;     // mdg_kv8_pitch(r_vo): the bytes of a V row that hold elements or their zero padding
  int vec_q, vec_o;
  float c;  // scale * log2(e)
};

template <int DT, int NQ, int NV, bool MASKED>
__global__ __launch_bounds__(THREADS, (NQ <= 8 && NV <= 4) ? 2 : 1) void attn_fwd_paged8_kernel(FwdPagedArgs a, MaskArgs mk) {
  typedef typename Mma<DT>::E E;
  typedef typename Mma<DT>::frag frag;
  constexpr int KP = NQ * 16 + 8;  // Ks pitch in elements
  static_assert(32 * NV <= THREADS, "one V item per thread");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  E* Ks = (E*)smem;                   // [KT][KP]
  E* Vs = Ks + KT * KP;               // [NV * 32][VP]
  int* tbl = (int*)(Vs + NV * 32 * VP);  // [WINDOW] page ids of the table window

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
  const int nq = (a.r_qk + 15) >> 4, nv = (a.r_vo + 31) >> 5;

  // the sequence's own key count; Se: the keys that can be admitted at all
  int64_t S = a.seq_lens[b];
  S = S < 0 ? 0 : S > a.limit ? a.limit : S;
  const int64_t Se = MASKED && a.max_S < S ? a.max_S : S;
  const int64_t shift = S - a.T;

  // key range of this wave and of the workgroup (its last live unit sees the most keys); <= 0 with S_b < T: no key
  int64_t wave_end = 0;
  if (live) {
    const int64_t qlast = q0 + QT - 1 < a.T - 1 ? q0 + QT - 1 : a.T - 1;
    wave_end = a.causal && qlast + shift + 1 < Se ? qlast + shift + 1 : Se;
  }
  int64_t wg_end;
  {
    const int64_t ul = u0 + WAVES - 1 < a.units - 1 ? u0 + WAVES - 1 : a.units - 1;
    const int64_t ql0 = (ul / a.G) * QT;
    const int64_t ql = ql0 + QT - 1 < a.T - 1 ? ql0 + QT - 1 : a.T - 1;
    wg_end = a.causal && ql + shift + 1 < Se ? ql + shift + 1 : Se;
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

  // The table window.  Entries at or beyond the pages the workgroup's range touches are not read; an id is clamped for memory safety.
  const int* trow = a.table + b * a.table_len;
  const int tiles_per_page = a.page / KT;
  const int pages = wg_end > 0 ? (int)((wg_end + a.page - 1) / a.page) : 0;
  auto page_of = [&](int64_t t0) { return (int)(t0 / KT) / tiles_per_page; };  // wave-uniform
  auto window_load = [&](int win) {  // the thread's entry of window `win`
    const int idx = win * WINDOW + tid;
    int pid = idx < pages ? trow[idx] : 0;
    return pid < 0 ? 0 : pid >= a.n_pages ? a.n_pages - 1 : pid;
  };
  int win = 0;  // the window in LDS

  // The tile at t0 (a multiple of KT, < wg_end <= limit) in page index pi of the window: `slot` is row 0 of a contiguous plane that has
  // the tile's rows where the page holds them (the page's first row of kv head g minus the page's first key), so the threads index
  // the four planes by slot + key as attn_fwd_kv8.hip does by slot0 + key; only rows of the tile are ever addressed.  (One uniform
  // row number instead of four uniform bases: the 256 / 256 template has no scalar register to spare.)
  // The row number of the NEXT tile is taken from the window before the iteration's first barrier, while the waves wait for the
  // current tile's bytes anyway: the LDS read, the division in page_of and the multiplications stand off the chain
  // barrier -> addresses -> loads -> commit that bounds a tile's time (only a tile in a new window looks its entry up after the refill).
  int64_t slot = 0;
  auto slot_of = [&](int pi) {
    const int pid = __builtin_amdgcn_readfirstlane(tbl[pi - win * WINDOW]);
    return ((int64_t)pid * a.n_kv + g) * a.page - (int64_t)pi * a.page;
  };

  // Staging in two halves: fetch (HBM -> registers, raw bytes and row scales) and commit (convert, registers -> LDS).  The next
  // tile's fetch is issued before the products of the current one, in every template.
  constexpr int KIT = NQ / 4;  // K chunks per thread at the template's widest r_qk: 64 NQ / 256
  const int mq = tid & 15;     // the thread's key quad: keys 4 mq .. 4 mq + 3 of the tile
  const int vc0 = (tid >> 4) * 16;  // its V chunk's first column (= byte of the row)
  const bool vitem = vc0 < 32 * nv;  // the chunk lies in a column tile the second product reads
  u32x4 kreg[KIT], vreg[4];
  float ksc[KIT], vsc[4];
  auto fetch = [&](int64_t t0) {  // from `slot`
#pragma unroll
    for (int it = 0; it < KIT; it++) {
      const int idx = tid + it * THREADS;
      kreg[it] = (u32x4){0u, 0u, 0u, 0u};
      ksc[it] = 1.f;
      if (idx < KT * nq) {
        const int row = idx / nq, ch = idx - row * nq;
        const int64_t key = t0 + row;
        if (key < S) {
          kreg[it] = *(const u32x4*)(a.kd + (slot + key) * a.kp + 16 * ch);
          ksc[it] = a.ks[slot + key];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t key = t0 + 4 * mq + i;
      vreg[i] = (u32x4){0u, 0u, 0u, 0u};
      vsc[i] = 1.f;
      if (vitem && vc0 < a.vbytes && key < S) {
        vreg[i] = *(const u32x4*)(a.vd + (slot + key) * a.vp + vc0);
        vsc[i] = a.vs[slot + key];
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
  int64_t first = 0, tn = 0;  // the first tile's key (MASKED: the first live one's), the next one's
  if constexpr (MASKED) {
    const int64_t hm = mk.per_head ? head : 0;
    mrow = mk.mask + b * mk.mbs + hm * mk.mhs + (qi < a.T ? qi : a.T - 1) * mk.mqs;
    first = next_live(0) * KT;
  }
  if (wg_end > first) {  // workgroup-uniform: a workgroup without keys enters no barrier
    const int pi = page_of(first);
    win = pi / WINDOW;
    tbl[tid] = window_load(win);
    __syncthreads();
    slot = slot_of(pi);
    fetch(first);
  }
  for (int64_t t0 = first; t0 < wg_end; t0 = tn) {
    bool none = false, mixed = false;
    if constexpr (MASKED) {  // this tile's state for the wave's unit, taken before next_live moves the words on
      const int x = (int)(t0 / KT) & 63;
      none = !((my_any >> x) & 1);
      mixed = (my_mix >> x) & 1;
      tn = next_live(t0 / KT + 1) * KT;  // the prefetch targets the next LIVE tile
    } else {
      tn = t0 + KT;
    }
    // the next tile's page, and its window: one that is not in LDS is loaded and stored between the two barriers
    const bool more = tn < wg_end;
    const int pn = more ? page_of(tn) : 0;
    const int wn = more ? pn / WINDOW : win;
    if (more && wn == win) slot = slot_of(pn);  // (the fetch of t0 was issued an iteration ago: its slot is no longer needed)
    __syncthreads();  // every wave is done with the previous tile, and with the window
    commit();
    if (wn != win) {  // workgroup-uniform, once per WINDOW pages
      win = wn;
      tbl[tid] = window_load(wn);
      __syncthreads();
      slot = slot_of(pn);
    }
    __syncthreads();
    if (more) fetch(tn);
    if (!live || t0 >= wave_end) continue;  // wave-uniform; the barriers above are outside
    unsigned mb[2] = {0u, 0u};
    if constexpr (MASKED) {
      if (none) continue;  // wave-uniform as well
      if (mixed) {         // issued before the first product, used after it
#pragma unroll
        for (int sub = 0; sub < 2; sub++) mb[sub] = mask_bits16(mrow, t0 + 32 * sub + 4 * hh, a.max_S, mk.vec != 0);
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
    const bool need_mask = t0 + KT > Se || (a.causal && t0 + KT - 1 > q0 + shift);
    if (need_mask) {
      int64_t lim = Se - 1;
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

template <int DT> int launch_fwd_paged8(const FwdPagedArgs& a, const MaskArgs* mk, dim3 grid, hipStream_t st) {
  return with_template(a.r_qk, a.r_vo, [&](auto nq, auto nv) {
    constexpr int NQ = decltype(nq)::value, NV = decltype(nv)::value;
    const size_t lds = ((size_t)KT * (NQ * 16 + 8) + (size_t)NV * 32 * VP) * 2 + (size_t)WINDOW * 4;
    if (mk) return launch(attn_fwd_paged8_kernel<DT, NQ, NV, true>, grid, THREADS, lds, st, a, *mk);
    return launch(attn_fwd_paged8_kernel<DT, NQ, NV, false>, grid, THREADS, lds, st, a, MaskArgs{});
  });
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int mdg_attn_fwd_paged8(const void* q, const void* k_data, const void* k_scale, const void* v_data, const void* v_scale,
                                   int dtype, int64_t B, int64_t T, int64_t max_S, int n_heads, int n_kv, int r_qk, int r_vo,
                                   int64_t n_pages, int64_t page, int64_t k_pitch, int64_t v_pitch, const void* block_table,
                                   int64_t table_len, const void* seq_lens, double scale, int causal, void* out, int64_t ld_out,
                                   void* stream, const void* mask, int Hm, int64_t mask_batch_stride, int64_t mask_head_stride,
                                   int64_t mask_query_stride, const void* summary, int64_t summary_bytes) {
  const char* fn = "mdg_attn_fwd_paged8";
  // what the shared checks read of a call; k and v stand for the data pools, their token strides for the pitches in bytes, S for max_S
  const Call p = {q, k_data, v_data, dtype, B, T, max_S, n_heads, n_kv, r_qk, r_vo, 0, 0, k_pitch, 0, 0, v_pitch, scale, causal, out, ld_out,
                  stream};
  MDG_CLEAR();
  MDG_TRY(check_widths(fn, p));
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
  MDG_CHECK_ARG(T == 0 || B <= INT64_MAX / T / n_heads / 256, "%s: B*T overflows", fn);
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
  // the targets every input lies apart from: out, and with a mask the summary (another launch wrote it)
  const size_t es = dtype_size(dtype);
  Span target[2] = {span_of("out", out, 1, 0, 1, 0, B * T, ld_out, (int64_t)n_heads * r_vo, es), Span{"summary", 0, 0}};
  MaskArgs mk{};
  Span ms{"mask", 0, 0};
  if (mask) {  // the mask's own checks come before its span, the summary's before the summary's
    const MaskCall m = {mask, Hm, mask_batch_stride, mask_head_stride, mask_query_stride};
    MDG_TRY(mask_args(fn, p, m, mk, ms));
    const int64_t need = mdg_attn_mask_summary_bytes(B, Hm, T, max_S);
    MDG_CHECK_ARG(summary != nullptr || need == 0, "%s: null summary", fn);
    MDG_CHECK_ARG(summary_bytes >= need, "%s: summary of %lld bytes is short of mdg_attn_mask_summary_bytes = %lld", fn,
                  (long long)summary_bytes, (long long)need);
    target[1] = Span{"summary", (uintptr_t)summary, (uintptr_t)summary + (uintptr_t)need};
    MDG_TRY(apart(fn, target, 1, target[1]));
    mk.summary = (const unsigned char*)summary;
  }
  const int64_t rows = keys ? n_pages * n_kv * page : 0;  // the pools' extents
  const Span in[8] = {span_of("q", q, 1, 0, 1, 0, B * n_heads * T, r_qk, r_qk, es),
                      Span{"k data", (uintptr_t)k_data, (uintptr_t)k_data + (uintptr_t)(rows * k_pitch)},
                      Span{"k scale", (uintptr_t)k_scale, (uintptr_t)k_scale + (uintptr_t)(rows * 4)},
                      Span{"v data", (uintptr_t)v_data, (uintptr_t)v_data + (uintptr_t)(rows * v_pitch)},
                      Span{"v scale", (uintptr_t)v_scale, (uintptr_t)v_scale + (uintptr_t)(rows * 4)},
                      Span{"block_table", (uintptr_t)block_table, (uintptr_t)block_table + (uintptr_t)(keys ? B * table_len * 4 : 0)},
                      Span{"seq_lens", (uintptr_t)seq_lens, (uintptr_t)seq_lens + (uintptr_t)(B * 4)},
                      ms};
  for (int i = 0; i < 8; i++) MDG_TRY(apart(fn, target, 2, in[i]));

  FwdPagedArgs a;
  a.q = q; a.kd = (const unsigned char*)k_data; a.vd = (const unsigned char*)v_data;
  a.ks = (const float*)k_scale; a.vs = (const float*)v_scale; a.out = out;
  a.table = (const int*)block_table; a.seq_lens = (const int*)seq_lens;
  a.T = T; a.max_S = max_S; a.limit = keys ? table_len * page : 0; a.table_len = table_len; a.kp = k_pitch; a.vp = v_pitch;
  a.ld_out = ld_out;
  a.page = (int)page; a.n_pages = (int)n_pages;
  a.n_heads = n_heads; a.n_kv = n_kv; a.G = n_heads / n_kv; a.r_qk = r_qk; a.r_vo = r_vo; a.causal = causal != 0;
  a.vbytes = (int)kv8::pitch_of(r_vo);
  a.units = ceil_div(T, QT) * a.G;
  const int64_t wg = ceil_div(a.units, WAVES);
  MDG_CHECK_ARG(wg <= 0x7fffffff && B * n_kv <= 0x7fffffff / wg, "%s: B=%lld, T=%lld exceed one launch", fn, (long long)B, (long long)T);
  a.wg_per_bg = (int)wg;
  a.vec_q = (uintptr_t)q % 16 == 0 && r_qk % 8 == 0;
  a.vec_o = (uintptr_t)out % 8 == 0 && ld_out % 4 == 0 && r_vo % 4 == 0;
  a.c = (float)(scale * 1.4426950408889634);
  const dim3 grid((unsigned)(B * n_kv * wg));
  const MaskArgs* pm = mask ? &mk : nullptr;
  if (dtype == MDG_BF16) MDG_TRY(launch_fwd_paged8<MDG_BF16>(a, pm, grid, (hipStream_t)stream));
  else MDG_TRY(launch_fwd_paged8<MDG_F16>(a, pm, grid, (hipStream_t)stream));
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
