// The tile summary of a bool attention mask, for mdg_attn_fwd_masked (attn.hip): one pass over mask [B, Hm, T, S] (one byte per
// element, non-zero admits; batch / head / query strides in bytes, any of them 0; key stride 1) writes
//   summary [B][Hm][ceil(T / 32)][ceil(S / 64)] bytes:  0 = no element of the 32-query x 64-key tile is admitted, 1 = every
//   element is, 2 = mixed;  positions beyond T or S are ignored.
// The prefill kernel then never stages a key tile that admits nothing for its workgroup, runs the unmasked code on a tile that
// admits everything and reads the mask only for a mixed tile -- without the host ever looking at the mask.
// One wave per tile, four tiles per workgroup.  Rows 4-byte aligned (chosen on the host from base and strides): a lane reads 4
// bytes, 16 lanes a tile row, the wave 4 rows per step; otherwise lane x reads byte x of every row.  Two ballots classify the tile.
// The summary is written in full by this launch and read by the next one on the same stream: no counters, no flags.
#include "attn_tile.hpp"

namespace mdg {
namespace {

using namespace attn;

constexpr int THREADS = 256;
constexpr int WAVES = 4;

struct SummaryArgs {
  const unsigned char* mask;
  unsigned char* summary;
  int64_t T, S, mbs, mhs, mqs, qtiles, ktiles, tiles;
  int Hm, vec;
};

__global__ __launch_bounds__(THREADS) void attn_mask_summary_kernel(SummaryArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (tile >= a.tiles) return;  // wave-uniform
  const int64_t kt = tile % a.ktiles, r1 = tile / a.ktiles;
  const int64_t qt = r1 % a.qtiles, bh = r1 / a.qtiles;
  const int64_t h = bh % a.Hm, b = bh / a.Hm;
  const unsigned char* base = a.mask + b * a.mbs + h * a.mhs;
  const int64_t q0 = qt * MASK_QT, k0 = kt * KT;
  bool any = false, all = true;
  if (a.vec && k0 + KT <= a.S) {
    const int64_t key = k0 + 4 * (lane & 15);
#pragma unroll
    for (int it = 0; it < MASK_QT / 4; it++) {
      const int64_t qi = q0 + 4 * it + (lane >> 4);
      if (qi < a.T) {
        const unsigned w = *(const unsigned*)(base + qi * a.mqs + key);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const bool on = (w & (0xffu << (8 * i))) != 0;
          any |= on;
          all &= on;
        }
      }
    }
  } else {
    const int64_t key = k0 + lane;
    if (key < a.S) {
      for (int it = 0; it < MASK_QT; it++) {
        const int64_t qi = q0 + it;
        if (qi < a.T) {
          const bool on = base[qi * a.mqs + key] != 0;
          any |= on;
          all &= on;
        }
      }
    }
  }
  const bool some = __ballot(any) != 0, hole = __ballot(!all) != 0;
  if (lane == 0) a.summary[tile] = !some ? MASK_NONE : !hole ? MASK_ALL : MASK_MIXED;
}

}  // namespace
}  // namespace mdg

using namespace mdg;

extern "C" int64_t mdg_attn_mask_summary_bytes(int64_t B, int Hm, int64_t T, int64_t S) {
  if (B <= 0 || Hm <= 0 || T <= 0 || S <= 0) return 0;
  return B * Hm * ceil_div(T, MASK_QT) * ceil_div(S, KT);
}

extern "C" int mdg_attn_mask_summary(const void* mask, int64_t B, int Hm, int64_t T, int64_t S, int64_t mask_batch_stride,
                                     int64_t mask_head_stride, int64_t mask_query_stride, void* summary, int64_t summary_bytes,
                                     void* stream) {
  MDG_CLEAR();
  MDG_CHECK_ARG(B >= 0 && T >= 0 && S >= 0, "mdg_attn_mask_summary: negative extent");
  MDG_CHECK_ARG(Hm >= 1, "mdg_attn_mask_summary: mask heads Hm=%d must be positive", Hm);
  MDG_CHECK_ARG(mask_batch_stride >= 0 && mask_head_stride >= 0 && mask_query_stride >= 0,
                "mdg_attn_mask_summary: negative mask stride (%lld, %lld, %lld)", (long long)mask_batch_stride,
                (long long)mask_head_stride, (long long)mask_query_stride);
  MDG_CHECK_ARG(T == 0 || S == 0 || B <= INT64_MAX / Hm / T / S, "mdg_attn_mask_summary: B*Hm*T*S overflows");
  const int64_t need = mdg_attn_mask_summary_bytes(B, Hm, T, S);
  if (need == 0) return MDG_OK;
  MDG_CHECK_ARG(mask != nullptr, "mdg_attn_mask_summary: null mask");
  MDG_CHECK_ARG(summary != nullptr, "mdg_attn_mask_summary: null summary");
  MDG_CHECK_ARG(summary_bytes >= need, "mdg_attn_mask_summary: summary of %lld bytes is short of mdg_attn_mask_summary_bytes = %lld",
                (long long)summary_bytes, (long long)need);
  {
    uintptr_t lo, hi;
    mask_span_of(mask, B, mask_batch_stride, Hm, mask_head_stride, T, mask_query_stride, S, lo, hi);
    const uintptr_t sl = (uintptr_t)summary, sh = sl + (uintptr_t)need;
    MDG_CHECK_ARG(hi <= sl || sh <= lo, "mdg_attn_mask_summary: summary overlaps mask");
  }
  MDG_CHECK_ARG(ceil_div(need, WAVES) <= 0x7fffffff, "mdg_attn_mask_summary: %lld tiles exceed one launch", (long long)need);
  SummaryArgs a;
  a.mask = (const unsigned char*)mask;
  a.summary = (unsigned char*)summary;
  a.T = T; a.S = S;
  a.mbs = mask_batch_stride; a.mhs = mask_head_stride; a.mqs = mask_query_stride;
  a.qtiles = ceil_div(T, MASK_QT); a.ktiles = ceil_div(S, KT); a.tiles = need;
  a.Hm = Hm;
  a.vec = (uintptr_t)mask % 4 == 0 && mask_batch_stride % 4 == 0 && mask_head_stride % 4 == 0 && mask_query_stride % 4 == 0;
  hipLaunchKernelGGL(attn_mask_summary_kernel, dim3((unsigned)ceil_div(need, WAVES)), dim3(THREADS), 0, (hipStream_t)stream, a);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
