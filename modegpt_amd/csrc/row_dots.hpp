// Rows of a weight matrix against one or two fp64 vectors, and the two squared norms of the result: the one routine under the bias
// kernels (mdg_nystrom_intercept in colsum.hip, mdg_vo_intercept in vo_mean.hip, mdg_vo_bias in vo.hip).
// A workgroup of 256 threads owns RD_ROWS rows, a wave RD_RPW of them; lanes go along the row (coalesced; 16-byte loads of eight
// 16-bit weights where the operand allows), the vectors are staged per chunk of RD_CHUNK columns in LDS by a stager, which decides
// what column j is multiplied with.  Every product enters its sum through fma (exact product, one rounding per addition); a lane adds
// its columns in ascending order -- elements 2k then 2k + 1 of each 32-bit word on the 16-byte path --, the chunks' partial sums are
// added in chunk order, the wave reduces by xor butterfly last: an order that depends on the shapes and the operand's alignment alone,
// so the bits repeat from run to run.  tests/test_gpu_row_dots_bits.py holds all three callers to recorded bits.
#pragma once
#include "common.hpp"

namespace mdg {

constexpr int RD_CHUNK = 2048, RD_ROWS = 16, RD_RPW = RD_ROWS / 4;      // (d = 4096: 256 workgroups, one per CU)

// Stagers: stage(j, sv) writes what column j meets into sv[v * RD_CHUNK], v < NV.
// v(j) = vec[j], or vec[idx[j]] with idx given; an index outside 0 .. nvecsrc-1 reads nothing and stages a quiet NaN
struct StageGather {
  const double* vec;
  int64_t nvecsrc;
  const int64_t* idx;
  __device__ __forceinline__ void operator()(int j, double* sv) const {
    if (idx) {
      const int64_t id = idx[j];
      sv[0] = (id >= 0 && id < nvecsrc) ? vec[id] : __longlong_as_double(0x7ff8000000000000ll);
    } else {
      sv[0] = vec[j];
    }
  }
};
// The vectors hold `width` entries per kv head; column j belongs to query head j / width, kv head j / (group width):
// v(j) = vec[(j / (group width)) width + j % width], for NV vectors at once (one pass over the matrix for both)
template <int NV>
struct StageHeads {
  const double* vec[NV];
  int width, group;
  __device__ __forceinline__ void operator()(int j, double* sv) const {
    const int src = (j / (group * width)) * width + j % width;
#pragma unroll
    for (int v = 0; v < NV; v++) sv[v * RD_CHUNK] = vec[v][src];
  }
};

// out[v * RD_RPW + rr] = sum_j M[row0 + rr, j] v_v(j), j < ncols.  sv_: NV * RD_CHUNK doubles of LDS.  vec16: M + row * ld is 16-byte
// aligned for every row (only read for 16-bit DT).  A row beyond nrows reads row nrows - 1; the caller drops it.  Columns are counted
// in 32 bits (the entry points refuse a matrix of 2^31 columns or more).  All 256 threads of the workgroup call this together.
template <int DT, int NV, class Stager>
__device__ __forceinline__ void row_dots(const void* M, int64_t ld, int64_t nrows, int64_t row0, int ncols, const Stager& stage,
                                         int vec16, double* sv_, double* out) {
  const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
  for (int i = 0; i < NV * RD_RPW; i++) out[i] = 0.;
  for (int a0 = 0; a0 < ncols; a0 += RD_CHUNK) {
    const int len = ncols - a0 < RD_CHUNK ? ncols - a0 : RD_CHUNK;
    __syncthreads();
    for (int e = tid; e < len; e += 256) stage(a0 + e, sv_ + e);
    __syncthreads();
    // the wave's rows side by side, so that RD_RPW loads per lane are in flight
    int64_t base[RD_RPW];
    double s[NV * RD_RPW];
#pragma unroll
    for (int rr = 0; rr < RD_RPW; rr++) {
      const int64_t row = row0 + rr < nrows ? row0 + rr : nrows - 1;
      base[rr] = row * ld + a0;
    }
#pragma unroll
    for (int i = 0; i < NV * RD_RPW; i++) s[i] = 0.;
    int done = 0;
    if ((DT == MDG_BF16 || DT == MDG_F16) && vec16) {
      for (int q = lane; q < len / 8; q += 64) {
        uint4 q4[RD_RPW];
#pragma unroll
        for (int rr = 0; rr < RD_RPW; rr++) q4[rr] = ((const uint4*)((const unsigned short*)M + base[rr]))[q];
        const double* vp = sv_ + 8 * q;
#pragma unroll
        for (int rr = 0; rr < RD_RPW; rr++) {
          const unsigned w[4] = {q4[rr].x, q4[rr].y, q4[rr].z, q4[rr].w};
#pragma unroll
          for (int k = 0; k < 8; k++) {          // (element 2k in the low half of word k)
            const unsigned short h = (unsigned short)(k & 1 ? w[k / 2] >> 16 : w[k / 2] & 0xffffu);
            const double x = DT == MDG_BF16 ? bf16_to_f64(h) : f16_to_f64(h);
#pragma unroll
            for (int v = 0; v < NV; v++) s[v * RD_RPW + rr] = fma(x, vp[v * RD_CHUNK + k], s[v * RD_RPW + rr]);
          }
        }
      }
      done = len / 8 * 8;
    }
    for (int e = done + lane; e < len; e += 64) {
      double ve[NV];
#pragma unroll
      for (int v = 0; v < NV; v++) ve[v] = sv_[v * RD_CHUNK + e];
#pragma unroll
      for (int rr = 0; rr < RD_RPW; rr++) {
        const double x = load_f64<DT>(M, base[rr] + e);
#pragma unroll
        for (int v = 0; v < NV; v++) s[v * RD_RPW + rr] = fma(x, ve[v], s[v * RD_RPW + rr]);
      }
    }
#pragma unroll
    for (int i = 0; i < NV * RD_RPW; i++) out[i] += s[i];
  }
#pragma unroll
  for (int i = 0; i < NV * RD_RPW; i++) {
    double s = out[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    out[i] = s;
  }
}

// out = (sum_i a_i^2, sum_i b_i^2): one workgroup, thread t sums rows t, t + 256, ... in ascending order through fma, then a fixed tree
static __global__ __launch_bounds__(256) void pair_norms_kernel(const double* a, const double* b, int64_t d, double* out) {
  __shared__ double pa_[256], pb_[256];
  const int tid = threadIdx.x;
  double sa = 0., sb = 0.;
  for (int64_t i = tid; i < d; i += 256) {
    sa = fma(a[i], a[i], sa);
    sb = fma(b[i], b[i], sb);
  }
  pa_[tid] = sa;
  pb_[tid] = sb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      pa_[tid] += pa_[tid + o];
      pb_[tid] += pb_[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = pa_[0];
    out[1] = pb_[0];
  }
}

}  // namespace mdg
