// The intercept of the mean-aware V/O truncation (mdg_vo_intercept; not upstream: compress_vo.py:112-223 looks at no first moment).
// Softmax rows sum to one, so the mean mu of the post-norm hidden state reaches the attention output as the constant
// sum_h W_o,h (W_v,kv(h) mu + b_v,kv(h)), whatever the attention weights are.  The stored factors v^ / o^ carry
// sum_h o^_h v^_kv(h) mu of it; the difference delta goes into o_proj's bias, for exactly the tensors that are stored:
//   head stage   a_g = W_v,g mu + b_v,g  [hd],  a'_g = v^_g mu  [rank]            n_kv (hd + rank) rows against mu   (one read of W_v, v^)
//   row stage    c_i = sum_h W_o,h[i, :] a_kv(h),  delta_i = c_i - sum_h o^_h[i, :] a'_kv(h),  bias = b_o + delta     (one read of W_o, o^)
//   norms        (sum_i delta_i^2, sum_i c_i^2)                                    one workgroup, a fixed tree
// No atomics; every sum is taken in an order that depends on the shapes and the operands' alignment alone, so the bits repeat
// from run to run.  The rows of both stages and the norms go through row_dots.hpp, shared with mdg_nystrom_intercept and mdg_vo_bias.
#include "common.hpp"
#include "row_dots.hpp"

using namespace mdg;

namespace mdg {

// Head stage.  Workgroups [0, nb_w) own the n_w = n_kv hd rows of W_v (a = W_v mu + b_v), the rest the n_n = n_kv rank rows of v^
// (a' = v^ mu): the choice is uniform over the workgroup.
template <int DTW, int DTN>
__global__ __launch_bounds__(256) void vo_intercept_head_kernel(const void* Wv, int64_t ld_wv, int64_t n_w, int vec_w, const void* Vn,
                                                                int64_t ld_v, int64_t n_n, int vec_n, int64_t d, const double* mu,
                                                                const void* b_v, int b_dtype, int nb_w, double* a, double* a2) {
  __shared__ double sv_[RD_CHUNK];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  double s[RD_RPW];
  if ((int)blockIdx.x < nb_w) {
    const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + (int64_t)w * RD_RPW;
    row_dots<DTW, 1>(Wv, ld_wv, n_w, row0, (int)d, StageGather{mu, d, nullptr}, vec_w, sv_, s);
#pragma unroll
    for (int rr = 0; rr < RD_RPW; rr++) {
      const int64_t row = row0 + rr;
      if (lane == 0 && row < n_w) a[row] = b_v ? s[rr] + load_any(b_v, b_dtype, row) : s[rr];
    }
  } else {
    const int64_t row0 = (int64_t)((int)blockIdx.x - nb_w) * RD_ROWS + (int64_t)w * RD_RPW;
    row_dots<DTN, 1>(Vn, ld_v, n_n, row0, (int)d, StageGather{mu, d, nullptr}, vec_n, sv_, s);
#pragma unroll
    for (int rr = 0; rr < RD_RPW; rr++) {
      const int64_t row = row0 + rr;
      if (lane == 0 && row < n_n) a2[row] = s[rr];
    }
  }
}

// Row stage: RD_ROWS rows of [W_o | o^] per workgroup against a and a', expanded to the query heads' columns in LDS per chunk.
template <int DTW, int DTN>
__global__ __launch_bounds__(256) void vo_intercept_rows_kernel(const void* Wo, int64_t ld_wo, int vec_w, const void* On, int64_t ld_o,
                                                                int vec_n, int64_t d, int n_heads, int group, int hd, int rank,
                                                                const double* a, const double* a2, const void* b_o, int b_dtype,
                                                                void* bias_out, int out_dtype, double* bias_f64, double* delta_rows,
                                                                double* const_rows) {
  __shared__ double sv_[RD_CHUNK];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + (int64_t)w * RD_RPW;
  double c[RD_RPW], c2[RD_RPW];
  row_dots<DTW, 1>(Wo, ld_wo, d, row0, n_heads * hd, StageHeads<1>{{a}, hd, group}, vec_w, sv_, c);
  if (rank > 0) {
    row_dots<DTN, 1>(On, ld_o, d, row0, n_heads * rank, StageHeads<1>{{a2}, rank, group}, vec_n, sv_, c2);
  } else {
#pragma unroll
    for (int rr = 0; rr < RD_RPW; rr++) c2[rr] = 0.;
  }
#pragma unroll
  for (int rr = 0; rr < RD_RPW; rr++) {
    const int64_t row = row0 + rr;
    if (lane == 0 && row < d) {
      const double delta = c[rr] - c2[rr];
      const double bias = b_o ? load_any(b_o, b_dtype, row) + delta : delta;
      delta_rows[row] = delta;
      const_rows[row] = c[rr];
      bias_f64[row] = bias;
      if (bias_out) store_any(bias_out, out_dtype, row, bias);
    }
  }
}

struct VoInterceptWs {
  double *a, *a2;                     // [n_kv][hd] W_v mu + b_v, [n_kv][rank] V^ mu: the heads' halves of the two products
  double *delta_rows, *const_rows;    // [d] each
  size_t bytes;
};
static VoInterceptWs vo_intercept_layout(void* ws, int64_t d, int n_kv, int hd, int rank) {
  Carve c(ws);
  VoInterceptWs w;
  w.a = c.take<double>((size_t)n_kv * (size_t)hd);
  w.a2 = c.take<double>((size_t)n_kv * (size_t)rank);
  w.delta_rows = c.take<double>((size_t)d);
  w.const_rows = c.take<double>((size_t)d);
  w.bytes = c.off;
  return w;
}

struct ViArgs {
  const void *Wv, *Wo, *Vn, *On, *b_v, *b_o;
  int64_t ld_wv, ld_wo, ld_v, ld_o, d;
  int n_heads, n_kv, hd, rank, b_dtype, out_dtype, vec_wv, vec_wo, vec_v, vec_o;
  const double* mu;
  void* bias_out;
  double *bias_f64, *norms;
  VoInterceptWs ws;
};

template <int DTW, int DTN>
static int vo_intercept_launch(const ViArgs& p, hipStream_t st) {
  const int64_t n_w = (int64_t)p.n_kv * p.hd, n_n = (int64_t)p.n_kv * p.rank;
  double *a = p.ws.a, *a2 = p.ws.a2, *delta_rows = p.ws.delta_rows, *const_rows = p.ws.const_rows;
  const int nb_w = (int)ceil_div(n_w, RD_ROWS), nb_n = (int)ceil_div(n_n, RD_ROWS);
  hipLaunchKernelGGL((vo_intercept_head_kernel<DTW, DTN>), dim3((unsigned)(nb_w + nb_n)), dim3(256), 0, st, p.Wv, p.ld_wv, n_w, p.vec_wv,
                     p.Vn, p.ld_v, n_n, p.vec_v, p.d, p.mu, p.b_v, p.b_dtype, nb_w, a, a2);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL((vo_intercept_rows_kernel<DTW, DTN>), dim3((unsigned)ceil_div(p.d, RD_ROWS)), dim3(256), 0, st, p.Wo, p.ld_wo,
                     p.vec_wo, p.On, p.ld_o, p.vec_o, p.d, p.n_heads, p.n_heads / p.n_kv, p.hd, p.rank, a, a2, p.b_o, p.b_dtype,
                     p.bias_out, p.out_dtype, p.bias_f64, delta_rows, const_rows);
  MDG_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_norms_kernel, dim3(1), dim3(256), 0, st, delta_rows, const_rows, p.d, p.norms);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

}  // namespace mdg

extern "C" size_t mdg_vo_intercept_ws_bytes(int64_t d, int n_kv, int hd, int rank) {
  if (d <= 0 || n_kv <= 0 || hd <= 0 || rank < 0 || rank > hd) return 0;
  return mdg::vo_intercept_layout(nullptr, d, n_kv, hd, rank).bytes;
}

extern "C" int mdg_vo_intercept(const void* Wv, int64_t ld_wv, const void* Wo, int64_t ld_wo, int w_dtype, const void* v_new, int64_t ld_v,
                                const void* o_new, int64_t ld_o, int new_dtype, int64_t d, int n_heads, int n_kv, int hd, int rank,
                                const double* mu, const void* b_v, const void* b_o, int b_dtype, void* bias_out, int out_dtype,
                                double* bias_f64, double* norms, void* ws, size_t ws_bytes, void* stream) {
  MDG_CHECK_ARG(Wv && Wo && mu && bias_f64 && norms, "mdg_vo_intercept: null pointer");
  MDG_CHECK_ARG(w_dtype == MDG_BF16 || w_dtype == MDG_F64, "mdg_vo_intercept: W_v / W_o must be bf16 or f64 (got %d)", w_dtype);
  MDG_CHECK_ARG(n_kv > 0 && n_heads > 0 && n_heads % n_kv == 0 && hd >= 2 && hd <= 128 && hd % 2 == 0,
                "mdg_vo_intercept: unsupported head layout (n_heads=%d n_kv=%d hd=%d)", n_heads, n_kv, hd);
  MDG_CHECK_ARG(rank >= 0 && rank <= hd, "mdg_vo_intercept: rank %d outside [0, %d]", rank, hd);
  MDG_CHECK_ARG(rank == 0 || (v_new && o_new), "mdg_vo_intercept: rank %d needs the stored factors (null pointer)", rank);
  MDG_CHECK_ARG(rank == 0 || new_dtype == MDG_BF16 || new_dtype == MDG_F64, "mdg_vo_intercept: the factors must be bf16 or f64 (got %d)",
                new_dtype);
  MDG_CHECK_ARG(((!b_v && !b_o) || known_dtype(b_dtype)) && (!bias_out || known_dtype(out_dtype)),
                "mdg_vo_intercept: unsupported bias dtype");
  MDG_CHECK_ARG(d > 0 && ld_wv >= d && ld_wo >= (int64_t)n_heads * hd && (rank == 0 || (ld_v >= d && ld_o >= (int64_t)n_heads * rank)),
                "mdg_vo_intercept: bad leading dimensions (d=%lld ld_wv=%lld ld_wo=%lld ld_v=%lld ld_o=%lld)", (long long)d,
                (long long)ld_wv, (long long)ld_wo, (long long)ld_v, (long long)ld_o);
  MDG_CHECK_ARG(ws && (uintptr_t)ws % 8 == 0 && ws_bytes >= mdg_vo_intercept_ws_bytes(d, n_kv, hd, rank),
                "mdg_vo_intercept: workspace %zu < required %zu", ws_bytes, mdg_vo_intercept_ws_bytes(d, n_kv, hd, rank));
  MDG_CHECK_ARG(d < (1ll << 31) && (int64_t)n_kv * (2 * hd) < (1ll << 31) && (int64_t)n_heads * hd < (1ll << 31),
                "mdg_vo_intercept: too many rows or columns");      // (row_dots counts columns in 32 bits)
  MDG_CLEAR();
  const auto vec = [](const void* p, int64_t ld, int dt) { return (int)(dt == MDG_BF16 && (uintptr_t)p % 16 == 0 && ld % 8 == 0); };
  const int ndt = rank > 0 ? new_dtype : MDG_BF16;      // (rank 0: the factors are not read)
  ViArgs p;
  p.Wv = Wv; p.Wo = Wo; p.Vn = v_new; p.On = o_new; p.b_v = b_v; p.b_o = b_o;
  p.ld_wv = ld_wv; p.ld_wo = ld_wo; p.ld_v = ld_v; p.ld_o = ld_o; p.d = d;
  p.n_heads = n_heads; p.n_kv = n_kv; p.hd = hd; p.rank = rank; p.b_dtype = b_dtype; p.out_dtype = out_dtype;
  p.vec_wv = vec(Wv, ld_wv, w_dtype); p.vec_wo = vec(Wo, ld_wo, w_dtype);
  p.vec_v = rank > 0 ? vec(v_new, ld_v, ndt) : 0; p.vec_o = rank > 0 ? vec(o_new, ld_o, ndt) : 0;
  p.mu = mu; p.bias_out = bias_out; p.bias_f64 = bias_f64; p.norms = norms; p.ws = vo_intercept_layout(ws, d, n_kv, hd, rank);
  hipStream_t st = (hipStream_t)stream;
  if (w_dtype == MDG_BF16)
    return ndt == MDG_BF16 ? vo_intercept_launch<MDG_BF16, MDG_BF16>(p, st) : vo_intercept_launch<MDG_BF16, MDG_F64>(p, st);
  return ndt == MDG_BF16 ? vo_intercept_launch<MDG_F64, MDG_BF16>(p, st) : vo_intercept_launch<MDG_F64, MDG_F64>(p, st);
}
