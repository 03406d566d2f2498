// The workspace mdg_vo_compress leaves behind (vo.hip): mdg_vo_spectrum and mdg_vo_rank_curve (vo_err.hip) read its spectra from it.
#pragma once
#include "common.hpp"

namespace mdg {

struct VoWs {
  double *T, *G, *evals, *evecs, *P, *Q, *Mh, *tmp, *Y, *evals2, *evecs2;
  int* flag;
  size_t bytes;
};

static inline VoWs vo_layout(void* ws, int64_t d, int n_heads, int n_kv, int hd) {
  VoWs w;
  Carve c(ws);
  const size_t hh = (size_t)hd * hd;
  w.T = c.take<double>((size_t)n_kv * hd * d);
  w.G = c.take<double>(n_kv * hh);
  w.evals = c.take<double>((size_t)n_kv * hd);
  w.evecs = c.take<double>(n_kv * hh);
  w.P = c.take<double>(n_kv * hh);
  w.Q = c.take<double>(n_kv * hh);
  w.Mh = c.take<double>(n_kv * hh);
  w.tmp = c.take<double>(n_kv * hh);
  w.Y = c.take<double>(n_kv * hh);
  w.evals2 = c.take<double>((size_t)n_kv * hd);
  w.evecs2 = c.take<double>(n_kv * hh);
  w.flag = c.take<int>(16);   // (the Jacobi flag: one used, 64 bytes reserved)
  w.bytes = c.off;
  return w;
}

// What mdg_vo_bias lays over T (free once the factors exist): the heads' two vectors [n_kv][hd] and the two row vectors [d]
struct VoBiasWs {
  double *bw, *u, *s_rows, *rho_rows;
  size_t bytes;
};
static inline VoBiasWs vo_bias_layout(double* T, int64_t d, int n_kv, int hd) {
  VoBiasWs w;
  Carve c(T);
  w.bw = c.take<double>((size_t)n_kv * hd);
  w.u = c.take<double>((size_t)n_kv * hd);
  w.s_rows = c.take<double>((size_t)d);
  w.rho_rows = c.take<double>((size_t)d);
  w.bytes = c.off;
  return w;
}

}  // namespace mdg
