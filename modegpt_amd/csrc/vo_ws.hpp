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
  double* p = (double*)ws;
  const size_t hh = (size_t)hd * hd;
  w.T = p;      p += (size_t)n_kv * hd * d;
  w.G = p;      p += n_kv * hh;
  w.evals = p;  p += (size_t)n_kv * hd;
  w.evecs = p;  p += n_kv * hh;
  w.P = p;      p += n_kv * hh;
  w.Q = p;      p += n_kv * hh;
  w.Mh = p;     p += n_kv * hh;
  w.tmp = p;    p += n_kv * hh;
  w.Y = p;      p += n_kv * hh;
  w.evals2 = p; p += (size_t)n_kv * hd;
  w.evecs2 = p; p += n_kv * hh;
  w.flag = (int*)p; p += 8;
  w.bytes = (size_t)((char*)p - (char*)ws);
  return w;
}

}  // namespace mdg
