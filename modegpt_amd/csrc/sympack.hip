// Packed storage of a finalized (exactly symmetric) fp64 statistic: full [n][ld] <-> row-packed lower triangle, n(n+1)/2 doubles.
//
// Serves load_calibs' `calibs_save_path` / `load_calibs_from` (calibration.py:23-24, declared and never read upstream): a saved
// sigma goes to disk as its lower triangle, half of the 1.64 GB a Llama-3-8B sigma_mlp takes, and comes back as the full matrix
// the compression stages read (compress_mlp.py:13-64, compress_vo.py:43-45).
//
// Launch shape (both): one 256-thread workgroup per 64x64 tile of the LOWER triangle (x batch), a wave per tile row, so every
// global access of a wave is one contiguous run of up to 512 B.  Unpack writes the mirrored tile from a transposed read of the
// tile in LDS (pitch 65 doubles: the column read of a half-wave touches every bank pair once), as cov_finalize_kernel does.
// Both move raw 64-bit patterns (no arithmetic touches a value) and all offsets are 64-bit: a packed matrix passes 4 GiB at
// n = 23 170.
#include "common.hpp"

namespace mdg {

constexpr int PK = 64;   // tile edge

__device__ __forceinline__ int64_t packed_row(int64_t i) { return i * (i + 1) / 2; }

// packed[i(i+1)/2 + j] = full[i][j], j <= i.  Nothing above the diagonal is read.
__global__ __launch_bounds__(256) void sym_pack_lower_kernel(const uint64_t* full, int n, int64_t ld, int64_t bs, int ntri,
                                                             uint64_t* packed) {
  const int b = blockIdx.x / ntri, t = blockIdx.x % ntri;
  int ti, tj;
  tri_decode(t, ti, tj);
  const uint64_t* src = full + (int64_t)b * bs;
  uint64_t* dst = packed + (int64_t)b * packed_row(n);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int gc = tj * PK + tx;
#pragma unroll 4
  for (int r = ty; r < PK; r += 4) {
    const int gr = ti * PK + r;
    if (gr < n && gc <= gr) dst[packed_row(gr) + gc] = src[(int64_t)gr * ld + gc];
  }
}

// full[i][j] = full[j][i] = packed[i(i+1)/2 + j], j <= i.  Columns [n, ld) of a row are not written.
__global__ __launch_bounds__(256) void sym_unpack_lower_kernel(const uint64_t* packed, int n, int64_t ld, int64_t bs, int ntri,
                                                               uint64_t* full) {
  __shared__ uint64_t tl[PK][PK + 1];
  const int b = blockIdx.x / ntri, t = blockIdx.x % ntri;
  int ti, tj;
  tri_decode(t, ti, tj);
  const uint64_t* src = packed + (int64_t)b * packed_row(n);
  uint64_t* dst = full + (int64_t)b * bs;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int gc = tj * PK + tx;
#pragma unroll 4
  for (int r = ty; r < PK; r += 4) {
    const int gr = ti * PK + r;
    uint64_t v = 0;
    if (gr < n && gc <= gr) {
      v = src[packed_row(gr) + gc];
      dst[(int64_t)gr * ld + gc] = v;
    }
    tl[r][tx] = v;
  }
  __syncthreads();
  // the mirror image: row tj*64 + r of the full matrix, columns ti*64 + tx, from the tile's column r
  const int uc = ti * PK + tx;
#pragma unroll 4
  for (int r = ty; r < PK; r += 4) {
    const int ur = tj * PK + r;
    if (ur < n && uc < n && uc > ur) dst[(int64_t)ur * ld + uc] = tl[tx][r];
  }
}

static int sym_args(const char* who, const void* full, const void* packed, int64_t n, int64_t batch, int64_t ld, int64_t bs,
                    int64_t* ntri) {
  MDG_CHECK_ARG(full && packed && n > 0 && n < (1ll << 31) && batch > 0 && ld >= n, "%s: bad arguments", who);
  MDG_CHECK_ARG(batch == 1 || bs >= (n - 1) * ld + n, "%s: batch stride %lld smaller than one matrix", who, (long long)bs);
  const int64_t tiles = ceil_div(n, PK);
  *ntri = tiles * (tiles + 1) / 2;
  MDG_CHECK_ARG(batch * *ntri < (1ll << 31), "%s: grid too large", who);
  return MDG_OK;
}

}  // namespace mdg

using namespace mdg;

extern "C" int mdg_sym_pack_lower(const double* full, int64_t n, int64_t batch, int64_t ld, int64_t batch_stride,
                                  double* packed, void* stream) {
  MDG_CLEAR();
  int64_t ntri;
  MDG_TRY(sym_args("mdg_sym_pack_lower", full, packed, n, batch, ld, batch_stride, &ntri));
  hipLaunchKernelGGL(sym_pack_lower_kernel, dim3((unsigned)(batch * ntri)), dim3(256), 0, (hipStream_t)stream,
                     (const uint64_t*)full, (int)n, ld, batch_stride, (int)ntri, (uint64_t*)packed);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}

extern "C" int mdg_sym_unpack_lower(const double* packed, int64_t n, int64_t batch, double* full, int64_t ld,
                                    int64_t batch_stride, void* stream) {
  MDG_CLEAR();
  int64_t ntri;
  MDG_TRY(sym_args("mdg_sym_unpack_lower", full, packed, n, batch, ld, batch_stride, &ntri));
  hipLaunchKernelGGL(sym_unpack_lower_kernel, dim3((unsigned)(batch * ntri)), dim3(256), 0, (hipStream_t)stream,
                     (const uint64_t*)packed, (int)n, ld, batch_stride, (int)ntri, (uint64_t*)full);
  MDG_LAUNCH_CHECK();
  return MDG_OK;
}
