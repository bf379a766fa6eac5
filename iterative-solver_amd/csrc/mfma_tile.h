// Device pieces of the f64 MFMA tile kernels: v_mfma_f64_4x4x4_f64 tiles, lane l = 16k + 4b + i holds
// A_b[i][k] and B_b[k][i], C_b[i][j] sits in lane 16i + 4b + j; group g of a tile's rows (or columns) is its
// vectors 4g .. 4g + 3, lane l feeding vector 4g + (l & 3).  k_mx_inner (kernels_mixed.hip) is built of
// them; k_gemm_inner (kernels_panel.hip) keeps its own text of the same prologue and epilogue, because
// its device assembly is held fixed: a change here goes there too.
#pragma once

#include "ssp_internal.h"

namespace ssp {

// The vector that lane r = l & 3 feeds for group g of `count` vectors v[] with scales s[].  Lanes of absent
// vectors (4g + r >= count, or a null v[4g + r]: a padding slot, never the first of its group) read their
// group's first vector -- the addresses of that group's valid lanes in the same load instruction, so no
// extra traffic -- with scale 1, and feed accumulator rows / columns that the caller never reads.
struct TileLane {
  bool ok;        // this lane's vector exists (remainder loop)
  const void* p;
  double s;
};

__device__ __forceinline__ TileLane tile_lane(const void* const* v, const double* s, int count, int g, int r) {
  TileLane t;
  // All three are read whether or not 4g + r < count (v[] and s[] hold 4 entries for every instantiated
  // group) and chosen afterwards: a load under the test of a loaded pointer would make every group's
  // loads wait for those of the group before it.
  const void* const own = v[4 * g + r];
  const void* const first = v[4 * g < count ? 4 * g : 0];
  const double scale = s[4 * g + r];
  t.ok = 4 * g + r < count && own != nullptr;
  t.p = t.ok ? own : first;
  t.s = t.ok ? scale : 1.0;
  return t;
}

// The tile epilogue: folds the 4 blocks of each accumulator (lane bits 2-3), then the 4 waves through LDS,
// and stores the workgroup's m x k partials (rows and columns past m, k are dropped) at
// partial[blockIdx.x][m][k].  Called once, by every thread of the workgroup.
template <int MG, int NG>
__device__ __forceinline__ void tile_store_partials(const double (&acc)[MG][NG], int m, int k, double* partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double red[kBlock / 64][MG * NG][16];
#pragma unroll
  for (int g = 0; g < MG; ++g)
#pragma unroll
    for (int h = 0; h < NG; ++h) {
      double v = acc[g][h];
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if ((lane & 12) == 0) red[wave][g * NG + h][(lane >> 4) * 4 + (lane & 3)] = v;
    }
  __syncthreads();
  const size_t mk = size_t(m) * k;
  double* out = partial + size_t(blockIdx.x) * mk;
  for (int s = threadIdx.x; s < MG * NG * 16; s += kBlock) {
    const int gh = s >> 4, e = s & 15;
    const int row = 4 * (gh / NG) + (e >> 2), col = 4 * (gh % NG) + (e & 3);
    if (row < m && col < k) {
      double v = red[0][gh][e];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) v += red[w][gh][e];
      out[size_t(row) * k + col] = v;
    }
  }
}

}  // namespace ssp
