// row_norms.h -- the norms of the rows of one operand, shared by the distance entry points (distance.hip) and the resident
// reference set (refset.hip): ONE body, so that a set's prepared norms are the bits a call would have computed.
#pragma once
#include "common.h"
#include "space_ops.h"

namespace kpop {

// ---------------------------------------------------------------------------
// norms + pre-normalised rows.  One thread per row walks the dimensions in
// order; 64-row x 32-dim tiles go through LDS so global traffic is coalesced.
// ---------------------------------------------------------------------------
constexpr int kNormRows = 64, kNormDims = 32;

// norms[i] = scale(sum_c m_c g(a_ic)), 0 -> 1 (lib/Matrix.ml:67); when `normalised` is non-null the
// block then re-reads its 64 rows (still in L2) and writes a_ic / n_i (adaptor_a/_b, lib/Matrix.ml:248)
template <int KIND>
__device__ __forceinline__ void row_norms_block(const double *__restrict__ m, uint32_t rows, uint32_t n_dims,
                                                const double *__restrict__ metric, double p,
                                                double *__restrict__ norms, double *__restrict__ normalised, uint32_t block,
                                                double *__restrict__ sumsq = nullptr) {
  // (sumsq: the sum itself, before the scale -- sum_c m_c a_ic^2 for the euclidean and the cosine form: what the matrix-core path wants of a row)
  __shared__ double tile[kNormRows][kNormDims + 1];
  __shared__ double s_metric[kNormDims];
  __shared__ double s_norm[kNormRows];
  const uint32_t row0 = block * kNormRows;
  double acc = 0.0;
  // (the next tile's loads fly while 64 of the block's threads walk this one: a tile at a time left the kernel at 2 TB/s on 1M x 64)
  constexpr int kPer = kNormRows * kNormDims / 256;
  double pre[kPer];
  auto fetch = [&](uint32_t c0) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const uint32_t e = threadIdx.x + 256u * u, i = e / kNormDims, c = e % kNormDims;
      // (addresses clamped into the matrix, what lies outside zeroed when the tile is stored: nothing here looks at a loaded value)
      pre[u] = m[(uint64_t)min(row0 + i, rows - 1u) * n_dims + min(c0 + c, n_dims - 1u)];
    }
  };
  fetch(0);
  for (uint32_t c0 = 0; c0 < n_dims; c0 += kNormDims) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const uint32_t e = threadIdx.x + 256u * u, i = e / kNormDims, c = e % kNormDims;
      tile[i][c] = (row0 + i < rows && c0 + c < n_dims) ? pre[u] : 0.0;
    }
    if (threadIdx.x < kNormDims) s_metric[threadIdx.x] = (c0 + threadIdx.x < n_dims) ? metric[c0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (c0 + kNormDims < n_dims) fetch(c0 + kNormDims);
    if (threadIdx.x < kNormRows) {
      const uint32_t lim = min((uint32_t)kNormDims, n_dims - c0);
      for (uint32_t c = 0; c < lim; ++c) {
        double el = tile[threadIdx.x][c];
        // lib/Space.ml:169-178: acc +. (el *. el *. m_i)  |  acc +. ((|el| ** p) *. m_i)
        acc = __dadd_rn(acc, component<KIND>(el, s_metric[c], p));
      }
    }
  }
  if (threadIdx.x < kNormRows) {
    double nv = scale_distance<KIND>(acc, p);
    nv = (nv == 0.0) ? 1.0 : nv;  // lib/Matrix.ml:67
    s_norm[threadIdx.x] = nv;
    if (row0 + threadIdx.x < rows) {
      norms[row0 + threadIdx.x] = nv;
      if (sumsq) sumsq[row0 + threadIdx.x] = acc;
    }
  }
  if (!normalised) return;
  __syncthreads();
  const uint32_t nrows = min((uint32_t)kNormRows, rows - row0);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (uint32_t i = wv; i < nrows; i += 4) {  // one wave per row: coalesced, no integer division
    const double *src = m + (uint64_t)(row0 + i) * n_dims;
    double *dst = normalised + (uint64_t)(row0 + i) * n_dims;
    const double nv = s_norm[i];
    for (uint32_t c = lane; c < n_dims; c += 64) dst[c] = src[c] / nv;
  }
}

}  // namespace kpop
