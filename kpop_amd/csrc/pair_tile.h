// pair_tile.h -- the f64 pair tile of the vector pipe, once: the loop that every kernel computing the reference chain's distances
// of a tile of pairs is built on (within.hip, clusters.hip, forest.hip, knn.hip, representatives.hip, dbscan.hip;
// distance_rowwise_kernel keeps the form it was written in, see distance.hip).  What the self-joins share around it: self_tile.h.
//
//   A workgroup of 256 threads owns columns i0 .. i1 (rows of the first operand) x rows j0 .. j1 (rows of the second); a thread
//   4 columns x TY rows.  The chain of a pair (lib/Space.ml:192-200 with the adaptors of lib/Matrix.ml:243-250) is ONE thread's,
//   the dimensions ascending: diff = a - b; acc += component<KIND>(diff, m, p).  Every result of these kernels is held, bit for
//   bit, to what kpop_refset_distance_rowwise writes: the order of the operations in pair_accumulate is the contract, and this
//   is the one place where it is written down.
//   The dimensions go through LDS kPairDC at a time, [dimension][row]: a thread's 4 columns are one 32-byte read.  Staging is
//   software-pipelined through registers.  A step of a kernel's loop:
//       __syncthreads();                       the step before has been read
//       stage.store(As, Bs, s_metric, ...);    what was loaded under the step before
//       __syncthreads();
//       stage.load(...);                       the next step's operands -- this tile's next dimensions, or the next tile's
//                                              first -- issued before the arithmetic, landing behind it
//       if (worker) pair_accumulate(...);
//   The tile's choice, the barriers, the LDS arrays and the epilogue are the kernel's; a kernel that computes one tile takes the
//   whole loop as pair_tile_distances.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "space_ops.h"

namespace kpop {

constexpr int kPairDC = 16;  // dimensions a step

// What a thread holds of the next step's operands.  MAXW, MAXTJ: the columns and rows the kernel's LDS arrays have room for;
// thread t stages dimension t % 16 of rows t / 16, t / 16 + 16, ...  (Nothing but the operands lives here: the indices are
// recomputed from threadIdx.x where they are used, which costs no register across the arithmetic.)
template <int MAXW, int MAXTJ>
struct PairStage {
  static constexpr int NA = MAXW * kPairDC / 256, NB = MAXTJ * kPairDC / 256;
  double ra[NA], rb[NB];

  // dimensions c0 .. c0 + 16 of columns i0 .. i1 of a and rows j0 .. j1 of b (i1 - i0 <= MAXW, j1 - j0 <= MAXTJ); zeroes beyond
  // a tile's edge and beyond d_end, the end of the dimensions that the workgroup walks
  __device__ __forceinline__ void load(const double *__restrict__ a, uint32_t i0, uint32_t i1, const double *__restrict__ b, uint32_t j0, uint32_t j1,
                                       uint32_t n_dims, uint32_t c0, uint32_t d_end) {
    const uint32_t sc = threadIdx.x % kPairDC, rbase = threadIdx.x / kPairDC;
    const bool cok = c0 + sc < d_end;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const uint32_t row = rbase + q * 16;
      ra[q] = (cok && i0 + row < i1) ? a[(uint64_t)(i0 + row) * n_dims + c0 + sc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t row = rbase + q * 16;
      rb[q] = (cok && j0 + row < j1) ? b[(uint64_t)(j0 + row) * n_dims + c0 + sc] : 0.0;
    }
  }

  // load, the columns gathered: column i0 + k of the tile is row idx[i0 + k] of a, i0 .. i1 positions in the index list (an index
  // is held below a_rows, the rows of a: a list that was never written cannot lead a load out of a); the rows of b as in load.  The
  // staging, and so store and the arithmetic, are the same
  __device__ __forceinline__ void load_indexed(const double *__restrict__ a, uint32_t a_rows, const uint32_t *__restrict__ idx, uint32_t i0, uint32_t i1,
                                               const double *__restrict__ b, uint32_t j0, uint32_t j1, uint32_t n_dims, uint32_t c0, uint32_t d_end) {
    const uint32_t sc = threadIdx.x % kPairDC, rbase = threadIdx.x / kPairDC;
    const bool cok = c0 + sc < d_end;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const uint32_t row = rbase + q * 16;
      ra[q] = (cok && i0 + row < i1) ? a[(uint64_t)min(idx[i0 + row], a_rows - 1) * n_dims + c0 + sc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t row = rbase + q * 16;
      rb[q] = (cok && j0 + row < j1) ? b[(uint64_t)(j0 + row) * n_dims + c0 + sc] : 0.0;
    }
  }

  // load_indexed, the rows gathered as well: row j0 + k of the tile is row jdx[j0 + k] of b, held below b_rows
  __device__ __forceinline__ void load_indexed_both(const double *__restrict__ a, uint32_t a_rows, const uint32_t *__restrict__ idx, uint32_t i0, uint32_t i1,
                                                    const double *__restrict__ b, uint32_t b_rows, const uint32_t *__restrict__ jdx, uint32_t j0, uint32_t j1,
                                                    uint32_t n_dims, uint32_t c0, uint32_t d_end) {
    const uint32_t sc = threadIdx.x % kPairDC, rbase = threadIdx.x / kPairDC;
    const bool cok = c0 + sc < d_end;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const uint32_t row = rbase + q * 16;
      ra[q] = (cok && i0 + row < i1) ? a[(uint64_t)min(idx[i0 + row], a_rows - 1) * n_dims + c0 + sc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t row = rbase + q * 16;
      rb[q] = (cok && j0 + row < j1) ? b[(uint64_t)min(jdx[j0 + row], b_rows - 1) * n_dims + c0 + sc] : 0.0;
    }
  }

  // registers -> LDS, and the step's 16 metric values
  __device__ __forceinline__ void store(double (*As)[MAXW + 2], double (*Bs)[MAXTJ + 2], double *s_metric, const double *__restrict__ metric, uint32_t c0,
                                        uint32_t d_end) const {
    const uint32_t sc = threadIdx.x % kPairDC, rbase = threadIdx.x / kPairDC;
#pragma unroll
    for (int q = 0; q < NA; ++q) As[sc][rbase + q * 16] = ra[q];
#pragma unroll
    for (int q = 0; q < NB; ++q) Bs[sc][rbase + q * 16] = rb[q];
    if (threadIdx.x < kPairDC) s_metric[threadIdx.x] = (c0 + threadIdx.x < d_end) ? metric[c0 + threadIdx.x] : 0.0;
  }
};

template <int TY>
__device__ __forceinline__ void pair_zero(double (&acc)[TY][4]) {
#pragma unroll
  for (int y = 0; y < TY; ++y)
#pragma unroll
    for (int x = 0; x < 4; ++x) acc[y][x] = 0.0;
}

// `lim` staged dimensions onto the sums of the thread's columns ti .. ti + 4 and rows tj .. tj + TY
template <int KIND, int TY, int LDA, int LDB>
__device__ __forceinline__ void pair_accumulate(double (&acc)[TY][4], double (*As)[LDA], double (*Bs)[LDB], const double *s_metric, uint32_t ti,
                                                uint32_t tj, uint32_t lim, double p) {
  for (uint32_t cc = 0; cc < lim; ++cc) {
    double av[4], bv[TY];
#pragma unroll
    for (int x = 0; x < 4; ++x) av[x] = As[cc][ti + x];
#pragma unroll
    for (int y = 0; y < TY; ++y) bv[y] = Bs[cc][tj + y];
    const double mc = s_metric[cc];
#pragma unroll
    for (int y = 0; y < TY; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        // lib/Space.ml:192-200: diff = a -. b ; acc +. (diff *. diff *. m)
        double diff = __dsub_rn(av[x], bv[y]);
        acc[y][x] = __dadd_rn(acc[y][x], component<KIND>(diff, mc, p));
      }
  }
}

// the kernels that compute ONE tile: the distances of columns i0 .. i1 of a x rows j0 .. j1 of b, the steps above over all the
// dimensions, then the scaling.  worker: the thread holds pairs (a literal `true` where the tile's shape says so costs nothing);
// every thread stages and meets the barriers
template <int KIND, int TY, int MAXW, int MAXTJ>
__device__ __forceinline__ void pair_tile_distances(double (&acc)[TY][4], double (*As)[MAXW + 2], double (*Bs)[MAXTJ + 2], double *s_metric,
                                                    const double *__restrict__ a, uint32_t i0, uint32_t i1, const double *__restrict__ b, uint32_t j0,
                                                    uint32_t j1, uint32_t n_dims, const double *__restrict__ metric, double p, uint32_t ti, uint32_t tj,
                                                    bool worker) {
  pair_zero(acc);
  PairStage<MAXW, MAXTJ> stage;
  stage.load(a, i0, i1, b, j0, j1, n_dims, 0, n_dims);
  for (uint32_t c0 = 0; c0 < n_dims; c0 += kPairDC) {
    __syncthreads();
    stage.store(As, Bs, s_metric, metric, c0, n_dims);
    __syncthreads();
    if (c0 + kPairDC < n_dims) stage.load(a, i0, i1, b, j0, j1, n_dims, c0 + kPairDC, n_dims);
    if (worker) pair_accumulate<KIND>(acc, As, Bs, s_metric, ti, tj, min((uint32_t)kPairDC, n_dims - c0), p);
  }
  if (worker) {
#pragma unroll
    for (int yy = 0; yy < TY; ++yy)
#pragma unroll
      for (int x = 0; x < 4; ++x) acc[yy][x] = scale_distance<KIND>(acc[yy][x], p);
  }
}

}  // namespace kpop
