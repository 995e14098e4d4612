// pair_tile.h -- the f64 pair tile of the vector pipe, once: the loop that every kernel computing the reference chain's distances
// of a tile of pairs is built on (distance_rowwise_kernel keeps the form it was written in, see distance.hip).  What the
// self-joins share around it: self_tile.h.
//
//   A workgroup of 256 threads owns columns i0 .. i1 (rows of the first operand) x rows j0 .. j1 (rows of the second); a thread
//   4 columns x TY rows.  The chain of a pair (lib/Space.ml:192-200 with the adaptors of lib/Matrix.ml:243-250) is ONE thread's,
//   the dimensions ascending: diff = a - b; acc += component<KIND>(diff, m, p).  Every result of these kernels is held, bit for
//   bit, to what kpop_refset_distance_rowwise writes: the order of the operations in pair_accumulate is the contract, and this
//   is the one place where it is written down.
//   The dimensions go through LDS kPairDC at a time, [dimension][row]: a thread's 4 columns are one 32-byte read.  Staging is
//   software-pipelined through registers.  A step:
//       __syncthreads();                       the step before has been read
//       stage.store(As, Bs, s_metric, ...);    what was loaded under the step before
//       __syncthreads();
//       stage.load(...);                       the next step's operands, issued before the arithmetic, landing behind it
//       if (worker) pair_accumulate(...);
//   An operand is a ROW VIEW: PairRows, position pos of a tile is row pos of the matrix, or PairRowsAt, it is row idx[pos] --
//   gathered rows, of which no compacted copy is kept.  PairStage::load takes one view an operand; the staging, and so store and
//   the arithmetic, do not know which.
//   The steps are written out twice:
//     pair_tile_distances  ONE tile, scaled: clusters.hip, dbscan.hip, representatives_hits_kernel; farthest_first_pass_kernel
//                          (its columns the picks of a group, gathered)
//     pair_sweep_tile      a strip of rows j0 .. j1 against a SEQUENCE of column tiles, the first 16 dimensions of the next tile
//                          loaded under the last step of the current one: knn.hip (knn_nearest_kernel, knn_ties_kernel, and
//                          knn_validate.hip through them), forest_nearest_kernel (reachability.hip through it),
//                          silhouette_pass_kernel, kmedoids_assign_kernel, kmedoids_own_kernel.
//                          The LDS arrays, the sequence, what is read at a tile's start and the epilogue are the kernel's
//   within_tile_kernel writes the one-tile steps out itself and representatives_cover_kernel the sweep's (each says why).
//   ONE CALL OF load A STEP.  In the sweep the next step's operands are this tile's next dimensions or the next tile's first:
//   the tile and the dimension are chosen first, then load is called once.  Written as two calls -- if (more dimensions)
//   load(this tile) else if (more tiles) load(next tile) -- the compiler keeps two copies of the loads, which cost
//   forest_nearest_kernel 28 to 30 VGPRs and a wave a SIMD (profiles/pair_tile_refactor.md, section 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "space_ops.h"

namespace kpop {

constexpr int kPairDC = 16;  // dimensions a step

// The rows of an operand, by position.  m: the matrix as the chain reads it; rows: its rows.  The plain view reads neither rows
// nor an index: it costs what a pointer costs
struct PairRows {
  const double *__restrict__ m;
  uint32_t rows;
  __device__ __forceinline__ uint32_t row(uint32_t pos) const { return pos; }
};
// position pos is row idx[pos].  An index is held below rows: a list that was never written cannot lead a load out of m
struct PairRowsAt {
  const double *__restrict__ m;
  uint32_t rows;
  const uint32_t *__restrict__ idx;
  __device__ __forceinline__ uint32_t row(uint32_t pos) const { return min(idx[pos], rows - 1); }
};

// What a thread holds of the next step's operands.  MAXW, MAXTJ: the columns and rows the kernel's LDS arrays have room for;
// thread t stages dimension t % 16 of rows t / 16, t / 16 + 16, ...  (Nothing but the operands lives here: the indices are
// recomputed from threadIdx.x where they are used, which costs no register across the arithmetic.)
template <int MAXW, int MAXTJ>
struct PairStage {
  static constexpr int NA = MAXW * kPairDC / 256, NB = MAXTJ * kPairDC / 256;
  double ra[NA], rb[NB];

  // dimensions c0 .. c0 + 16 of positions i0 .. i1 of a and j0 .. j1 of b (i1 - i0 <= MAXW, j1 - j0 <= MAXTJ); zeroes beyond
  // a tile's edge and beyond d_end, the end of the dimensions that the workgroup walks
  template <class A, class B>
  __device__ __forceinline__ void load(const A &a, uint32_t i0, uint32_t i1, const B &b, uint32_t j0, uint32_t j1, uint32_t n_dims, uint32_t c0,
                                       uint32_t d_end) {
    const uint32_t sc = threadIdx.x % kPairDC, rbase = threadIdx.x / kPairDC;
    const bool cok = c0 + sc < d_end;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const uint32_t row = rbase + q * 16;
      ra[q] = (cok && i0 + row < i1) ? a.m[(uint64_t)a.row(i0 + row) * n_dims + c0 + sc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t row = rbase + q * 16;
      rb[q] = (cok && j0 + row < j1) ? b.m[(uint64_t)b.row(j0 + row) * n_dims + c0 + sc] : 0.0;
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

// the kernels that compute ONE tile: the distances of positions i0 .. i1 of a x j0 .. j1 of b, the steps above over all the
// dimensions, then the scaling.  worker: the thread holds pairs (a literal `true` where the tile's shape says so costs nothing);
// every thread stages and meets the barriers
template <int KIND, int TY, int MAXW, int MAXTJ, class A, class B>
__device__ __forceinline__ void pair_tile_distances(double (&acc)[TY][4], double (*As)[MAXW + 2], double (*Bs)[MAXTJ + 2], double *s_metric, const A &a,
                                                    uint32_t i0, uint32_t i1, const B &b, uint32_t j0, uint32_t j1, uint32_t n_dims,
                                                    const double *__restrict__ metric, double p, uint32_t ti, uint32_t tj, bool worker) {
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

// A column tile of a sweep: positions i0 .. i1 of the first operand.  A kernel's own tile type may carry more (its number, its
// class); an EMPTY range, i0 >= i1, is the end of the sequence
struct PairTile {
  uint32_t i0, i1;
};
// the plainest sequence: tiles of w positions up to `end`, the last one ragged.  (after: the start is i0 + w and not i1, so that
// what the compiler knows of the first start's low bits holds for every start; behind the tile that reaches `end` comes an
// empty one whatever the sums do at 2^32)
struct PairTilesOf {
  uint32_t w, end;
  __device__ __forceinline__ PairTile at(uint32_t i0) const { return PairTile{i0, min(end, i0 + w)}; }
  __device__ __forceinline__ PairTile after(const PairTile &t) const { return PairTile{t.i0 + w, t.i1 < end ? min(end, t.i0 + w + w) : 0u}; }
};

// the kernels that walk MANY tiles against one strip of rows j0 .. j1 of b.  The kernel keeps the loop over its tiles, what it
// reads of a tile's columns and its epilogue; the pipelined steps of a tile are here:
//     PairStage<MAXW, MAXTJ> stage;
//     Tile cur = the first tile, nxt;
//     for (pair_sweep_open(stage, a, cur, b, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
//       nxt = the tile after cur             (FIRST: it is needed under this tile's last step, and a `continue` below goes to it)
//       ...                                  the tile's column data, read in front of the arithmetic
//       double acc[TY][4];
//       pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, a, cur, nxt, b, j0, j1, n_dims, metric, p, ti, tj, worker);
//       ...                                  the epilogue, over the UNSCALED sums of the tile
//     }
// "No more tiles" -- an empty nxt -- must be the same for every thread of the workgroup, which meets the barriers together.
// worker as above.  (The tile loop and the epilogue are the kernel's text, not callables of a shared function, and the sweep's
// state is the kernel's variables, not a struct's members, on evidence: profiles/pair_sweep_refactor.md, section 1.)

// in front of the loop: the first tile's first dimensions
template <int MAXW, int MAXTJ, class A, class B, class Tile>
__device__ __forceinline__ void pair_sweep_open(PairStage<MAXW, MAXTJ> &stage, const A &a, const Tile &first, const B &b, uint32_t j0, uint32_t j1,
                                                uint32_t n_dims) {
  if (first.i0 < first.i1) stage.load(a, first.i0, first.i1, b, j0, j1, n_dims, 0, n_dims);
}
// the steps of tile cur over all the dimensions; under the last of them the first dimensions of nxt.  One call of load a step,
// its tile and dimension chosen first (the header says why)
template <int KIND, int TY, int MAXW, int MAXTJ, class A, class B, class Tile>
__device__ __forceinline__ void pair_sweep_tile(PairStage<MAXW, MAXTJ> &stage, double (&acc)[TY][4], double (*As)[MAXW + 2], double (*Bs)[MAXTJ + 2],
                                                double *s_metric, const A &a, const Tile &cur, const Tile &nxt, const B &b, uint32_t j0, uint32_t j1,
                                                uint32_t n_dims, const double *__restrict__ metric, double p, uint32_t ti, uint32_t tj, bool worker) {
  pair_zero(acc);
  for (uint32_t c0 = 0; c0 < n_dims; c0 += kPairDC) {
    __syncthreads();
    stage.store(As, Bs, s_metric, metric, c0, n_dims);
    __syncthreads();
    const bool more = c0 + kPairDC < n_dims;  // this tile's next dimensions, or the next tile's first
    const uint32_t ni0 = more ? cur.i0 : nxt.i0, ni1 = more ? cur.i1 : nxt.i1;
    if (more || nxt.i0 < nxt.i1) stage.load(a, ni0, ni1, b, j0, j1, n_dims, more ? c0 + kPairDC : 0u, n_dims);
    if (worker) pair_accumulate<KIND>(acc, As, Bs, s_metric, ti, tj, min((uint32_t)kPairDC, n_dims - c0), p);
  }
}

}  // namespace kpop
