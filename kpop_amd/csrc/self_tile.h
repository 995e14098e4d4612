// self_tile.h -- the self-join of a resident set, once: what clusters.hip, dbscan.hip, forest.hip and representatives.hip share around
// the loops of pair_tile.h (one tile's distances: pair_tile_distances there; a strip against many tiles: pair_sweep_tile).  The tile shapes and the folded upper triangle are
// tri_tile.h's (plain integers); here are the triangle's host loop, the compare, the tile's forest in LDS, and the reductions over
// the thread layout.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "pair_tile.h"
#include "space_ops.h"
#include "tri_tile.h"
#include "union_find.h"

namespace kpop {

// the shape's kernel instantiation: f(TY), TY an integral_constant (8 or 4)
template <class F>
static void by_shape_rows(const SelfShape &s, F &&f) {
  if (s.TY == 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 4>{});
}

// the host loop over the triangle's grid of a set of r1 rows whose row tiles from by_first on are wanted: launch(TY, grid, ybase)
// enqueues one grid; grid.y is cut at 65,535 lines
template <class F>
static int self_triangle_launch(const SelfShape &s, uint32_t r1, uint32_t by_first, F &&launch) {
  const TriGrid g = tri_grid(div_up(r1, s.TJ), by_first, s.kf);
  for (uint32_t ybase = 0; ybase < g.lines; ybase += 65535u) {
    const dim3 grid(g.gx, std::min(65535u, g.lines - ybase));
    by_shape_rows(s, [&](auto TY) { launch(TY, grid, ybase); });
    KPOP_LAUNCH_CHECK();
  }
  return 0;
}

// the hits of a thread's pairs, bit yy * 4 + x: inside the tile, i < j only, d <= T (a NaN compares false: it is within nothing);
// known_rows: no pair of two known rows (i < j: the pair is one iff j is known)
template <int TY>
__device__ __forceinline__ uint32_t self_hit_mask(const double (&acc)[TY][4], const TriTile &t, uint32_t ti, uint32_t tj, double T, uint32_t known_rows = 0) {
  uint32_t mask = 0;
#pragma unroll
  for (int yy = 0; yy < TY; ++yy)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const uint32_t i = t.i0 + ti + x, j = t.j0 + tj + yy;
      if (j < t.j1 && i < t.i1 && i < j && j >= known_rows && acc[yy][x] <= T) mask |= 1u << (yy * 4 + x);
    }
  return mask;
}

// the tile's own forest, in LDS (s_par[n] = n over its w + TJ nodes, the columns first, then the rows, set before the loop's barriers):
// thousands of hits inside a dense lineage cost LDS traffic alone, and what leaves the tile is one union per node that is not its
// local root, whatever the number of hits.  Every thread of the workgroup calls
template <int TY>
__device__ __forceinline__ void tile_forest_unite(uint32_t mask, uint32_t *s_par, const TriTile &t, uint32_t w, uint32_t TJ, uint32_t ti, uint32_t tj,
                                                  uint32_t *parent) {
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP, DEV = __HIP_MEMORY_SCOPE_AGENT;
  if (mask) {
#pragma unroll
    for (int yy = 0; yy < TY; ++yy)
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (mask & (1u << (yy * 4 + x))) uf_unite<WG>(s_par, ti + x, w + tj + yy);
  }
  __syncthreads();
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) {
    const uint32_t root = uf_find_readonly<WG>(s_par, n);
    if (root != n) uf_unite<DEV>(parent, n < w ? t.i0 + n : t.j0 + (n - w), root < w ? t.i0 + root : t.j0 + (root - w));
  }
}

// Reductions over the thread layout (thread = rg n_cg + cg, n_cg a power of two that divides 64).  A row's n_cg threads are
// neighbouring lanes of one wavefront, a row group starting at a multiple of n_cg: every one of them gets the row's value.  A column's
// threads are the lanes of a wavefront that share cg, in every wavefront: the lanes below n_cg get their wavefront's value
struct KeyAt {  // a distance's key and where it was found; the least under (key, at)
  uint64_t k;
  uint32_t c;
};
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, uint32_t o) { return (uint32_t)__shfl_xor((int)v, (int)o, 64); }
__device__ __forceinline__ uint64_t lane_xor(uint64_t v, uint32_t o) { return (uint64_t)__shfl_xor((unsigned long long)v, (int)o, 64); }
__device__ __forceinline__ KeyAt lane_xor(KeyAt v, uint32_t o) { return KeyAt{lane_xor(v.k, o), lane_xor(v.c, o)}; }
__device__ __forceinline__ KeyAt key_at_min(KeyAt x, KeyAt y) { return key_less(y.k, y.c, x.k, x.c) ? y : x; }

template <class T, class Op>
__device__ __forceinline__ T reduce_row_lanes(T v, uint32_t n_cg, Op op) {
  for (uint32_t o = n_cg >> 1; o > 0; o >>= 1) v = op(v, lane_xor(v, o));
  return v;
}
template <class T, class Op>
__device__ __forceinline__ T reduce_column_lanes(T v, uint32_t n_cg, Op op) {
  for (uint32_t o = n_cg; o < 64; o <<= 1) v = op(v, lane_xor(v, o));
  return v;
}

// dbscan.hip: the degree pass alone, for density_peaks.hip.  *cnt [r1], inside d_work's dbscan_degree_workspace_bytes: the OTHER rows
// within eps of every row (kpop_dbscan's degree - 1), all zero for eps < 0.  Enqueues only; eps a number, r1 > 0
uint64_t dbscan_degree_workspace_bytes(uint32_t r1);
int dbscan_degree_dev(kpop_refset *rs, double eps, void *d_work, const uint32_t **cnt, hipStream_t st);

}  // namespace kpop
