// dbscan.hip -- DBSCAN on a resident set: core rows, border rows and noise, the density-based cut of the graph of clusters.hip.
//
//   The graph: the set's r1 rows, d(j, i) the reference chain's distance (lib/Space.ml:182-205 with the adaptors of
//   lib/Matrix.ml:243-250): the bits kpop_refset_distance_rowwise writes on the vector pipe when the set's own rows are the query -- no
//   kpop_tune setting is read.  Symmetric bit for bit (clusters.hip), so only i < j is examined and i == j never; a NaN is within
//   nothing.  degree[i] = 1 + #{ j != i : d(i, j) <= eps }; row i is a CORE row iff degree[i] >= min_pts; the clusters are the
//   connected components of the graph restricted to the core rows, a core row's label the smallest core row index of its component;
//   a row that is not core and has a core row within eps is a BORDER row: core_of[i] the core row least under (d with -0 taken as +0,
//   index), labels[i] = labels[core_of[i]], and it joins nothing; every other row is NOISE (labels = core_of = KPOP_NOISE).
//   Integer sums, canonical labels, the minimum of a strict total order: a function of the distances alone, the same bits on every run.
//
// Neither the matrix nor a neighbour list is formed, nothing is read back, nothing synchronises.  Three launches walk the folded
// upper triangle (tri_tile.h, both tile shapes) with the tile's distances and the compare of self_tile.h (the loop pair_tile.h's);
// the second and the third compute only the tiles that a bitmap of the launch before names:
//   dbscan_degree_kernel    a hit (i, j) counts for both ends: the counts of a tile's w + TJ nodes are summed in registers, across
//                           lanes with shuffles and across the wavefronts in LDS, and one global atomicAdd a node whose count is not
//                           zero leaves the tile -- a dense lineage costs LDS traffic, not a global atomic a hit.  A tile with a hit
//                           sets its bit in the tile bitmap
//   dbscan_classify_kernel  degree[i] = 1 + counter, parent[i] = i (the forest lives in the labels), counts[1]
//   dbscan_union_kernel     a block whose tile bit is clear returns before it loads anything, and so does one whose nodes hold no
//                           core row.  A hit between two core rows goes into the tile's forest in LDS, then one global union a node
//                           (tile_forest_unite, self_tile.h); a row that is not core is never hooked.  A hit with ONE core end is a border row's: the
//                           least distance key of a node -- registers, shuffles -- goes into best_k[row] by one 64-bit atomicMin a
//                           wavefront and node, and the tile sets its bit in the second bitmap
//   dbscan_border_kernel    the tiles of the second bitmap, the same arithmetic, the same bits: among a border row's hits whose key
//                           IS best_k[row], the least core row index goes into best_c[row] by a 32-bit atomicMin.  (key, then index:
//                           the least under (d, index), with two integer minima and no 96-bit atomic)
//   dbscan_finalize_kernel  a core row: its root (uf_settle, union_find.h) and the count of the roots; any other row:
//                           best_c[row] and that core row's root, or KPOP_NOISE, and the count of the noise
// On a sparse graph the second launch costs its share of tiles with a hit and the third next to nothing: this is the point of the
// bitmaps.  eps < 0: no tile kernel runs (every degree is 1).  No known_rows: a new row can turn old rows that were not core into core
// rows, so no earlier result is a valid start; after kpop_refset_append the call is made again in full.
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr int kDbMaxW = 64, kDbMaxTJ = 256;
constexpr uint64_t kDbNone = ~0ull;         // (no key: distance_key maps only a NaN's bits there, and a NaN is never a key)
constexpr uint32_t kDbNoise = 0xFFFFFFFFu;  // KPOP_NOISE; best_k and best_c start as all ones: one memset

// cnt[r1]: the hits of a row (degree - 1); hit_map, mixed_map: a bit a tile, line by (of n_rt, the set's row tiles) of n_rt kf bits --
// a tile with a hit, a tile with a hit that has one core end; these three are cleared by one memset.  best_k[r1], best_c[r1]: the
// least key of a row's hits with one core end, and the least core row index among the hits of that key; filled with ones by one memset
struct DbWork {
  uint32_t *cnt, *hit_map, *mixed_map, *best_c;
  uint64_t *best_k;
  uint64_t clear_bytes, fill_bytes, bytes;
  uint32_t n_rt;
};

static DbWork dbscan_carve(void *base, uint32_t r1) {
  const uint64_t n = std::max(r1, 1u);
  const SelfShape s = self_shape(r1);
  Carver c(base);
  DbWork f;
  f.n_rt = div_up(n, s.TJ);
  const uint64_t map_bytes = ((uint64_t)f.n_rt * f.n_rt * s.kf + 31) / 32 * 4;
  f.cnt = c.take<uint32_t>(n * 4);
  f.hit_map = c.take<uint32_t>(map_bytes);
  f.mixed_map = c.take<uint32_t>(map_bytes);
  f.clear_bytes = c.off;
  f.best_k = c.take<uint64_t>(n * 8);
  f.best_c = c.take<uint32_t>(n * 4);
  f.fill_bytes = c.off - f.clear_bytes;
  f.bytes = c.off;
  return f;
}

__device__ __forceinline__ bool dbscan_tile_bit(const uint32_t *__restrict__ map, const TriTile &t, uint32_t n_ct) {
  const uint64_t bit = (uint64_t)t.by * n_ct + t.bx;
  return (map[bit >> 5] >> (bit & 31)) & 1u;
}

__device__ __forceinline__ void dbscan_set_tile_bit(uint32_t *__restrict__ map, const TriTile &t, uint32_t n_ct) {
  const uint64_t bit = (uint64_t)t.by * n_ct + t.bx;
  atomicOr(map + (bit >> 5), 1u << (bit & 31));
}

// the tile's core flags, the columns first, then the rows (a node beyond the set is not core) -> does the tile hold a core row
__device__ __forceinline__ bool dbscan_stage_core(uint8_t *s_core, const TriTile &t, uint32_t w, uint32_t TJ, uint32_t r1, const uint32_t *__restrict__ cnt,
                                                  uint32_t need) {
  bool any = false;
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) {
    const uint32_t row = n < w ? t.i0 + n : t.j0 + (n - w);
    const bool core = row < r1 && cnt[row] >= need;
    s_core[n] = core ? 1 : 0;
    any = any || core;
  }
  return __syncthreads_or(any);
}

// the hits of a thread's pairs: bit yy * 4 + x of `both` when both ends are core rows, of `mixed` when one is
struct DbHits {
  uint32_t both, mixed;
};

template <int TY>
__device__ __forceinline__ DbHits dbscan_hits(const double (&acc)[TY][4], const TriTile &t, uint32_t w, uint32_t ti, uint32_t tj, double eps,
                                              const uint8_t *s_core) {
  const uint32_t hits = self_hit_mask<TY>(acc, t, ti, tj, eps);
  uint32_t both = 0, mixed = 0;
#pragma unroll
  for (int yy = 0; yy < TY; ++yy)
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (hits & (1u << (yy * 4 + x))) {
        const bool ci = s_core[ti + x], cj = s_core[w + tj + yy];
        if (ci && cj) both |= 1u << (yy * 4 + x);
        else if (ci != cj) mixed |= 1u << (yy * 4 + x);
      }
  return DbHits{both, mixed};
}

// a: the set's rows as the chain reads them (divided by their norms when the set normalises), both operands.  The grid, the tiles
// and the thread's pairs are tri_tile.h's: every row is new (by_first = 0, all n_rt row tiles), and n_cg n_rg = 256 in both shapes --
// every thread of the workgroup holds pairs.  cnt[i] += the hits of row i in this tile, from either side
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void dbscan_degree_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                               const double *__restrict__ metric, double p, double eps, uint32_t n_cg, uint32_t n_rg,
                                                               uint32_t kf, uint32_t n_rt, uint32_t ybase, uint32_t *__restrict__ cnt,
                                                               uint32_t *__restrict__ hit_map) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kDbMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kDbMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_cnt[kDbMaxW + kDbMaxTJ];  // the tile's counts: the columns first, then the rows
  const uint32_t TJ = TY * n_rg;
  const TriTile t = tri_tile(blockIdx.x, ybase + blockIdx.y, w, TJ, kf, 0, n_rt, r1);
  if (!t.live) return;
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) s_cnt[n] = 0;  // (the loop's barriers come before anybody adds)
  double acc[TY][4];
  const PairRows rows{a, r1};
  pair_tile_distances<KIND, TY, kDbMaxW, kDbMaxTJ>(acc, As, Bs, s_metric, rows, t.i0, t.i1, rows, t.j0, t.j1, n_dims, metric, p, ti, tj, true);
  const uint32_t mask = self_hit_mask<TY>(acc, t, ti, tj, eps);
  if (!__syncthreads_or(mask != 0)) return;  // most tiles of a sparse graph
  const auto sum = [](uint32_t x, uint32_t y) { return x + y; };
  // nobody else holds the row: the sum over its lanes and a plain store
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t c = reduce_row_lanes((uint32_t)__popc((mask >> (4 * yy)) & 0xFu), n_cg, sum);
    if (cg == 0) s_cnt[w + tj + yy] = c;
  }
  // a column's sum over a wavefront's lanes, then one LDS add a wavefront and column
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const uint32_t c = reduce_column_lanes((uint32_t)__popc(mask & (0x11111111u << x)), n_cg, sum);
    if ((threadIdx.x & 63) < n_cg && c) atomicAdd(&s_cnt[ti + x], c);
  }
  __syncthreads();
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) {
    const uint32_t c = s_cnt[n];
    if (c) atomicAdd(cnt + (n < w ? t.i0 + n : t.j0 + (n - w)), c);  // (a node with a count lies inside the set: its pair was in bounds)
  }
  if (threadIdx.x == 0) dbscan_set_tile_bit(hit_map, t, n_rt * kf);
}

// after the degrees: row i is a core row iff 1 + cnt[i] >= min_pts, that is cnt[i] >= need = min_pts - 1.  The degrees, a forest of
// single rows in the labels, and the number of core rows, an integer sum
__global__ __launch_bounds__(256) void dbscan_classify_kernel(const uint32_t *__restrict__ cnt, uint32_t r1, uint32_t need, uint32_t *__restrict__ parent,
                                                              uint32_t *__restrict__ degree, uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_core;
  if (threadIdx.x == 0) s_core = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = cnt[i];
    parent[i] = (uint32_t)i;
    if (degree) degree[i] = c + 1;
    if (c >= need) ++mine;
  }
  if (mine) atomicAdd(&s_core, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_core) atomicAdd(counts + 1, s_core);
}

// the grid, the tiles and the arithmetic of dbscan_degree_kernel, in the tiles where it found a hit.  A hit between two core rows
// goes into the tile's forest (tile_forest_unite); a hit with one core end gives the end that is not core a key
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void dbscan_union_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                              const double *__restrict__ metric, double p, double eps, uint32_t n_cg, uint32_t n_rg,
                                                              uint32_t kf, uint32_t n_rt, uint32_t ybase, const uint32_t *__restrict__ cnt, uint32_t need,
                                                              const uint32_t *__restrict__ hit_map, uint32_t *__restrict__ mixed_map, uint32_t *parent,
                                                              uint64_t *__restrict__ best_k) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kDbMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kDbMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_par[kDbMaxW + kDbMaxTJ];  // the tile's forest: the columns first, then the rows
  __shared__ uint8_t s_core[kDbMaxW + kDbMaxTJ];
  const uint32_t TJ = TY * n_rg;
  const TriTile t = tri_tile(blockIdx.x, ybase + blockIdx.y, w, TJ, kf, 0, n_rt, r1);
  if (!t.live) return;
  if (!dbscan_tile_bit(hit_map, t, n_rt * kf)) return;  // no hit in this tile: most tiles of a sparse graph, and nothing was loaded
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) s_par[n] = n;
  if (!dbscan_stage_core(s_core, t, w, TJ, r1, cnt, need)) return;  // hits, but no core row at either end of any
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  double acc[TY][4];
  const PairRows rows{a, r1};
  pair_tile_distances<KIND, TY, kDbMaxW, kDbMaxTJ>(acc, As, Bs, s_metric, rows, t.i0, t.i1, rows, t.j0, t.j1, n_dims, metric, p, ti, tj, true);
  const DbHits hits = dbscan_hits<TY>(acc, t, w, ti, tj, eps, s_core);
  const uint32_t mask = hits.both, mixed = hits.mixed;
  if (__syncthreads_or(mixed != 0)) {
    // the end of a mixed hit that is not core: the row when the column is core, otherwise the column.  The least key over the
    // node's lanes, one atomicMin a wavefront and node
    const auto least = [](uint64_t x, uint64_t y) { return min(x, y); };
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      uint64_t k = kDbNone;
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if ((mixed & (1u << (yy * 4 + x))) && s_core[ti + x]) k = min(k, distance_key(acc[yy][x]));
      k = reduce_row_lanes(k, n_cg, least);
      if (cg == 0 && k != kDbNone) atomicMin(reinterpret_cast<unsigned long long *>(best_k + t.j0 + tj + yy), (unsigned long long)k);
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      uint64_t k = kDbNone;
#pragma unroll
      for (int yy = 0; yy < TY; ++yy)
        if ((mixed & (1u << (yy * 4 + x))) && !s_core[ti + x]) k = min(k, distance_key(acc[yy][x]));
      k = reduce_column_lanes(k, n_cg, least);
      if ((threadIdx.x & 63) < n_cg && k != kDbNone) atomicMin(reinterpret_cast<unsigned long long *>(best_k + t.i0 + ti + x), (unsigned long long)k);
    }
    if (threadIdx.x == 0) dbscan_set_tile_bit(mixed_map, t, n_rt * kf);
  }
  if (!__syncthreads_or(mask != 0)) return;
  tile_forest_unite<TY>(mask, s_par, t, w, TJ, ti, tj, parent);
}

// the same grid a third time, in the tiles where dbscan_union_kernel found a hit with one core end; the same arithmetic gives the
// same bits, so a hit's key IS best_k of its end that is not core or lies above it.  Among those that are it: the least core row index
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void dbscan_border_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                               const double *__restrict__ metric, double p, double eps, uint32_t n_cg, uint32_t n_rg,
                                                               uint32_t kf, uint32_t n_rt, uint32_t ybase, const uint32_t *__restrict__ cnt, uint32_t need,
                                                               const uint32_t *__restrict__ mixed_map, const uint64_t *__restrict__ best_k,
                                                               uint32_t *__restrict__ best_c) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kDbMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kDbMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint8_t s_core[kDbMaxW + kDbMaxTJ];
  const uint32_t TJ = TY * n_rg;
  const TriTile t = tri_tile(blockIdx.x, ybase + blockIdx.y, w, TJ, kf, 0, n_rt, r1);
  if (!t.live) return;
  if (!dbscan_tile_bit(mixed_map, t, n_rt * kf)) return;  // no border row's hit in this tile: nothing is loaded
  dbscan_stage_core(s_core, t, w, TJ, r1, cnt, need);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  double acc[TY][4];
  const PairRows rows{a, r1};
  pair_tile_distances<KIND, TY, kDbMaxW, kDbMaxTJ>(acc, As, Bs, s_metric, rows, t.i0, t.i1, rows, t.j0, t.j1, n_dims, metric, p, ti, tj, true);
  const uint32_t mixed = dbscan_hits<TY>(acc, t, w, ti, tj, eps, s_core).mixed;
  if (!__syncthreads_or(mixed != 0)) return;
  const auto least = [](uint32_t x, uint32_t y) { return min(x, y); };
  // rows that are not core against core columns: the least column index among the hits of the row's key
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    uint32_t c = kDbNoise;
    const uint32_t m = (mixed >> (4 * yy)) & 0xFu;
    if (m) {
      const uint64_t k = best_k[t.j0 + tj + yy];  // (a mixed hit lies inside the set)
#pragma unroll
      for (int x = 3; x >= 0; --x)
        if ((m & (1u << x)) && s_core[ti + x] && distance_key(acc[yy][x]) == k) c = t.i0 + ti + x;
    }
    c = reduce_row_lanes(c, n_cg, least);
    if (cg == 0 && c != kDbNoise) atomicMin(best_c + t.j0 + tj + yy, c);
  }
  // columns that are not core against core rows
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    uint32_t c = kDbNoise;
    if ((mixed & (0x11111111u << x)) && !s_core[ti + x]) {
      const uint64_t k = best_k[t.i0 + ti + x];
#pragma unroll
      for (int yy = TY - 1; yy >= 0; --yy)
        if ((mixed & (1u << (yy * 4 + x))) && distance_key(acc[yy][x]) == k) c = t.j0 + tj + yy;
    }
    c = reduce_column_lanes(c, n_cg, least);
    if ((threadIdx.x & 63) < n_cg && c != kDbNoise) atomicMin(best_c + t.i0 + ti + x, c);
  }
}

// after everything else.  A core row: its root (uf_settle; only core rows lie on a path).  Any other row: its core row's root, or the
// noise.  counts[0]: the roots; counts[2]: the noise
__global__ __launch_bounds__(256) void dbscan_finalize_kernel(const uint32_t *__restrict__ cnt, uint32_t r1, uint32_t need, const uint32_t *__restrict__ best_c,
                                                              uint32_t *parent, uint32_t *__restrict__ core_of, uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_roots, s_noise;
  if (threadIdx.x == 0) s_roots = s_noise = 0;
  __syncthreads();
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  uint32_t roots = 0, noise = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    if (cnt[i] >= need) {
      if (uf_settle<DEV>(parent, (uint32_t)i) == (uint32_t)i) ++roots;
      if (core_of) core_of[i] = (uint32_t)i;
      continue;
    }
    const uint32_t of = best_c[i];
    uint32_t label = kDbNoise;
    if (of < r1) label = uf_find_readonly<DEV>(parent, of);  // (an index a kernel wrote is a core row of the set; all ones: none)
    else ++noise;
    __hip_atomic_store(parent + i, label, __ATOMIC_RELAXED, DEV);  // (nobody's path holds a row that is not core)
    if (core_of) core_of[i] = of < r1 ? of : kDbNoise;
  }
  if (roots) atomicAdd(&s_roots, roots);
  if (noise) atomicAdd(&s_noise, noise);
  __syncthreads();
  if (threadIdx.x == 0 && s_roots) atomicAdd(counts, s_roots);
  if (threadIdx.x == 0 && s_noise) atomicAdd(counts + 2, s_noise);
}

static int dbscan_check(double eps, uint32_t min_pts, const char *who) {
  if (eps != eps) KPOP_FAIL(KPOP_ERR_INVALID, "%s: eps is not a number", who);
  if (min_pts == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: min_pts is zero (a row counts itself: 1 makes every row a core row)", who);
  return 0;
}

// the body of both entry points: enqueues only
static int dbscan_dev(kpop_refset *rs, double eps, uint32_t min_pts, void *d_work, uint32_t *d_labels, uint32_t *d_core_of, uint32_t *d_degree,
                      uint32_t *d_counts, hipStream_t st, const char *who) {
  KPOP_TRY(dbscan_check(eps, min_pts, who));
  if (!d_counts) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null counts", who);
  KPOP_HIP(hipMemsetAsync(d_counts, 0, 12, st));
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 == 0) return KPOP_OK;
  if (!d_labels) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null labels", who);
  const SelfShape s = self_shape(r1);
  const DbWork f = dbscan_carve(d_work, r1);
  const uint32_t need = min_pts - 1;
  const bool tiles = eps >= 0.0;  // (no distance is negative: below zero every degree is 1)
  const double *a = rs->rows;
  if (tiles) KPOP_TRY(refset_chain_rows(rs, st, &a));
  KPOP_HIP(hipMemsetAsync(f.cnt, 0, f.clear_bytes, st));
  KPOP_HIP(hipMemsetAsync(f.best_k, 0xFF, f.fill_bytes, st));
  // one of the three launches over the triangle's grid: launch(K, TY, grid, ybase), K and TY integral_constants
  const auto pass = [&](auto launch) {
    return by_kind(rs->kind, [&](auto K) { return self_triangle_launch(s, r1, 0, [&](auto TY, dim3 grid, uint32_t ybase) { launch(K, TY, grid, ybase); }); });
  };
  if (tiles)
    KPOP_TRY(pass([&](auto K, auto TY, dim3 grid, uint32_t ybase) {
      dbscan_degree_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, eps, s.n_cg, s.n_rg, s.kf, f.n_rt, ybase,
                                                                                               f.cnt, f.hit_map);
    }));
  const dim3 rows_grid(std::min(div_up(r1, 256), 4096u));
  dbscan_classify_kernel<<<rows_grid, dim3(256), 0, st>>>(f.cnt, r1, need, d_labels, d_degree, d_counts);
  KPOP_LAUNCH_CHECK();
  if (tiles) {
    KPOP_TRY(pass([&](auto K, auto TY, dim3 grid, uint32_t ybase) {
      dbscan_union_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, eps, s.n_cg, s.n_rg, s.kf, f.n_rt, ybase,
                                                                                              f.cnt, need, f.hit_map, f.mixed_map, d_labels, f.best_k);
    }));
    KPOP_TRY(pass([&](auto K, auto TY, dim3 grid, uint32_t ybase) {
      dbscan_border_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, eps, s.n_cg, s.n_rg, s.kf, f.n_rt, ybase,
                                                                                               f.cnt, need, f.mixed_map, f.best_k, f.best_c);
    }));
  }
  dbscan_finalize_kernel<<<rows_grid, dim3(256), 0, st>>>(f.cnt, r1, need, f.best_c, d_labels, d_core_of, d_counts);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

// the degree pass alone (declared in self_tile.h; density_peaks.hip's densities): the counters cleared, then dbscan_degree_kernel over
// the triangle as dbscan_dev launches it.  The workspace is the whole call's, so that one carve describes both
uint64_t dbscan_degree_workspace_bytes(uint32_t r1) { return dbscan_carve(nullptr, r1).bytes; }

int dbscan_degree_dev(kpop_refset *rs, double eps, void *d_work, const uint32_t **cnt, hipStream_t st) {
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  const SelfShape s = self_shape(r1);
  const DbWork f = dbscan_carve(d_work, r1);
  *cnt = f.cnt;
  KPOP_HIP(hipMemsetAsync(f.cnt, 0, f.clear_bytes, st));
  if (!(eps >= 0.0)) return 0;  // (no distance is negative: below zero every degree is 1)
  const double *a;
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  return by_kind(rs->kind, [&](auto K) {
    return self_triangle_launch(s, r1, 0, [&](auto TY, dim3 grid, uint32_t ybase) {
      dbscan_degree_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, eps, s.n_cg, s.n_rg, s.kf, f.n_rt, ybase,
                                                                                               f.cnt, f.hit_map);
    });
  });
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_dbscan_workspace_bytes(const kpop_refset *rs) {
  if (!rs) return 0;
  return dbscan_carve(nullptr, rs->r1).bytes;
}

extern "C" int kpop_dev_dbscan(kpop_refset *rs, double eps, uint32_t min_pts, void *d_work, uint32_t *d_labels, uint32_t *d_core_of, uint32_t *d_degree,
                               uint32_t *d_counts, void *stream) {
  const char *who = "kpop_dev_dbscan";
  KPOP_TRY(refset_check_handle(rs, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return dbscan_dev(rs, eps, min_pts, d_work, d_labels, d_core_of, d_degree, d_counts, as_stream(stream), who);
}

extern "C" int kpop_dbscan(kpop_refset *rs, double eps, uint32_t min_pts, uint32_t *labels, uint32_t *core_of, uint32_t *degree, uint32_t *counts) {
  const char *who = "kpop_dbscan";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(dbscan_check(eps, min_pts, who));
  if (!counts || (rs->r1 && !labels)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  counts[0] = counts[1] = counts[2] = 0;
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  HostCall h;
  void *work = h.work(dbscan_carve(nullptr, r1).bytes);
  uint32_t *dl = h.out(labels, r1), *dc = h.out(core_of, r1), *dd = h.out(degree, r1), *dn = h.scalars(counts, 3);
  KPOP_TRY(h.upload());
  KPOP_TRY(dbscan_dev(rs, eps, min_pts, work, dl, dc, dd, dn, h.st, who));
  return h.finish();
}

extern "C" int kpop_distance_dbscan(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize, double eps,
                                    uint32_t min_pts, uint32_t *labels, uint32_t *core_of, uint32_t *degree, uint32_t *counts) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) { return kpop_dbscan(rs, eps, min_pts, labels, core_of, degree, counts); });
}
