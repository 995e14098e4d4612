// class_tiles.h -- the rows of a labelled resident set grouped by class, once: what silhouette.hip and kmedoids.hip do before their
// passes over the pair tiles.
//
//   silhouette_keys_kernel   a row's sort key (its class; a row left out: n_classes, behind every class) and the class sizes
//   exclusive_scan (scan.h), twice: where a class starts in the grouped order, and its first column tile -- a class's rows are cut
//                             into column tiles of at most w positions, so every column tile holds ONE class; at most r1 / w + n_classes
//   radix_sort_pairs_u64      (radix_sort.h, 16-bit keys) the row indices grouped by class, stable: ascending inside a class
//   silhouette_tiles_kernel   the column tiles: positions, class, whether the class ends there
// A pass then gathers a tile's columns through the grouped order (PairRowsAt of pair_tile.h).  THE SUMS over a class that both passes
// take: position k of the class goes to lane (k % w) / 4, a lane adds its positions ascending, the lanes meet in a fixed tree
// (reduce_row_lanes over LaneSum) at the class's last tile -- an order that depends on r1 (the tile shape) and on the class's members
// in ascending row order alone.
//
// stop: null, or a word of device memory; where it is not zero the kernels of this file return at once and leave what they wrote the
// time before (a caller that enqueues more rounds than it needs: the scans and the sort then run again on unchanged data and write
// what is there already).  (The kernels are templates, as radix_sort.h's are: a header's kernel in two translation units.)
#pragma once
#include <algorithm>

#include "common.h"
#include "radix_sort.h"
#include "refset_call.h"
#include "scan.h"
#include "self_tile.h"

namespace kpop {

constexpr int kSilMaxW = 64, kSilMaxTJ = 256;
constexpr uint32_t kSilNone = 0xFFFFFFFFu;    // KPOP_NO_CLASS
constexpr uint32_t kSilMaxClasses = 65535u;  // (kpop_knn_vote's limit: a class and "left out" are a 16-bit sort key)
constexpr uint32_t kSilLast = 1u << 31;       // SilTile::c: the class ends with this tile

__device__ __forceinline__ double sil_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// a lane's share of a row's sum, for reduce_row_lanes (self_tile.h): x + y is what both partners of an exchange compute
struct LaneSum {
  double v;
};
__device__ __forceinline__ LaneSum lane_xor(LaneSum s, uint32_t o) { return LaneSum{__shfl_xor(s.v, (int)o, 64)}; }

// a column tile: positions i0 .. i1 of the grouped order, all of class c (| kSilLast), which has n rows
struct SilTile {
  uint32_t i0, i1, c, n;
};

// cnt[n_classes + 1]: the rows of a class, [n_classes] the rows left out; start[n_classes + 1]: where a class begins in the grouped
// order; first_tile[n_classes + 1]: its first column tile, [n_classes] the number of tiles; tiles[max_tiles]; keys / vals: the sort's
// two buffers each; perm: the grouped order, set by class_tiles_group (one of the two vals buffers)
struct ClassTiles {
  uint32_t *cnt, *start, *first_tile, *vals_a, *vals_b;
  uint64_t *sums, *keys_a, *keys_b;
  SilTile *tiles;
  void *radix;
  uint32_t max_tiles;
  const uint32_t *perm;
};

static inline ClassTiles class_tiles_carve(Carver &c, uint32_t r1, uint32_t n_classes) {
  const uint64_t n = std::max(r1, 1u), nc = (uint64_t)n_classes + 1;
  const SelfShape s = self_shape(r1);
  ClassTiles f;
  f.max_tiles = (uint32_t)(n / s.w + nc);
  f.cnt = c.take<uint32_t>(nc * 4);
  f.start = c.take<uint32_t>(nc * 4);
  f.first_tile = c.take<uint32_t>(nc * 4);
  f.sums = c.take<uint64_t>((scan_blocks(nc) + 1) * 8);
  f.keys_a = c.take<uint64_t>(n * 8);
  f.keys_b = c.take<uint64_t>(n * 8);
  f.vals_a = c.take<uint32_t>(n * 4);
  f.vals_b = c.take<uint32_t>(n * 4);
  f.radix = c.take<char>(radix_scratch_bytes(n));
  f.tiles = c.take<SilTile>((uint64_t)f.max_tiles * sizeof(SilTile));
  f.perm = f.vals_a;
  return f;
}

template <int kDummy = 0>
__global__ __launch_bounds__(256) void class_tiles_clear_kernel(uint32_t *__restrict__ cnt, uint32_t n, const uint32_t *__restrict__ stop) {
  if (stop && *stop) return;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) cnt[i] = 0;
}

// the table is trusted and guarded: a class beyond n_classes counts as left out
template <int kDummy = 0>
__global__ __launch_bounds__(256) void silhouette_keys_kernel(const uint32_t *__restrict__ class_of, uint32_t r1, uint32_t n_classes, uint64_t *__restrict__ keys,
                                                               uint32_t *__restrict__ vals, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ stop) {
  if (stop && *stop) return;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = min(class_of[i], n_classes);
    keys[i] = c;
    vals[i] = (uint32_t)i;
    atomicAdd(cnt + c, 1u);
  }
}

struct SilRowsIn {
  const uint32_t *cnt;
  __device__ uint32_t operator()(uint64_t i) const { return cnt[i]; }
};
struct SilTilesIn {  // (the rows left out get no tile)
  const uint32_t *cnt;
  uint32_t n_classes, w;
  __device__ uint32_t operator()(uint64_t i) const { return i < n_classes ? (cnt[i] + w - 1) / w : 0u; }
};
struct SilPrefixOut {
  uint32_t *out;
  __device__ void operator()(uint64_t i, uint64_t prefix, uint32_t) const { out[i] = (uint32_t)prefix; }
};

// a block a class at a time, a thread a tile of it
template <int kDummy = 0>
__global__ __launch_bounds__(256) void silhouette_tiles_kernel(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                          const uint32_t *__restrict__ first_tile, uint32_t n_classes, uint32_t w, uint32_t max_tiles,
                                                          SilTile *__restrict__ tiles, const uint32_t *__restrict__ stop) {
  if (stop && *stop) return;
  for (uint32_t c = blockIdx.x; c < n_classes; c += gridDim.x) {
    const uint32_t n = cnt[c], s = start[c], t0 = first_tile[c], nt = (n + w - 1) / w;
    for (uint32_t k = threadIdx.x; k < nt; k += 256) {
      const uint32_t i0 = s + k * w, i1 = min(s + n, i0 + w);
      if (t0 + k < max_tiles) tiles[t0 + k] = SilTile{i0, i1, c | (i1 == s + n ? kSilLast : 0u), n};
    }
  }
}

// tile t as a pass reads it, held to the set: a table that was never written walks nobody out of the grouped order.  Beyond n_tiles
// an empty tile, which ends the pass's walk (pair_sweep_tile in pair_tile.h; the tile after it is tile t + 1)
struct SilStep : SilTile {
  uint32_t t;
};
__device__ __forceinline__ SilStep silhouette_tile(const SilTile *__restrict__ tiles, uint32_t t, uint32_t n_tiles, uint32_t r1, uint32_t w) {
  SilStep x{{0u, 0u, kSilLast, 1u}, t};
  if (t < n_tiles) {
    static_cast<SilTile &>(x) = tiles[t];
    x.i0 = min(x.i0, r1);
    x.i1 = min(min(x.i1, r1), x.i0 + w);
    x.i1 = max(x.i1, x.i0);
  }
  return x;
}

// enqueues the grouping of the set's r1 > 0 rows under d_class_of; afterwards f.perm is the grouped order
static inline int class_tiles_group(ClassTiles &f, const uint32_t *d_class_of, uint32_t r1, uint32_t n_classes, const uint32_t *stop, hipStream_t st) {
  const SelfShape s = self_shape(r1);
  if (stop) {
    class_tiles_clear_kernel<0><<<dim3(std::min(div_up((uint64_t)n_classes + 1, 256), 256u)), dim3(256), 0, st>>>(f.cnt, n_classes + 1, stop);
    KPOP_LAUNCH_CHECK();
  } else {
    KPOP_HIP(hipMemsetAsync(f.cnt, 0, ((uint64_t)n_classes + 1) * 4, st));
  }
  const dim3 rows_grid(std::min(div_up(r1, 256), 4096u));
  silhouette_keys_kernel<0><<<rows_grid, dim3(256), 0, st>>>(d_class_of, r1, n_classes, f.keys_a, f.vals_a, f.cnt, stop);
  KPOP_LAUNCH_CHECK();
  KPOP_TRY(exclusive_scan(SilRowsIn{f.cnt}, SilPrefixOut{f.start}, (uint64_t)n_classes + 1, f.sums, st));
  KPOP_TRY(exclusive_scan(SilTilesIn{f.cnt, n_classes, s.w}, SilPrefixOut{f.first_tile}, (uint64_t)n_classes + 1, f.sums, st));
  uint64_t *keys = nullptr;
  uint32_t *perm = nullptr;
  KPOP_TRY(radix_sort_pairs_u64(f.keys_a, f.keys_b, f.vals_a, f.vals_b, r1, 16, f.radix, st, &keys, &perm));
  f.perm = perm;
  silhouette_tiles_kernel<0><<<dim3(std::min(n_classes, 4096u)), dim3(256), 0, st>>>(f.cnt, f.start, f.first_tile, n_classes, s.w, f.max_tiles, f.tiles, stop);
  KPOP_LAUNCH_CHECK();
  return 0;
}

}  // namespace kpop
