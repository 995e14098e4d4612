// kmedoids.hip -- alternating k-medoids (Voronoi iteration; Park & Jun 2009) on a resident set: k groups around k real rows when a
// count is known and no radius is.  The count-based partner of the clustering calls, as farthest_first.hip is of the thinning calls.
//
//   The distances of clusters.hip: the set's r1 rows, d(j, i) the reference chain's distance (lib/Space.ml:182-205 with the adaptors of
//   lib/Matrix.ml:243-250), symmetric bit for bit, the pair i == j never examined; no kpop_tune setting is read.
//   ASSIGNMENT to a medoid list M[0 .. k): row M[c] has class c and dist +0; every other row j the class least under (d(j, M[c]) with -0
//   as +0, c ascending) over the c whose distance is a number, dist that distance; a row without such a c is LEFT OUT (KPOP_NO_CLASS,
//   +inf, own_mean NaN, in no sum).  own_mean: kpop_silhouette's for that labelling, bit for bit.  UPDATE: M'[c] the member of class c
//   least under (own_mean with -0 as +0, row index) among those whose own_mean is a number; a class without one keeps M[c].
//   L = assign(init); for t = 0, 1, ...: own_mean, M' of L; M' == M: converged, stop; t == max_iter: stop; M = M', L = assign(M).
//
// Neither the r1 x r1 matrix nor an r1 x k table is formed.  A round is a chain of launches, the launch boundary the one synchronisation:
//   kmedoids_pos_*_kernel     pos_of[r1]: a medoid's own position, KPOP_NO_CLASS for every other row
//   kmedoids_assign_kernel    the rows of the set against ALL k medoids in one read of the set.  farthest_first_pass_kernel's tile: a
//                             workgroup takes strips of 256 rows, the medoids gathered as the tile's columns (PairRowsAt of pair_tile.h) in
//                             groups of 32, a thread 4 medoids x 8 rows, the chain of a pair in one thread, the dimensions ascending.  New:
//                             the loop over the groups inside a strip -- a row's least (key, position) is carried across the groups and
//                             written once.  Where the strips are so few that whole segments fit beside each other under two workgroups
//                             a CU (256 strips and fewer) the medoid list is cut into up to 16 segments of whole groups (blockIdx.y);
//                             a row's least a segment, merged in segment order: exact
//   kmedoids_merge_kernel     class_of and dist of a row out of pos_of and the segments' leasts, and the sum of dist over each 256 rows
//                             in a fixed tree
//   kmedoids_cost_kernel      one workgroup: cost[n_iter] from those partial sums, a thread its partials ascending, then a fixed tree --
//                             an order that is a function of r1 alone; no floating-point atomic
//   class_tiles_group         (class_tiles.h, the silhouette's) the rows grouped by class, column tiles of one class each
//   kmedoids_own_kernel       the within-class sums.  A workgroup owns TJ consecutive positions of the GROUPED order and walks the column
//                             tiles of the classes those positions belong to, and no others: the sum of n_c^2 pairs and not r1^2 (a row
//                             tile that spans several small classes computes their cross pairs and drops them: bounded by the tile).
//                             Both operands gathered (a PairRowsAt each).  The sum order is silhouette_pass_kernel's, position
//                             for position, so own_mean has kpop_silhouette's bits; a class's column walk is never cut
//   kmedoids_rows_kernel, kmedoids_medoid_kernel   the two integer minima of silhouette.hip: the key of own_mean, then the row index
//   kmedoids_update_kernel    one workgroup: M' against M; sets the done word and converged, or takes M' and counts the round
//   kmedoids_finish_kernel    the outputs out of the workspace
// Every kernel of this file returns at once behind the done word, so the rounds a caller enqueues beyond the stop alter nothing: the
// device form enqueues the worst case, max_iter + 1 rounds (the scans and the sort of a round behind the stop run on unchanged data
// and write what is there: O(r1) a round), the host form reads the done word back after every round and stops.
#include <algorithm>
#include <vector>

#include "class_tiles.h"
#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr uint32_t kKmGroup = 32;     // medoids a group: the columns of the assignment's tile
constexpr uint32_t kKmStrip = 256;    // rows a strip
constexpr uint32_t kKmMaxGrid = 512;  // workgroups of the assignment the strips are spread over: two a CU
constexpr uint32_t kKmMaxSeg = 16;
constexpr uint64_t kKmNone = ~0ull;   // (no key: a NaN is never a key)
constexpr int kKmTY = 8, kKmCG = 8;   // a thread 4 columns x 8 rows; 8 lanes a row
static_assert(kKmGroup == 4 * kKmCG && kKmStrip == kKmTY * (256 / kKmCG), "the tile is a group x a strip");

enum { kKmIter = 0, kKmDone = 1, kKmConverged = 2 };  // the control words

struct KmWork {
  uint32_t *words, *med, *pos_of, *lab, *seg_pos, *med_i;
  uint64_t *seg_key, *med_k;
  double *dist, *own, *partial, *cost;
  ClassTiles g;
  uint32_t n_seg, gps;  // segments of the medoid list, groups a segment
  uint64_t bytes;
};

// the segments of the medoid list: a function of r1 and k
static void kmedoids_segments(uint32_t r1, uint32_t k, uint32_t *n_seg, uint32_t *gps) {
  const uint32_t strips = div_up(std::max(r1, 1u), kKmStrip), groups = div_up(std::max(k, 1u), kKmGroup);
  const uint32_t want = std::min(std::min(groups, kKmMaxSeg), std::max(1u, kKmMaxGrid / strips));
  *gps = div_up(groups, want);
  *n_seg = div_up(groups, *gps);
}

static KmWork kmedoids_carve(void *base, uint32_t r1, uint32_t k, uint32_t max_iter) {
  const uint64_t n = std::max(r1, 1u), nk = std::max(k, 1u);
  Carver c(base);
  KmWork f;
  kmedoids_segments(r1, k, &f.n_seg, &f.gps);
  f.words = c.take<uint32_t>(256);
  f.med = c.take<uint32_t>(nk * 4);
  f.med_i = c.take<uint32_t>(nk * 4);
  f.med_k = c.take<uint64_t>(nk * 8);
  f.pos_of = c.take<uint32_t>(n * 4);
  f.lab = c.take<uint32_t>(n * 4);
  f.dist = c.take<double>(n * 8);
  f.own = c.take<double>(n * 8);
  f.seg_key = c.take<uint64_t>(n * f.n_seg * 8);
  f.seg_pos = c.take<uint32_t>(n * f.n_seg * 4);
  f.partial = c.take<double>((uint64_t)div_up(n, kKmStrip) * 8);
  f.cost = c.take<double>(((uint64_t)max_iter + 1) * 8);
  f.g = class_tiles_carve(c, r1, k);
  f.bytes = c.off;
  return f;
}

// init[] is trusted to hold distinct rows; an index is held inside the set
__global__ __launch_bounds__(256) void kmedoids_init_kernel(const uint32_t *__restrict__ init, uint32_t k, uint32_t r1, uint64_t n_cost, uint32_t *__restrict__ med,
                                                            double *__restrict__ cost) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < max((uint64_t)k, n_cost); i += (uint64_t)gridDim.x * 256) {
    if (i < k) med[i] = min(init[i], r1 - 1);
    if (i < n_cost) cost[i] = sil_nan();
  }
}

__global__ __launch_bounds__(256) void kmedoids_pos_clear_kernel(uint32_t *__restrict__ pos_of, uint32_t r1, uint32_t *__restrict__ med_i, uint64_t *__restrict__ med_k,
                                                                 uint32_t k, const uint32_t *__restrict__ words) {
  if (words[kKmDone]) return;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < max(r1, k); i += (uint64_t)gridDim.x * 256) {
    if (i < r1) pos_of[i] = kSilNone;
    if (i < k) {
      med_i[i] = kSilNone;
      med_k[i] = kKmNone;
    }
  }
}

// (a row that stands twice in the list, which the host form refuses, keeps its first position)
__global__ __launch_bounds__(256) void kmedoids_pos_set_kernel(const uint32_t *__restrict__ med, uint32_t k, uint32_t r1, uint32_t *__restrict__ pos_of,
                                                               const uint32_t *__restrict__ words) {
  if (words[kKmDone]) return;
  for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < k; c += gridDim.x * 256) atomicMin(pos_of + min(med[c], r1 - 1), c);
}

// a: the set's rows as the chain reads them, both operands.  Segment blockIdx.y: the groups gps blockIdx.y .. of the medoid list med[k].
// seg_key, seg_pos [gridDim.y][r1]: a row's least (key, position) over the segment's medoids, kKmNone where no distance is a number
template <int KIND>
__global__ __launch_bounds__(256, 2) void kmedoids_assign_kernel(const double *__restrict__ a, uint32_t r1, uint32_t n_dims, const double *__restrict__ metric, double p,
                                                                 const uint32_t *__restrict__ med, uint32_t k, uint32_t gps, uint64_t *__restrict__ seg_key,
                                                                 uint32_t *__restrict__ seg_pos, const uint32_t *__restrict__ words) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kKmGroup + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kKmStrip + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint64_t s_key[kKmStrip];  // a row's least so far, kept by the first lane of the row: no register is held across the groups
  __shared__ uint32_t s_pos[kKmStrip];
  if (words[kKmDone]) return;
  const uint32_t n_groups = (k + kKmGroup - 1) / kKmGroup, seg = blockIdx.y;
  const uint32_t g_begin = min(seg * gps, n_groups), g_end = min(g_begin + gps, n_groups);
  const uint32_t cg = threadIdx.x % kKmCG, rg = threadIdx.x / kKmCG, ti = cg * 4, tj = rg * kKmTY;
  for (uint64_t s = blockIdx.x; s * kKmStrip < r1; s += gridDim.x) {
    const uint32_t j0 = (uint32_t)(s * kKmStrip), j1 = (uint32_t)min((uint64_t)r1, (uint64_t)j0 + kKmStrip);
    if (cg == 0) {
#pragma unroll
      for (int yy = 0; yy < kKmTY; ++yy) {
        s_key[tj + yy] = kKmNone;
        s_pos[tj + yy] = kSilNone;
      }
    }
    const PairTilesOf groups{kKmGroup, min(k, g_end * kKmGroup)};  // positions in med
    const PairRowsAt cols{a, r1, med};
    const PairRows rows{a, r1};
    PairStage<kKmGroup, kKmStrip> stage;
    PairTile cur = groups.at(g_begin * kKmGroup), nxt;
    for (pair_sweep_open(stage, cols, cur, rows, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
      nxt = groups.after(cur);
      const uint32_t i0 = cur.i0, i1 = cur.i1;
      uint32_t mrow[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) mrow[x] = (i0 + ti + x < i1) ? min(med[i0 + ti + x], r1 - 1) : kSilNone;
      double acc[kKmTY][4];
      pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, rows, j0, j1, n_dims, metric, p, ti, tj, true);
      // positions ascend within a thread, with the lane and from group to group: the least (key, position) of the group, and `<` on
      // the key alone against the groups before, keep among equal distances the first medoid.  A NaN is no key; the row itself is no pair
#pragma unroll
      for (int yy = 0; yy < kKmTY; ++yy) {
        const uint32_t j = j0 + tj + yy;
        KeyAt best{kKmNone, kSilNone};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const double d = scale_distance<KIND>(acc[yy][x], p);
          if (mrow[x] != kSilNone && mrow[x] != j && d == d) {
            const uint64_t key = distance_key(d);
            if (key < best.k) best = KeyAt{key, i0 + ti + x};
          }
        }
        best = reduce_row_lanes(best, kKmCG, key_at_min);
        if (cg == 0 && best.k < s_key[tj + yy]) {
          s_key[tj + yy] = best.k;
          s_pos[tj + yy] = best.c;
        }
      }
    }
    if (cg == 0) {
#pragma unroll
      for (int yy = 0; yy < kKmTY; ++yy) {
        const uint32_t j = j0 + tj + yy;
        if (j < j1) {
          seg_key[(uint64_t)seg * r1 + j] = s_key[tj + yy];
          seg_pos[(uint64_t)seg * r1 + j] = s_pos[tj + yy];
        }
      }
    }
  }
}

// the sum of the workgroup's 256 values in a fixed tree, in thread 0
__device__ __forceinline__ double kmedoids_block_sum(double v, double *s_v) {
  s_v[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_v[threadIdx.x] = __dadd_rn(s_v[threadIdx.x], s_v[threadIdx.x + o]);
    __syncthreads();
  }
  return s_v[0];
}

// a block 256 rows.  The segments hold ascending positions: `<` alone keeps, among equal distances, the first medoid
__global__ __launch_bounds__(256) void kmedoids_merge_kernel(uint32_t r1, uint32_t k, const uint32_t *__restrict__ pos_of, const uint64_t *__restrict__ seg_key,
                                                             const uint32_t *__restrict__ seg_pos, uint32_t n_seg, uint32_t *__restrict__ lab, double *__restrict__ dist,
                                                             double *__restrict__ partial, const uint32_t *__restrict__ words) {
  __shared__ double s_v[256];
  if (words[kKmDone]) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  double mine = 0.0;
  if (i < r1) {
    uint32_t c = pos_of[i];
    double d = 0.0;
    if (c >= k) {
      uint64_t bk = kKmNone;
      c = kSilNone;
      for (uint32_t sg = 0; sg < n_seg; ++sg) {
        const uint64_t key = seg_key[(uint64_t)sg * r1 + i];
        if (key < bk) {
          bk = key;
          c = seg_pos[(uint64_t)sg * r1 + i];
        }
      }
      if (bk == kKmNone || c >= k) {
        c = kSilNone;
        d = __longlong_as_double(0x7FF0000000000000ll);
      } else {
        d = key_f64(bk);
        mine = d;
      }
    }
    lab[i] = c;
    dist[i] = d;
  }
  const double total = kmedoids_block_sum(mine, s_v);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void kmedoids_cost_kernel(const double *__restrict__ partial, uint32_t n_partial, uint32_t max_iter, double *__restrict__ cost,
                                                            const uint32_t *__restrict__ words) {
  __shared__ double s_v[256];
  if (words[kKmDone]) return;
  double mine = 0.0;
  for (uint32_t b = threadIdx.x; b < n_partial; b += 256) mine = __dadd_rn(mine, partial[b]);
  const double total = kmedoids_block_sum(mine, s_v);
  if (threadIdx.x == 0) cost[min(words[kKmIter], max_iter)] = total;
}

// a: as above.  Workgroup blockIdx.x: positions q0 .. q0 + TJ of the grouped order perm (the rows left out lie behind start[k] and get no
// workgroup), TJ = TY n_rg; a thread 4 columns x TY rows as in silhouette_pass_kernel.  The column tiles of the classes of positions q0 and
// q1 - 1 and of those between them; lab: the labelling the grouping was made of.  own_out[r1]: a row's mean over its own class
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void kmedoids_own_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims, const double *__restrict__ metric,
                                                              double p, uint32_t n_cg, uint32_t n_rg, const uint32_t *__restrict__ lab, uint32_t k,
                                                              const uint32_t *__restrict__ perm, const SilTile *__restrict__ tiles, const uint32_t *__restrict__ first_tile,
                                                              const uint32_t *__restrict__ start, uint32_t max_tiles, double *__restrict__ own_out,
                                                              const uint32_t *__restrict__ words) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kSilMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kSilMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_row[kSilMaxTJ], s_cls[kSilMaxTJ];  // the tile's rows and their classes
  if (words[kKmDone]) return;
  const uint32_t TJ = TY * n_rg;
  const uint32_t q0 = blockIdx.x * TJ, n_in = min(start[k], r1);
  if (q0 >= n_in) return;
  const uint32_t q1 = min(n_in, q0 + TJ);
  const uint32_t n_tiles = min(first_tile[k], max_tiles);
  const uint32_t c_lo = min(lab[min(perm[q0], r1 - 1)], k - 1), c_hi = max(min(lab[min(perm[q1 - 1], r1 - 1)], k - 1), c_lo);
  const uint32_t t_begin = min(first_tile[c_lo], n_tiles), t_end = max(min(first_tile[c_hi + 1], n_tiles), t_begin);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < TJ; n += 256) {
    const uint32_t row = q0 + n < q1 ? min(perm[q0 + n], r1 - 1) : kSilNone;
    s_row[n] = row;
    s_cls[n] = row != kSilNone ? min(lab[row], k) : k;
  }
  __syncthreads();  // (s_row is the strip's index list: the first load reads it)
  double run[TY], own[TY];
  uint32_t own_seen = 0;  // bit yy: the row's class has been walked
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) run[yy] = own[yy] = 0.0;
  const auto sum = [](LaneSum x, LaneSum y) { return LaneSum{__dadd_rn(x.v, y.v)}; };
  // both operands gathered.  The strip's rows do not change from step to step: their numbers come from s_row, positions 0 .. q1 - q0, an
  // LDS read in front of each row's load where the grouped order would be a trip to memory (profiles/pair_sweep_refactor.md, section 4)
  const PairRowsAt cols{a, r1, perm}, strip{a, r1, s_row};
  const uint32_t n_strip = q1 - q0;
  PairStage<kSilMaxW, kSilMaxTJ> stage;
  SilStep cur = silhouette_tile(tiles, t_begin, t_end, r1, w), nxt;
  for (pair_sweep_open(stage, cols, cur, strip, 0u, n_strip, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = silhouette_tile(tiles, cur.t + 1, t_end, r1, w);
    uint32_t ri[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) ri[x] = (cur.i0 + ti + x < cur.i1) ? perm[cur.i0 + ti + x] : kSilNone;
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, strip, 0u, n_strip, n_dims, metric, p, ti, tj, true);
    // silhouette_pass_kernel's sum, operation for operation: the columns ascending, the row itself and a column beyond the tile add +0
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t j = s_row[tj + yy];
      double s = run[yy];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        s = __dadd_rn(s, (ri[x] != kSilNone && ri[x] != j) ? d : 0.0);
      }
      run[yy] = s;
    }
    if (!(cur.c & kSilLast)) continue;  // (the same for every thread of the workgroup)
    const uint32_t c = cur.c & ~kSilLast;
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const double total = reduce_row_lanes(LaneSum{run[yy]}, n_cg, sum).v;
      run[yy] = 0.0;
      if (s_cls[tj + yy] == c) {
        own[yy] = cur.n > 1 ? total / (double)(cur.n - 1) : 0.0;
        own_seen |= 1u << yy;
      }
    }
  }
#pragma unroll
  for (int yy = 0; yy < TY; ++yy)
    if (cg == 0 && q0 + tj + yy < q1 && (own_seen & (1u << yy))) own_out[min(perm[q0 + tj + yy], r1 - 1)] = own[yy];
}

// a row left out gets its NaN; per class a 64-bit atomicMin of the key of own_mean
__global__ __launch_bounds__(256) void kmedoids_rows_kernel(const uint32_t *__restrict__ lab, uint32_t r1, uint32_t k, double *__restrict__ own, uint64_t *__restrict__ med_k,
                                                            const uint32_t *__restrict__ words) {
  if (words[kKmDone]) return;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = lab[i];
    if (c < k) {
      const double o = own[i];
      if (o == o) atomicMin(reinterpret_cast<unsigned long long *>(med_k + c), (unsigned long long)distance_key(o));
    } else {
      own[i] = sil_nan();
    }
  }
}

// key, then index: the least under (own_mean, row index) with two integer minima
__global__ __launch_bounds__(256) void kmedoids_medoid_kernel(const uint32_t *__restrict__ lab, uint32_t r1, uint32_t k, const double *__restrict__ own,
                                                              const uint64_t *__restrict__ med_k, uint32_t *__restrict__ med_i, const uint32_t *__restrict__ words) {
  if (words[kKmDone]) return;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = lab[i];
    if (c >= k) continue;
    const double o = own[i];
    if (o == o && distance_key(o) == med_k[c]) atomicMin(med_i + c, (uint32_t)i);
  }
}

// one workgroup.  last: this is round max_iter, whose update is only compared
__global__ __launch_bounds__(1024) void kmedoids_update_kernel(uint32_t k, uint32_t r1, int last, const uint32_t *__restrict__ med_i, uint32_t *__restrict__ med,
                                                               uint32_t *__restrict__ words) {
  if (words[kKmDone]) return;
  int changed = 0;
  for (uint32_t c = threadIdx.x; c < k; c += 1024) {
    const uint32_t m = med_i[c];
    changed |= (m < r1 && m != med[c]) ? 1 : 0;
  }
  changed = __syncthreads_or(changed);
  if (changed && !last) {
    for (uint32_t c = threadIdx.x; c < k; c += 1024) {
      const uint32_t m = med_i[c];
      if (m < r1) med[c] = m;
    }
  }
  if (threadIdx.x == 0) {
    if (!changed) {
      words[kKmConverged] = 1;
      words[kKmDone] = 1;
    } else if (last) {
      words[kKmDone] = 1;
    } else {
      words[kKmIter] += 1;
    }
  }
}

__global__ __launch_bounds__(256) void kmedoids_finish_kernel(uint32_t r1, uint32_t k, uint64_t n_cost, const uint32_t *__restrict__ words, const uint32_t *__restrict__ med,
                                                              const uint32_t *__restrict__ lab, const double *__restrict__ dist, const double *__restrict__ own,
                                                              const uint32_t *__restrict__ cnt, const double *__restrict__ cost, uint32_t *__restrict__ out_medoid,
                                                              uint32_t *__restrict__ out_class_of, double *__restrict__ out_dist, double *__restrict__ out_own,
                                                              uint32_t *__restrict__ out_class_rows, double *__restrict__ out_cost, uint32_t *__restrict__ counts) {
  const uint64_t n = max(max((uint64_t)r1, (uint64_t)k), n_cost);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (i < r1) {
      if (out_class_of) out_class_of[i] = lab[i];
      if (out_dist) out_dist[i] = dist[i];
      if (out_own) out_own[i] = own[i];
    }
    if (i < k) {
      if (out_medoid) out_medoid[i] = med[i];
      if (out_class_rows) out_class_rows[i] = cnt[i];
    }
    if (i < n_cost && out_cost) out_cost[i] = cost[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[0] = words[kKmIter];
    counts[1] = words[kKmConverged];
  }
}

static int kmedoids_arguments(const kpop_refset *rs, uint32_t k, const void *init, const void *counts, const char *who) {
  if (k == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: no medoids", who);
  if (k > rs->r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u medoids in a set of %u rows", who, k, rs->r1);
  if (k > kSilMaxClasses) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u medoids (at most %u)", who, k, kSilMaxClasses);
  if (!init) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null init", who);
  if (!counts) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  return 0;
}

struct KmCall {
  uint32_t r1, k, max_iter, n_dims;
  const double *a, *metric;
  double p;
  KmWork f;
};

// one round: the assignment to med[], its cost, the within-class means, the update
template <int KIND>
static int kmedoids_round(KmCall &c, int last, hipStream_t st) {
  KmWork &f = c.f;
  const uint32_t r1 = c.r1, k = c.k, strips = div_up(r1, kKmStrip);
  const SelfShape s = self_shape(r1);
  const uint32_t *done = f.words + kKmDone;
  const dim3 rows_grid(std::min(strips, 4096u)), b256(256);
  kmedoids_pos_clear_kernel<<<rows_grid, b256, 0, st>>>(f.pos_of, r1, f.med_i, f.med_k, k, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_pos_set_kernel<<<dim3(std::min(div_up(k, 256), 256u)), b256, 0, st>>>(f.med, k, r1, f.pos_of, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_assign_kernel<KIND><<<dim3(std::min(strips, kKmMaxGrid), f.n_seg), b256, 0, st>>>(c.a, r1, c.n_dims, c.metric, c.p, f.med, k, f.gps, f.seg_key, f.seg_pos, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_merge_kernel<<<dim3(strips), b256, 0, st>>>(r1, k, f.pos_of, f.seg_key, f.seg_pos, f.n_seg, f.lab, f.dist, f.partial, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_cost_kernel<<<dim3(1), b256, 0, st>>>(f.partial, strips, c.max_iter, f.cost, f.words);
  KPOP_LAUNCH_CHECK();
  KPOP_TRY(class_tiles_group(f.g, f.lab, r1, k, done, st));
  by_shape_rows(s, [&](auto TY) {
    kmedoids_own_kernel<KIND, decltype(TY)::value><<<dim3(div_up(r1, s.TJ)), b256, 0, st>>>(c.a, s.w, r1, c.n_dims, c.metric, c.p, s.n_cg, s.n_rg, f.lab, k, f.g.perm, f.g.tiles,
                                                                                           f.g.first_tile, f.g.start, f.g.max_tiles, f.own, f.words);
  });
  KPOP_LAUNCH_CHECK();
  kmedoids_rows_kernel<<<rows_grid, b256, 0, st>>>(f.lab, r1, k, f.own, f.med_k, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_medoid_kernel<<<rows_grid, b256, 0, st>>>(f.lab, r1, k, f.own, f.med_k, f.med_i, f.words);
  KPOP_LAUNCH_CHECK();
  kmedoids_update_kernel<<<dim3(1), dim3(1024), 0, st>>>(k, r1, last, f.med_i, f.med, f.words);
  KPOP_LAUNCH_CHECK();
  return 0;
}

// the body of both entry points.  host_loop: the done word is read back after every round; otherwise max_iter + 1 rounds are enqueued
static int kmedoids_dev(kpop_refset *rs, uint32_t k, const uint32_t *d_init, uint32_t max_iter, void *d_work, uint32_t *d_medoid, uint32_t *d_class_of, double *d_dist,
                        double *d_own_mean, uint32_t *d_class_rows, double *d_cost, uint32_t *d_counts, bool host_loop, hipStream_t st, const char *who) {
  KPOP_TRY(kmedoids_arguments(rs, k, d_init, d_counts, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  KmCall c;
  c.r1 = rs->r1;
  c.k = k;
  c.max_iter = max_iter;
  c.n_dims = rs->n_dims;
  c.metric = rs->metric;
  c.p = rs->p;
  c.f = kmedoids_carve(d_work, c.r1, k, max_iter);
  const uint64_t n_cost = (uint64_t)max_iter + 1;
  KPOP_TRY(refset_chain_rows(rs, st, &c.a));
  KPOP_HIP(hipMemsetAsync(c.f.words, 0, 256, st));
  kmedoids_init_kernel<<<dim3(std::min(div_up(std::max((uint64_t)k, n_cost), 256), 4096u)), dim3(256), 0, st>>>(d_init, k, c.r1, n_cost, c.f.med, c.f.cost);
  KPOP_LAUNCH_CHECK();
  KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
    constexpr int KIND = decltype(K)::value;
    for (uint64_t t = 0; t <= max_iter; ++t) {
      KPOP_TRY(kmedoids_round<KIND>(c, t == max_iter, st));
      if (!host_loop) continue;
      uint32_t done = 0;
      KPOP_HIP(hipMemcpyAsync(&done, c.f.words + kKmDone, 4, hipMemcpyDeviceToHost, st));
      KPOP_HIP(hipStreamSynchronize(st));
      if (done) break;
    }
    return 0;
  }));
  const uint64_t n = std::max(std::max((uint64_t)c.r1, (uint64_t)k), n_cost);
  kmedoids_finish_kernel<<<dim3(std::min(div_up(n, 256), 4096u)), dim3(256), 0, st>>>(c.r1, k, n_cost, c.f.words, c.f.med, c.f.lab, c.f.dist, c.f.own, c.f.g.cnt, c.f.cost, d_medoid,
                                                                                     d_class_of, d_dist, d_own_mean, d_class_rows, d_cost, d_counts);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_kmedoids_workspace_bytes(const kpop_refset *rs, uint32_t n_medoids, uint32_t max_iter) {
  if (!rs || n_medoids == 0 || n_medoids > kSilMaxClasses || n_medoids > rs->r1) return 0;
  return kmedoids_carve(nullptr, rs->r1, n_medoids, max_iter).bytes;
}

extern "C" int kpop_dev_kmedoids(kpop_refset *rs, uint32_t n_medoids, const uint32_t *d_init, uint32_t max_iter, void *d_work, uint32_t *d_medoid, uint32_t *d_class_of,
                                 double *d_dist, double *d_own_mean, uint32_t *d_class_rows, double *d_cost, uint32_t *d_counts, void *stream) {
  const char *who = "kpop_dev_kmedoids";
  KPOP_TRY(refset_check_handle(rs, who));
  return kmedoids_dev(rs, n_medoids, d_init, max_iter, d_work, d_medoid, d_class_of, d_dist, d_own_mean, d_class_rows, d_cost, d_counts, false, as_stream(stream), who);
}

extern "C" int kpop_kmedoids(kpop_refset *rs, uint32_t n_medoids, const uint32_t *init, uint32_t max_iter, uint32_t *medoid, uint32_t *class_of, double *dist,
                             double *own_mean, uint32_t *class_rows, double *cost, uint32_t *n_iter, int *converged) {
  const char *who = "kpop_kmedoids";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(kmedoids_arguments(rs, n_medoids, init, n_iter, who));
  if (!converged) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  const uint32_t r1 = rs->r1, k = n_medoids;
  KPOP_TRY(check_distinct_rows(init, k, r1, who, "init", "row"));
  const uint64_t n_cost = (uint64_t)max_iter + 1;
  uint32_t counts[2] = {0, 0};
  HostCall h;
  void *work = h.work(kmedoids_carve(nullptr, r1, k, max_iter).bytes);
  const uint32_t *di = h.in(init, k);
  uint32_t *dn = h.scalars(counts, 2);
  uint32_t *dm = h.out(medoid, k), *dc = h.out(class_of, r1);
  double *dd = h.out(dist, r1), *dow = h.out(own_mean, r1);
  uint32_t *dr = h.out(class_rows, k);
  double *dco = h.out(cost, n_cost);
  KPOP_TRY(h.upload());
  KPOP_TRY(kmedoids_dev(rs, k, di, max_iter, work, dm, dc, dd, dow, dr, dco, dn, true, h.st, who));
  KPOP_TRY(h.finish());
  *n_iter = counts[0];
  *converged = (int)counts[1];
  return KPOP_OK;
}

extern "C" int kpop_distance_kmedoids(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize, uint32_t n_medoids,
                                      const uint32_t *init, uint32_t max_iter, uint32_t *medoid, uint32_t *class_of, double *dist, double *own_mean,
                                      uint32_t *class_rows, double *cost, uint32_t *n_iter, int *converged) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_kmedoids(rs, n_medoids, init, max_iter, medoid, class_of, dist, own_mean, class_rows, cost, n_iter, converged);
  });
}
