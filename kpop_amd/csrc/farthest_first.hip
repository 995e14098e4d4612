// farthest_first.hip -- the farthest-first traversal of a resident set (Gonzalez 1985): k diverse rows for every k, each prefix a cover
// of the set with its radius beside it.  The radius-free partner of representatives.hip.
//
//   The distances of clusters.hip: the set's r1 rows, d(j, i) the reference chain's distance (lib/Space.ml:182-205 with the adaptors of
//   lib/Matrix.ml:243-250), symmetric bit for bit, the pair i == j never examined; no kpop_tune setting is read.  Every row has a COVER
//   DISTANCE (+inf at first) and a COVER ROW (KPOP_NOISE at first).  Picking row c marks it; for every unpicked row x, d(x, c) replaces the
//   cover distance iff it is a number and strictly less (-0 taken as +0): a NaN covers nothing, a tie keeps the earlier pick.  After the
//   seeds, the next pick is the unpicked row greatest under (cover distance descending, row index ascending) -- a strict total order, so
//   the result is defined without reference to an algorithm: the same bits on every run.
//
// A pass over the set per pick would read the set k times.  Here a pass applies a GROUP of up to kFfGroup picks, and between two passes
// one workgroup resolves the next group from what the pass left behind.  The state lives in the workspace: ckey[] (a row's cover
// distance as a distance_key word, 0 for a picked row: no distance's key is 0), crow[], the picks with their radii and parents, the
// buckets, and the control words.
//   farthest_first_pass_kernel     the rows of the set against the group, the group's rows gathered as the tile's columns (the indexed
//                                  row view of pair_tile.h, PairRowsAt, under pair_tile_distances: no copy of a row is kept).  A
//                                  workgroup takes strips of 256 rows, strip s going to workgroup s mod the grid; a thread 4 picks x 8 rows, the chain of a pair in one thread, the dimensions
//                                  ascending.  The least (key, position in the group) of a row over the row's lanes is what applying the
//                                  group's updates in pick order leaves; it replaces the row's key iff strictly less.  A row belongs to
//                                  BUCKET (workgroup, row mod nb) -- by stride, not by range: rows that lie together in the file
//                                  tend to be near each other, and one lineage should not own one bucket.  The workgroup leaves, a
//                                  bucket, the best and the second-best unpicked row under the order, as (key, index) words
//   farthest_first_resolve_kernel  one workgroup, a bucket a thread.  The buckets' best rows are the CANDIDATES; the greatest of the
//                                  second-best entries is the BOUND on every row that is not a candidate (a key only ever falls).  While
//                                  the greatest candidate precedes the bound it is the set's greatest row: it is picked, and the chain
//                                  from it to every candidate that still precedes the bound updates that candidate -- the same operations
//                                  in the same order as the pass, so the same bits.  The first pick of a group always precedes the bound
//                                  (the bound is some bucket's second, which its own best precedes), so every pass makes progress.
//                                  Stops the traversal at max_picks picks, or when the greatest row's cover distance is <= cover_radius
//   farthest_first_seeds_kernel    a forced group: seeds[s0 .. s0 + g), each with its cover distance against everything picked before it
//   farthest_first_finish_kernel   rep_of and rep_dist out of ckey and crow, the picks and the counts to where the caller wants them
// The boundary between pass and resolve is a launch boundary; no kernel waits for another workgroup.  A pass with an empty group and a
// resolve behind the done word return at once: the device form enqueues the worst case (a pick a pass), the host form reads the done
// word back every few passes and stops.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr uint32_t kFfGroup = 32;     // picks a group at most: the columns of the pass kernel's tile
constexpr uint32_t kFfResolvePicks = kFfGroup;  // picks the resolve makes a pass at most (1: the pick-a-pass form that profiles/farthest_first.md times beside this one)
constexpr uint32_t kFfStrip = 256;    // rows a strip
constexpr uint32_t kFfMaxGrid = 512;  // workgroups of the pass kernel at most: two a CU, as its registers admit
constexpr uint32_t kFfResolve = 1024; // buckets at most: the candidates, a thread each of the resolve
constexpr uint64_t kFfNone = ~0ull;                     // (no key: a NaN is never a key)
constexpr uint64_t kFfInfKey = 0xFFF0000000000000ull;  // distance_key(+inf)
constexpr uint32_t kFfNoRow = 0xFFFFFFFFu;
constexpr int kFfTY = 8, kFfCG = 8;  // a thread 4 columns x 8 rows; 8 lanes a row
static_assert(kFfGroup == 4 * kFfCG && kFfStrip == kFfTY * (256 / kFfCG), "the tile is the group x a strip");
static_assert(kFfResolvePicks >= 1 && kFfResolvePicks <= kFfGroup, "a group fits the tile's columns");
static_assert(kFfResolve == 1024 && 2 * kFfMaxGrid <= kFfResolve, "the resolving workgroup holds a bucket a thread");
// buckets a workgroup of a grid (row mod 2, 4 or 8): as many as the resolve has threads for
static uint32_t farthest_first_buckets(uint32_t grid) { return grid > 256 ? 2u : grid > 128 ? 4u : 8u; }

enum { kFfPicks = 0, kFfPasses = 1, kFfDone = 2, kFfStart = 3, kFfSize = 4 };  // the control words: picks made, passes, done, the pending group

struct FfBucket {
  uint64_t best_k, second_k;
  uint32_t best_i, second_i;
};

struct FfWork {
  uint32_t *words, *crow, *pick, *parent;
  uint64_t *ckey;
  double *radius;
  FfBucket *buckets;
  uint64_t bytes;
};

static FfWork farthest_first_carve(void *base, uint32_t r1, uint32_t max_picks) {
  const uint64_t n = std::max(r1, 1u), k = std::max(std::min(max_picks, r1), 1u);
  Carver c(base);
  FfWork f;
  f.words = c.take<uint32_t>(256);
  f.buckets = c.take<FfBucket>(sizeof(FfBucket) * kFfResolve);
  f.ckey = c.take<uint64_t>(n * 8);
  f.crow = c.take<uint32_t>(n * 4);
  f.pick = c.take<uint32_t>(k * 4);
  f.radius = c.take<double>(k * 8);
  f.parent = c.take<uint32_t>(k * 4);
  f.bytes = c.off;
  return f;
}

// (key, index) a precedes (key, index) b: the greater cover distance, then the smaller row.  A picked row and an empty bucket are
// (0, kFfNoRow), which every row precedes
__device__ __forceinline__ bool ff_precedes(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka > kb || (ka == kb && ia < ib); }

struct FfTop2 {
  uint64_t bk = 0, sk = 0;
  uint32_t bi = kFfNoRow, si = kFfNoRow;
  __device__ __forceinline__ void insert(uint64_t k, uint32_t i) {
    if (k == 0) return;
    if (ff_precedes(k, i, bk, bi)) {
      sk = bk;
      si = bi;
      bk = k;
      bi = i;
    } else if (ff_precedes(k, i, sk, si)) {
      sk = k;
      si = i;
    }
  }
};

// one pair's chain, as pair_accumulate writes it (lib/Space.ml:192-200): row i first
template <int KIND>
__device__ __forceinline__ double ff_chain(const double *__restrict__ a, uint32_t n_dims, const double *__restrict__ metric, double p, uint32_t i, uint32_t j) {
  const double *__restrict__ x = a + (uint64_t)i * n_dims, *__restrict__ y = a + (uint64_t)j * n_dims;
  double acc = 0.0;
  for (uint32_t c = 0; c < n_dims; ++c) {
    const double diff = __dsub_rn(x[c], y[c]);
    acc = __dadd_rn(acc, component<KIND>(diff, metric[c], p));
  }
  return scale_distance<KIND>(acc, p);
}

__global__ __launch_bounds__(256) void farthest_first_init_kernel(uint32_t r1, uint64_t *__restrict__ ckey, uint32_t *__restrict__ crow) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    ckey[i] = kFfInfKey;
    crow[i] = KPOP_NOISE;
  }
}

// a: the set's rows as the chain reads them, both operands; the group: pick[start .. start + g), both from the control words, held to the
// capacity of pick[] (cap) and to kFfGroup.  first: the launch that opens a traversal without seeds walks the keys with an empty group,
// for the buckets alone.  nb: the buckets a workgroup, a power of two
template <int KIND>
__global__ __launch_bounds__(256, 2) void farthest_first_pass_kernel(const double *__restrict__ a, uint32_t r1, uint32_t n_dims, const double *__restrict__ metric,
                                                                     double p, int first, uint32_t nb, uint32_t cap, const uint32_t *__restrict__ words,
                                                                     const uint32_t *__restrict__ pick, uint64_t *__restrict__ ckey, uint32_t *__restrict__ crow,
                                                                     FfBucket *__restrict__ buckets) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kFfGroup + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kFfStrip + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint64_t s_key[kFfStrip], s_sk[256];
  __shared__ uint32_t s_bi[256], s_si[256];
  const uint32_t start = min(words[kFfStart], cap), g = min(min(words[kFfSize], kFfGroup), cap - start);
  if (g == 0 && !first) return;
  const uint32_t cg = threadIdx.x % kFfCG, rg = threadIdx.x / kFfCG, ti = cg * 4, tj = rg * kFfTY;
  FfTop2 top;
  for (uint64_t s = blockIdx.x; s * kFfStrip < r1; s += gridDim.x) {
    const uint32_t j0 = (uint32_t)(s * kFfStrip), j1 = (uint32_t)min((uint64_t)r1, (uint64_t)j0 + kFfStrip);
    uint64_t mine = 0;
    if (g) {
      double acc[kFfTY][4];
      pair_tile_distances<KIND, kFfTY, kFfGroup, kFfStrip>(acc, As, Bs, s_metric, PairRowsAt{a, r1, pick}, start, start + g, PairRows{a, r1}, j0, j1, n_dims,
                                                           metric, p, ti, tj, true);
      // the epilogue: positions ascend within a thread and with the lane, so the least (key, position) is the first pick of the group
      // that brings the least distance: what the group's updates in pick order leave.  A NaN is no key
#pragma unroll
      for (int yy = 0; yy < kFfTY; ++yy) {
        KeyAt best{kFfNone, 0u};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const double d = acc[yy][x];
          if (ti + x < g && d == d) {
            const uint64_t key = distance_key(d);
            if (key < best.k) best = KeyAt{key, ti + x};
          }
        }
        best = reduce_row_lanes(best, kFfCG, key_at_min);
        const uint32_t j = j0 + tj + yy;
        if (cg == 0) {
          uint64_t cur = 0;
          if (j < j1) {
            cur = ckey[j];
            if (cur != 0 && best.k < cur) {  // (a picked row stays picked; kFfNone is below no key)
              cur = best.k;
              ckey[j] = cur;
              crow[j] = pick[start + min(best.c, g - 1)];
            }
          }
          s_key[tj + yy] = cur;
        }
      }
      __syncthreads();
      mine = s_key[threadIdx.x];
    } else if (j0 + threadIdx.x < j1) {
      mine = ckey[j0 + threadIdx.x];
    }
    top.insert(mine, j0 + threadIdx.x);
  }
  // the workgroup's buckets: thread t holds rows t mod 256, so bucket b is the threads t mod nb == b
  __syncthreads();
  s_key[threadIdx.x] = top.bk;
  s_bi[threadIdx.x] = top.bi;
  s_sk[threadIdx.x] = top.sk;
  s_si[threadIdx.x] = top.si;
  __syncthreads();
  if (threadIdx.x < nb) {
    FfTop2 m;
    for (uint32_t u = threadIdx.x; u < 256; u += nb) {
      m.insert(s_key[u], s_bi[u]);
      m.insert(s_sk[u], s_si[u]);
    }
    buckets[blockIdx.x * nb + threadIdx.x] = FfBucket{m.bk, m.sk, m.bi, m.si};
  }
}

// the greatest (key, index) of the workgroup's 1,024 threads, in every thread
__device__ __forceinline__ KeyAt ff_block_greatest(KeyAt v, uint64_t *s_k, uint32_t *s_i) {
  const auto greater = [](KeyAt x, KeyAt y) { return ff_precedes(y.k, y.c, x.k, x.c) ? y : x; };
  for (uint32_t o = 32; o > 0; o >>= 1) v = greater(v, lane_xor(v, o));
  __syncthreads();  // (the words of the call before have been read)
  if ((threadIdx.x & 63u) == 0) {
    s_k[threadIdx.x >> 6] = v.k;
    s_i[threadIdx.x >> 6] = v.c;
  }
  __syncthreads();
  v = KeyAt{s_k[0], s_i[0]};
  for (uint32_t w = 1; w < kFfResolve / 64; ++w) v = greater(v, KeyAt{s_k[w], s_i[w]});
  return v;
}

// n_buckets: what the pass kernel's grid wrote.  radius_key: distance_key(cover_radius), 0 for a radius that never stops the traversal.
// max_picks <= r1 and the capacity of pick[]
template <int KIND>
__global__ __launch_bounds__(1024) void farthest_first_resolve_kernel(const double *__restrict__ a, uint32_t r1, uint32_t n_dims, const double *__restrict__ metric,
                                                                      double p, uint32_t max_picks, uint64_t radius_key, uint32_t n_buckets,
                                                                      const FfBucket *__restrict__ buckets, uint32_t *__restrict__ words,
                                                                      uint64_t *__restrict__ ckey, const uint32_t *__restrict__ crow, uint32_t *__restrict__ pick,
                                                                      double *__restrict__ radius, uint32_t *__restrict__ parent) {
  __shared__ uint64_t s_k[kFfResolve / 64];
  __shared__ uint32_t s_i[kFfResolve / 64];
  const bool was_done = words[kFfDone] != 0;
  const uint32_t n_start = min(words[kFfPicks], max_picks);
  if (was_done) {  // (the pass before this launch applied the last group)
    __syncthreads();
    if (threadIdx.x == 0) words[kFfSize] = 0;
    return;
  }
  uint64_t ck = 0, sk = 0;
  uint32_t ci = kFfNoRow, si = kFfNoRow, cpar = KPOP_NOISE;
  if (threadIdx.x < n_buckets) {
    const FfBucket b = buckets[threadIdx.x];
    // an index is used only when it lies inside the set
    if (b.best_i < r1 && b.best_k != 0) {
      ck = b.best_k;
      ci = b.best_i;
      cpar = crow[ci];
    }
    if (b.second_i < r1 && b.second_k != 0) {
      sk = b.second_k;
      si = b.second_i;
    }
  }
  const KeyAt bound = ff_block_greatest(KeyAt{sk, si}, s_k, s_i);
  uint32_t n = n_start;
  bool done = false;
  for (uint32_t it = 0; it < kFfResolvePicks; ++it) {
    if (n >= max_picks) {
      done = true;
      break;
    }
    const KeyAt top = ff_block_greatest(KeyAt{ck, ci}, s_k, s_i);
    if (top.k == 0) {  // the candidates are used up; no unpicked row is left iff no bucket had a second
      done = bound.k == 0;
      break;
    }
    if (!ff_precedes(top.k, top.c, bound.k, bound.c)) break;
    if (radius_key != 0 && top.k <= radius_key) {
      done = true;
      break;
    }
    if (ci == top.c && ck != 0) {
      pick[n] = ci;
      radius[n] = key_f64(ck);
      parent[n] = cpar;
      ckey[ci] = 0;
      ck = 0;
      ci = kFfNoRow;
    }
    ++n;
    if (ck != 0 && ff_precedes(ck, ci, bound.k, bound.c)) {  // (any other candidate is out of this group's reach: the pass will see to it)
      const double d = ff_chain<KIND>(a, n_dims, metric, p, top.c, ci);
      if (d == d) {
        const uint64_t key = distance_key(d);
        if (key < ck) {
          ck = key;
          cpar = top.c;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    words[kFfStart] = n_start;
    words[kFfSize] = n - n_start;
    words[kFfPicks] = n;
    if (n > n_start) words[kFfPasses] += 1;
    if (done) words[kFfDone] = 1;
  }
}

// one workgroup of kFfGroup threads or more.  seeds[s0 .. s0 + g) are trusted to be distinct; an index is held inside the set
template <int KIND>
__global__ __launch_bounds__(64) void farthest_first_seeds_kernel(const double *__restrict__ a, uint32_t r1, uint32_t n_dims, const double *__restrict__ metric, double p,
                                                                  const uint32_t *__restrict__ seeds, uint32_t s0, uint32_t g, uint32_t *__restrict__ words,
                                                                  uint64_t *__restrict__ ckey, const uint32_t *__restrict__ crow, uint32_t *__restrict__ pick,
                                                                  double *__restrict__ radius, uint32_t *__restrict__ parent) {
  const uint32_t t = threadIdx.x;
  uint32_t s = 0;
  if (t < g) {
    s = min(seeds[s0 + t], r1 - 1);
    uint64_t ck = ckey[s];
    uint32_t cpar = crow[s];
    for (uint32_t u = 0; u < t; ++u) {  // the seeds of this group before it, in order
      const uint32_t su = min(seeds[s0 + u], r1 - 1);
      const double d = ff_chain<KIND>(a, n_dims, metric, p, su, s);
      if (d == d) {
        const uint64_t key = distance_key(d);
        if (key < ck) {
          ck = key;
          cpar = su;
        }
      }
    }
    pick[s0 + t] = s;
    radius[s0 + t] = ck ? key_f64(ck) : 0.0;  // (a repeated seed, which the host form refuses)
    parent[s0 + t] = cpar;
  }
  __syncthreads();
  if (t < g) ckey[s] = 0;
  if (t == 0) {
    words[kFfStart] = s0;
    words[kFfSize] = g;
    words[kFfPicks] = s0 + g;
    words[kFfPasses] += 1;
  }
}

__global__ __launch_bounds__(256) void farthest_first_finish_kernel(uint32_t r1, uint32_t cap, const uint32_t *__restrict__ words, const uint64_t *__restrict__ ckey,
                                                                    const uint32_t *__restrict__ crow, const uint32_t *__restrict__ pick,
                                                                    const double *__restrict__ radius, const uint32_t *__restrict__ parent,
                                                                    uint32_t *__restrict__ out_pick, double *__restrict__ out_radius,
                                                                    uint32_t *__restrict__ out_parent, uint32_t *__restrict__ rep_of,
                                                                    double *__restrict__ rep_dist, uint32_t *__restrict__ counts) {
  const uint32_t n = min(words[kFfPicks], cap);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint64_t k = ckey[i];
    if (rep_of) rep_of[i] = k == 0 ? (uint32_t)i : crow[i];
    if (rep_dist) rep_dist[i] = k == 0 ? 0.0 : key_f64(k);
    if (i < n) {
      if (out_pick) out_pick[i] = pick[i];
      if (out_radius) out_radius[i] = radius[i];
      if (out_parent) out_parent[i] = parent[i];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[0] = n;
    counts[1] = words[kFfPasses];
  }
}

struct FfCall {
  uint32_t r1, max_picks, n_seeds, n_dims;
  const uint32_t *d_seeds;
  const double *a, *metric;
  double p;
  uint64_t radius_key;
  uint32_t grid, nb;
  FfWork f;
};

template <int KIND>
static int farthest_first_pass(const FfCall &c, int first, hipStream_t st) {
  farthest_first_pass_kernel<KIND><<<dim3(c.grid), dim3(256), 0, st>>>(c.a, c.r1, c.n_dims, c.metric, c.p, first, c.nb, c.max_picks, c.f.words, c.f.pick, c.f.ckey, c.f.crow,
                                                                      c.f.buckets);
  KPOP_LAUNCH_CHECK();
  return 0;
}

template <int KIND>
static int farthest_first_resolve(const FfCall &c, hipStream_t st) {
  farthest_first_resolve_kernel<KIND><<<dim3(1), dim3(kFfResolve), 0, st>>>(c.a, c.r1, c.n_dims, c.metric, c.p, c.max_picks, c.radius_key, c.grid * c.nb,
                                                                            c.f.buckets, c.f.words, c.f.ckey, c.f.crow, c.f.pick, c.f.radius, c.f.parent);
  KPOP_LAUNCH_CHECK();
  return 0;
}

// the seeds as forced groups, each followed by its pass; without seeds the pass that fills the buckets
template <int KIND>
static int farthest_first_open(const FfCall &c, hipStream_t st) {
  for (uint32_t s0 = 0; s0 < c.n_seeds; s0 += kFfGroup) {
    farthest_first_seeds_kernel<KIND><<<dim3(1), dim3(64), 0, st>>>(c.a, c.r1, c.n_dims, c.metric, c.p, c.d_seeds, s0, std::min(kFfGroup, c.n_seeds - s0), c.f.words,
                                                                    c.f.ckey, c.f.crow, c.f.pick, c.f.radius, c.f.parent);
    KPOP_LAUNCH_CHECK();
    KPOP_TRY(farthest_first_pass<KIND>(c, 0, st));
  }
  if (c.n_seeds == 0) KPOP_TRY(farthest_first_pass<KIND>(c, 1, st));
  return 0;
}

// `rounds` times: the next group, and its pass
template <int KIND>
static int farthest_first_rounds(const FfCall &c, uint32_t rounds, hipStream_t st) {
  for (uint32_t r = 0; r < rounds; ++r) {
    KPOP_TRY(farthest_first_resolve<KIND>(c, st));
    KPOP_TRY(farthest_first_pass<KIND>(c, 0, st));
  }
  return 0;
}

static int farthest_first_arguments(const kpop_refset *rs, uint32_t max_picks, double cover_radius, uint32_t n_seeds, const void *seeds, const void *counts,
                                    const char *who) {
  if (cover_radius != cover_radius) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the radius is not a number", who);
  if (!counts) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  if (n_seeds && !seeds) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null seeds", who);
  if (n_seeds > max_picks) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u seeds for %u picks", who, n_seeds, max_picks);
  if (n_seeds > rs->r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u seeds in a set of %u", who, n_seeds, rs->r1);
  return 0;
}

// the body of both entry points: enqueues only.  d_done: where the host form wants the done word read from (the workspace's), or null:
// then the worst case is enqueued, a pick a pass, every launch behind the stop returning at once
static int farthest_first_dev(kpop_refset *rs, uint32_t max_picks, double cover_radius, const uint32_t *d_seeds, uint32_t n_seeds, void *d_work, uint32_t *d_pick,
                              double *d_pick_radius, uint32_t *d_pick_parent, uint32_t *d_rep_of, double *d_rep_dist, uint32_t *d_counts, bool host_loop,
                              hipStream_t st, const char *who) {
  KPOP_TRY(farthest_first_arguments(rs, max_picks, cover_radius, n_seeds, d_seeds, d_counts, who));
  const uint32_t r1 = rs->r1;
  max_picks = std::min(max_picks, r1);
  if (max_picks == 0 && r1 == 0) {
    KPOP_HIP(hipMemsetAsync(d_counts, 0, 8, st));
    return KPOP_OK;
  }
  FfCall c;
  c.r1 = r1;
  c.max_picks = max_picks;
  c.n_seeds = n_seeds;
  c.n_dims = rs->n_dims;
  c.d_seeds = d_seeds;
  c.metric = rs->metric;
  c.p = rs->p;
  c.f = farthest_first_carve(d_work, r1, max_picks);
  c.grid = std::min(div_up(r1, kFfStrip), kFfMaxGrid);
  c.nb = farthest_first_buckets(c.grid);
  // (no distance is negative: below zero nothing stops the traversal.  -0 is 0)
  c.radius_key = 0;
  if (cover_radius >= 0.0) {
    const double r = cover_radius + 0.0;
    uint64_t bits;
    memcpy(&bits, &r, 8);
    c.radius_key = bits | (1ull << 63);  // distance_key of a number that is not negative
  }
  KPOP_HIP(hipMemsetAsync(c.f.words, 0, 256, st));
  farthest_first_init_kernel<<<dim3(std::min(div_up(r1, 256), 4096u)), dim3(256), 0, st>>>(r1, c.f.ckey, c.f.crow);
  KPOP_LAUNCH_CHECK();
  if (max_picks) {
    KPOP_TRY(refset_chain_rows(rs, st, &c.a));
    KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
      constexpr int KIND = decltype(K)::value;
      KPOP_TRY(farthest_first_open<KIND>(c, st));
      // every round but the last makes a pick or more; the last finds the stop
      const uint32_t worst = max_picks - n_seeds + 1;
      if (!host_loop) return farthest_first_rounds<KIND>(c, worst, st);
      uint32_t made = 0, batch = 4;
      while (made < worst) {
        const uint32_t rounds = std::min(batch, worst - made);
        KPOP_TRY(farthest_first_rounds<KIND>(c, rounds, st));
        made += rounds;
        uint32_t done = 0;
        KPOP_HIP(hipMemcpyAsync(&done, c.f.words + kFfDone, 4, hipMemcpyDeviceToHost, st));
        KPOP_HIP(hipStreamSynchronize(st));
        if (done) break;
        batch = std::min(batch * 2, 64u);
      }
      return 0;
    }));
  }
  farthest_first_finish_kernel<<<dim3(std::min(div_up(r1, 256), 4096u)), dim3(256), 0, st>>>(r1, max_picks, c.f.words, c.f.ckey, c.f.crow, c.f.pick, c.f.radius,
                                                                                            c.f.parent, d_pick, d_pick_radius, d_pick_parent, d_rep_of, d_rep_dist,
                                                                                            d_counts);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_farthest_first_workspace_bytes(const kpop_refset *rs, uint32_t max_picks) {
  if (!rs) return 0;
  return farthest_first_carve(nullptr, rs->r1, max_picks).bytes;
}

extern "C" int kpop_dev_farthest_first(kpop_refset *rs, uint32_t max_picks, double cover_radius, const uint32_t *d_seeds, uint32_t n_seeds, void *d_work,
                                       uint32_t *d_pick, double *d_pick_radius, uint32_t *d_pick_parent, uint32_t *d_rep_of, double *d_rep_dist,
                                       uint32_t *d_counts, void *stream) {
  const char *who = "kpop_dev_farthest_first";
  KPOP_TRY(refset_check_handle(rs, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return farthest_first_dev(rs, max_picks, cover_radius, d_seeds, n_seeds, d_work, d_pick, d_pick_radius, d_pick_parent, d_rep_of, d_rep_dist, d_counts, false,
                            as_stream(stream), who);
}

extern "C" int kpop_farthest_first(kpop_refset *rs, uint32_t max_picks, double cover_radius, const uint32_t *seeds, uint32_t n_seeds, uint32_t *n_picks,
                                   uint32_t *pick, double *pick_radius, uint32_t *pick_parent, uint32_t *rep_of, double *rep_dist, uint32_t *n_passes) {
  const char *who = "kpop_farthest_first";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(farthest_first_arguments(rs, max_picks, cover_radius, n_seeds, seeds, n_picks, who));
  const uint32_t r1 = rs->r1;
  KPOP_TRY(check_distinct_rows(seeds, n_seeds, r1, who, "seeds", "seed"));
  *n_picks = 0;
  if (n_passes) *n_passes = 0;
  if (r1 == 0) return KPOP_OK;
  const uint32_t k = std::min(max_picks, r1);
  HostCall h;
  void *work = h.work(farthest_first_carve(nullptr, r1, k).bytes);
  uint32_t *dn = h.scalars<uint32_t>();
  const uint32_t *ds = n_seeds ? h.in(seeds, n_seeds) : nullptr;
  uint32_t *dp = h.counted(pick, k);
  double *dr = h.counted(pick_radius, k);
  uint32_t *da = h.counted(pick_parent, k), *dof = h.out(rep_of, r1);
  double *dd = h.out(rep_dist, r1);
  KPOP_TRY(h.upload());
  KPOP_TRY(farthest_first_dev(rs, max_picks, cover_radius, ds, n_seeds, work, dp, dr, da, dof, dd, dn, true, h.st, who));
  uint32_t counts[2] = {0, 0};
  KPOP_TRY(h.read(counts, dn, 2));
  const uint32_t n = std::min(counts[0], k);
  KPOP_TRY(h.finish(n));
  *n_picks = n;
  if (n_passes) *n_passes = counts[1];
  return KPOP_OK;
}

extern "C" int kpop_distance_farthest_first(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                            uint32_t max_picks, double cover_radius, const uint32_t *seeds, uint32_t n_seeds, uint32_t *n_picks, uint32_t *pick,
                                            double *pick_radius, uint32_t *pick_parent, uint32_t *rep_of, double *rep_dist, uint32_t *n_passes) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_farthest_first(rs, max_picks, cover_radius, seeds, n_seeds, n_picks, pick, pick_radius, pick_parent, rep_of, rep_dist, n_passes);
  });
}
