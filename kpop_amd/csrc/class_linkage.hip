// class_linkage.hip -- the distances between every two classes of a labelled resident set, in one pass over the pair tiles, and the tree
// the classes form under them.
//
//   The set's r1 rows, class_of[r1] (a class in [0, n_classes) or KPOP_NO_CLASS: the row is LEFT OUT of everything), d(i, j) the
//   reference chain's distance, kpop_silhouette's: the bits kpop_refset_distance_rowwise writes on the vector pipe when the set's own
//   rows are the query -- no kpop_tune setting is read; the pair i == j is never examined.  P(a, b), a != b: the pairs of one row of a and
//   one row of b; P(a, a): the pairs i < j of two rows of a.  For every two classes: mean_dist, the sum of d over P divided by |P| (the
//   declared NaN where P is empty; a NaN distance makes it a NaN); min_dist, max_dist over the pairs whose distance is a number (-0 as +0;
//   none: the declared NaN); min_i < min_j, the least pair under (d with -0 as +0, i, j) (none: KPOP_NO_CLASS).  class_rows: the rows of a class.
//
// Neither the r1 x r1 matrix nor an r1 x n_classes table is formed, nothing is read back, nothing synchronises:
//   class_tiles_group         (class_tiles.h, shared with silhouette.hip and kmedoids.hip) the rows grouped by class, and the column
//                             tiles, each of ONE class
//   class_linkage_sweep_kernel  a workgroup owns a STRIP, TJ consecutive positions of the grouped order (kmedoids_own_kernel's strip, both
//                             operands gathered: PairRowsAt, the sweep of pair_tile.h, both tile shapes of self_shape), and a SEGMENT of
//                             the column tiles of the classes up to the strip's highest: THE TRIANGLE.  A row of class rc meets a
//                             column class cc <= rc; what a strip that spans several classes computes of cc > rc is dropped: it belongs
//                             to the strip that holds cc's rows.  Inside a diagonal block (cc == rc) both orders of a pair are computed.
//                             A thread keeps, for each of its TY rows, the running sum of the column class, the least (key, column)
//                             and the greatest key.  Where the column class ends a row's n_cg lanes meet (reduce_row_lanes), the rows'
//                             values go to LDS, and every RUN of the strip -- its rows of one class, contiguous -- is folded by one
//                             thread in ascending position: one partial per (run, column class) leaves the workgroup, at
//                             part[(strip + rc) n_classes + cc] (strip + rc grows strictly along the runs of the grouped order).
//   class_linkage_combine_kernel  a thread a class pair a <= b: the partials of b's strips in ascending strip order, one division, and the
//                             entry written to both halves of the table: the symmetry is exact because nothing is computed twice.
// THE SUMS: the sum of (a, b), a <= b, is taken in an order that is a function of r1 (the tile shape) and of the labelling alone: position
// k of class a goes to lane (k % w) / 4 of a row of b, a lane adds its positions ascending, a row's lanes meet in a fixed tree, a run's rows
// are added in ascending position, b's runs in ascending strip.  On the diagonal every pair is added twice, once from each of its rows, and
// the divisor is n (n - 1).  No floating-point atomic, nothing that depends on timing: the same bits on every run.  Under a renumbering
// of the classes the minima, the maxima and the least pairs keep their bits (they do not depend on any order); a mean stays within the
// rounding of its sum but not bit for bit: which class of a pair supplies the strip's rows is the numbering's to say.
// THE LOAD: a late strip walks more column tiles than an early one.  The walk is cut into segments of WHOLE classes at the same tile
// numbers for every strip (silhouette_pass_kernel's cuts); a segment that begins behind the strip's walk returns at once, so the
// workgroups that run are of one size, and the late strips' are launched first.  Segments write disjoint partials: nothing is merged.
// THE WORKSPACE: the grouping and (r1 / TJ + 1 + n_classes) n_classes partials of 32 bytes.  No known_rows: a new row changes every mean.
//
// kpop_class_tree: the agglomeration of the classes under such a table, host arithmetic alone (no GPU, no kpop_init).
#include <algorithm>
#include <vector>

#include "class_tiles.h"
#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr uint32_t kLinkMaxClasses = 4096u;  // the tables are n_classes^2 entries: 134 MB each at 4,096
constexpr uint32_t kLinkSegments = 16u;      // the cuts of a strip's walk
constexpr uint64_t kLinkNoKey = ~0ull;       // no pair whose distance is a number (distance_key gives it to nothing but a NaN)

// what a run of a strip leaves for a column class: the sum over its pairs, the least pair and the greatest key (0: none)
struct LinkPart {
  double sum;
  uint64_t min_k, max_k;
  uint32_t min_i, min_j;
};

struct LinkWork {
  ClassTiles g;
  LinkPart *part;
  uint32_t n_strips;
  uint64_t bytes;
};

static LinkWork class_linkage_carve(void *base, uint32_t r1, uint32_t n_classes) {
  Carver c(base);
  LinkWork f;
  f.g = class_tiles_carve(c, r1, n_classes);
  f.n_strips = div_up(std::max(r1, 1u), self_shape(r1).TJ);
  f.part = c.take<LinkPart>(((uint64_t)f.n_strips + n_classes) * n_classes * sizeof(LinkPart));
  f.bytes = c.off;
  return f;
}

// the least under (key, i, j), i < j the two rows
__device__ __forceinline__ bool link_pair_less(uint64_t ka, uint32_t ia, uint32_t ja, uint64_t kb, uint32_t ib, uint32_t jb) {
  return ka < kb || (ka == kb && (ia < ib || (ia == ib && ja < jb)));
}

// a: the set's rows as the chain reads them, both operands.  Strip gridDim.x - 1 - blockIdx.x (the longest walks first): positions
// q0 .. q0 + TJ of the grouped order perm, TJ = TY n_rg; a thread 4 columns x TY rows as in kmedoids_own_kernel.  Segment blockIdx.y of
// gridDim.y of the column tiles.  part: [(gridDim.x + n_classes) n_classes]
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void class_linkage_sweep_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                                     const double *__restrict__ metric, double p, uint32_t n_cg, uint32_t n_rg,
                                                                     const uint32_t *__restrict__ class_of, uint32_t n_classes, const uint32_t *__restrict__ perm,
                                                                     const SilTile *__restrict__ tiles, const uint32_t *__restrict__ first_tile,
                                                                     const uint32_t *__restrict__ start, uint32_t max_tiles, LinkPart *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kSilMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kSilMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_row[kSilMaxTJ], s_cls[kSilMaxTJ];  // the strip's rows and their classes
  __shared__ double s_sum[kSilMaxTJ];                      // a row's values over the column class that ends
  __shared__ uint64_t s_min_k[kSilMaxTJ], s_max_k[kSilMaxTJ];
  __shared__ uint32_t s_min_c[kSilMaxTJ];
  const uint32_t TJ = TY * n_rg;
  const uint32_t strip = gridDim.x - 1 - blockIdx.x;
  const uint32_t q0 = strip * TJ, n_in = min(start[n_classes], r1);
  if (q0 >= n_in) return;
  const uint32_t q1 = min(n_in, q0 + TJ);
  const uint32_t n_tiles = min(first_tile[n_classes], max_tiles);
  const uint32_t c_hi = min(class_of[min(perm[q1 - 1], r1 - 1)], n_classes - 1);
  const uint32_t walk_end = min(first_tile[c_hi + 1], n_tiles);
  // segment blockIdx.y: cut where a class starts -- the first tile of the class that holds tile seg n_tiles / n_seg, the same for every
  // strip -- and held to the strip's walk
  const uint32_t seg = blockIdx.y, n_seg = gridDim.y;
  const auto cut = [&](uint32_t s) -> uint32_t {
    if (s == 0 || n_tiles == 0) return 0u;
    if (s >= n_seg) return n_tiles;
    const uint32_t c = min(tiles[(uint32_t)((uint64_t)s * n_tiles / n_seg)].c & ~kSilLast, n_classes - 1);
    return min(first_tile[c], n_tiles);
  };
  const uint32_t t_begin = min(cut(seg), walk_end), t_end = max(min(cut(seg + 1), walk_end), t_begin);
  if (t_begin >= t_end) return;  // (the same for every thread of the workgroup)
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < kSilMaxTJ; n += 256) {
    const uint32_t row = (n < TJ && q0 + n < q1) ? min(perm[q0 + n], r1 - 1) : kSilNone;
    s_row[n] = row;
    s_cls[n] = row != kSilNone ? min(class_of[row], n_classes) : n_classes;
  }
  __syncthreads();  // (s_row is the strip's index list: the first load reads it)
  double run[TY];
  uint64_t min_k[TY], max_k[TY];
  uint32_t min_c[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    run[yy] = 0.0;
    min_k[yy] = kLinkNoKey;
    max_k[yy] = 0;
    min_c[yy] = kSilNone;
  }
  const auto sum = [](LaneSum x, LaneSum y) { return LaneSum{__dadd_rn(x.v, y.v)}; };
  const auto greatest = [](uint64_t x, uint64_t y) { return x > y ? x : y; };
  const PairRowsAt cols{a, r1, perm}, rows{a, r1, s_row};
  const uint32_t n_strip = q1 - q0;
  PairStage<kSilMaxW, kSilMaxTJ> stage;
  SilStep cur = silhouette_tile(tiles, t_begin, t_end, r1, w), nxt;
  for (pair_sweep_open(stage, cols, cur, rows, 0u, n_strip, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = silhouette_tile(tiles, cur.t + 1, t_end, r1, w);
    uint32_t ri[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) ri[x] = (cur.i0 + ti + x < cur.i1) ? perm[cur.i0 + ti + x] : kSilNone;
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, rows, 0u, n_strip, n_dims, metric, p, ti, tj, true);
    // the sum as silhouette_pass_kernel takes it: the columns ascending, the row itself and a column beyond the tile add +0.  A class's
    // columns ascend with the position, so `<` alone keeps, among equal keys, the smallest column
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t j = s_row[tj + yy];
      double s = run[yy];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const bool pair = ri[x] != kSilNone && ri[x] != j;
        s = __dadd_rn(s, pair ? d : 0.0);
        if (pair && d == d) {
          const uint64_t k = distance_key(d);
          if (k < min_k[yy]) {
            min_k[yy] = k;
            min_c[yy] = ri[x];
          }
          max_k[yy] = greatest(max_k[yy], k);
        }
      }
      run[yy] = s;
    }
    if (!(cur.c & kSilLast)) continue;  // (the same for every thread of the workgroup)
    const uint32_t cc = min(cur.c & ~kSilLast, n_classes - 1);
    __syncthreads();  // the fold of the class before has been read
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const double total = reduce_row_lanes(LaneSum{run[yy]}, n_cg, sum).v;
      const KeyAt least = reduce_row_lanes(KeyAt{min_k[yy], min_c[yy]}, n_cg, key_at_min);
      const uint64_t most = reduce_row_lanes(max_k[yy], n_cg, greatest);
      if (cg == 0) {
        s_sum[tj + yy] = total;
        s_min_k[tj + yy] = least.k;
        s_min_c[tj + yy] = least.c;
        s_max_k[tj + yy] = most;
      }
      run[yy] = 0.0;
      min_k[yy] = kLinkNoKey;
      max_k[yy] = 0;
      min_c[yy] = kSilNone;
    }
    __syncthreads();
    // the thread of a run's first row folds the run, its rows in ascending position; a run of a class below cc is dropped
    const uint32_t n = threadIdx.x;
    if (n < n_strip) {
      const uint32_t rc = s_cls[n];
      if (rc < n_classes && rc >= cc && (n == 0 || s_cls[n - 1] != rc)) {
        LinkPart f{0.0, kLinkNoKey, 0, kSilNone, kSilNone};
        for (uint32_t m = n; m < n_strip && s_cls[m] == rc; ++m) {
          f.sum = __dadd_rn(f.sum, s_sum[m]);
          const uint64_t k = s_min_k[m];
          if (k != kLinkNoKey) {
            const uint32_t r = s_row[m], c = s_min_c[m];
            const uint32_t i = min(r, c), j = max(r, c);
            if (link_pair_less(k, i, j, f.min_k, f.min_i, f.min_j)) {
              f.min_k = k;
              f.min_i = i;
              f.min_j = j;
            }
          }
          f.max_k = greatest(f.max_k, s_max_k[m]);
        }
        part[((uint64_t)strip + rc) * n_classes + cc] = f;
      }
    }
  }
}

// a thread a class pair a <= b: b's runs in ascending strip order, and the entry to both halves of the five tables (each may be null)
__global__ __launch_bounds__(256) void class_linkage_combine_kernel(uint32_t n_classes, uint32_t TJ, uint32_t n_strips, const uint32_t *__restrict__ cnt,
                                                                    const uint32_t *__restrict__ start, const LinkPart *__restrict__ part,
                                                                    uint32_t *__restrict__ class_rows, double *__restrict__ mean_dist, double *__restrict__ min_dist,
                                                                    double *__restrict__ max_dist, uint32_t *__restrict__ min_i, uint32_t *__restrict__ min_j) {
  const uint64_t total = (uint64_t)n_classes * n_classes;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    const uint32_t a = (uint32_t)(e / n_classes), b = (uint32_t)(e % n_classes);
    if (a > b) continue;
    const uint32_t na = cnt[a], nb = cnt[b];
    if (a == b && class_rows) class_rows[a] = na;
    LinkPart f{0.0, kLinkNoKey, 0, kSilNone, kSilNone};
    if (na && nb) {
      const uint32_t y0 = start[b] / TJ, y1 = min((start[b] + nb - 1) / TJ, n_strips - 1);
      for (uint32_t y = y0; y <= y1; ++y) {
        const LinkPart q = part[((uint64_t)y + b) * n_classes + a];
        f.sum = __dadd_rn(f.sum, q.sum);
        if (q.min_k != kLinkNoKey && link_pair_less(q.min_k, q.min_i, q.min_j, f.min_k, f.min_i, f.min_j)) {
          f.min_k = q.min_k;
          f.min_i = q.min_i;
          f.min_j = q.min_j;
        }
        f.max_k = q.max_k > f.max_k ? q.max_k : f.max_k;
      }
    }
    // on the diagonal every pair was added from both of its rows
    const uint64_t pairs = a == b ? (uint64_t)na * (na ? na - 1 : 0) : (uint64_t)na * nb;
    const double mean = pairs ? __ddiv_rn(f.sum, (double)pairs) : sil_nan();
    const bool any = f.min_k != kLinkNoKey;
    const double lo = any ? key_f64(f.min_k) : sil_nan(), hi = any ? key_f64(f.max_k) : sil_nan();
    const uint64_t ab = (uint64_t)a * n_classes + b, ba = (uint64_t)b * n_classes + a;
    if (mean_dist) mean_dist[ab] = mean_dist[ba] = mean;
    if (min_dist) min_dist[ab] = min_dist[ba] = lo;
    if (max_dist) max_dist[ab] = max_dist[ba] = hi;
    if (min_i) min_i[ab] = min_i[ba] = any ? f.min_i : kSilNone;
    if (min_j) min_j[ab] = min_j[ba] = any ? f.min_j : kSilNone;
  }
}

static int class_linkage_check(uint32_t n_classes, const char *who) {
  if (n_classes == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: no classes", who);
  if (n_classes > kLinkMaxClasses) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u classes (at most %u)", who, n_classes, kLinkMaxClasses);
  return 0;
}

// the body of both entry points: enqueues only
static int class_linkage_dev(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work, uint32_t *d_class_rows, double *d_mean, double *d_min,
                             double *d_max, uint32_t *d_min_i, uint32_t *d_min_j, hipStream_t st, const char *who) {
  KPOP_TRY(class_linkage_check(n_classes, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 && !d_class_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null class_of", who);
  const SelfShape s = self_shape(r1);
  LinkWork f = class_linkage_carve(d_work, r1, n_classes);
  if (r1) {
    const double *a = rs->rows;
    KPOP_TRY(refset_chain_rows(rs, st, &a));
    KPOP_TRY(class_tiles_group(f.g, d_class_of, r1, n_classes, nullptr, st));
    const uint32_t *perm = f.g.perm;
    const dim3 grid(f.n_strips, kLinkSegments);
    KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
      by_shape_rows(s, [&](auto TY) {
        class_linkage_sweep_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, s.n_cg, s.n_rg, d_class_of,
                                                                                                       n_classes, perm, f.g.tiles, f.g.first_tile, f.g.start, f.g.max_tiles,
                                                                                                       f.part);
      });
      KPOP_LAUNCH_CHECK();
      return 0;
    }));
  } else {
    KPOP_HIP(hipMemsetAsync(f.g.cnt, 0, ((uint64_t)n_classes + 1) * 4, st));
    KPOP_HIP(hipMemsetAsync(f.g.start, 0, ((uint64_t)n_classes + 1) * 4, st));
  }
  const dim3 pairs_grid((uint32_t)std::min<uint64_t>(((uint64_t)n_classes * n_classes + 255) / 256, 65536u));
  class_linkage_combine_kernel<<<pairs_grid, dim3(256), 0, st>>>(n_classes, s.TJ, f.n_strips, f.g.cnt, f.g.start, f.part, d_class_rows, d_mean, d_min, d_max, d_min_i,
                                                                 d_min_j);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_class_linkage_workspace_bytes(const kpop_refset *rs, uint32_t n_classes) {
  if (!rs || n_classes == 0 || n_classes > kLinkMaxClasses) return 0;
  return class_linkage_carve(nullptr, rs->r1, n_classes).bytes;
}

extern "C" int kpop_dev_class_linkage(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work, uint32_t *d_class_rows, double *d_mean_dist,
                                      double *d_min_dist, double *d_max_dist, uint32_t *d_min_i, uint32_t *d_min_j, void *stream) {
  const char *who = "kpop_dev_class_linkage";
  KPOP_TRY(refset_check_handle(rs, who));
  return class_linkage_dev(rs, d_class_of, n_classes, d_work, d_class_rows, d_mean_dist, d_min_dist, d_max_dist, d_min_i, d_min_j, as_stream(stream), who);
}

extern "C" int kpop_class_linkage(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, uint32_t *class_rows, double *mean_dist, double *min_dist,
                                  double *max_dist, uint32_t *min_i, uint32_t *min_j) {
  const char *who = "kpop_class_linkage";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(class_linkage_check(n_classes, who));
  const uint32_t r1 = rs->r1;
  if (r1 && !class_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null class_of", who);
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, true, who));
  const uint64_t nn = (uint64_t)n_classes * n_classes;
  HostCall h;
  void *work = h.work(class_linkage_carve(nullptr, r1, n_classes).bytes);
  const uint32_t *dc = h.in(class_of, r1);
  uint32_t *d_rows = h.out(class_rows, n_classes);
  double *d_mean = h.out(mean_dist, nn), *d_min = h.out(min_dist, nn), *d_max = h.out(max_dist, nn);
  uint32_t *d_i = h.out(min_i, nn), *d_j = h.out(min_j, nn);
  KPOP_TRY(h.upload());
  KPOP_TRY(class_linkage_dev(rs, dc, n_classes, work, d_rows, d_mean, d_min, d_max, d_i, d_j, h.st, who));
  return h.finish();
}

extern "C" int kpop_distance_class_linkage(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                           const uint32_t *class_of, uint32_t n_classes, uint32_t *class_rows, double *mean_dist, double *min_dist, double *max_dist,
                                           uint32_t *min_i, uint32_t *min_j) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_class_linkage(rs, class_of, n_classes, class_rows, mean_dist, min_dist, max_dist, min_i, min_j);
  });
}

// host arithmetic alone: no GPU, no kpop_init.  The leaves are compacted into slots; a merged node takes its left child's slot.  Every
// live slot keeps its least partner under (key, lower id, higher id), so a merge costs a pass over the live slots and a rescan only of
// those whose partner died
namespace {

struct TreeKey {  // a distance that is a number, as it orders: -0 as +0
  static bool is(double d) { return d == d; }
  static double of(double d) { return d == 0.0 ? 0.0 : d; }
};

// (d, lo, hi) below (e, lo2, hi2); both distances numbers
inline bool tree_less(double d, uint32_t lo, uint32_t hi, double e, uint32_t lo2, uint32_t hi2) {
  return d < e || (d == e && (lo < lo2 || (lo == lo2 && hi < hi2)));
}

}  // namespace

extern "C" int kpop_class_tree(uint32_t n_classes, const uint32_t *class_rows, const double *dist, int linkage, uint32_t *n_merges, uint32_t *left,
                               uint32_t *right, double *height, uint32_t *size) {
  const char *who = "kpop_class_tree";
  KPOP_TRY(class_linkage_check(n_classes, who));
  if (linkage != KPOP_LINK_SINGLE && linkage != KPOP_LINK_COMPLETE && linkage != KPOP_LINK_AVERAGE)
    KPOP_FAIL(KPOP_ERR_INVALID, "%s: linkage %d (KPOP_LINK_SINGLE, KPOP_LINK_COMPLETE or KPOP_LINK_AVERAGE)", who, linkage);
  if (!class_rows || !dist || !n_merges || (n_classes > 1 && (!left || !right || !height || !size))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  std::vector<uint32_t> id, rows;
  for (uint32_t c = 0; c < n_classes; ++c)
    if (class_rows[c]) {
      id.push_back(c);
      rows.push_back(class_rows[c]);
    }
  const uint32_t m = (uint32_t)id.size();
  std::vector<double> d((size_t)m * m, 0.0);
  for (uint32_t s = 0; s < m; ++s)
    for (uint32_t t = s + 1; t < m; ++t) d[(size_t)s * m + t] = d[(size_t)t * m + s] = dist[(size_t)id[s] * n_classes + id[t]];
  std::vector<uint8_t> live(m, 1);
  std::vector<uint32_t> nn(m, kNone);
  // slot s's least partner among the live slots, kNone where no distance is a number
  const auto rescan = [&](uint32_t s) {
    uint32_t best = kNone;
    for (uint32_t t = 0; t < m; ++t) {
      if (t == s || !live[t]) continue;
      const double e = d[(size_t)s * m + t];
      if (!TreeKey::is(e)) continue;
      if (best == kNone || tree_less(TreeKey::of(e), std::min(id[s], id[t]), std::max(id[s], id[t]), TreeKey::of(d[(size_t)s * m + best]), std::min(id[s], id[best]),
                                     std::max(id[s], id[best])))
        best = t;
    }
    nn[s] = best;
  };
  for (uint32_t s = 0; s < m; ++s) rescan(s);
  uint32_t t_merge = 0;
  for (; t_merge + 1 < m; ++t_merge) {
    uint32_t x = kNone;
    for (uint32_t s = 0; s < m; ++s) {
      if (!live[s] || nn[s] == kNone) continue;
      if (x == kNone || tree_less(TreeKey::of(d[(size_t)s * m + nn[s]]), std::min(id[s], id[nn[s]]), std::max(id[s], id[nn[s]]), TreeKey::of(d[(size_t)x * m + nn[x]]),
                                  std::min(id[x], id[nn[x]]), std::max(id[x], id[nn[x]])))
        x = s;
    }
    if (x == kNone) break;  // no two live nodes have a number between them: a forest
    uint32_t y = nn[x];
    if (id[y] < id[x]) std::swap(x, y);
    const double h = TreeKey::of(d[(size_t)x * m + y]);
    const double nx = (double)rows[x], ny = (double)rows[y];
    left[t_merge] = id[x];
    right[t_merge] = id[y];
    height[t_merge] = h;
    size[t_merge] = rows[x] + rows[y];
    live[y] = 0;
    for (uint32_t z = 0; z < m; ++z) {
      if (!live[z] || z == x) continue;
      const double dx = d[(size_t)x * m + z], dy = d[(size_t)y * m + z];
      double v;
      if (dx != dx || dy != dy) v = __builtin_nan("");
      else if (linkage == KPOP_LINK_SINGLE) v = dx < dy ? dx : dy;
      else if (linkage == KPOP_LINK_COMPLETE) v = dx > dy ? dx : dy;
      else v = (nx * dx + ny * dy) / (nx + ny);
      d[(size_t)x * m + z] = d[(size_t)z * m + x] = v;
    }
    rows[x] += rows[y];
    id[x] = n_classes + t_merge;
    rescan(x);
    for (uint32_t z = 0; z < m; ++z) {
      if (!live[z] || z == x) continue;
      if (nn[z] == x || nn[z] == y) {
        rescan(z);
        continue;
      }
      const double e = d[(size_t)z * m + x];
      if (!TreeKey::is(e)) continue;
      if (nn[z] == kNone || tree_less(TreeKey::of(e), std::min(id[z], id[x]), std::max(id[z], id[x]), TreeKey::of(d[(size_t)z * m + nn[z]]), std::min(id[z], id[nn[z]]),
                                      std::max(id[z], id[nn[z]])))
        nn[z] = x;
    }
  }
  *n_merges = t_merge;
  return KPOP_OK;
}
