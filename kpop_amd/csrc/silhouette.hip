// silhouette.hip -- the silhouette and the medoids of a labelled resident set, in one pass over the pair tiles.
//
//   The set's r1 rows, class_of[r1] (a class in [0, n_classes) or KPOP_NO_CLASS: the row is LEFT OUT -- in no sum, nothing computed
//   for it), d(j, i) the reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250): the bits
//   kpop_refset_distance_rowwise writes on the vector pipe when the set's own rows are the query -- no kpop_tune setting is read; the
//   pair i == j is never examined.  S(j, c) = the sum of d(j, i) over the rows i != j of class c, n_c the rows of class c.  For a row j
//   of class c:  own_mean = S(j, c) / (n_c - 1), +0 when n_c == 1;  other_mean, other_class = the least S(j, c') / n_c' over the
//   classes c' != c that have rows, and that class (ties to the smaller class, a NaN mean never the least, none: NaN and KPOP_NO_CLASS);
//   silhouette = (other_mean - own_mean) / max(own_mean, other_mean), a zero as +0, +0 when n_c == 1.  For a class: its rows, its
//   medoid -- the member least under (own_mean with -0 as +0, row index) among those whose own_mean is a number -- and that mean.
//
// Neither the r1 x r1 matrix nor an r1 x n_classes table is formed, nothing is read back, nothing synchronises:
//   class_tiles_group         (class_tiles.h, shared with kmedoids.hip) the rows grouped by class:
//     silhouette_keys_kernel    a row's sort key (its class; a row left out: n_classes, behind every class) and the class sizes
//     exclusive_scan (scan.h), twice: where a class starts in the grouped order, and its first column tile -- a class's rows are cut
//                               into column tiles of at most w positions, so every column tile holds ONE class; at most r1 / w + n_classes
//     radix_sort_pairs_u64      (radix_sort.h, 16-bit keys) the row indices grouped by class, stable: ascending inside a class
//     silhouette_tiles_kernel   the column tiles: positions, class, whether the class ends there
//   silhouette_pass_kernel    a workgroup owns a row tile j0 .. j1 in natural order and walks the column tiles in order, the columns
//                             gathered through the grouped order (PairRowsAt, the sweep of pair_tile.h), both tile shapes of self_shape.  After a
//                             tile a thread adds its four columns' distances onto its running sum of the row (the row itself and the
//                             tile's edge add +0); where a class ends the row's n_cg lanes reduce (reduce_row_lanes: a fixed tree), one
//                             division, and the mean is the row's own or folds into (other_mean, other_class).  A row tile's column
//                             tiles are cut into up to 16 segments of WHOLE classes, a workgroup each, so that a short set fills the
//                             device; a segment keeps one (own, least, its class) a row, merged in segment order: exact
//   silhouette_rows_kernel    the silhouette, the left-out rows' NaNs, and per class a 64-bit atomicMin of the key of own_mean
//   silhouette_medoid_kernel  among the rows that hold their class's key, a 32-bit atomicMin of the index (dbscan.hip's two minima)
//   silhouette_classes_kernel class_rows, medoid, medoid_mean
// THE SUMS: a class's sum for a row is taken in an order that depends on r1 (the tile shape) and on the class's members in ascending row
// order alone -- position k of the class goes to lane (k % w) / 4, a lane adds its positions ascending, the lanes meet in a fixed tree.
// No floating-point atomic, nothing that depends on timing: the same bits on every run, and the same bits when the classes are
// renumbered (what moves is where a class's tiles lie in the walk, not what any of them adds).
// THE COST is the full rectangle, r1^2 pairs, twice the triangle of clusters.hip: d(j, i) is computed for (j, i) and again for (i, j).
// Column-side sums would need a partial table per tile to stay deterministic; the symmetric form is not attempted.  No known_rows: a new
// row changes every mean.
#include <algorithm>

#include "class_tiles.h"
#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

// g: the grouping (class_tiles.h); own [r1], other, ocls [n_seg][r1]: what the pass leaves for a row and a segment; med_k, med_i
// [n_classes]: the medoid's two minima, filled with ones by one memset
struct SilWork {
  ClassTiles g;
  uint32_t *ocls, *med_i;
  uint64_t *med_k;
  double *own, *other;
  uint64_t fill_bytes, bytes;
  uint32_t n_seg;
};

// the column segments of a row tile: enough workgroups for a short set (2,048 and more where the set has the rows), a function of r1
static uint32_t silhouette_segments(uint32_t r1) {
  const uint32_t n_rt = div_up(std::max(r1, 1u), self_shape(r1).TJ);
  return std::min(16u, std::max(1u, div_up(2048, n_rt)));
}

static SilWork silhouette_carve(void *base, uint32_t r1, uint32_t n_classes) {
  const uint64_t n = std::max(r1, 1u), nc = (uint64_t)n_classes + 1;
  Carver c(base);
  SilWork f;
  f.g = class_tiles_carve(c, r1, n_classes);
  f.n_seg = silhouette_segments(r1);
  f.own = c.take<double>(n * 8);
  f.other = c.take<double>(n * f.n_seg * 8);
  f.ocls = c.take<uint32_t>(n * f.n_seg * 4);
  const uint64_t before = c.off;
  f.med_k = c.take<uint64_t>(nc * 8);
  f.med_i = c.take<uint32_t>(nc * 4);
  f.fill_bytes = c.off - before;
  f.bytes = c.off;
  return f;
}

// a: the set's rows as the chain reads them (divided by their norms when the set normalises), both operands.  Row tile blockIdx.x:
// rows j0 .. j0 + TJ, TJ = TY n_rg; a thread 4 columns x TY rows, n_cg n_rg = 256 in both shapes: every thread holds pairs.  The
// sweep of pair_tile.h over the column tiles of segment blockIdx.y; perm: the grouped order.  own_out[r1]: written by the
// segment that holds the row's class; other_out, ocls_out [gridDim.y][r1]: a segment's least mean to another class, merged in
// segment order by silhouette_rows_kernel
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void silhouette_pass_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                                 const double *__restrict__ metric, double p, uint32_t n_cg, uint32_t n_rg,
                                                                 const uint32_t *__restrict__ class_of, uint32_t n_classes, const uint32_t *__restrict__ perm,
                                                                 const SilTile *__restrict__ tiles, const uint32_t *__restrict__ first_tile, uint32_t max_tiles,
                                                                 double *__restrict__ own_out, double *__restrict__ other_out, uint32_t *__restrict__ ocls_out) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kSilMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kSilMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_cls[kSilMaxTJ];  // the classes of the tile's rows (the loop's barriers come before anybody reads)
  const uint32_t TJ = TY * n_rg;
  const uint32_t j0 = blockIdx.x * TJ;
  if (j0 >= r1) return;
  const uint32_t j1 = min(r1, j0 + TJ);
  const uint32_t n_tiles = min(first_tile[n_classes], max_tiles);
  // segment blockIdx.y of gridDim.y: its share of the column tiles, cut where a class starts -- the first tile of the class that holds
  // tile seg n_tiles / n_seg -- so that every class lies in one segment, whole: no sum is split, and the bits do not depend on the cuts
  const uint32_t seg = blockIdx.y, n_seg = gridDim.y;
  const auto cut = [&](uint32_t s) -> uint32_t {
    if (s == 0 || n_tiles == 0) return 0u;
    if (s >= n_seg) return n_tiles;
    const uint32_t c = min(tiles[(uint32_t)((uint64_t)s * n_tiles / n_seg)].c & ~kSilLast, n_classes - 1);
    return min(first_tile[c], n_tiles);
  };
  const uint32_t t_begin = cut(seg), t_end = max(cut(seg + 1), t_begin);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < TJ; n += 256) s_cls[n] = j0 + n < j1 ? min(class_of[j0 + n], n_classes) : n_classes;
  double run[TY], own[TY], best[TY];
  uint32_t best_c[TY], own_seen = 0;  // bit yy: the row's own class lies in this segment
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    run[yy] = own[yy] = 0.0;
    best[yy] = sil_nan();
    best_c[yy] = kSilNone;
  }
  const auto sum = [](LaneSum x, LaneSum y) { return LaneSum{__dadd_rn(x.v, y.v)}; };
  const PairRowsAt cols{a, r1, perm};
  const PairRows rows{a, r1};
  PairStage<kSilMaxW, kSilMaxTJ> stage;
  SilStep cur = silhouette_tile(tiles, t_begin, t_end, r1, w), nxt;
  for (pair_sweep_open(stage, cols, cur, rows, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = silhouette_tile(tiles, cur.t + 1, t_end, r1, w);
    uint32_t ri[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) ri[x] = (cur.i0 + ti + x < cur.i1) ? perm[cur.i0 + ti + x] : kSilNone;
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, rows, j0, j1, n_dims, metric, p, ti, tj, true);
    // the tile's distances onto the row's running sum, the columns ascending; the row itself and a column beyond the tile add +0
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t j = j0 + tj + yy;
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
      } else {
        // the classes come ascending: `<` alone keeps, among equal means, the smaller class; a NaN is less than nothing
        const double mean = total / (double)cur.n;
        if (mean == mean && (best_c[yy] == kSilNone || mean < best[yy])) {
          best[yy] = mean;
          best_c[yy] = c;
        }
      }
    }
  }
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t j = j0 + tj + yy;
    if (cg == 0 && j < j1) {
      if (own_seen & (1u << yy)) own_out[j] = own[yy];  // (the one segment that holds the row's class)
      other_out[(uint64_t)seg * r1 + j] = best[yy];
      ocls_out[(uint64_t)seg * r1 + j] = best_c[yy];
    }
  }
}

// a row's outputs (each may be null), and the least key of own_mean of its class
__global__ __launch_bounds__(256) void silhouette_rows_kernel(const uint32_t *__restrict__ class_of, uint32_t r1, uint32_t n_classes, const uint32_t *__restrict__ cnt,
                                                              const double *__restrict__ own, const double *__restrict__ other, const uint32_t *__restrict__ ocls,
                                                              uint32_t n_seg, double *__restrict__ own_mean, double *__restrict__ other_mean, uint32_t *__restrict__ other_class,
                                                              double *__restrict__ silhouette, uint64_t *__restrict__ med_k) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = class_of[i];
    double o = sil_nan(), b = sil_nan(), s = sil_nan();
    uint32_t bc = kSilNone;
    if (c < n_classes) {
      o = own[i];
      // the segments hold ascending classes: `<` alone keeps, among equal means, the smaller class; a segment's NaN is never its least
      for (uint32_t sg = 0; sg < n_seg; ++sg) {
        const uint32_t c2 = ocls[(uint64_t)sg * r1 + i];
        if (c2 == kSilNone) continue;
        const double m = other[(uint64_t)sg * r1 + i];
        if (bc == kSilNone || m < b) {
          b = m;
          bc = c2;
        }
      }
      if (cnt[c] == 1) {
        s = 0.0;  // Rousseeuw's convention
      } else {
        s = __ddiv_rn(__dsub_rn(b, o), o > b ? o : b);
        if (s == 0.0) s = 0.0;
      }
      if (o == o) atomicMin(reinterpret_cast<unsigned long long *>(med_k + c), (unsigned long long)distance_key(o));
    }
    if (own_mean) own_mean[i] = o;
    if (other_mean) other_mean[i] = b;
    if (other_class) other_class[i] = bc;
    if (silhouette) silhouette[i] = s;
  }
}

// key, then index: the least under (own_mean, row index) with two integer minima
__global__ __launch_bounds__(256) void silhouette_medoid_kernel(const uint32_t *__restrict__ class_of, uint32_t r1, uint32_t n_classes, const double *__restrict__ own,
                                                                const uint64_t *__restrict__ med_k, uint32_t *__restrict__ med_i) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t c = class_of[i];
    if (c >= n_classes) continue;
    const double o = own[i];
    if (o == o && distance_key(o) == med_k[c]) atomicMin(med_i + c, (uint32_t)i);
  }
}

__global__ __launch_bounds__(256) void silhouette_classes_kernel(uint32_t n_classes, uint32_t r1, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ med_i,
                                                                 const double *__restrict__ own, uint32_t *__restrict__ class_rows, uint32_t *__restrict__ medoid,
                                                                 double *__restrict__ medoid_mean) {
  for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < n_classes; c += gridDim.x * 256) {
    const uint32_t m = med_i[c];
    if (class_rows) class_rows[c] = cnt[c];
    if (medoid) medoid[c] = m < r1 ? m : kSilNone;
    if (medoid_mean) medoid_mean[c] = m < r1 ? own[m] : sil_nan();
  }
}

static int silhouette_check(uint32_t n_classes, const char *who) {
  if (n_classes == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: no classes", who);
  if (n_classes > kSilMaxClasses) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u classes (at most %u)", who, n_classes, kSilMaxClasses);
  return 0;
}

// the body of both entry points: enqueues only
static int silhouette_dev(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work, double *d_own_mean, double *d_other_mean,
                          uint32_t *d_other_class, double *d_silhouette, uint32_t *d_class_rows, uint32_t *d_medoid, double *d_medoid_mean, hipStream_t st,
                          const char *who) {
  KPOP_TRY(silhouette_check(n_classes, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 && !d_class_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null class_of", who);
  const SelfShape s = self_shape(r1);
  SilWork f = silhouette_carve(d_work, r1, n_classes);
  if (!r1) KPOP_HIP(hipMemsetAsync(f.g.cnt, 0, ((uint64_t)n_classes + 1) * 4, st));
  KPOP_HIP(hipMemsetAsync(f.med_k, 0xFF, f.fill_bytes, st));
  const dim3 classes_grid(div_up(n_classes, 256));
  if (r1) {
    const double *a = rs->rows;
    KPOP_TRY(refset_chain_rows(rs, st, &a));
    const dim3 rows_grid(std::min(div_up(r1, 256), 4096u));
    KPOP_TRY(class_tiles_group(f.g, d_class_of, r1, n_classes, nullptr, st));
    const uint32_t *perm = f.g.perm;
    const dim3 grid(div_up(r1, s.TJ), f.n_seg);
    KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
      by_shape_rows(s, [&](auto TY) {
        silhouette_pass_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, s.n_cg, s.n_rg, d_class_of, n_classes,
                                                                                                   perm, f.g.tiles, f.g.first_tile, f.g.max_tiles, f.own, f.other, f.ocls);
      });
      KPOP_LAUNCH_CHECK();
      return 0;
    }));
    silhouette_rows_kernel<<<rows_grid, dim3(256), 0, st>>>(d_class_of, r1, n_classes, f.g.cnt, f.own, f.other, f.ocls, f.n_seg, d_own_mean, d_other_mean, d_other_class, d_silhouette,
                                                            f.med_k);
    KPOP_LAUNCH_CHECK();
    silhouette_medoid_kernel<<<rows_grid, dim3(256), 0, st>>>(d_class_of, r1, n_classes, f.own, f.med_k, f.med_i);
    KPOP_LAUNCH_CHECK();
  }
  silhouette_classes_kernel<<<classes_grid, dim3(256), 0, st>>>(n_classes, r1, f.g.cnt, f.med_i, f.own, d_class_rows, d_medoid, d_medoid_mean);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_silhouette_workspace_bytes(const kpop_refset *rs, uint32_t n_classes) {
  if (!rs || n_classes == 0 || n_classes > kSilMaxClasses) return 0;
  return silhouette_carve(nullptr, rs->r1, n_classes).bytes;
}

extern "C" int kpop_dev_silhouette(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, void *d_work, double *d_own_mean, double *d_other_mean,
                                   uint32_t *d_other_class, double *d_silhouette, uint32_t *d_class_rows, uint32_t *d_medoid, double *d_medoid_mean, void *stream) {
  const char *who = "kpop_dev_silhouette";
  KPOP_TRY(refset_check_handle(rs, who));
  return silhouette_dev(rs, d_class_of, n_classes, d_work, d_own_mean, d_other_mean, d_other_class, d_silhouette, d_class_rows, d_medoid, d_medoid_mean,
                        as_stream(stream), who);
}

extern "C" int kpop_silhouette(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, double *own_mean, double *other_mean, uint32_t *other_class,
                               double *silhouette, uint32_t *class_rows, uint32_t *medoid, double *medoid_mean) {
  const char *who = "kpop_silhouette";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(silhouette_check(n_classes, who));
  const uint32_t r1 = rs->r1;
  if (r1 && !class_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null class_of", who);
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, true, who));
  HostCall h;
  void *work = h.work(silhouette_carve(nullptr, r1, n_classes).bytes);
  const uint32_t *dc = h.in(class_of, r1);
  double *d_own = h.out(own_mean, r1), *d_other = h.out(other_mean, r1);
  uint32_t *d_ocls = h.out(other_class, r1);
  double *d_sil = h.out(silhouette, r1);
  uint32_t *d_rows = h.out(class_rows, n_classes), *d_med = h.out(medoid, n_classes);
  double *d_mm = h.out(medoid_mean, n_classes);
  KPOP_TRY(h.upload());
  KPOP_TRY(silhouette_dev(rs, dc, n_classes, work, d_own, d_other, d_ocls, d_sil, d_rows, d_med, d_mm, h.st, who));
  return h.finish();
}

extern "C" int kpop_distance_silhouette(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                        const uint32_t *class_of, uint32_t n_classes, double *own_mean, double *other_mean, uint32_t *other_class,
                                        double *silhouette, uint32_t *class_rows, uint32_t *medoid, double *medoid_mean) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_silhouette(rs, class_of, n_classes, own_mean, other_mean, other_class, silhouette, class_rows, medoid, medoid_mean);
  });
}

// host arithmetic alone: no GPU, no kpop_init.  Both means are summed in ascending row order
extern "C" int kpop_silhouette_summary(uint32_t r1, const uint32_t *class_of, uint32_t n_classes, const double *silhouette, double *class_mean,
                                       double *overall_mean) {
  const char *who = "kpop_silhouette_summary";
  KPOP_TRY(silhouette_check(n_classes, who));
  if (!class_mean || !overall_mean || (r1 && (!class_of || !silhouette))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, true, who));
  std::vector<uint64_t> rows(n_classes, 0);
  for (uint32_t c = 0; c < n_classes; ++c) class_mean[c] = 0.0;
  double all = 0.0;
  uint64_t n_all = 0;
  for (uint32_t i = 0; i < r1; ++i) {
    const uint32_t c = class_of[i];
    if (c == KPOP_NO_CLASS) continue;
    class_mean[c] += silhouette[i];
    all += silhouette[i];
    ++rows[c];
    ++n_all;
  }
  const double nan = __builtin_nan("");
  for (uint32_t c = 0; c < n_classes; ++c) class_mean[c] = rows[c] ? class_mean[c] / (double)rows[c] : nan;
  *overall_mean = n_all ? all / (double)n_all : nan;
  return KPOP_OK;
}
