// reachability.hip -- the mutual-reachability forest of a resident set: DBSCAN at every radius.
//
//   The graph and the distance of clusters.hip, forest.hip and dbscan.hip: the set's r1 rows, d(j, i) the reference chain's distance
//   (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250), symmetric bit for bit, the pair i == j never examined; no
//   kpop_tune setting is read.
//   core_dist[i], for min_pts in 1 .. 129: +0 for min_pts = 1; otherwise the (min_pts - 1)-th least of { d(i, j) : j != i, d a number }
//   (+inf is one; -0 taken as +0), and the quiet NaN when there are fewer.  core_dist[i] <= eps iff row i is a core row of
//   kpop_dbscan(eps, min_pts).
//   mr(i, j) = max(d(i, j), core_dist[i], core_dist[j]); i < j is an edge iff all three are numbers and mr <= max_distance.  The
//   result is THE minimum spanning forest under the strict order (mr, i, j): unique, the same bits on every run.  Cut at any
//   T <= max_distance, the core rows (core_dist <= T) get kpop_dbscan(T, min_pts)'s labels and every other row is alone: DBSCAN*,
//   border rows not attached (kpop_reachability_cut).
//
// The launches (the device form reads nothing back and allocates nothing):
//   knn_nearest_kernel   the first two passes of the leave-self-out k-NN at k = min_pts - 1 (knn.hip, launched from there:
//   knn_merge_kernel     knn_run_leave_self_out_lists): every row's k nearest OTHER rows under (key, index), of which only the last
//                        key is wanted.  The tie pass settles which tied rows are members, never the k-th key's value, and is not
//                        run; no class array exists.  The set is walked in SLABS of kRcSlabRows query rows, so that the lists take
//                        what a slab needs and not r1 x k entries
//   reach_core_kernel    core_dist = (the merged list is full) ? the distance of its last key : NaN
//   reach_fill_kernel    the two cases that need no list: min_pts = 1 (+0) and min_pts > r1 (NaN: nobody has that many others)
//   forest.hip's rounds  under ForestReachWeight (forest_rounds.h): forest_nearest_kernel loads its rows' core distances once a
//                        launch and the four columns' once a tile, refuses a pair with a NaN among the three values and takes
//                        distance_key(max(d, core_i, core_j)); every other kernel of a round, the two sorts and the writer are the
//                        single-linkage tree's, one body each
#include <algorithm>
#include <vector>

#include "common.h"
#include "forest_rounds.h"
#include "knn_lists.h"
#include "refset.h"
#include "refset_call.h"
#include "space_ops.h"

namespace kpop {

constexpr uint32_t kRcSlabRows = 16384;  // query rows a slab: at k = 128 one strip of 16 rows a workgroup, 1,024 workgroups, 49 MiB of lists
constexpr uint32_t kRcMaxMinPts = kKMaxK + 1;

// rows first .. first + n_rows of core_dist from their merged lists
__global__ __launch_bounds__(256) void reach_core_kernel(const uint32_t *__restrict__ m_n, const uint64_t *__restrict__ m_tau, uint32_t k, uint32_t n_rows,
                                                         double *__restrict__ core) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * 256)
    core[i] = m_n[i] == k ? key_f64(m_tau[i]) : __longlong_as_double(0x7FF8000000000000ll);  // (a key gives back +0 for a zero)
}

__global__ __launch_bounds__(256) void reach_fill_kernel(double *__restrict__ core, uint32_t r1, double value) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) core[i] = value;
}

static int reach_check_min_pts(uint32_t min_pts, const char *who) {
  if (min_pts == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: min_pts is zero (a row counts itself: 1 makes every core distance zero)", who);
  if (min_pts > kRcMaxMinPts) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: min_pts = %u (at most %u: the lists hold %d neighbours)", who, min_pts, kRcMaxMinPts, kKMaxK);
  return 0;
}

// The slab rule: slabs of kRcSlabRows rows, the last one what is left.  A slab's bytes are knn_carve's without a query side, a class
// or a tie table: a row takes (12 k + 8) bytes a segment of its strip (the segments' lists), 12 k for the merged list and 16 more; a
// slab of 16,384 rows is cut into 1 segment (k > 32) or 2 (k <= 32), a shorter last slab into more -- hence the larger of the two.
// (Declared in knn_lists.h, with core_dev: lof.hip's k-distances)
uint64_t core_workspace_bytes(uint32_t r1, uint32_t min_pts, uint32_t n_dims) {
  const uint32_t k = min_pts - 1;
  if (k == 0 || k >= r1) return 256;
  const uint32_t slab = std::min(r1, kRcSlabRows), last = r1 % slab ? r1 % slab : slab;
  return std::max(knn_carve(nullptr, slab, k, 0, n_dims, false).bytes, knn_carve(nullptr, last, k, 0, n_dims, false).bytes);
}

// the body of the core distances' entry points: enqueues only.  min_pts is checked, r1 > 0
int core_dev(kpop_refset *rs, uint32_t min_pts, void *d_work, double *d_core, hipStream_t st) {
  const uint32_t r1 = rs->r1, D = rs->n_dims, k = min_pts - 1;
  const dim3 rows_grid(std::min(div_up(r1, 256), 4096u));
  if (k == 0 || k >= r1) {
    reach_fill_kernel<<<rows_grid, dim3(256), 0, st>>>(d_core, r1, k == 0 ? 0.0 : __builtin_nan(""));
    KPOP_LAUNCH_CHECK();
    return KPOP_OK;
  }
  const double *a;  // both operands
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  const uint32_t slab = std::min(r1, kRcSlabRows);
  for (uint32_t j0 = 0; j0 < r1; j0 += slab) {
    const uint32_t nr = std::min(slab, r1 - j0);
    const KnnWork w = knn_carve(d_work, nr, k, 0, D, false);
    uint32_t n_seg = 0;
    KPOP_TRY(knn_run_leave_self_out_lists(rs->kind, a, r1, j0, nr, D, rs->metric, rs->p, k, w, &n_seg, st));
    reach_core_kernel<<<dim3(std::min(div_up(nr, 256), 4096u)), dim3(256), 0, st>>>(w.m_n, w.m_tau, k, nr, d_core + j0);
    KPOP_LAUNCH_CHECK();
  }
  return KPOP_OK;
}

// the forest's workspace: the core distances (when the caller keeps none), then the lists' bytes and the rounds' bytes in one place --
// the rounds begin when the lists are done with it, on the one stream
struct ReachWork {
  double *core;
  void *rest;
  uint64_t bytes;
};
static ReachWork reach_carve(void *base, uint32_t r1, uint32_t min_pts, uint32_t n_dims) {
  Carver c(base);
  ReachWork f;
  f.core = c.take<double>((uint64_t)std::max(r1, 1u) * 8);
  f.rest = c.take<void>(std::max(core_workspace_bytes(r1, min_pts, n_dims), forest_workspace_bytes(r1)));
  f.bytes = c.off;
  return f;
}

// the body of the forest's entry points.  host_reads: forest_dev's
static int reach_dev(kpop_refset *rs, uint32_t min_pts, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i, uint32_t *d_edge_j,
                     double *d_edge_dist, double *d_core_dist, uint32_t *d_labels, hipStream_t st, bool host_reads, const char *who) {
  KPOP_TRY(reach_check_min_pts(min_pts, who));
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!d_n_edges) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  const uint32_t r1 = rs->r1;
  if (r1 > 1 && (!d_edge_i || !d_edge_j || !d_edge_dist)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null edge arrays", who);
  if (r1 > 0) {
    const ReachWork f = reach_carve(d_work, r1, min_pts, rs->n_dims);
    double *core = d_core_dist ? d_core_dist : f.core;
    KPOP_TRY(core_dev(rs, min_pts, f.rest, core, st));
    return forest_dev(rs, core, max_distance, f.rest, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_labels, st, host_reads, who);
  }
  return forest_dev(rs, nullptr, max_distance, d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_labels, st, host_reads, who);  // (no rows: the count alone)
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_core_distances_workspace_bytes(const kpop_refset *rs, uint32_t min_pts) {
  if (!rs || min_pts == 0 || min_pts > kRcMaxMinPts) return 0;
  return core_workspace_bytes(rs->r1, min_pts, rs->n_dims);
}

extern "C" int kpop_dev_core_distances(kpop_refset *rs, uint32_t min_pts, void *d_work, double *d_core_dist, void *stream) {
  const char *who = "kpop_dev_core_distances";
  KPOP_TRY(refset_check_handle(rs, who));
  KPOP_TRY(reach_check_min_pts(min_pts, who));
  if (rs->r1 == 0) return KPOP_OK;
  if (!d_work || !d_core_dist) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  return core_dev(rs, min_pts, d_work, d_core_dist, as_stream(stream));
}

extern "C" int kpop_core_distances(kpop_refset *rs, uint32_t min_pts, double *core_dist) {
  const char *who = "kpop_core_distances";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(reach_check_min_pts(min_pts, who));
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  if (!core_dist) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  HostCall h;
  void *work = h.work(core_workspace_bytes(r1, min_pts, rs->n_dims));
  double *dc = h.out(core_dist, r1);
  KPOP_TRY(h.upload());
  KPOP_TRY(core_dev(rs, min_pts, work, dc, h.st));
  return h.finish();
}

extern "C" uint64_t kpop_dev_reachability_tree_workspace_bytes(const kpop_refset *rs, uint32_t min_pts) {
  if (!rs || min_pts == 0 || min_pts > kRcMaxMinPts) return 0;
  return reach_carve(nullptr, rs->r1, min_pts, rs->n_dims).bytes;
}

extern "C" int kpop_dev_reachability_tree(kpop_refset *rs, uint32_t min_pts, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i,
                                          uint32_t *d_edge_j, double *d_edge_dist, double *d_core_dist, uint32_t *d_labels, void *stream) {
  const char *who = "kpop_dev_reachability_tree";
  KPOP_TRY(refset_check_handle(rs, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return reach_dev(rs, min_pts, max_distance, d_work, d_n_edges, d_edge_i, d_edge_j, d_edge_dist, d_core_dist, d_labels, as_stream(stream), false, who);
}

extern "C" int kpop_reachability_tree(kpop_refset *rs, uint32_t min_pts, double max_distance, uint32_t *n_edges, uint32_t *edge_i, uint32_t *edge_j,
                                      double *edge_dist, double *core_dist, uint32_t *labels) {
  const char *who = "kpop_reachability_tree";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(reach_check_min_pts(min_pts, who));
  KPOP_TRY(check_distance_is_a_number(max_distance, who));
  const uint32_t r1 = rs->r1;
  if (!n_edges || (r1 > 1 && (!edge_i || !edge_j || !edge_dist))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  *n_edges = 0;
  if (r1 == 0) return KPOP_OK;
  const uint64_t m = std::max(r1, 2u) - 1;
  HostCall h;
  void *work = h.work(reach_carve(nullptr, r1, min_pts, rs->n_dims).bytes);
  uint32_t *dn = h.scalars<uint32_t>(), *di = h.counted(edge_i, m), *dj = h.counted(edge_j, m);
  double *dd = h.counted(edge_dist, m), *dc = h.out(core_dist, r1);
  uint32_t *dl = h.out(labels, r1);
  KPOP_TRY(h.upload());
  KPOP_TRY(reach_dev(rs, min_pts, max_distance, work, dn, di, dj, dd, dc, dl, h.st, true, who));
  uint32_t n = 0;
  KPOP_TRY(h.read(&n, dn, 1));
  if (n > m) KPOP_FAIL(KPOP_ERR_HIP, "%s: %u edges on %u rows", who, n, r1);  // (cannot happen: a forest)
  KPOP_TRY(h.finish(n));
  *n_edges = n;
  return KPOP_OK;
}

extern "C" int kpop_distance_reachability_tree(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                               uint32_t min_pts, double max_distance, uint32_t *n_edges, uint32_t *edge_i, uint32_t *edge_j, double *edge_dist,
                                               double *core_dist, uint32_t *labels) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_reachability_tree(rs, min_pts, max_distance, n_edges, edge_i, edge_j, edge_dist, core_dist, labels);
  });
}

// host arithmetic alone: kpop_forest_cut's union-find over the edges within T, then the rows that are not core at T made noise
extern "C" int kpop_reachability_cut(uint32_t r1, uint32_t n_edges, const uint32_t *edge_i, const uint32_t *edge_j, const double *edge_dist,
                                     const double *core_dist, double T, uint32_t *labels, uint32_t *counts) {
  const char *who = "kpop_reachability_cut";
  KPOP_TRY(check_distance_is_a_number(T, who));
  if (!counts || (r1 && (!labels || !core_dist)) || (n_edges && (!edge_i || !edge_j || !edge_dist))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  uint32_t n_components = 0;
  KPOP_TRY(kpop_forest_cut(r1, n_edges, edge_i, edge_j, edge_dist, T, labels, &n_components));
  // a cluster: a component with a core row in it, counted at its first
  std::vector<uint8_t> seen(r1, 0);
  uint32_t clusters = 0, core = 0;
  for (uint32_t i = 0; i < r1; ++i) {
    if (!(core_dist[i] <= T)) continue;  // (a NaN is no core distance)
    ++core;
    if (!seen[labels[i]]) {
      seen[labels[i]] = 1;
      ++clusters;
    }
  }
  for (uint32_t i = 0; i < r1; ++i)
    if (!(core_dist[i] <= T)) labels[i] = KPOP_NOISE;
  counts[0] = clusters;
  counts[1] = core;
  counts[2] = r1 - core;
  return KPOP_OK;
}
