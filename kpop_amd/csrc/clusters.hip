// clusters.hip -- clusters at a distance: the connected components of a resident set.
//
//   The graph on the set's r1 rows: i < j are joined iff d(j, i) <= max_distance, where d(j, i) is the reference chain's distance
//   (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250): the bits kpop_refset_distance_rowwise writes to out[j][i] on
//   the vector pipe when the set's own rows are the query -- no kpop_tune setting is read here.  The chain is symmetric bit for bit
//   (a - b and b - a differ in sign only, component<KIND> squares the difference or takes fabs, space_ops.h), so only i < j is
//   examined.  labels[i] = the smallest row index of row i's component; a NaN distance joins nothing.
//
// Neither a pair nor a list is ever written: the self-join's hits go straight into a union-find forest that lives in the labels.
//   clusters_init_kernel     parent[i] = i for the rows that are new (i >= known_rows); the rows below carry the labels of an earlier
//                            call at the same distance, which are a forest of depth one already
//   clusters_tile_kernel     one tile of the folded upper triangle (tri_tile.h), none that lies below known_rows on both sides; both
//                            operands the set (its divided copy when it normalises).  The tile's distances and the compare are
//                            self_tile.h's (the loop pair_tile.h's); the hits are united in the tile's forest in LDS, and then
//                            every node of the tile that is not its local root is united with that root in `parent`: at most
//                            one global union per column and row of the tile, whatever the number of hits
//   the union                lock-free (union_find.h): the LARGER root hooked under the smaller, so that the last root of a
//                            component is its smallest index whoever arrives first, and nothing waits on another workgroup
//   clusters_flatten_kernel  a launch of its own after the tiles: labels[i] = the root of i (uf_settle), and the count of the roots,
//                            an integer sum
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr int kCMaxW = 64, kCMaxTJ = 256;

__global__ __launch_bounds__(256) void clusters_init_kernel(uint32_t *__restrict__ parent, uint32_t known_rows, uint32_t r1) {
  for (uint64_t i = (uint64_t)known_rows + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) parent[i] = (uint32_t)i;
}

// a: the set's rows as the chain reads them, both operands.  The tile, the thread's pairs and the shapes: tri_tile.h; the row tiles from
// by_first on -- the first with a row that is not known -- are walked.
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void clusters_tile_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                               const double *__restrict__ metric, double p, double max_distance, uint32_t n_cg,
                                                               uint32_t n_rg, uint32_t kf, uint32_t by_first, uint32_t n_act, uint32_t ybase,
                                                               uint32_t known_rows, uint32_t *parent) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kCMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kCMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_par[kCMaxW + kCMaxTJ];  // the tile's forest: the columns first, then the rows
  const uint32_t TJ = TY * n_rg;
  const TriTile t = tri_tile(blockIdx.x, ybase + blockIdx.y, w, TJ, kf, by_first, n_act, r1);
  if (!t.live) return;
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;  // (n_cg n_rg = 256 in both shapes: every thread holds pairs)
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) s_par[n] = n;  // (the loop's barriers come before anybody unites)
  double acc[TY][4];
  const PairRows rows{a, r1};
  pair_tile_distances<KIND, TY, kCMaxW, kCMaxTJ>(acc, As, Bs, s_metric, rows, t.i0, t.i1, rows, t.j0, t.j1, n_dims, metric, p, ti, tj, true);
  const uint32_t mask = self_hit_mask<TY>(acc, t, ti, tj, max_distance, known_rows);
  if (!__syncthreads_or(mask != 0)) return;  // most tiles of a sparse graph
  tile_forest_unite<TY>(mask, s_par, t, w, TJ, ti, tj, parent);
}

// after the tiles: every row's root, and the number of roots
__global__ __launch_bounds__(256) void clusters_flatten_kernel(uint32_t *parent, uint32_t r1, uint32_t *__restrict__ n_clusters) {
  __shared__ uint32_t s_roots;
  if (threadIdx.x == 0) s_roots = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256)
    if (uf_settle<__HIP_MEMORY_SCOPE_AGENT>(parent, (uint32_t)i) == (uint32_t)i) ++mine;
  if (mine) atomicAdd(&s_roots, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_roots) atomicAdd(n_clusters, s_roots);
}

template <int KIND>
static int clusters_tiles(const double *a, uint32_t r1, uint32_t n_dims, const double *metric, double p, double max_distance, uint32_t known_rows,
                          uint32_t *parent, hipStream_t st) {
  const SelfShape s = self_shape(r1);
  const uint32_t by_first = known_rows / s.TJ, n_act = div_up(r1, s.TJ) - by_first;  // (known_rows < r1: by_first is a row tile)
  return self_triangle_launch(s, r1, by_first, [&](auto TY, dim3 grid, uint32_t ybase) {
    clusters_tile_kernel<KIND, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, n_dims, metric, p, max_distance, s.n_cg, s.n_rg, s.kf, by_first, n_act, ybase,
                                                                               known_rows, parent);
  });
}

// the body of both entry points: enqueues only
static int clusters_dev(kpop_refset *rs, double max_distance, uint32_t known_rows, uint32_t *d_labels, uint32_t *d_n_clusters, hipStream_t st) {
  const char *who = "kpop_dev_clusters_within";
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!d_n_clusters) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  if (known_rows > rs->r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u known rows in a set of %u", who, known_rows, rs->r1);
  KPOP_HIP(hipMemsetAsync(d_n_clusters, 0, 4, st));
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  if (!d_labels) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null labels", who);
  if (known_rows < r1) {
    clusters_init_kernel<<<dim3(std::min(div_up(r1 - known_rows, 256), 4096u)), dim3(256), 0, st>>>(d_labels, known_rows, r1);
    KPOP_LAUNCH_CHECK();
    if (max_distance >= 0.0) {  // (no distance is negative: below zero every row stays alone)
      const double *a;
      KPOP_TRY(refset_chain_rows(rs, st, &a));
      KPOP_TRY(by_kind(rs->kind, [&](auto K) {
        return clusters_tiles<decltype(K)::value>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, known_rows, d_labels, st);
      }));
    }
  }
  clusters_flatten_kernel<<<dim3(std::min(div_up(r1, 256), 4096u)), dim3(256), 0, st>>>(d_labels, r1, d_n_clusters);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_clusters_within_workspace_bytes(const kpop_refset *rs) {
  if (!rs) return 0;
  return 256;  // the forest lives in the labels; the set holds its own divided copy
}

extern "C" int kpop_dev_clusters_within(kpop_refset *rs, double max_distance, uint32_t known_rows, void *d_work, uint32_t *d_labels, uint32_t *d_n_clusters,
                                        void *stream) {
  KPOP_TRY(refset_check_handle(rs, "kpop_dev_clusters_within"));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_dev_clusters_within: null workspace");
  return clusters_dev(rs, max_distance, known_rows, d_labels, d_n_clusters, as_stream(stream));
}

extern "C" int kpop_clusters_within(kpop_refset *rs, double max_distance, uint32_t known_rows, uint32_t *labels, uint32_t *n_clusters) {
  const char *who = "kpop_clusters_within";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(check_distance_is_a_number(max_distance, who));
  if (!n_clusters || (rs->r1 && !labels)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t r1 = rs->r1;
  if (known_rows > r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u known rows in a set of %u", who, known_rows, r1);
  KPOP_TRY(check_known_prefix(labels, known_rows, who, "labels", "a label"));
  *n_clusters = 0;
  if (r1 == 0) return KPOP_OK;
  HostCall h;
  uint32_t *dl = h.out(labels, r1);
  uint32_t *dn = h.scalars(n_clusters, 1);
  h.up(dl, labels, known_rows);
  KPOP_TRY(h.upload());
  KPOP_TRY(clusters_dev(rs, max_distance, known_rows, dl, dn, h.st));
  return h.finish();
}

extern "C" int kpop_distance_clusters(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                      double max_distance, uint32_t *labels, uint32_t *n_clusters) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) { return kpop_clusters_within(rs, max_distance, 0, labels, n_clusters); });
}
