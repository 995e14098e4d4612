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
//   clusters_tile_kernel     the arithmetic of within_tile_kernel (within.hip), the same loop (pair_tile.h), both operands the set (its
//                            divided copy when it normalises); tiles of the upper triangle only, none that lies below known_rows on
//                            both sides.  The epilogue compares where that kernel compares, unites the tile's hits in LDS (a forest
//                            over the tile's columns and rows: thousands of hits inside a dense lineage cost LDS traffic alone), and
//                            then every node of the tile that is not its local root is united with that root in `parent`: at most
//                            one global union per column and row of the tile, whatever the number of hits
//   the union                lock-free (union_find.h): the LARGER root hooked under the smaller, so that the last root of a
//                            component is its smallest index whoever arrives first, and nothing waits on another workgroup
//   clusters_flatten_kernel  a launch of its own after the tiles: labels[i] = the root of i (finds that store nothing but that), and
//                            the count of the roots, an integer sum
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "pair_tile.h"
#include "space_ops.h"
#include "union_find.h"

namespace kpop {

constexpr int kCMaxW = 64, kCMaxTJ = 256;

__global__ __launch_bounds__(256) void clusters_init_kernel(uint32_t *__restrict__ parent, uint32_t known_rows, uint32_t r1) {
  for (uint64_t i = (uint64_t)known_rows + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) parent[i] = (uint32_t)i;
}

// a: the set's rows as the chain reads them (divided by their norms when the set normalises), both operands.  Tiles of w columns
// (rows i of the set) x TJ = TY n_rg rows (rows j), TJ = kf w; a thread 4 columns x TY rows, the dimensions ascending in one thread,
// 16 at a time through LDS: within_tile_kernel's.  Row tile `by` needs the column tiles 0 .. (by + 1) kf - 1 (those with a column
// below its last row); the row tiles from by_first on -- the first with a row that is not known -- are folded, the y-th with the
// y-th from the end, so that every line of the grid holds the same number of tiles and no block is launched for the lower triangle.
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
  // which tile
  const uint32_t y = ybase + blockIdx.y;
  const uint32_t by_lo = by_first + y, by_hi = by_first + n_act - 1 - y;
  const uint32_t n_lo = (by_lo + 1) * kf;
  uint32_t bx = blockIdx.x, by = by_lo;
  if (bx >= n_lo) {
    if (by_hi == by_lo) return;  // (the middle line of an odd number: once)
    bx -= n_lo;
    by = by_hi;
  }
  const uint32_t i0 = bx * w, j0 = by * TJ;
  const uint32_t j1 = min(r1, j0 + TJ);
  if (i0 + 1 >= j1) return;  // (the last row tile is ragged: no column below its last row)
  const uint32_t i1 = min(r1, i0 + w);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const bool worker = rg < n_rg;
  const uint32_t ti = cg * 4, tj = (worker ? rg : 0) * TY;
  for (uint32_t n = threadIdx.x; n < w + TJ; n += 256) s_par[n] = n;  // (the loop's barriers come before anybody unites)
  double acc[TY][4];
  pair_zero(acc);
  PairStage<kCMaxW, kCMaxTJ> stage;
  stage.load(a, i0, i1, a, j0, j1, n_dims, 0, n_dims);
  for (uint32_t c0 = 0; c0 < n_dims; c0 += kPairDC) {
    __syncthreads();
    stage.store(As, Bs, s_metric, metric, c0, n_dims);
    __syncthreads();
    if (c0 + kPairDC < n_dims) stage.load(a, i0, i1, a, j0, j1, n_dims, c0 + kPairDC, n_dims);
    if (worker) pair_accumulate<KIND>(acc, As, Bs, s_metric, ti, tj, min((uint32_t)kPairDC, n_dims - c0), p);
  }
  // the epilogue: compare where within_tile_kernel compares (a NaN compares false: it joins nothing); only i < j, and no pair of
  // two known rows (i < j: the pair is one iff j is known)
  uint32_t mask = 0;
  if (worker) {
#pragma unroll
    for (int yy = 0; yy < TY; ++yy)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        acc[yy][x] = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t i = i0 + ti + x, j = j0 + tj + yy;
        if (j < j1 && i < i1 && i < j && j >= known_rows && acc[yy][x] <= max_distance) mask |= 1u << (yy * 4 + x);
      }
  }
  if (!__syncthreads_or(mask != 0)) return;  // most tiles of a sparse graph
  // the tile's own forest, in LDS: whatever the number of hits, what leaves the tile is one union per node
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
    if (root != n) uf_unite<DEV>(parent, n < w ? i0 + n : j0 + (n - w), root < w ? i0 + root : j0 + (root - w));
  }
}

// after the tiles: every row's root, and the number of roots.  A root is a row whose word is its own index: no store here changes
// that, and a word on somebody's path is that row's ancestor before the store and after it
__global__ __launch_bounds__(256) void clusters_flatten_kernel(uint32_t *parent, uint32_t r1, uint32_t *__restrict__ n_clusters) {
  __shared__ uint32_t s_roots;
  if (threadIdx.x == 0) s_roots = 0;
  __syncthreads();
  constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t root = uf_find_readonly<DEV>(parent, (uint32_t)i);
    if (root == (uint32_t)i) ++mine;
    else __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, DEV);
  }
  if (mine) atomicAdd(&s_roots, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_roots) atomicAdd(n_clusters, s_roots);
}

template <int KIND>
static int clusters_tiles(const double *a, uint32_t r1, uint32_t n_dims, const double *metric, double p, double max_distance, uint32_t known_rows,
                          uint32_t *parent, hipStream_t st) {
  // within_tiles' two shapes (within.hip): 32 columns x 256 rows, a thread 4 x 8, for a long set; 64 x 64, a thread 4 x 4, below.
  // (The choice moves no bit: a pair's chain is one thread's either way.)
  const bool big = r1 >= 65536;
  const uint32_t w = big ? 32 : 64, n_cg = w / 4, n_rg = 256 / n_cg, TJ = (big ? 8 : 4) * n_rg, kf = TJ / w;
  const uint32_t n_rt = div_up(r1, TJ), by_first = known_rows / TJ;  // (known_rows < r1: by_first < n_rt)
  const uint32_t n_act = n_rt - by_first, lines = (n_act + 1) / 2;
  const uint32_t gx = (2 * by_first + n_act + 1) * kf;  // the tiles of a row tile and of its partner from the end
  for (uint32_t ybase = 0; ybase < lines; ybase += 65535u) {
    const dim3 grid(gx, std::min(65535u, lines - ybase));
    if (big)
      clusters_tile_kernel<KIND, 8><<<grid, dim3(256), 0, st>>>(a, w, r1, n_dims, metric, p, max_distance, n_cg, n_rg, kf, by_first, n_act, ybase, known_rows, parent);
    else
      clusters_tile_kernel<KIND, 4><<<grid, dim3(256), 0, st>>>(a, w, r1, n_dims, metric, p, max_distance, n_cg, n_rg, kf, by_first, n_act, ybase, known_rows, parent);
    KPOP_LAUNCH_CHECK();
  }
  return 0;
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
      const double *a = rs->rows;
      if (rs->normalize) {
        KPOP_TRY(rs->prepared(st));
        KPOP_TRY(rs->divided(st, &a));
      }
      switch (rs->kind) {
        case KPOP_EUCLIDEAN: KPOP_TRY(clusters_tiles<KPOP_EUCLIDEAN>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, known_rows, d_labels, st)); break;
        case KPOP_COSINE: KPOP_TRY(clusters_tiles<KPOP_COSINE>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, known_rows, d_labels, st)); break;
        default: KPOP_TRY(clusters_tiles<KPOP_MINKOWSKI>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, known_rows, d_labels, st)); break;
      }
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
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!n_clusters || (rs->r1 && !labels)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t r1 = rs->r1;
  if (known_rows > r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u known rows in a set of %u", who, known_rows, r1);
  // what an earlier call returned: every label the smallest index of its component, hence no larger than its row and its own label
  for (uint32_t i = 0; i < known_rows; ++i)
    if (labels[i] > i || labels[labels[i]] != labels[i])
      KPOP_FAIL(KPOP_ERR_INVALID, "%s: labels[%u] = %u is not a label this call returns (labels[i] <= i, labels[labels[i]] == labels[i])", who, i, labels[i]);
  *n_clusters = 0;
  if (r1 == 0) return KPOP_OK;
  hipStream_t st = nullptr;
  DevBuf dl, dn;
  KPOP_TRY(dl.alloc((uint64_t)r1 * 4));
  KPOP_TRY(dn.alloc(256));
  if (known_rows) KPOP_HIP(hipMemcpyAsync(dl.p, labels, (uint64_t)known_rows * 4, hipMemcpyHostToDevice, st));
  KPOP_TRY(clusters_dev(rs, max_distance, known_rows, dl.as<uint32_t>(), dn.as<uint32_t>(), st));
  KPOP_HIP(hipMemcpyAsync(labels, dl.p, (uint64_t)r1 * 4, hipMemcpyDeviceToHost, st));
  KPOP_HIP(hipMemcpyAsync(n_clusters, dn.p, 4, hipMemcpyDeviceToHost, st));
  KPOP_HIP(hipStreamSynchronize(st));
  return KPOP_OK;
}

extern "C" int kpop_distance_clusters(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                      double max_distance, uint32_t *labels, uint32_t *n_clusters) {
  kpop_refset *rs = nullptr;
  KPOP_TRY(kpop_refset_create(m, rows, n_dims, metric, kind, p, normalize, 0, &rs));
  const int rc = kpop_clusters_within(rs, max_distance, 0, labels, n_clusters);
  const int rc_free = kpop_refset_free(rs);
  return rc ? rc : rc_free;
}
