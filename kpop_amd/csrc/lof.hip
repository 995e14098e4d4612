// lof.hip -- the local outlier factor of a resident set, and of query rows against it.
//
//   Breunig, Kriegel, Ng, Sander 2000.  d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with the adaptors of
//   lib/Matrix.ml:243-250): the bits kpop_refset_distance_rowwise writes on the vector pipe, symmetric bit for bit; no kpop_tune setting
//   is read; a NaN distance is within nothing.  k in 1 .. 128.
//   THE SET FORM, every row j against the other rows (the pair i == j is never examined):
//     kdist[j]   = kpop_core_distances(k + 1)[j], bit for bit: the k-th least of the numbers among d(j, i), i != j; the quiet NaN
//                  when there are fewer than k
//     N(j)       = { i != j : d(j, i) <= kdist[j] } -- the WHOLE tie group of the k-th distance, so nothing depends on the row order
//     n_neigh[j] = |N(j)|, 0 when kdist[j] is a NaN
//     lrd[j]     = n_neigh[j] / S1(j), S1(j) the sum over N(j) of max(d(j, i), kdist[i]); +inf when S1 = 0, 0 when S1 = +inf
//     lof[j]     = (S2(j) / n_neigh[j]) / lrd[j], S2(j) the sum over N(j) of lrd[i]; IEEE arithmetic with ONE exception: inf / inf is
//                  1.0 (a row inside a clump of copies is as dense as its neighbours).  A finite lrd beside a clump gives +inf, 0 / 0 a
//                  NaN; n_neigh = 0 gives the quiet NaN for lrd and lof; a NaN term poisons the sum it is in; a zero is +0
//   THE QUERY FORM, row q of m2 against the set as it stands, the set's kdist and lrd passed in (the set's rows are not re-scored):
//     the same with nothing left out -- a query equal to a set row has that row at distance 0 -- and kdist[i], lrd[i] the set's.
//
// The launches (the device forms read nothing back and allocate nothing):
//   core_dev            (reachability.hip) the set form's k-distances: the leave-self-out lists at min_pts = k + 1
//   knn_run_lists       (knn.hip) the query form's: the first two k-NN passes of a slab of query rows, no tie pass; then
//   lof_kdist_kernel    the k-th key of a full merged list, the quiet NaN of a shorter one
//   lof_pass_kernel     THE SWEEP.  A workgroup owns a row strip and walks the plain column tiles of its segment (pair_tile.h), both
//                       tile shapes of self_shape.  The strip's k-distances are read once into LDS, the four columns' values once a tile
//                       in front of the arithmetic.  member = inside the tile && !(LEAVE_SELF && i == j) && d <= kdist_row (a NaN on
//                       either side compares false); cnt += member; sum += member ? TERM(d, colval) : +0.  Launch A: colval = kdist,
//                       TERM = max(d, colval); launch B: colval = lrd, TERM = colval.  One body for both launches and both forms.
//                       A strip's column tiles are cut into up to 16 segments (lof_segments), a workgroup each, so that a set of a few
//                       hundred rows, or three query rows against a long set, still fills the device; a segment leaves (cnt, sum) a row
//   lof_rows_kernel     merges the segments in segment order; after launch A n_neigh and lrd, after launch B lof
// THE SUMS: within a thread the columns ascend and a non-member adds +0; a row's lanes meet in a fixed tree (reduce_row_lanes); the
// segments are added in segment order.  The order is a fixed function of r1 (and r2), n_dims and k; no floating-point atomic: the same
// bits on every run.
// THE COST is three full rectangles (the lists, launch A, launch B).  No known_rows: a new row can lower old rows' k-distances, so
// after kpop_refset_append the set form is called again in full.  Neither the matrix nor a neighbour list longer than k is formed; apart
// from the lists of the k-distances the workspace is O(r1), or O(slab x segments) for a slab of query rows.
#include <algorithm>

#include "class_tiles.h"  // (the silhouette's tile limits kSilMaxW / kSilMaxTJ, LaneSum and sil_nan: one sweep shape, one lane sum)
#include "common.h"
#include "distance_routes.h"
#include "knn_lists.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr uint32_t kLofMaxSeg = 16;
constexpr uint32_t kLofSlabRows = 16384;  // query rows a slab (reachability.hip's kRcSlabRows, and its reason)

// how a strip's column tiles are cut: enough workgroups for a short set or a few query rows (2,048 and more where there are the
// strips), never more segments than column tiles, none of them empty.  A function of the row and column counts alone
struct LofSegments {
  uint32_t n_seg, tiles_per_seg;
};
static LofSegments lof_segments(uint32_t n_rows, uint32_t r1) {
  const SelfShape s = self_shape(r1);
  const uint32_t n_rt = div_up(std::max(n_rows, 1u), s.TJ), n_ct = std::max(1u, div_up(r1, s.w));
  const uint32_t want = std::min(std::min(kLofMaxSeg, n_ct), std::max(1u, div_up(2048, n_rt)));
  const uint32_t per = div_up(n_ct, want);
  return LofSegments{div_up(n_ct, per), per};
}

// kdist, lrd [n_rows]: the two outputs the body needs itself, used where the caller passes NULL; cnt, sum [kLofMaxSeg][n_rows]: what a
// launch of the sweep leaves; rest: the lists of the k-distances
struct LofWork {
  double *kdist, *lrd, *sum;
  uint32_t *cnt;
  void *rest;
  uint64_t bytes;
};
static LofWork lof_carve(void *base, uint32_t n_rows, uint64_t rest_bytes) {
  const uint64_t n = std::max(n_rows, 1u);
  Carver c(base);
  LofWork f;
  f.kdist = c.take<double>(n * 8);
  f.lrd = c.take<double>(n * 8);
  f.sum = c.take<double>(n * kLofMaxSeg * 8);
  f.cnt = c.take<uint32_t>(n * kLofMaxSeg * 4);
  f.rest = c.take<void>(rest_bytes);
  f.bytes = c.off;
  return f;
}

// a slab's lists, and the divided copy of its rows when the set normalises (knn_carve without a class or a tie table); the last slab
// may be cut into more segments than a whole one: the larger of the two
static uint64_t lof_score_rest_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k) {
  const uint32_t slab = std::max(1u, std::min(r2, kLofSlabRows)), last = r2 % slab ? r2 % slab : slab;
  return std::max(knn_carve(nullptr, slab, k, 0, rs->n_dims, rs->normalize != 0).bytes, knn_carve(nullptr, last, k, 0, rs->n_dims, rs->normalize != 0).bytes);
}

constexpr int kLofTermMax = 0, kLofTermValue = 1;

// a: the set's rows, the columns; b: the rows of the strips -- a itself (LEAVE_SELF: row j of b is row j of the set) or the query rows;
// both as the chain reads them.  Strip blockIdx.x: rows j0 .. j0 + TJ, TJ = TY n_rg; a thread 4 columns x TY rows, n_cg n_rg = 256.
// Segment blockIdx.y: column tiles blockIdx.y tiles_per_seg onwards.  kdist_row [n_rows]; colval [r1]; cnt_out, sum_out
// [gridDim.y][n_rows]
template <int KIND, int TY, int TERM, bool LEAVE_SELF>
__global__ __launch_bounds__(256, 1) void lof_pass_kernel(const double *__restrict__ a, uint32_t r1, const double *__restrict__ b, uint32_t n_rows, uint32_t n_dims,
                                                          const double *__restrict__ metric, double p, uint32_t w, uint32_t n_cg, uint32_t n_rg,
                                                          uint32_t tiles_per_seg, const double *__restrict__ kdist_row, const double *__restrict__ colval,
                                                          uint32_t *__restrict__ cnt_out, double *__restrict__ sum_out) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kSilMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kSilMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ double s_kd[kSilMaxTJ];  // the k-distances of the strip's rows; beyond the strip's end a NaN, which nothing is within
  const uint32_t TJ = TY * n_rg;
  const uint32_t j0 = blockIdx.x * TJ;
  if (j0 >= n_rows) return;
  const uint32_t j1 = min(n_rows, j0 + TJ);
  const uint32_t n_ct = r1 / w + (r1 % w ? 1u : 0u);
  const uint32_t seg = blockIdx.y;
  const uint32_t t_begin = min(n_ct, seg * tiles_per_seg), t_end = min(n_ct, t_begin + tiles_per_seg);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < TJ; n += 256) s_kd[n] = j0 + n < j1 ? kdist_row[j0 + n] : sil_nan();
  __syncthreads();
  uint32_t cnt[TY];
  double sum[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    cnt[yy] = 0;
    sum[yy] = 0.0;
  }
  const PairTilesOf tiles{w, (uint32_t)min((uint64_t)r1, (uint64_t)t_end * w)};
  const PairRows cols{a, r1}, rows{b, n_rows};
  PairStage<kSilMaxW, kSilMaxTJ> stage;
  PairTile cur = tiles.at(t_begin * w), nxt;
  for (pair_sweep_open(stage, cols, cur, rows, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = tiles.after(cur);
    double cv[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) cv[x] = (cur.i0 + ti + x < cur.i1) ? colval[cur.i0 + ti + x] : 0.0;
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, rows, j0, j1, n_dims, metric, p, ti, tj, true);
    // the tile's members onto the row's count and running sum, the columns ascending; everybody else adds +0
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t j = j0 + tj + yy;
      const double kd = s_kd[tj + yy];
      uint32_t c = cnt[yy];
      double s = sum[yy];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t i = cur.i0 + ti + x;
        const bool member = i < cur.i1 && !(LEAVE_SELF && i == j) && d <= kd;  // (a NaN, d or kd, is within nothing)
        // max as doubles, a NaN k-distance of the column kept: it poisons the sum
        const double term = TERM == kLofTermMax ? (d > cv[x] ? d : cv[x]) : cv[x];
        c += member ? 1u : 0u;
        s = __dadd_rn(s, member ? term : 0.0);
      }
      cnt[yy] = c;
      sum[yy] = s;
    }
  }
  const auto add = [](uint32_t x, uint32_t y) { return x + y; };
  const auto dadd = [](LaneSum x, LaneSum y) { return LaneSum{__dadd_rn(x.v, y.v)}; };
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t j = j0 + tj + yy;
    const uint32_t c = reduce_row_lanes(cnt[yy], n_cg, add);
    const double s = reduce_row_lanes(LaneSum{sum[yy]}, n_cg, dadd).v;
    if (cg == 0 && j < j1) {
      cnt_out[(uint64_t)seg * n_rows + j] = c;
      sum_out[(uint64_t)seg * n_rows + j] = s;
    }
  }
}

// the k-distances of n query rows from their merged lists (a key gives back +0 for a zero)
__global__ __launch_bounds__(256) void lof_kdist_kernel(const uint32_t *__restrict__ m_n, const uint64_t *__restrict__ m_tau, uint32_t k, uint32_t n,
                                                        double *__restrict__ kdist) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) kdist[i] = m_n[i] == k ? key_f64(m_tau[i]) : sil_nan();
}

// the segments of n rows merged in segment order.  STAGE 0, after launch A: n_neigh (may be null) and lrd.  STAGE 1, after launch B:
// lof from lrd -- inf / inf is 1.0, a row without neighbours and any other NaN the quiet NaN, a zero +0
template <int STAGE>
__global__ __launch_bounds__(256) void lof_rows_kernel(const uint32_t *__restrict__ cnt, const double *__restrict__ sum, uint32_t n_seg, uint32_t n,
                                                       uint32_t *__restrict__ n_neigh, double *lrd, double *__restrict__ lof) {
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    uint32_t c = 0;
    double s = 0.0;
    for (uint32_t sg = 0; sg < n_seg; ++sg) {
      c += cnt[(uint64_t)sg * n + i];
      s = __dadd_rn(s, sum[(uint64_t)sg * n + i]);
    }
    double out = sil_nan();
    if (STAGE == 0) {
      if (c) out = __ddiv_rn((double)c, s);
      if (n_neigh) n_neigh[i] = c;
    } else if (c) {
      const double mean = __ddiv_rn(s, (double)c), l = lrd[i];
      out = (mean == inf && l == inf) ? 1.0 : __ddiv_rn(mean, l);
    }
    if (out != out) out = sil_nan();
    if (out == 0.0) out = 0.0;
    if (STAGE == 0) lrd[i] = out;
    else lof[i] = out;
  }
}

// rows without a k-th neighbour, all of them: the quiet NaN and no neighbours (each output may be null)
__global__ __launch_bounds__(256) void lof_fill_kernel(uint32_t n, double *__restrict__ kdist, uint32_t *__restrict__ n_neigh, double *__restrict__ lrd,
                                                       double *__restrict__ lof) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (kdist) kdist[i] = sil_nan();
    if (n_neigh) n_neigh[i] = 0;
    if (lrd) lrd[i] = sil_nan();
    if (lof) lof[i] = sil_nan();
  }
}

static int lof_check_k(uint32_t k, const char *who) {
  if (k == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: k = 0", who);
  if (k > (uint32_t)kKMaxK) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: k = %u (at most %d: the lists hold that many neighbours)", who, k, kKMaxK);
  return 0;
}

static dim3 lof_rows_grid(uint32_t n) { return dim3(std::min(div_up(std::max(n, 1u), 256), 4096u)); }

// one launch of the sweep over n_rows rows of b against the set's rows a, and the merge behind it
template <int TERM, bool LEAVE_SELF>
static int lof_launch(kpop_refset *rs, const double *a, const double *b, uint32_t n_rows, const double *kdist_row, const double *colval, const LofWork &f,
                      uint32_t *n_neigh, double *lrd, double *lof, hipStream_t st) {
  const uint32_t r1 = rs->r1;
  const SelfShape s = self_shape(r1);
  const LofSegments g = lof_segments(n_rows, r1);
  const dim3 grid(div_up(n_rows, s.TJ), g.n_seg);
  KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
    by_shape_rows(s, [&](auto TY) {
      lof_pass_kernel<decltype(K)::value, decltype(TY)::value, TERM, LEAVE_SELF><<<grid, dim3(256), 0, st>>>(a, r1, b, n_rows, rs->n_dims, rs->metric, rs->p, s.w, s.n_cg, s.n_rg,
                                                                                                            g.tiles_per_seg, kdist_row, colval, f.cnt, f.sum);
    });
    KPOP_LAUNCH_CHECK();
    return 0;
  }));
  constexpr int STAGE = TERM == kLofTermMax ? 0 : 1;  // launch A, launch B
  lof_rows_kernel<STAGE><<<lof_rows_grid(n_rows), dim3(256), 0, st>>>(f.cnt, f.sum, g.n_seg, n_rows, n_neigh, lrd, lof);
  KPOP_LAUNCH_CHECK();
  return 0;
}

// launch A and, when lof is wanted, launch B, over rows whose k-distances are in kdist
template <bool LEAVE_SELF>
static int lof_two_launches(kpop_refset *rs, const double *a, const double *b, uint32_t n_rows, const double *kdist, const double *set_kdist, const double *set_lrd_or_null,
                            const LofWork &f, uint32_t *n_neigh, double *lrd, double *lof, hipStream_t st) {
  KPOP_TRY((lof_launch<kLofTermMax, LEAVE_SELF>(rs, a, b, n_rows, kdist, set_kdist, f, n_neigh, lrd, nullptr, st)));
  if (!lof) return 0;
  return lof_launch<kLofTermValue, LEAVE_SELF>(rs, a, b, n_rows, kdist, set_lrd_or_null ? set_lrd_or_null : lrd, f, nullptr, lrd, lof, st);
}

// the body of the set form's entry points: enqueues only.  k is checked, r1 > 0
static int lof_dev(kpop_refset *rs, uint32_t k, void *d_work, double *d_kdist, uint32_t *d_n_neigh, double *d_lrd, double *d_lof, hipStream_t st) {
  const uint32_t r1 = rs->r1;
  const LofWork f = lof_carve(d_work, r1, core_workspace_bytes(r1, k + 1, rs->n_dims));
  double *kdist = d_kdist ? d_kdist : f.kdist, *lrd = d_lrd ? d_lrd : f.lrd;
  if (k >= r1) {  // nobody has k other rows
    lof_fill_kernel<<<lof_rows_grid(r1), dim3(256), 0, st>>>(r1, d_kdist, d_n_neigh, d_lrd, d_lof);
    KPOP_LAUNCH_CHECK();
    return KPOP_OK;
  }
  KPOP_TRY(core_dev(rs, k + 1, f.rest, kdist, st));
  if (!d_n_neigh && !d_lrd && !d_lof) return KPOP_OK;  // (the k-distances alone)
  const double *a;  // both operands
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  return lof_two_launches<true>(rs, a, a, r1, kdist, kdist, nullptr, f, d_n_neigh, lrd, d_lof, st);
}

// the body of the query form's entry points: enqueues only.  k is checked, r2 > 0
static int lof_score_dev(kpop_refset *rs, uint32_t k, const double *d_set_kdist, const double *d_set_lrd, const double *d_m2, uint32_t r2, void *d_work,
                         double *d_kdist, uint32_t *d_n_neigh, double *d_lrd, double *d_lof, hipStream_t st) {
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 < k) {  // no query row has k rows of the set
    lof_fill_kernel<<<lof_rows_grid(r2), dim3(256), 0, st>>>(r2, d_kdist, d_n_neigh, d_lrd, d_lof);
    KPOP_LAUNCH_CHECK();
    return KPOP_OK;
  }
  const double *a;
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  const uint32_t slab = std::min(r2, kLofSlabRows);
  const LofWork f = lof_carve(d_work, slab, lof_score_rest_bytes(rs, r2, k));
  for (uint32_t j0 = 0; j0 < r2; j0 += slab) {
    const uint32_t nr = std::min(slab, r2 - j0);
    const KnnWork w = knn_carve(f.rest, nr, k, 0, D, rs->normalize != 0);
    const double *b = d_m2 + (uint64_t)j0 * D;
    if (rs->normalize) {  // the query rows' quotients from the norms' pass, as in knn_dev
      KPOP_TRY(refset_query_norms(rs, b, nr, w.n2, w.b, st));
      b = w.b;
    }
    double *kdist = d_kdist ? d_kdist + j0 : f.kdist, *lrd = d_lrd ? d_lrd + j0 : f.lrd;
    uint32_t n_seg = 0;
    KPOP_TRY(knn_run_lists(rs->kind, a, r1, b, nr, D, rs->metric, rs->p, k, w, &n_seg, st));
    lof_kdist_kernel<<<lof_rows_grid(nr), dim3(256), 0, st>>>(w.m_n, w.m_tau, k, nr, kdist);
    KPOP_LAUNCH_CHECK();
    if (!d_n_neigh && !d_lrd && !d_lof) continue;
    KPOP_TRY((lof_two_launches<false>(rs, a, b, nr, kdist, d_set_kdist, d_set_lrd, f, d_n_neigh ? d_n_neigh + j0 : nullptr, lrd, d_lof ? d_lof + j0 : nullptr, st)));
  }
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_lof_workspace_bytes(const kpop_refset *rs, uint32_t k) {
  if (!rs || k == 0 || k > (uint32_t)kKMaxK) return 0;
  return lof_carve(nullptr, rs->r1, core_workspace_bytes(rs->r1, k + 1, rs->n_dims)).bytes;
}

extern "C" int kpop_dev_lof(kpop_refset *rs, uint32_t k, void *d_work, double *d_kdist, uint32_t *d_n_neigh, double *d_lrd, double *d_lof, void *stream) {
  const char *who = "kpop_dev_lof";
  KPOP_TRY(refset_check_handle(rs, who));
  KPOP_TRY(lof_check_k(k, who));
  if (rs->r1 == 0) return KPOP_OK;
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return lof_dev(rs, k, d_work, d_kdist, d_n_neigh, d_lrd, d_lof, as_stream(stream));
}

extern "C" int kpop_lof(kpop_refset *rs, uint32_t k, double *kdist, uint32_t *n_neigh, double *lrd, double *lof) {
  const char *who = "kpop_lof";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(lof_check_k(k, who));
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  HostCall h;
  void *work = h.work(kpop_dev_lof_workspace_bytes(rs, k));
  double *dk = h.out(kdist, r1);
  uint32_t *dn = h.out(n_neigh, r1);
  double *dl = h.out(lrd, r1), *df = h.out(lof, r1);
  KPOP_TRY(h.upload());
  KPOP_TRY(lof_dev(rs, k, work, dk, dn, dl, df, h.st));
  return h.finish();
}

extern "C" int kpop_distance_lof(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize, uint32_t k,
                                 double *kdist, uint32_t *n_neigh, double *lrd, double *lof) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) { return kpop_lof(rs, k, kdist, n_neigh, lrd, lof); });
}

extern "C" uint64_t kpop_dev_lof_score_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k) {
  if (!rs || k == 0 || k > (uint32_t)kKMaxK) return 0;
  return lof_carve(nullptr, std::min(r2, kLofSlabRows), lof_score_rest_bytes(rs, r2, k)).bytes;
}

extern "C" int kpop_dev_lof_score(kpop_refset *rs, uint32_t k, const double *d_set_kdist, const double *d_set_lrd, const double *d_m2, uint32_t r2, void *d_work,
                                  double *d_kdist, uint32_t *d_n_neigh, double *d_lrd, double *d_lof, void *stream) {
  const char *who = "kpop_dev_lof_score";
  KPOP_TRY(refset_check_handle(rs, who));
  KPOP_TRY(lof_check_k(k, who));
  if (r2 == 0) return KPOP_OK;
  if (!d_work || (rs->r1 >= k && (!d_set_kdist || !d_set_lrd || !d_m2))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  return lof_score_dev(rs, k, d_set_kdist, d_set_lrd, d_m2, r2, d_work, d_kdist, d_n_neigh, d_lrd, d_lof, as_stream(stream));
}

extern "C" int kpop_lof_score(kpop_refset *rs, uint32_t k, const double *set_kdist, const double *set_lrd, const double *m2, uint32_t r2, double *kdist,
                              uint32_t *n_neigh, double *lrd, double *lof) {
  const char *who = "kpop_lof_score";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(lof_check_k(k, who));
  if (r2 == 0) return KPOP_OK;
  const uint32_t r1 = rs->r1;
  if (r1 >= k && (!set_kdist || !set_lrd || !m2)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  HostCall h;  // (eight buffers)
  void *work = h.work(kpop_dev_lof_score_workspace_bytes(rs, r2, k));
  const double *sk = h.in(set_kdist, r1), *sl = h.in(set_lrd, r1), *d2 = h.in(m2, (uint64_t)r2 * rs->n_dims);
  double *dk = h.out(kdist, r2);
  uint32_t *dn = h.out(n_neigh, r2);
  double *dl = h.out(lrd, r2), *df = h.out(lof, r2);
  KPOP_TRY(h.upload());
  KPOP_TRY(lof_score_dev(rs, k, sk, sl, d2, r2, work, dk, dn, dl, df, h.st));
  return h.finish();
}
