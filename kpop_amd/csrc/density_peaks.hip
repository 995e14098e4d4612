// density_peaks.hip -- the density peaks of a resident set: every row's nearest row of higher density, the forest these make, and its cut
// (INTEGRATION.md section 6p).
//
//   Rodriguez, Laio 2014.  d(j, i) is the reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250):
//   the bits kpop_refset_distance_rowwise writes on the vector pipe, symmetric bit for bit; no kpop_tune setting is read; the pair i == j
//   is never examined; a NaN distance is no candidate; a zero is written as +0.
//   DENSITY  the caller's density[r1], or (double) degree[i], kpop_dbscan's at eps (1 + the other rows within eps).  A row whose density is
//            a NaN is LEFT OUT: nobody's candidate, delta the quiet NaN, parent = label = KPOP_NOISE.  -0 equals +0; +-inf are numbers.
//   RANK     row i ranks above row j iff density[i] > density[j], or they are equal and i < j: a strict total order of the rows kept.
//   PARENT   the least, under (d with -0 as +0, row index), of the rows that rank above j and whose distance to j is a number;
//   DELTA    that distance.  None: parent[j] = j, delta[j] = +inf, a ROOT.  A parent ranks above its child: a forest.
//   CUT      row j is a CENTRE iff it is a root or delta[j] > min_delta && density[j] >= min_density; labels[j] = j for a centre, else
//            labels[parent[j]].  counts = {centres, roots, rows left out}.
//   The minimum of a strict order and integer sums: a function of the distances and the densities alone, the same bits on every run.
//
// The launches (the device form reads nothing back and allocates nothing):
//   dbscan_degree_dev          (dbscan.hip, through self_tile.h) the hits of every row at eps, when no density is given; then
//   density_peaks_degree_kernel  1 + cnt as a double
//   density_peaks_key_kernel   a u64 key a row, ascending key = descending density (-0 as +0, a NaN all ones: last), the row index the
//                              value, and the number of rows kept; radix_sort_pairs_u64 over 64 bits, stable: perm[q], the row at
//                              POSITION q of the rank order -- equal densities keep their row order, which is the rank's tie rule
//   density_peaks_sweep_kernel THE SWEEP, in rank order: the row at position q needs only the columns at positions < q.  THE TRIANGLE,
//                              in which every row owns its own minimum: half the pairs of the rectangle, no cross-strip update, no atomic,
//                              no second pass.  A workgroup owns a STRIP of TJ consecutive positions and a SEGMENT of the column tiles
//                              0 .. the strip's own; both operands are gathered (PairRowsAt over perm, the strip's rows from LDS), both
//                              tile shapes of self_shape, the pipelined steps of pair_sweep_tile.  A pair is a candidate iff its column
//                              position is below its row position and its distance is a number; a thread keeps, for each of its TY rows,
//                              the least (distance key, perm[column]) -- the ROW INDEX, not the position; a row's lanes meet in
//                              reduce_row_lanes with key_at_min; one (key, index) a row and segment leaves the workgroup
//   density_peaks_merge_kernel the minimum over a row's segments; delta and parent at perm[q]; the rows left out
//   density_peaks_flags_kernel the centres, the first labels (a centre itself, any other row its parent) and the three counts
//   density_peaks_jump_kernel  pointer doubling between two buffers, ceil(log2 r1) rounds; a round returns at once when the one before
//                              changed nothing (both buffers then hold the labels)
// THE LOAD: a late strip walks more column tiles than an early one.  The walk is cut at the same tile numbers for every strip
// (class_linkage.hip's balance): a segment that begins behind the strip's walk returns before it loads anything, so the workgroups that
// run are of one size, and the longest strips are launched first.  Segments write disjoint slots, cleared to "none" by one memset.
// THE WORKSPACE is O(r1): 12 bytes a row and segment (16 at most), the sort's buffers, two label buffers, and dbscan's for the degrees.
// No known_rows: a new row changes degrees; after kpop_refset_append the call is made again in full.
//
// kpop_density_peaks_cut: the cut alone, host arithmetic (no GPU, no kpop_init), so that the thresholds can be chosen after a look at
// (density, delta).
#include <algorithm>
#include <vector>

#include "class_tiles.h"  // (the sweep's tile limits kSilMaxW / kSilMaxTJ and sil_nan: one sweep shape)
#include "common.h"
#include "distance_routes.h"
#include "radix_sort.h"
#include "refset_call.h"
#include "self_tile.h"

namespace kpop {

constexpr uint32_t kPeakMaxSeg = 16;
constexpr uint32_t kPeakNone = 0xFFFFFFFFu;  // KPOP_NOISE; no candidate's index
constexpr uint64_t kPeakNoKey = ~0ull;       // no candidate (distance_key gives it to nothing but a NaN), and a NaN density's sort key
constexpr uint32_t kPeakMaxRounds = 32;

// how a strip's walk is cut: tiles_per_seg column tiles a segment, the same cuts for every strip; never more segments than column
// tiles.  A function of r1 alone
struct PeakSegments {
  uint32_t n_seg, tiles_per_seg;
};
static PeakSegments density_peaks_segments(uint32_t r1) {
  const SelfShape s = self_shape(r1);
  const uint32_t n_ct = std::max(1u, div_up(r1, s.w));
  const uint32_t per = div_up(n_ct, std::min(kPeakMaxSeg, n_ct));
  return PeakSegments{div_up(n_ct, per), per};
}

// density, delta [r1], parent [r1]: the outputs the body needs itself, used where the caller passes NULL; key, val: the sort's two
// buffers each; scal: [0] the rows kept, [1 .. 3] the counts when nobody wants them, [8 .. 40) a round's "changed"; seg_key, seg_idx
// [kPeakMaxSeg][r1]: what the sweep leaves, by POSITION; lab: the two label buffers; rest: the sort's scratch, then dbscan's workspace
struct PeakWork {
  double *density, *delta;
  uint32_t *parent, *val[2], *scal, *seg_idx, *lab[2];
  uint64_t *key[2], *seg_key;
  void *sort, *degree;
  uint64_t seg_off, seg_bytes, bytes;
};
static PeakWork density_peaks_carve(void *base, uint32_t r1) {
  const uint64_t n = std::max(r1, 1u);
  Carver c(base);
  PeakWork f;
  f.density = c.take<double>(n * 8);
  f.delta = c.take<double>(n * 8);
  f.parent = c.take<uint32_t>(n * 4);
  for (int b = 0; b < 2; ++b) f.key[b] = c.take<uint64_t>(n * 8);
  for (int b = 0; b < 2; ++b) f.val[b] = c.take<uint32_t>(n * 4);
  f.scal = c.take<uint32_t>(256);
  f.seg_off = c.off;
  f.seg_key = c.take<uint64_t>(n * kPeakMaxSeg * 8);
  f.seg_idx = c.take<uint32_t>(n * kPeakMaxSeg * 4);
  f.seg_bytes = c.off - f.seg_off;
  for (int b = 0; b < 2; ++b) f.lab[b] = c.take<uint32_t>(n * 4);
  f.sort = c.take<void>(radix_scratch_bytes(n));
  f.degree = c.take<void>(dbscan_degree_workspace_bytes(r1));
  f.bytes = c.off;
  return f;
}

static dim3 density_peaks_rows_grid(uint32_t n) { return dim3(std::min(div_up(std::max(n, 1u), 256), 4096u)); }

__global__ __launch_bounds__(256) void density_peaks_degree_kernel(const uint32_t *__restrict__ cnt, uint32_t n, double *__restrict__ density) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) density[i] = (double)(cnt[i] + 1u);
}

// ascending key = descending density; a NaN all ones, which no number maps to (f64_key is zero for nothing but a NaN's bits).  *kept:
// the rows whose density is a number, an integer sum
__global__ __launch_bounds__(256) void density_peaks_key_kernel(const double *__restrict__ density, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                                uint32_t *__restrict__ kept) {
  __shared__ uint32_t s_kept;
  if (threadIdx.x == 0) s_kept = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    double x = density[i];
    if (x == 0.0) x = 0.0;
    const bool is = x == x;
    key[i] = is ? ~f64_key(x) : kPeakNoKey;
    val[i] = (uint32_t)i;
    mine += is ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_kept, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_kept) atomicAdd(kept, s_kept);
}

// a: the set's rows as the chain reads them, both operands.  Strip gridDim.x - 1 - blockIdx.x (the longest walks first): positions
// q0 .. q0 + TJ of the rank order perm, TJ = TY n_rg; a thread 4 columns x TY rows, n_cg n_rg = 256.  Segment blockIdx.y: column tiles
// blockIdx.y tiles_per_seg onwards, held to the strip's walk -- the tiles with a position below the strip's last.  *kept: the rows of
// the rank order (the rest were left out).  seg_key, seg_idx [gridDim.y][r1], by position, cleared to all ones before the launch
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void density_peaks_sweep_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, uint32_t n_dims,
                                                                     const double *__restrict__ metric, double p, uint32_t n_cg, uint32_t n_rg,
                                                                     const uint32_t *__restrict__ perm, const uint32_t *__restrict__ kept, uint32_t tiles_per_seg,
                                                                     uint64_t *__restrict__ seg_key, uint32_t *__restrict__ seg_idx) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kSilMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kSilMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_row[kSilMaxTJ];  // the strip's rows
  const uint32_t TJ = TY * n_rg;
  const uint32_t strip = gridDim.x - 1 - blockIdx.x;
  const uint32_t q0 = strip * TJ, n_in = min(*kept, r1);
  if (q0 >= n_in) return;
  const uint32_t q1 = min(n_in, q0 + TJ);
  const uint32_t col_end = q1 - 1;  // the columns of the strip: the positions below its last row's
  const uint32_t walk_end = col_end / w + (col_end % w ? 1u : 0u);
  const uint32_t seg = blockIdx.y;
  const uint32_t t_begin = min(seg * tiles_per_seg, walk_end), t_end = min(t_begin + tiles_per_seg, walk_end);
  if (t_begin >= t_end) return;  // (the same for every thread of the workgroup; its slots keep "none")
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const uint32_t ti = cg * 4, tj = rg * TY;
  for (uint32_t n = threadIdx.x; n < kSilMaxTJ; n += 256) s_row[n] = (n < TJ && q0 + n < q1) ? min(perm[q0 + n], r1 - 1) : kPeakNone;
  __syncthreads();  // (s_row is the strip's index list: the first load reads it)
  uint64_t min_k[TY];
  uint32_t min_c[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    min_k[yy] = kPeakNoKey;
    min_c[yy] = kPeakNone;
  }
  const PairRowsAt cols{a, r1, perm}, rows{a, r1, s_row};
  const uint32_t n_strip = q1 - q0;
  const PairTilesOf tiles{w, (uint32_t)min((uint64_t)col_end, (uint64_t)t_end * w)};
  PairStage<kSilMaxW, kSilMaxTJ> stage;
  PairTile cur = tiles.at(t_begin * w), nxt;
  for (pair_sweep_open(stage, cols, cur, rows, 0u, n_strip, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = tiles.after(cur);
    uint32_t ri[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) ri[x] = (cur.i0 + ti + x < cur.i1) ? perm[cur.i0 + ti + x] : kPeakNone;
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, cols, cur, nxt, rows, 0u, n_strip, n_dims, metric, p, ti, tj, true);
    // a candidate: inside the tile, a position below the row's, a distance that is a number.  The rank order is not the row order:
    // among equal keys the smaller ROW INDEX wins, whichever column comes first
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t q = q0 + tj + yy;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t c = cur.i0 + ti + x;
        if (c < cur.i1 && c < q && d == d) {
          const uint64_t k = distance_key(d);
          if (key_less(k, ri[x], min_k[yy], min_c[yy])) {
            min_k[yy] = k;
            min_c[yy] = ri[x];
          }
        }
      }
    }
  }
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t q = q0 + tj + yy;
    const KeyAt least = reduce_row_lanes(KeyAt{min_k[yy], min_c[yy]}, n_cg, key_at_min);
    if (cg == 0 && q < q1) {
      seg_key[(uint64_t)seg * r1 + q] = least.k;
      seg_idx[(uint64_t)seg * r1 + q] = least.c;
    }
  }
}

// position q of the rank order: the least over its segments, written at perm[q]; beyond the rows kept: the rows left out
__global__ __launch_bounds__(256) void density_peaks_merge_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ kept, uint32_t r1, uint32_t n_seg,
                                                                  const uint64_t *__restrict__ seg_key, const uint32_t *__restrict__ seg_idx, double *__restrict__ delta,
                                                                  uint32_t *__restrict__ parent) {
  const uint32_t n_in = min(*kept, r1);
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < r1; q += (uint64_t)gridDim.x * 256) {
    const uint32_t row = min(perm[q], r1 - 1);
    if (q >= n_in) {
      delta[row] = sil_nan();
      parent[row] = kPeakNone;
      continue;
    }
    KeyAt best{kPeakNoKey, kPeakNone};
    for (uint32_t sg = 0; sg < n_seg; ++sg) best = key_at_min(best, KeyAt{seg_key[(uint64_t)sg * r1 + q], seg_idx[(uint64_t)sg * r1 + q]});
    const bool any = best.k != kPeakNoKey && best.c < r1;
    delta[row] = any ? key_f64(best.k) : __longlong_as_double(0x7FF0000000000000ll);
    parent[row] = any ? best.c : row;
  }
}

// the centres, the labels before the first round (lab may be null) and the three counts, integer sums
__global__ __launch_bounds__(256) void density_peaks_flags_kernel(const double *__restrict__ density, const double *__restrict__ delta, const uint32_t *__restrict__ parent,
                                                                  uint32_t r1, double min_density, double min_delta, uint32_t *__restrict__ lab,
                                                                  uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_n[3];
  if (threadIdx.x < 3) s_n[threadIdx.x] = 0;
  __syncthreads();
  uint32_t centres = 0, roots = 0, out = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t par = parent[i];
    uint32_t l = kPeakNone;
    if (par == kPeakNone) ++out;
    else {
      const bool root = par == (uint32_t)i;
      const bool centre = root || (delta[i] > min_delta && density[i] >= min_density);
      roots += root ? 1u : 0u;
      centres += centre ? 1u : 0u;
      l = centre ? (uint32_t)i : par;
    }
    if (lab) lab[i] = l;
  }
  if (centres) atomicAdd(&s_n[0], centres);
  if (roots) atomicAdd(&s_n[1], roots);
  if (out) atomicAdd(&s_n[2], out);
  __syncthreads();
  if (threadIdx.x < 3 && s_n[threadIdx.x]) atomicAdd(counts + threadIdx.x, s_n[threadIdx.x]);
}

// one round of pointer doubling, src -> dst (never in place: other threads read src).  A centre points at itself, a row left out at
// nothing.  changed[round] is set when a label moved; a round whose predecessor moved none returns at once: src and dst are then equal
__global__ __launch_bounds__(256) void density_peaks_jump_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t r1, uint32_t round,
                                                                 uint32_t *__restrict__ changed) {
  if (round > 0 && changed[round - 1] == 0) return;
  bool moved = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    const uint32_t l = src[i];
    const uint32_t next = l < r1 ? src[l] : l;
    dst[i] = next;
    moved = moved || next != l;
  }
  if (__syncthreads_or(moved) && threadIdx.x == 0) atomicOr(changed + round, 1u);
}

static int density_peaks_check(double eps, bool given, double min_density, double min_delta, const char *who) {
  if (min_density != min_density || min_delta != min_delta) KPOP_FAIL(KPOP_ERR_INVALID, "%s: a threshold is not a number", who);
  if (!given && eps != eps) KPOP_FAIL(KPOP_ERR_INVALID, "%s: eps is not a number and no density is given", who);
  return 0;
}

static uint32_t density_peaks_rounds(uint32_t r1) {
  uint32_t rounds = 0;
  while (rounds < kPeakMaxRounds && (1ull << rounds) < r1) ++rounds;
  return rounds;
}

// the body of both entry points: enqueues only.  The arguments are checked, r1 > 0
static int density_peaks_dev(kpop_refset *rs, double eps, const double *d_density, double min_density, double min_delta, void *d_work, double *d_density_out,
                             double *d_delta, uint32_t *d_parent, uint32_t *d_labels, uint32_t *d_counts, hipStream_t st) {
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  const SelfShape s = self_shape(r1);
  const PeakSegments g = density_peaks_segments(r1);
  const PeakWork f = density_peaks_carve(d_work, r1);
  const dim3 rows_grid = density_peaks_rows_grid(r1);
  KPOP_HIP(hipMemsetAsync(f.scal, 0, 256, st));
  if (d_counts) KPOP_HIP(hipMemsetAsync(d_counts, 0, 12, st));
  const double *density = d_density;
  if (!density) {
    const uint32_t *cnt;
    KPOP_TRY(dbscan_degree_dev(rs, eps, f.degree, &cnt, st));
    double *out = d_density_out ? d_density_out : f.density;
    density_peaks_degree_kernel<<<rows_grid, dim3(256), 0, st>>>(cnt, r1, out);
    KPOP_LAUNCH_CHECK();
    density = out;
  } else if (d_density_out) {
    KPOP_HIP(hipMemcpyAsync(d_density_out, d_density, (uint64_t)r1 * 8, hipMemcpyDeviceToDevice, st));
  }
  density_peaks_key_kernel<<<rows_grid, dim3(256), 0, st>>>(density, r1, f.key[0], f.val[0], f.scal);
  KPOP_LAUNCH_CHECK();
  uint64_t *keys;
  uint32_t *perm;
  KPOP_TRY(radix_sort_pairs_u64(f.key[0], f.key[1], f.val[0], f.val[1], r1, 64, f.sort, st, &keys, &perm));
  const double *a;  // both operands
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  KPOP_HIP(hipMemsetAsync(reinterpret_cast<char *>(d_work) + f.seg_off, 0xFF, f.seg_bytes, st));
  const dim3 grid(div_up(r1, s.TJ), g.n_seg);
  KPOP_TRY(by_kind(rs->kind, [&](auto K) -> int {
    by_shape_rows(s, [&](auto TY) {
      density_peaks_sweep_kernel<decltype(K)::value, decltype(TY)::value><<<grid, dim3(256), 0, st>>>(a, s.w, r1, D, rs->metric, rs->p, s.n_cg, s.n_rg, perm, f.scal,
                                                                                                     g.tiles_per_seg, f.seg_key, f.seg_idx);
    });
    KPOP_LAUNCH_CHECK();
    return 0;
  }));
  double *delta = d_delta ? d_delta : f.delta;
  uint32_t *parent = d_parent ? d_parent : f.parent;
  density_peaks_merge_kernel<<<rows_grid, dim3(256), 0, st>>>(perm, f.scal, r1, g.n_seg, f.seg_key, f.seg_idx, delta, parent);
  KPOP_LAUNCH_CHECK();
  if (!d_labels && !d_counts) return KPOP_OK;
  density_peaks_flags_kernel<<<rows_grid, dim3(256), 0, st>>>(density, delta, parent, r1, min_density, min_delta, d_labels ? f.lab[0] : nullptr,
                                                              d_counts ? d_counts : f.scal + 1);
  KPOP_LAUNCH_CHECK();
  if (!d_labels) return KPOP_OK;
  const uint32_t rounds = density_peaks_rounds(r1);
  for (uint32_t t = 0; t < rounds; ++t) {
    density_peaks_jump_kernel<<<rows_grid, dim3(256), 0, st>>>(f.lab[t & 1], f.lab[(t + 1) & 1], r1, t, f.scal + 8);
    KPOP_LAUNCH_CHECK();
  }
  KPOP_HIP(hipMemcpyAsync(d_labels, f.lab[rounds & 1], (uint64_t)r1 * 4, hipMemcpyDeviceToDevice, st));
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_density_peaks_workspace_bytes(const kpop_refset *rs) {
  if (!rs) return 0;
  return density_peaks_carve(nullptr, rs->r1).bytes;
}

extern "C" int kpop_dev_density_peaks(kpop_refset *rs, double eps, const double *d_density, double min_density, double min_delta, void *d_work,
                                      double *d_density_out, double *d_delta, uint32_t *d_parent, uint32_t *d_labels, uint32_t *d_counts, void *stream) {
  const char *who = "kpop_dev_density_peaks";
  KPOP_TRY(refset_check_handle(rs, who));
  KPOP_TRY(density_peaks_check(eps, d_density != nullptr, min_density, min_delta, who));
  if (rs->r1 == 0) {
    if (d_counts) KPOP_HIP(hipMemsetAsync(d_counts, 0, 12, as_stream(stream)));
    return KPOP_OK;
  }
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return density_peaks_dev(rs, eps, d_density, min_density, min_delta, d_work, d_density_out, d_delta, d_parent, d_labels, d_counts, as_stream(stream));
}

extern "C" int kpop_density_peaks(kpop_refset *rs, double eps, const double *density, double min_density, double min_delta, double *density_out, double *delta,
                                  uint32_t *parent, uint32_t *labels, uint32_t *counts) {
  const char *who = "kpop_density_peaks";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(density_peaks_check(eps, density != nullptr, min_density, min_delta, who));
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  const uint32_t r1 = rs->r1;
  if (r1 == 0) return KPOP_OK;
  HostCall h;
  void *work = h.work(density_peaks_carve(nullptr, r1).bytes);
  const double *dd = density ? h.in(density, r1) : nullptr;
  double *d_out = h.out(density_out, r1), *d_delta = h.out(delta, r1);
  uint32_t *d_parent = h.out(parent, r1), *d_labels = h.out(labels, r1), *d_counts = counts ? h.scalars(counts, 3) : nullptr;
  KPOP_TRY(h.upload());
  KPOP_TRY(density_peaks_dev(rs, eps, dd, min_density, min_delta, work, d_out, d_delta, d_parent, d_labels, d_counts, h.st));
  return h.finish();
}

extern "C" int kpop_distance_density_peaks(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize, double eps,
                                           const double *density, double min_density, double min_delta, double *density_out, double *delta, uint32_t *parent,
                                           uint32_t *labels, uint32_t *counts) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_density_peaks(rs, eps, density, min_density, min_delta, density_out, delta, parent, labels, counts);
  });
}

// host arithmetic alone: no GPU, no kpop_init.  A parent is KPOP_NOISE (the row is left out), the row itself (a root) or a row that
// ranks strictly above it -- checked for every row before anything is written, which is what rules a cycle out.  A label is found by
// walking up to a centre or to a row that has its label, and given to the rows of the walk
extern "C" int kpop_density_peaks_cut(uint32_t r1, const double *density, const double *delta, const uint32_t *parent, double min_density, double min_delta,
                                      uint32_t *labels, uint32_t *counts) {
  const char *who = "kpop_density_peaks_cut";
  if (min_density != min_density || min_delta != min_delta) KPOP_FAIL(KPOP_ERR_INVALID, "%s: a threshold is not a number", who);
  if (r1 && (!density || !delta || !parent)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  for (uint32_t j = 0; j < r1; ++j) {
    const uint32_t i = parent[j];
    if (i == KPOP_NOISE || i == j) continue;
    if (i >= r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: parent[%u] = %u in a set of %u rows", who, j, i, r1);
    if (!(density[i] > density[j] || (density[i] == density[j] && i < j)))
      KPOP_FAIL(KPOP_ERR_INVALID, "%s: parent[%u] = %u does not rank above its child (a higher density, or an equal one and a smaller index)", who, j, i);
  }
  uint32_t n[3] = {0, 0, 0};
  std::vector<uint8_t> centre(r1, 0);
  for (uint32_t j = 0; j < r1; ++j) {
    if (parent[j] == KPOP_NOISE) {
      ++n[2];
      continue;
    }
    const bool root = parent[j] == j;
    centre[j] = root || (delta[j] > min_delta && density[j] >= min_density);
    n[1] += root ? 1u : 0u;
    n[0] += centre[j] ? 1u : 0u;
  }
  if (counts) std::copy(n, n + 3, counts);
  if (!labels) return KPOP_OK;
  std::vector<uint8_t> done(r1, 0);
  std::vector<uint32_t> walk;
  for (uint32_t j = 0; j < r1; ++j) {
    if (done[j]) continue;
    walk.clear();
    uint32_t at = j, label;
    for (;;) {
      if (parent[at] == KPOP_NOISE) {  // a row left out, and whoever was handed one as a parent
        label = KPOP_NOISE;
        walk.push_back(at);
        break;
      }
      if (done[at]) {
        label = labels[at];
        break;
      }
      walk.push_back(at);
      if (centre[at]) {
        label = at;
        break;
      }
      at = parent[at];
    }
    for (const uint32_t x : walk) {
      labels[x] = label;
      done[x] = 1;
    }
  }
  return KPOP_OK;
}
