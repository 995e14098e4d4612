// representatives.hip -- representatives at a distance: the greedy cover of a resident set in row order (leader clustering, the
// dereplication step), which is the lexicographically first maximal independent set of the threshold graph.
//
//   The graph of clusters.hip: the set's r1 rows, d(j, i) the reference chain's distance (lib/Space.ml:182-205 with the adaptors of
//   lib/Matrix.ml:243-250), symmetric bit for bit, a NaN within nothing; no kpop_tune setting is read.  Row i is a representative iff
//   no representative r < i has d(i, r) <= max_distance; every other row is assigned to the representative BELOW it that is least
//   under (d with -0 taken as +0, r).  The result is defined without reference to an algorithm: the same bits on every run.
//
// What no other kernel here has is the dependence of a row on the rows before it.  It is confined to steps of kRepStep consecutive
// rows, and inside a step to one wavefront that does no arithmetic.  The state lives in the workspace: reps[], the representatives'
// row indices ascending, and the device word n_reps.  A step over rows js .. je:
//   representatives_cover_kernel    the step's rows against reps[0 .. n0), n0 read from the device word (the grid is fixed, the tile
//                                   bounds come from the word, clamped to the capacity the workspace was sized for).
//                                   A workgroup owns a strip of rows (the self-join's tile shapes, tri_tile.h) and a segment of
//                                   the column tiles, every thread keeps the best (key, position in reps) of its rows, the lanes of a
//                                   row reduce with shuffles (self_tile.h), one store a row and segment.  The columns are gathered rows: the
//                                   indexed row view of pair_tile.h (PairRowsAt) -- no compacted copy of the representatives' rows is kept.
//                                   Positions ascend with the row index, so (key, position) orders as (d, r)
//   representatives_row_min_kernel  the least of a row's segments; key none: not covered
//   representatives_hits_kernel     a tile's distances and compare (self_tile.h) over the lower triangle of the step's rows against themselves,
//                                   a row tile whose rows are all covered skipped: the bit matrix H[j][i], i < j, d(j, i) <= T
//   representatives_resolve_kernel  the sequential part, one wavefront: the rows that are not covered, ascending; lane l holds bits
//                                   32 l .. 32 l + 32 of the set chosen in this step, a row is chosen iff H[row] & chosen is empty --
//                                   one load, one AND and one ballot a row, the loads (which do not depend on the state) sixteen
//                                   rows ahead.  The chosen rows are appended to reps[] in order
//   representatives_cover_kernel    again, over reps[n0 .. n1) with the condition representative < row: a representative chosen
//                                   inside the step may be nearer than an older one
//   representatives_row_min_kernel  merges the two under (key, position) and writes rep_of and rep_dist of the step's rows
// known_rows > 0: reps[] is first rebuilt from the incoming rep_of[0 .. known_rows) by an ordered compaction (scan.h), and the first
// step starts at known_rows.  max_distance < 0: no tile kernel runs.  Nothing synchronises, nothing is read back: the host knows
// the number of steps, ceil((r1 - known_rows) / kRepStep), and the host form enqueues what the device form enqueues.
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "refset_call.h"
#include "scan.h"
#include "self_tile.h"

namespace kpop {

constexpr int kRepMaxW = 64, kRepMaxTJ = 256, kRepMaxSeg = 64;
constexpr uint32_t kRepStep = 2048;            // rows a step: a power of two
constexpr uint32_t kRepHWords = kRepStep / 32;  // 32-bit words a row of H: one a lane of the resolving wavefront
constexpr uint64_t kRepNone = ~0ull;           // (no key: distance_key maps only a NaN's bits there, and a NaN is never a key)
static_assert(kRepHWords == 64, "the resolving wavefront holds a word of the chosen set a lane");

// words[0]: n_reps; words[1]: what it was before the step's resolve (n0)
struct RepWork {
  uint32_t *words, *chosen, *reps, *part_c, *best_c, *H;
  uint64_t *part_k, *best_k, *sums;
  uint64_t bytes;
};

static RepWork representatives_carve(void *base, uint32_t r1) {
  const uint64_t n = std::max(r1, 1u);
  Carver c(base);
  RepWork f;
  f.words = c.take<uint32_t>(256);
  f.chosen = c.take<uint32_t>(4 * kRepHWords);
  f.reps = c.take<uint32_t>(n * 4);
  f.part_k = c.take<uint64_t>((uint64_t)kRepMaxSeg * kRepStep * 8);
  f.part_c = c.take<uint32_t>((uint64_t)kRepMaxSeg * kRepStep * 4);
  f.best_k = c.take<uint64_t>((uint64_t)kRepStep * 8);
  f.best_c = c.take<uint32_t>((uint64_t)kRepStep * 4);
  f.H = c.take<uint32_t>((uint64_t)kRepStep * kRepHWords * 4);
  f.sums = c.take<uint64_t>((scan_blocks(n) + 1) * 8);
  f.bytes = c.off;
  return f;
}

// the ordered compaction of the known rows: row i is a representative iff rep_of[i] == i
struct RepIsOwn {
  const uint32_t *rep_of;
  __device__ uint32_t operator()(uint64_t i) const { return rep_of[i] == (uint32_t)i ? 1u : 0u; }
};
struct RepAppend {
  uint32_t *reps;
  uint32_t cap;
  __device__ void operator()(uint64_t i, uint64_t pre, uint32_t v) const {
    if (v && pre < cap) reps[pre] = (uint32_t)i;
  }
};

__global__ void representatives_known_count_kernel(const uint64_t *__restrict__ total, uint32_t cap, uint32_t *__restrict__ words) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    words[0] = (uint32_t)min(*total, (uint64_t)cap);
    words[1] = words[0];
  }
}

// max_distance below zero: every row from known_rows on is its own representative (reps[] is not needed any more)
__global__ __launch_bounds__(256) void representatives_alone_kernel(uint32_t known_rows, uint32_t r1, uint32_t *__restrict__ rep_of,
                                                                    double *__restrict__ rep_dist, uint32_t *__restrict__ words) {
  for (uint64_t i = (uint64_t)known_rows + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < r1; i += (uint64_t)gridDim.x * 256) {
    rep_of[i] = (uint32_t)i;
    if (rep_dist) rep_dist[i] = 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) words[0] = min(words[0], known_rows) + (r1 - known_rows);
}

// a: the set's rows as the chain reads them (divided by their norms when the set normalises), both operands; cap: its rows.  Strip
// blockIdx.x: rows j0 .. j0 + TJ of the step js .. je, TJ = TY n_rg; segment blockIdx.y of gridDim.y: its share of the column tiles,
// w positions of reps[lo .. hi) each -- lo = 0, hi = n_reps (newer = 0: the representatives before the step), or lo = the count
// before the step's resolve, hi = n_reps (newer = 1: those the step chose, of which only the ones below a row are eligible to it).
// A thread 4 columns x TY rows, the dimensions ascending in one thread, 16 at a time through LDS: the steps of pair_tile.h's sweep.
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void representatives_cover_kernel(const double *__restrict__ a, uint32_t cap, uint32_t w, uint32_t n_dims,
                                                                       const double *__restrict__ metric, double p, double max_distance, uint32_t n_cg,
                                                                       uint32_t n_rg, uint32_t js, uint32_t je, const uint32_t *__restrict__ words,
                                                                       int newer, const uint32_t *__restrict__ reps, uint64_t *__restrict__ part_k,
                                                                       uint32_t *__restrict__ part_c) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kRepMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kRepMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  const uint32_t TJ = TY * n_rg;
  const uint32_t strip = blockIdx.x, seg = blockIdx.y, n_seg = gridDim.y;
  const uint32_t j0 = js + strip * TJ;
  if (j0 >= je) return;  // (the last step is ragged)
  const uint32_t j1 = min(je, j0 + TJ);
  // the bounds that come from device memory, held to the capacity: a word that was never written walks nobody out of reps[]
  const uint32_t hi = min(words[0], cap), lo = newer ? min(words[1], hi) : 0u;
  const uint32_t n_ct = (hi - lo + w - 1) / w, tiles_per_seg = (n_ct + n_seg - 1) / n_seg;
  const uint32_t t_begin = min(n_ct, seg * tiles_per_seg), t_end = min(n_ct, t_begin + tiles_per_seg);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const bool worker = rg < n_rg;
  const uint32_t ti = cg * 4, tj = (worker ? rg : 0) * TY;
  uint32_t best_c[TY];
  uint64_t best_k[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    best_k[yy] = kRepNone;
    best_c[yy] = 0u;
  }
  // (the sweep's steps written out, with its one call of load a step: on pair_sweep_tile this kernel has the same registers and
  // instructions within two, and the call ran 1 to 4 % slower; profiles/pair_sweep_refactor.md, section 4)
  const PairRowsAt cols{a, cap, reps};
  const PairRows rows{a, cap};
  PairStage<kRepMaxW, kRepMaxTJ> stage;
  if (t_begin < t_end) stage.load(cols, lo + t_begin * w, min(hi, lo + t_begin * w + w), rows, j0, j1, n_dims, 0, n_dims);
  for (uint32_t t = t_begin; t < t_end; ++t) {
    const uint32_t i0 = lo + t * w, i1 = min(hi, i0 + w);  // positions in reps
    uint32_t ri[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) ri[x] = (i0 + ti + x < i1) ? reps[i0 + ti + x] : 0xFFFFFFFFu;
    double acc[TY][4];
    pair_zero(acc);
    for (uint32_t c0 = 0; c0 < n_dims; c0 += kPairDC) {
      __syncthreads();
      stage.store(As, Bs, s_metric, metric, c0, n_dims);
      __syncthreads();
      const bool more = c0 + kPairDC < n_dims;  // this tile's next dimensions, or the next tile's first
      const uint32_t ni0 = more ? i0 : i0 + w;
      if (more || t + 1 < t_end) stage.load(cols, ni0, min(hi, ni0 + w), rows, j0, j1, n_dims, more ? c0 + kPairDC : 0u, n_dims);
      if (worker) pair_accumulate<KIND>(acc, As, Bs, s_metric, ti, tj, min((uint32_t)kPairDC, n_dims - c0), p);
    }
    // the epilogue: the scaled distance against the bound (a NaN compares false: within nothing); a representative below the
    // row only.  Positions ascend within the tile and from tile to tile, so that `below` alone keeps, among equal keys, the least
    if (worker) {
#pragma unroll
      for (int yy = 0; yy < TY; ++yy)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const double d = scale_distance<KIND>(acc[yy][x], p);
          const uint32_t j = j0 + tj + yy;
          if (j < j1 && ri[x] < j && d <= max_distance) {
            const uint64_t key = distance_key(d);
            if (key < best_k[yy]) {
              best_k[yy] = key;
              best_c[yy] = i0 + ti + x;
            }
          }
        }
    }
  }
  // the least (key, position) over a row's lanes
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const KeyAt best = reduce_row_lanes(KeyAt{best_k[yy], best_c[yy]}, n_cg, key_at_min);
    const uint32_t j = j0 + tj + yy;
    if (worker && cg == 0 && j < j1) {
      part_k[(uint64_t)seg * kRepStep + (j - js)] = best.k;
      part_c[(uint64_t)seg * kRepStep + (j - js)] = best.c;
    }
  }
}

// the segments hold ascending positions: among equal keys the first segment's.  last = 0: the step's rows against the representatives
// before it -> best_k, best_c.  last = 1: the parts are those of the step's own representatives, whose positions lie behind every
// older one; merged with best under (key, position), and the step's rows written: a chosen row stands for itself at +0, any other
// row has a key (what left it out of the chosen set is a hit that the cover found again, the same bits)
__global__ __launch_bounds__(256) void representatives_row_min_kernel(const uint64_t *__restrict__ part_k, const uint32_t *__restrict__ part_c, uint32_t n_seg,
                                                                      uint32_t js, uint32_t je, uint32_t cap, uint64_t *__restrict__ best_k,
                                                                      uint32_t *__restrict__ best_c, int last, const uint32_t *__restrict__ chosen,
                                                                      const uint32_t *__restrict__ reps, uint32_t *__restrict__ rep_of,
                                                                      double *__restrict__ rep_dist) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= je - js) return;
  uint64_t k = part_k[r];
  uint32_t c = part_c[r];
  for (uint32_t s = 1; s < n_seg; ++s) {
    const uint64_t kk = part_k[(uint64_t)s * kRepStep + r];
    if (kk < k) {
      k = kk;
      c = part_c[(uint64_t)s * kRepStep + r];
    }
  }
  if (!last) {
    best_k[r] = k;
    best_c[r] = c;
    return;
  }
  if (best_k[r] <= k) {
    k = best_k[r];
    c = best_c[r];
  }
  const bool own = ((chosen[r / 32] >> (r % 32)) & 1u) || k == kRepNone;
  rep_of[js + r] = own ? js + r : reps[min(c, cap - 1)];
  if (rep_dist) rep_dist[js + r] = own ? 0.0 : key_f64(k);
}

// a: as above, both operands.  Tile blockIdx.x, blockIdx.y of the step's rows js .. je against themselves: w columns from
// js + blockIdx.x w, TJ = TY n_rg rows from js + blockIdx.y TJ; the lower triangle only, and no row tile whose rows are all covered
// (best_k has a key): nobody reads their rows of H.  A thread 4 columns x TY rows: the tile of self_tile.h.  H: a row
// kRepHWords words of 32 bits, bit i - js of row j - js set iff i < j and d(j, i) <= max_distance; a tile writes all the words
// of its rows that it covers, zero bits included, so that H needs no clearing
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void representatives_hits_kernel(const double *__restrict__ a, uint32_t w, uint32_t n_dims, const double *__restrict__ metric,
                                                                      double p, double max_distance, uint32_t n_cg, uint32_t n_rg, uint32_t js, uint32_t je,
                                                                      const uint64_t *__restrict__ best_k, uint32_t *__restrict__ H) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kRepMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kRepMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  const uint32_t TJ = TY * n_rg;
  const uint32_t i0 = js + blockIdx.x * w, j0 = js + blockIdx.y * TJ;
  if (j0 >= je) return;
  const uint32_t j1 = min(je, j0 + TJ);
  if (i0 + 1 >= j1) return;  // no column below the tile's last row
  const uint32_t i1 = min(je, i0 + w);
  bool open = false;
  for (uint32_t n = threadIdx.x; n < j1 - j0; n += 256) open = open || best_k[j0 - js + n] == kRepNone;
  if (!__syncthreads_or(open)) return;
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const bool worker = rg < n_rg;
  const uint32_t ti = cg * 4, tj = (worker ? rg : 0) * TY;
  double acc[TY][4];
  const PairRows rows{a, je};  // (a plain view never reads its row count; what this kernel knows of it: the step's rows end at je)
  pair_tile_distances<KIND, TY, kRepMaxW, kRepMaxTJ>(acc, As, Bs, s_metric, rows, i0, i1, rows, j0, j1, n_dims, metric, p, ti, tj, worker);
  const uint32_t mask = worker ? self_hit_mask<TY>(acc, TriTile{blockIdx.x, blockIdx.y, i0, i1, j0, j1, true}, ti, tj, max_distance) : 0u;
  // the epilogue: a thread's 4 columns are 4 bits of its row's word, OR-ed over the row's lanes
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t j = j0 + tj + yy;
    const uint64_t bits = reduce_row_lanes((uint64_t)((mask >> (4 * yy)) & 0xFu) << ti, n_cg, [](uint64_t x, uint64_t y) { return x | y; });
    if (worker && cg == 0 && j < j1) {
      uint32_t *row = H + (uint64_t)(j - js) * kRepHWords + (i0 - js) / 32;
      row[0] = (uint32_t)bits;
      if (w > 32) row[1] = (uint32_t)(bits >> 32);
    }
  }
}

// one wavefront.  The rows of the step that no earlier representative covers (best_k without a key) are listed ascending; then, in
// that order, a row is chosen iff its row of H holds no bit of a row chosen before it.  Lane l holds bits 32 l .. 32 l + 32 of the
// chosen set; the rows of H do not depend on it and are loaded sixteen ahead.  (A bit of H at or beyond the row's own column meets
// no chosen bit: only rows below it have been decided.)
__global__ __launch_bounds__(64) void representatives_resolve_kernel(const uint64_t *__restrict__ best_k, const uint32_t *__restrict__ H, uint32_t js,
                                                                     uint32_t je, uint32_t cap, uint32_t *__restrict__ words, uint32_t *__restrict__ reps,
                                                                     uint32_t *__restrict__ chosen_out) {
  __shared__ uint16_t s_list[kRepStep];
  const uint32_t lane = threadIdx.x, n = min(je - js, kRepStep);
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t r = base + lane;
    const bool open = r < n && best_k[r] == kRepNone;
    const uint64_t m = __ballot(open);
    if (open) s_list[cnt + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)r;
    cnt += (uint32_t)__popcll(m);
  }
  __syncthreads();
  const uint32_t n0 = min(words[0], cap);
  uint32_t chosen = 0, added = 0;
  for (uint32_t q0 = 0; q0 < cnt; q0 += 16) {
    uint32_t h[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) h[u] = H[(uint64_t)s_list[min(q0 + u, cnt - 1)] * kRepHWords + lane];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (q0 + u >= cnt) break;
      const uint32_t r = s_list[q0 + u];
      if (__ballot((h[u] & chosen) != 0) == 0) {
        if (lane == r / 32) chosen |= 1u << (r % 32);
        if (lane == 0 && n0 + added < cap) reps[n0 + added] = js + r;
        ++added;
      }
    }
  }
  chosen_out[lane] = chosen;
  if (lane == 0) {
    words[1] = n0;
    words[0] = min(n0 + added, cap);
  }
}

template <int KIND>
static int representatives_steps(const double *a, uint32_t r1, uint32_t n_dims, const double *metric, double p, double max_distance, uint32_t known_rows,
                                 const RepWork &f, uint32_t *rep_of, double *rep_dist, hipStream_t st) {
  const SelfShape sh = self_shape(r1);
  const uint32_t strips = kRepStep / sh.TJ, n_seg = std::min<uint32_t>(kRepMaxSeg, 512 / strips);  // two workgroups a CU, as the registers admit
  const dim3 cover_grid(strips, n_seg), hits_grid(kRepStep / sh.w, kRepStep / sh.TJ), rows_grid(kRepStep / 256);
  for (uint64_t s = known_rows; s < r1; s += kRepStep) {
    const uint32_t js = (uint32_t)s, je = (uint32_t)std::min<uint64_t>(r1, s + kRepStep);
    for (int last = 0; last < 2; ++last) {
      by_shape_rows(sh, [&](auto TY) {
        representatives_cover_kernel<KIND, decltype(TY)::value><<<cover_grid, dim3(256), 0, st>>>(a, r1, sh.w, n_dims, metric, p, max_distance, sh.n_cg, sh.n_rg, js, je,
                                                                                                 f.words, last, f.reps, f.part_k, f.part_c);
      });
      KPOP_LAUNCH_CHECK();
      representatives_row_min_kernel<<<rows_grid, dim3(256), 0, st>>>(f.part_k, f.part_c, n_seg, js, je, r1, f.best_k, f.best_c, last, f.chosen, f.reps, rep_of,
                                                                      rep_dist);
      KPOP_LAUNCH_CHECK();
      if (last) break;
      by_shape_rows(sh, [&](auto TY) {
        representatives_hits_kernel<KIND, decltype(TY)::value><<<hits_grid, dim3(256), 0, st>>>(a, sh.w, n_dims, metric, p, max_distance, sh.n_cg, sh.n_rg, js, je, f.best_k,
                                                                                               f.H);
      });
      KPOP_LAUNCH_CHECK();
      representatives_resolve_kernel<<<dim3(1), dim3(64), 0, st>>>(f.best_k, f.H, js, je, r1, f.words, f.reps, f.chosen);
      KPOP_LAUNCH_CHECK();
    }
  }
  return 0;
}

// the body of both entry points: enqueues only
static int representatives_dev(kpop_refset *rs, double max_distance, uint32_t known_rows, void *d_work, uint32_t *d_rep_of, double *d_rep_dist,
                               uint32_t *d_n_reps, hipStream_t st, const char *who) {
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!d_n_reps) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null count", who);
  if (known_rows > rs->r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u known rows in a set of %u", who, known_rows, rs->r1);
  const uint32_t r1 = rs->r1;
  if (r1 == 0) {
    KPOP_HIP(hipMemsetAsync(d_n_reps, 0, 4, st));
    return KPOP_OK;
  }
  if (!d_rep_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null rep_of", who);
  const RepWork f = representatives_carve(d_work, r1);
  if (known_rows) {
    KPOP_TRY(exclusive_scan(RepIsOwn{d_rep_of}, RepAppend{f.reps, r1}, known_rows, f.sums, st));
    representatives_known_count_kernel<<<dim3(1), dim3(64), 0, st>>>(f.sums + scan_blocks(known_rows), r1, f.words);
    KPOP_LAUNCH_CHECK();
  } else {
    KPOP_HIP(hipMemsetAsync(f.words, 0, 256, st));
  }
  if (known_rows < r1) {
    if (!(max_distance >= 0.0)) {  // (no distance is negative: below zero every row stands for itself)
      representatives_alone_kernel<<<dim3(std::min(div_up(r1 - known_rows, 256), 4096u)), dim3(256), 0, st>>>(known_rows, r1, d_rep_of, d_rep_dist, f.words);
      KPOP_LAUNCH_CHECK();
    } else {
      const double *a;
      KPOP_TRY(refset_chain_rows(rs, st, &a));
      KPOP_TRY(by_kind(rs->kind, [&](auto K) {
        return representatives_steps<decltype(K)::value>(a, r1, rs->n_dims, rs->metric, rs->p, max_distance, known_rows, f, d_rep_of, d_rep_dist, st);
      }));
    }
  }
  KPOP_HIP(hipMemcpyAsync(d_n_reps, f.words, 4, hipMemcpyDeviceToDevice, st));
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_representatives_within_workspace_bytes(const kpop_refset *rs) {
  if (!rs) return 0;
  return representatives_carve(nullptr, rs->r1).bytes;
}

extern "C" int kpop_dev_representatives_within(kpop_refset *rs, double max_distance, uint32_t known_rows, void *d_work, uint32_t *d_rep_of, double *d_rep_dist,
                                               uint32_t *d_n_reps, void *stream) {
  const char *who = "kpop_dev_representatives_within";
  KPOP_TRY(refset_check_handle(rs, who));
  if (!d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null workspace", who);
  return representatives_dev(rs, max_distance, known_rows, d_work, d_rep_of, d_rep_dist, d_n_reps, as_stream(stream), who);
}

extern "C" int kpop_representatives_within(kpop_refset *rs, double max_distance, uint32_t known_rows, uint32_t *rep_of, double *rep_dist, uint32_t *n_reps) {
  const char *who = "kpop_representatives_within";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(check_distance_is_a_number(max_distance, who));
  if (!n_reps || (rs->r1 && !rep_of)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t r1 = rs->r1;
  if (known_rows > r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %u known rows in a set of %u", who, known_rows, r1);
  KPOP_TRY(check_known_prefix(rep_of, known_rows, who, "rep_of", "an entry"));
  *n_reps = 0;
  if (r1 == 0) return KPOP_OK;
  HostCall h;
  void *work = h.work(representatives_carve(nullptr, r1).bytes);
  // (the known rows' entries are the caller's: neither array is written there, neither comes down there)
  uint32_t *dr = h.out(rep_of, r1, known_rows);
  double *dd = h.out(rep_dist, r1, known_rows);
  uint32_t *dn = h.scalars(n_reps, 1);
  h.up(dr, rep_of, known_rows);
  KPOP_TRY(h.upload());
  KPOP_TRY(representatives_dev(rs, max_distance, known_rows, work, dr, dd, dn, h.st, who));
  return h.finish();
}

extern "C" int kpop_distance_representatives(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                             double max_distance, uint32_t *rep_of, double *rep_dist, uint32_t *n_reps) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize,
                               [&](kpop_refset *rs) { return kpop_representatives_within(rs, max_distance, 0, rep_of, rep_dist, n_reps); });
}
