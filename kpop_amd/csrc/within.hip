// within.hip -- range queries on a resident set: every row of the set within a distance of a query row.
//
//   H_j = { i < r1 : d(j, i) <= max_distance }, each row's hits in ascending (distance, index) order (-0 as +0): the
//   FloatIntMultimap of summarize_distance_matrix_row (lib/Matrix.ml:632-690, its order :641-650) cut at a DISTANCE instead of at
//   a count -- what Space.Distance.Iterator (lib/Space.ml:231-487) bounds with its max_distance_component.  d(j, i) is the
//   reference chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250): the bits of
//   distance_rowwise_kernel (distance.hip), whatever kpop_tune says -- no setting is read here.
//
// The r2 x r1 matrix is never formed.  Five steps, each its own launch (no inter-workgroup hand-off inside a launch):
//   within_tile_kernel     the arithmetic of distance_rowwise_kernel, operation for operation (pair_tile.h); its epilogue compares where that
//                          one stores.  A row's hits are counted through LDS, then with ONE global add per row and block (sums:
//                          the counts do not depend on the order); the adds' old values give every hit a slot of its own inside
//                          its row.  The hits of a wavefront go to a pool of `capacity` entries (distance, index, row, slot) at a
//                          position taken with ONE atomic per wavefront (ballot, prefix over the lanes).  Hits beyond the capacity
//                          are counted and dropped.
//   scan_block_sums_kernel the counts, accumulated in out_offsets itself, become the offsets in place (scan.h); the total lands in [r2]
//   within_scatter_kernel  pool -> the rows' segments, no atomics (only when everything fitted).  Which slot of its row a hit has
//                          depends on who arrived first; nothing else does, and the next step removes it:
//   within_sort_kernel     a block sorts 4,096 hits of a row in LDS by (distance, index); a row of up to 4,096 is final there.
//   within_merge_kernel    longer rows: every hit's final place is its place in its own sorted chunk plus its lower bounds in the
//                          row's other chunks (the pairs of a row are all distinct: they differ in the index).  All rows and
//                          chunks in ONE launch, no synchronisation: the device form never learns the counts.  (A device-wide
//                          radix sort wants its length on the host; this form costs chunks x log 4,096 probes a hit, fine for rows
//                          of tens of thousands, slow for rows of millions.)
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "pair_tile.h"
#include "refset_call.h"
#include "scan.h"

namespace kpop {

constexpr int kWMaxW = 128, kWMaxTJ = 256;
constexpr uint32_t kWithinChunk = 4096;

// a, b: the operands as the chain reads them (divided by their rows' norms when the set normalises).  Tiles as
// distance_rowwise_kernel's: w columns (rows of the set) x TY n_rg query rows, a thread 4 columns x TY rows, the dimensions ascending
// in one thread, 16 at a time through LDS.  jbase: the first query row of this launch (counts, pool rows: whole-call numbering).
template <int KIND, int TY>
__global__ __launch_bounds__(256, 1) void within_tile_kernel(const double *__restrict__ a, uint32_t w, uint32_t r1, const double *__restrict__ b, uint32_t r2,
                                                             uint32_t n_dims, const double *__restrict__ metric, double p, double max_distance,
                                                             uint32_t n_cg, uint32_t n_rg, uint32_t jbase, unsigned long long *__restrict__ counts,
                                                             uint64_t capacity, unsigned long long *__restrict__ cursor, double *__restrict__ pool_d,
                                                             uint32_t *__restrict__ pool_i, uint32_t *__restrict__ pool_r, uint32_t *__restrict__ pool_k) {
  __shared__ __attribute__((aligned(16))) double As[kPairDC][kWMaxW + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][kWMaxTJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint32_t s_cnt[kWMaxTJ];
  const uint32_t TJ = TY * n_rg;
  const uint32_t i0 = blockIdx.x * w, j0 = blockIdx.y * TJ;
  const uint32_t i1 = min(r1, i0 + w), j1 = min(r2, j0 + TJ);
  const uint32_t cg = threadIdx.x % n_cg, rg = threadIdx.x / n_cg;
  const bool worker = rg < n_rg;
  const uint32_t ti = cg * 4, tj = (worker ? rg : 0) * TY;
  s_cnt[threadIdx.x] = 0;  // (kWMaxTJ == blockDim.x; the loop's barriers come before anybody adds)
  // (the loop of pair_tile_distances, written out: built on it the kernel assembles to other arithmetic, profiles/self_tile_refactor.md)
  double acc[TY][4];
  pair_zero(acc);
  PairStage<kWMaxW, kWMaxTJ> stage;
  const PairRows rows_a{a, r1}, rows_b{b, r2};
  stage.load(rows_a, i0, i1, rows_b, j0, j1, n_dims, 0, n_dims);
  for (uint32_t c0 = 0; c0 < n_dims; c0 += kPairDC) {
    __syncthreads();
    stage.store(As, Bs, s_metric, metric, c0, n_dims);
    __syncthreads();
    if (c0 + kPairDC < n_dims) stage.load(rows_a, i0, i1, rows_b, j0, j1, n_dims, c0 + kPairDC, n_dims);
    if (worker) pair_accumulate<KIND>(acc, As, Bs, s_metric, ti, tj, min((uint32_t)kPairDC, n_dims - c0), p);
  }
  // the epilogue: compare where distance_rowwise_kernel stores (a NaN compares false: never a hit)
  uint32_t mask = 0;
  if (worker) {
#pragma unroll
    for (int y = 0; y < TY; ++y)
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        acc[y][x] = scale_distance<KIND>(acc[y][x], p);
        if (j0 + tj + y < r2 && i0 + ti + x < i1 && acc[y][x] <= max_distance) mask |= 1u << (y * 4 + x);
      }
  }
  // a row's hits are counted through LDS; the old value of a thread's add is where its hits stand among the block's of that row
  const uint32_t nh = (uint32_t)__popc(mask);
  uint32_t loc[TY];
#pragma unroll
  for (int y = 0; y < TY; ++y) {
    const uint32_t c = (uint32_t)__popc((mask >> (y * 4)) & 15u);
    loc[y] = c ? atomicAdd(&s_cnt[tj + y], c) : 0u;
  }
  __syncthreads();
  // ONE global add per row and block (a sum: the count does not depend on who comes first); its old value is where the block's hits
  // stand in the row -- a slot that is the hit's alone, in an order that the sort puts right
  if (threadIdx.x < TJ) {
    const uint32_t c = s_cnt[threadIdx.x];
    if (c) s_cnt[threadIdx.x] = (uint32_t)atomicAdd(&counts[(uint64_t)jbase + j0 + threadIdx.x], (unsigned long long)c);  // (c > 0: the row exists)
  }
  __syncthreads();
  if (capacity && __ballot(nh != 0)) {  // (uniform over the wavefront; hits are few: most wavefronts pass by)
    // the pool: ONE atomic per wavefront, the lanes' places by a prefix over their counts
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = nh;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= (uint32_t)o) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cursor, (unsigned long long)total);
    base = (unsigned long long)__shfl((unsigned long long)base, 0, 64);
    uint64_t pos = base + incl - nh;
#pragma unroll
    for (int y = 0; y < TY; ++y) {
      uint32_t k = s_cnt[tj + y] + loc[y];
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (mask & (1u << (y * 4 + x))) {
          if (pos < capacity) {
            pool_d[pos] = acc[y][x];
            pool_i[pos] = i0 + ti + x;
            pool_r[pos] = jbase + j0 + tj + y;
            pool_k[pos] = k;
          }
          ++pos;
          ++k;
        }
    }
  }
}

// pool -> the rows' segments, when the whole result fits
__global__ __launch_bounds__(256) void within_scatter_kernel(const uint64_t *__restrict__ offsets, uint32_t r2, uint64_t capacity, const double *__restrict__ pool_d,
                                                             const uint32_t *__restrict__ pool_i, const uint32_t *__restrict__ pool_r, const uint32_t *__restrict__ pool_k,
                                                             double *__restrict__ tmp_d, uint32_t *__restrict__ tmp_i) {
  const uint64_t total = offsets[r2];
  if (total > capacity) return;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    const uint64_t q = offsets[pool_r[e]] + pool_k[e];  // (below the row's count: the slots of a row are 0 .. count - 1, each taken once)
    tmp_d[q] = pool_d[e];
    tmp_i[q] = pool_i[e];
  }
}

// the multimap's order (lib/Matrix.ml:641-650): distance, then column; IEEE comparison, so -0 orders as +0
__device__ __forceinline__ bool within_less(double da, uint32_t ia, double db, uint32_t ib) { return (da < db) || (da == db && ia < ib); }

// a block sorts one chunk of kWithinChunk hits of a row in LDS; a row of one chunk goes straight to the output, the chunks of a
// longer row go back where they came from
__global__ __launch_bounds__(1024) void within_sort_kernel(const uint64_t *__restrict__ offsets, uint32_t r2, uint64_t capacity, double *__restrict__ tmp_d,
                                                           uint32_t *__restrict__ tmp_i, uint32_t *__restrict__ out_idx, double *__restrict__ out_dist) {
  __shared__ double kd[kWithinChunk];
  __shared__ uint32_t ki[kWithinChunk];
  if (offsets[r2] > capacity) return;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (uint32_t j = blockIdx.x; j < r2; j += gridDim.x) {
    const uint64_t off = offsets[j], n = offsets[j + 1] - off;
    const uint64_t n_chunks = (n + kWithinChunk - 1) / kWithinChunk;
    for (uint64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {
      const uint64_t base = off + c * kWithinChunk;
      const uint32_t len = (uint32_t)min((uint64_t)kWithinChunk, n - c * kWithinChunk);
      uint32_t NP = 2;
      while (NP < len) NP <<= 1;
      for (uint32_t q = threadIdx.x; q < NP; q += blockDim.x) {
        kd[q] = q < len ? tmp_d[base + q] : inf;  // (padding after every hit: +inf with the largest index)
        ki[q] = q < len ? tmp_i[base + q] : 0xFFFFFFFFu;
      }
      for (uint32_t s = 2; s <= NP; s <<= 1)
        for (uint32_t t = s >> 1; t > 0; t >>= 1) {
          __syncthreads();
          for (uint32_t q = threadIdx.x; q < NP / 2; q += blockDim.x) {
            const uint32_t i = 2 * q - (q & (t - 1)), k = i + t;
            const bool asc = (i & s) == 0;
            const double di = kd[i], dk = kd[k];
            const uint32_t ii = ki[i], ik = ki[k];
            if (within_less(dk, ik, di, ii) == asc) {
              kd[i] = dk; kd[k] = di;
              ki[i] = ik; ki[k] = ii;
            }
          }
        }
      __syncthreads();
      if (n_chunks == 1) {
        for (uint32_t q = threadIdx.x; q < len; q += blockDim.x) {
          out_idx[base + q] = ki[q];
          out_dist[base + q] = kd[q];
        }
      } else {
        for (uint32_t q = threadIdx.x; q < len; q += blockDim.x) {
          tmp_i[base + q] = ki[q];
          tmp_d[base + q] = kd[q];
        }
      }
      __syncthreads();
    }
  }
}

// rows of more than one chunk: a hit's place in the row = its place in its chunk + the hits of every other chunk below it
__global__ __launch_bounds__(256) void within_merge_kernel(const uint64_t *__restrict__ offsets, uint32_t r2, uint64_t capacity, const double *__restrict__ tmp_d,
                                                           const uint32_t *__restrict__ tmp_i, uint32_t *__restrict__ out_idx, double *__restrict__ out_dist) {
  if (offsets[r2] > capacity) return;
  for (uint32_t j = blockIdx.x; j < r2; j += gridDim.x) {
    const uint64_t off = offsets[j], n = offsets[j + 1] - off;
    const uint64_t n_chunks = (n + kWithinChunk - 1) / kWithinChunk;
    if (n_chunks <= 1) continue;
    for (uint64_t c = blockIdx.y; c < n_chunks; c += gridDim.y) {
      const uint64_t base = off + c * kWithinChunk;
      const uint32_t len = (uint32_t)min((uint64_t)kWithinChunk, n - c * kWithinChunk);
      for (uint32_t e = threadIdx.x; e < len; e += blockDim.x) {
        const double d = tmp_d[base + e];
        const uint32_t i = tmp_i[base + e];
        uint64_t rank = e;
        for (uint64_t c2 = 0; c2 < n_chunks; ++c2) {
          if (c2 == c) continue;
          const uint64_t b2 = off + c2 * kWithinChunk;
          uint32_t lo = 0, hi = (uint32_t)min((uint64_t)kWithinChunk, n - c2 * kWithinChunk);
          while (lo < hi) {  // the first entry of the chunk that is not below (d, i)
            const uint32_t mid = (lo + hi) >> 1;
            if (within_less(tmp_d[b2 + mid], tmp_i[b2 + mid], d, i)) lo = mid + 1;
            else hi = mid;
          }
          rank += lo;
        }
        out_idx[off + rank] = i;
        out_dist[off + rank] = d;
      }
    }
  }
}

// the workspace of a call: the query rows' norms and divided copy, the pool's cursor, the pool, the segments
struct WithinWork {
  double *n2, *b;
  unsigned long long *cursor;
  double *pool_d, *tmp_d;
  uint32_t *pool_i, *pool_r, *pool_k, *tmp_i;
  uint64_t bytes;
};
static WithinWork within_carve(void *work, uint32_t r2, uint32_t n_dims, bool normalize, uint64_t capacity) {
  Carver c(work);
  WithinWork w;
  w.n2 = c.take<double>(normalize ? (uint64_t)r2 * 8 : 0);
  w.b = c.take<double>(normalize ? (uint64_t)r2 * n_dims * 8 : 0);
  w.cursor = c.take<unsigned long long>(256);
  w.pool_d = c.take<double>(capacity * 8);
  w.tmp_d = c.take<double>(capacity * 8);
  w.pool_i = c.take<uint32_t>(capacity * 4);
  w.pool_r = c.take<uint32_t>(capacity * 4);
  w.pool_k = c.take<uint32_t>(capacity * 4);
  w.tmp_i = c.take<uint32_t>(capacity * 4);
  w.bytes = c.off + 256;
  return w;
}

template <int KIND>
static int within_tiles(const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, double max_distance,
                        unsigned long long *counts, uint64_t capacity, const WithinWork &w, hipStream_t st) {
  // the tiles of rowwise_block (distance.hip): against a very long set the long-set shape of the self-joins (self_shape, tri_tile.h),
  // 32 columns x 256 rows; balanced column tiles of 64..127 otherwise, a choice of this file's own.  (It moves no bit.)
  if (r1 >= 65536 && r2 <= 4096) {
    within_tile_kernel<KIND, 8><<<dim3(div_up(r1, 32), div_up(r2, 256)), dim3(256), 0, st>>>(a, 32, r1, b, r2, n_dims, metric, p, max_distance, 8, 32, 0, counts, capacity,
                                                                                              w.cursor, w.pool_d, w.pool_i, w.pool_r, w.pool_k);
    KPOP_LAUNCH_CHECK();
    return 0;
  }
  const uint32_t n_tiles = std::max(1u, r1 / 64);
  const uint32_t wt = div_up(r1, n_tiles), n_cg = div_up(wt, 4);
  const uint32_t n_rg = std::min(256u / n_cg, (uint32_t)kWMaxTJ / 4), TJ = 4 * n_rg;
  const uint32_t rows_per_launch = 65535u * TJ;  // query rows ride on grid.y
  for (uint32_t j0 = 0; j0 < r2; j0 += rows_per_launch) {
    const uint32_t nr = std::min(rows_per_launch, r2 - j0);
    within_tile_kernel<KIND, 4><<<dim3(div_up(r1, wt), div_up(nr, TJ)), dim3(256), 0, st>>>(a, wt, r1, b + (uint64_t)j0 * n_dims, nr, n_dims, metric, p, max_distance,
                                                                                             n_cg, n_rg, j0, counts, capacity, w.cursor, w.pool_d, w.pool_i, w.pool_r, w.pool_k);
    KPOP_LAUNCH_CHECK();
  }
  return 0;
}

// the body of both entry points: enqueues only
static int within_dev(kpop_refset *rs, const double *d_m2, uint32_t r2, double max_distance, uint64_t capacity, void *d_work, uint64_t *d_out_offsets,
                      uint32_t *d_out_idx, double *d_out_dist, hipStream_t st) {
  const char *who = "kpop_dev_neighbours_within";
  if (max_distance != max_distance) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  if (!d_out_offsets) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null offsets", who);
  if ((d_out_idx == nullptr) != (d_out_dist == nullptr)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: one of the two lists is null", who);
  if (!d_out_idx) capacity = 0;  // count only
  KPOP_HIP(hipMemsetAsync(d_out_offsets, 0, ((uint64_t)r2 + 1) * 8, st));
  if (rs->r1 == 0 || r2 == 0) return KPOP_OK;
  if (!d_m2 || !d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t D = rs->n_dims;
  const WithinWork w = within_carve(d_work, r2, D, rs->normalize != 0, capacity);
  KPOP_HIP(hipMemsetAsync(w.cursor, 0, 256, st));
  const double *a, *b = d_m2;
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  if (rs->normalize) {  // the query rows' quotients from the norms' pass: prepare_operands' (distance.hip)
    KPOP_TRY(refset_query_norms(rs, d_m2, r2, w.n2, w.b, st));
    b = w.b;
  }
  unsigned long long *counts = reinterpret_cast<unsigned long long *>(d_out_offsets);
  KPOP_TRY(by_kind(rs->kind, [&](auto K) { return within_tiles<decltype(K)::value>(a, rs->r1, b, r2, D, rs->metric, rs->p, max_distance, counts, capacity, w, st); }));
  scan_block_sums_kernel<0><<<dim3(1), dim3(1024), 0, st>>>(d_out_offsets, r2);  // counts -> offsets in place, the total to [r2]
  KPOP_LAUNCH_CHECK();
  if (capacity == 0) return KPOP_OK;
  within_scatter_kernel<<<dim3(std::max(1u, std::min(div_up(capacity, 256), 4096u))), dim3(256), 0, st>>>(d_out_offsets, r2, capacity, w.pool_d, w.pool_i, w.pool_r, w.pool_k,
                                                                                                          w.tmp_d, w.tmp_i);
  KPOP_LAUNCH_CHECK();
  // a block a (row, chunk); rows and chunks beyond the grid are walked by the blocks there are
  const uint32_t gx = std::min(r2, 1u << 20);
  const uint64_t max_chunks = std::max<uint64_t>(1, (std::min<uint64_t>(capacity, rs->r1) + kWithinChunk - 1) / kWithinChunk);
  const uint32_t gy = (uint32_t)std::min<uint64_t>(max_chunks, std::max<uint32_t>(1u, std::min<uint32_t>(65535u, (1u << 21) / gx)));
  within_sort_kernel<<<dim3(gx, gy), dim3(1024), 0, st>>>(d_out_offsets, r2, capacity, w.tmp_d, w.tmp_i, d_out_idx, d_out_dist);
  KPOP_LAUNCH_CHECK();
  if (max_chunks > 1) {
    within_merge_kernel<<<dim3(gx, gy), dim3(256), 0, st>>>(d_out_offsets, r2, capacity, w.tmp_d, w.tmp_i, d_out_idx, d_out_dist);
    KPOP_LAUNCH_CHECK();
  }
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_neighbours_within_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint64_t capacity) {
  if (!rs) return 0;
  return within_carve(nullptr, r2, rs->n_dims, rs->normalize != 0, capacity).bytes;
}

extern "C" int kpop_dev_neighbours_within(kpop_refset *rs, const double *d_m2, uint32_t r2, double max_distance, uint64_t capacity, void *d_work,
                                          uint64_t *d_out_offsets, uint32_t *d_out_idx, double *d_out_dist, void *stream) {
  KPOP_TRY(refset_check_handle(rs, "kpop_dev_neighbours_within"));
  return within_dev(rs, d_m2, r2, max_distance, capacity, d_work, d_out_offsets, d_out_idx, d_out_dist, as_stream(stream));
}

extern "C" int kpop_neighbours_within(kpop_refset *rs, const double *m2, uint32_t r2, double max_distance, uint64_t capacity, uint64_t *out_offsets,
                                      uint32_t *out_idx, double *out_dist) {
  KPOP_TRY(refset_check_handle(rs, "kpop_neighbours_within"));
  ArenaScope scratch;
  KPOP_TRY(check_distance_is_a_number(max_distance, "kpop_neighbours_within"));
  if (!out_offsets || (r2 && rs->r1 && !m2)) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_neighbours_within: null argument");
  if ((out_idx == nullptr) != (out_dist == nullptr)) KPOP_FAIL(KPOP_ERR_INVALID, "kpop_neighbours_within: one of the two lists is null");
  if (!out_idx) capacity = 0;
  HostCall h;
  const double *d2 = h.in(rs->r1 ? m2 : nullptr, (uint64_t)r2 * rs->n_dims);
  void *dw = h.work(kpop_dev_neighbours_within_workspace_bytes(rs, r2, capacity));
  uint64_t *doff = h.dev<uint64_t>((uint64_t)r2 + 1);
  uint32_t *di = h.counted(out_idx, capacity);
  double *dd = h.counted(out_dist, capacity);
  KPOP_TRY(h.upload());
  KPOP_TRY(within_dev(rs, d2, r2, max_distance, capacity, dw, doff, di, dd, h.st));
  KPOP_TRY(h.read(out_offsets, doff, (uint64_t)r2 + 1));
  const uint64_t total = out_offsets[r2];
  if (!out_idx) return KPOP_OK;
  if (total > capacity)
    KPOP_FAIL(KPOP_ERR_CAPACITY, "kpop_neighbours_within: %llu neighbours, room for %llu (the offsets are complete)", (unsigned long long)total,
              (unsigned long long)capacity);
  return total ? h.finish(total) : KPOP_OK;
}

extern "C" int kpop_distance_within(const double *m1, uint32_t r1, const double *m2, uint32_t r2, uint32_t n_dims, const double *metric, int kind, double p,
                                    int normalize, double max_distance, uint64_t capacity, uint64_t *out_offsets, uint32_t *out_idx, double *out_dist) {
  return with_temporary_refset(m1, r1, n_dims, metric, kind, p, normalize,
                               [&](kpop_refset *rs) { return kpop_neighbours_within(rs, m2, r2, max_distance, capacity, out_offsets, out_idx, out_dist); });
}
