// knn_validate.hip -- k-NN validation: the votes of one neighbour list at many k, and the leave-out votes of a labelled resident set
// over its own rows.  Everything not said here is knn.hip's (section 6f): the distance, the key order
// (d with -0 taken as +0, index), whole tie groups, a NaN never a neighbour, +inf a number, the vote's tie-break.
//
//   Votes for many k.  ks[n_ks] strictly ascending, K = its last.  The list of the K nearest determines the vote for every k <= K: one
//   nearest pass at K, one merge and one tie pass serve every k; slice t of the [n_ks][rows] outputs is what the vote at k = ks[t] gives,
//   bit for bit.
//   Leave-out votes.  The query rows are rows first_row .. first_row + n_rows of the set itself (its divided copy at an offset when it
//   normalises: no second copy).  Left out of row j's list: row j itself (group_of == NULL), or every row i with group_of[i] ==
//   group_of[j] (j among them).  By index or group, never by distance: a duplicate of j in another group stays, at distance 0.  d(j, i) is
//   the bits distance_rowwise_kernel writes with the set's rows as the query: clusters.hip's definition.  out_correct[t]: the rows whose
//   class at ks[t] is their own.  No setting is read; every step is a function of the distances, classes and groups alone.
//
// The launches of a validation, always the same (the device form reads nothing back):
//   knnv_nearest_kernel  knn_nearest_kernel's shape (KnnShape, the lists in LDS, knn_insert, the dropped ties, the column segments) with
//                        its own copy of the tile loop, so that knn.hip's kernels stay the kernels they were.  The epilogue refuses an
//                        excluded column before it can be inserted OR counted as a dropped tie: a row whose own index ties with its
//                        k-th key would otherwise flag itself.  The groups of the tile's four columns are loaded once a tile, those of
//                        the thread's rows once a launch.
//   knn_merge_kernel     knn.hip's, as it is, with k = K (knn_run_merge).
//   knnv_ties_kernel     knn_ties_kernel's shape with the same refusal.
//   knn_vote_ks_kernel   per row, the merged list read at every cut (below).  Also the vote of kpop_knn_ks_vote, whose three passes
//                        are knn.hip's own (knn_run_passes).
//   knn_correct_kernel   integers summed: any order gives the same bits.
#include <algorithm>

#include "common.h"
#include "distance_routes.h"
#include "knn_lists.h"
#include "refset.h"
#include "space_ops.h"

namespace kpop {

// the cut points, by value: at most 32 words, no copy from the caller's (pageable) memory
struct KnnKs {
  uint32_t n;
  uint32_t k[kKMaxKs];
};

// The tile loop: knn_tiles (knn.hip), operation for operation; the query rows are rows of `a` too, from row jbase on.  The workgroup's
// rows j0 .. j1 of the range (at most TJ), its column tiles t_begin .. t_end of W rows of the set each.  A thread 4 columns x TY rows, the
// dimensions ascending in one thread, 16 at a time through LDS; the next step's operands are loaded under the arithmetic.
// epi(i0, i1, acc): what to do with a tile's finished sums.
template <int KIND, int TY, int W, class Epi>
__device__ __forceinline__ void knnv_tiles(const double *__restrict__ a, uint32_t r1, uint32_t jbase, uint32_t j0, uint32_t j1, uint32_t n_dims,
                                           const double *__restrict__ metric, double p, uint32_t t_begin, uint32_t t_end, double (*As)[W + 2],
                                           double (*Bs)[KnnShape<TY, W>::TJ + 2], double *s_metric, Epi &&epi) {
  using S = KnnShape<TY, W>;
  constexpr uint32_t TJ = S::TJ;
  const uint32_t cg = threadIdx.x % S::NCG, rg = threadIdx.x / S::NCG;
  const uint32_t ti = cg * 4, tj = rg * TY;
  constexpr int NA = W * kKDC / 256, NB = TJ * kKDC / 256;
  double ra[NA], rb[NB];
  const uint32_t sc = threadIdx.x % kKDC, rbase = threadIdx.x / kKDC;
  const double *b = a + (uint64_t)jbase * n_dims;
  auto prefetch = [&](uint32_t i0, uint32_t c0) {
    const uint32_t i1 = min(r1, i0 + W);
    const bool cok = c0 + sc < n_dims;
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const uint32_t row = rbase + q * 16;
      ra[q] = (cok && i0 + row < i1) ? a[(uint64_t)(i0 + row) * n_dims + c0 + sc] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const uint32_t row = rbase + q * 16;
      rb[q] = (cok && j0 + row < j1) ? b[(uint64_t)(j0 + row) * n_dims + c0 + sc] : 0.0;
    }
  };
  if (t_begin < t_end) prefetch(t_begin * W, 0);
  for (uint32_t t = t_begin; t < t_end; ++t) {
    const uint32_t i0 = t * W, i1 = min(r1, i0 + W);
    double acc[TY][4];
#pragma unroll
    for (int yy = 0; yy < TY; ++yy)
#pragma unroll
      for (int x = 0; x < 4; ++x) acc[yy][x] = 0.0;
    for (uint32_t c0 = 0; c0 < n_dims; c0 += kKDC) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NA; ++q) As[sc][rbase + q * 16] = ra[q];
#pragma unroll
      for (int q = 0; q < NB; ++q) Bs[sc][rbase + q * 16] = rb[q];
      if (threadIdx.x < kKDC) s_metric[threadIdx.x] = (c0 + threadIdx.x < n_dims) ? metric[c0 + threadIdx.x] : 0.0;
      __syncthreads();
      if (c0 + kKDC < n_dims) prefetch(i0, c0 + kKDC);
      else if (t + 1 < t_end) prefetch((t + 1) * W, 0);
      const uint32_t lim = min((uint32_t)kKDC, n_dims - c0);
      for (uint32_t cc = 0; cc < lim; ++cc) {
        double av[4], bv[TY];
#pragma unroll
        for (int x = 0; x < 4; ++x) av[x] = As[cc][ti + x];
#pragma unroll
        for (int yy = 0; yy < TY; ++yy) bv[yy] = Bs[cc][tj + yy];
        const double mc = s_metric[cc];
#pragma unroll
        for (int yy = 0; yy < TY; ++yy)
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            // lib/Space.ml:192-200: diff = a -. b ; acc +. (diff *. diff *. m)
            double diff = __dsub_rn(av[x], bv[yy]);
            acc[yy][x] = __dadd_rn(acc[yy][x], component<KIND>(diff, mc, p));
          }
      }
    }
    epi(i0, i1, acc);
  }
}

// What a thread knows of who is left out: its rows' groups (or their indices in the set) for the launch, the tile's four columns' groups
// for the tile.  left_out(yy, x, i): column i, the thread's x-th, is not a neighbour of its yy-th row
template <int TY>
struct KnnvLeftOut {
  const uint32_t *group_of;
  uint32_t own[TY], col[4];  // group_of set: groups; not set: own[] the rows' indices in the set
  __device__ __forceinline__ void rows(const uint32_t *g, uint32_t jfirst, uint32_t r1) {
    group_of = g;
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) own[yy] = (g && jfirst + yy < r1) ? g[jfirst + yy] : jfirst + yy;
  }
  __device__ __forceinline__ void columns(uint32_t ifirst, uint32_t i1) {
    if (!group_of) return;
#pragma unroll
    for (int x = 0; x < 4; ++x) col[x] = ifirst + x < i1 ? group_of[ifirst + x] : 0u;
  }
  __device__ __forceinline__ bool left_out(int yy, int x, uint32_t i) const { return group_of ? col[x] == own[yy] : i == own[yy]; }
};

// Strip blockIdx.x: rows first_row + j0 .. + TJ of the set as query rows; segment blockIdx.y.  seg_key, seg_idx: [segment][n_rows][k],
// the list's first seg_n entries ascending; seg_drop: the dropped ties of the list's last key.  TJ k <= SLOTS (the launch sees to it).
template <int KIND, int TY, int W>
__global__ __launch_bounds__(256, 1) void knnv_nearest_kernel(const double *__restrict__ a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims,
                                                              const double *__restrict__ metric, double p, uint32_t k, uint32_t n_ct, uint32_t tiles_per_seg,
                                                              const uint32_t *__restrict__ group_of, uint64_t *__restrict__ seg_key,
                                                              uint32_t *__restrict__ seg_idx, uint32_t *__restrict__ seg_n, uint32_t *__restrict__ seg_drop) {
  using S = KnnShape<TY, W>;
  constexpr uint32_t TJ = S::TJ;
  __shared__ __attribute__((aligned(16))) double As[kKDC][W + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kKDC][TJ + 2];
  __shared__ double s_metric[kKDC];
  __shared__ uint64_t s_key[S::SLOTS];
  __shared__ uint32_t s_idx[S::SLOTS];
  __shared__ uint64_t s_bound[TJ];
  __shared__ uint32_t s_n[TJ], s_drop[TJ], s_bidx[TJ];
  const uint32_t j0 = blockIdx.x * TJ, j1 = min(n_rows, j0 + TJ);  // (the grid has div_up(n_rows, TJ) strips: j0 < n_rows)
  uint32_t t_begin, t_end;
  knn_segment(n_ct, tiles_per_seg, &t_begin, &t_end);
  if (threadIdx.x < TJ) {
    s_bound[threadIdx.x] = kKNone;
    s_bidx[threadIdx.x] = 0;
    s_n[threadIdx.x] = 0;
    s_drop[threadIdx.x] = 0;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ti = (threadIdx.x % S::NCG) * 4, tj = (threadIdx.x / S::NCG) * TY;  // (the rows of a wavefront: TJ / 4 in a row, nobody else's)
  KnnvLeftOut<TY> out;
  out.rows(group_of, first_row + j0 + tj, r1);
  knnv_tiles<KIND, TY, W>(a, r1, first_row, j0, j1, n_dims, metric, p, t_begin, t_end, As, Bs, s_metric, [&](uint32_t i0, uint32_t i1, double(&acc)[TY][4]) {
    out.columns(i0 + ti, i1);
    // the rows' bounds as the step before left them (a row is this wavefront's alone): read again after every step that inserted
    uint64_t bound[TY];
    uint32_t bidx[TY];
    auto bounds = [&]() {
#pragma unroll
      for (int yy = 0; yy < TY; ++yy) {
        bound[yy] = *(volatile uint64_t *)&s_bound[tj + yy];
        bidx[yy] = *(volatile uint32_t *)&s_bidx[tj + yy];
      }
    };
    bounds();
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      const uint32_t row = tj + yy;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t i = i0 + ti + x;
        const uint64_t key = knn_key(d);
        // a NaN is never a neighbour, and neither is a column that is left out: refused here, in front of the count of dropped ties
        const bool number = j0 + row < j1 && i < i1 && d == d && !out.left_out(yy, x, i);
        // a tie of the k-th key behind the k-th entry is dropped and counted where it stands: a sum, whatever the order.  These
        // come first, the entries that go into the list after them: one of the orders of arrival, all of which give the same
        if (number && key == bound[yy] && i > bidx[yy]) atomicAdd(&s_drop[row], 1u);
        __builtin_amdgcn_wave_barrier();
        const bool c = number && (key < bound[yy] || (key == bound[yy] && i < bidx[yy]));
        uint64_t m = __ballot(c);
        const bool inserted = m != 0;
        while (m) {  // (the same in every lane)
          const int src = __ffsll((unsigned long long)m) - 1;
          m &= m - 1;
          const uint64_t ck = (uint64_t)__shfl((unsigned long long)key, src, 64);
          const uint32_t ci = (uint32_t)__shfl((int)i, src, 64);
          const uint32_t cr = (uint32_t)__shfl((int)row, src, 64);
          knn_insert(s_key + cr * k, s_idx + cr * k, s_n + cr, s_bound + cr, s_bidx + cr, s_drop + cr, k, ck, ci, lane);
        }
        if (inserted) bounds();
      }
    }
  });
  __syncthreads();
  const uint32_t seg = blockIdx.y;
  for (uint32_t e = threadIdx.x; e < TJ * k; e += 256) {
    const uint32_t row = e / k, q = e % k;
    if (j0 + row < j1) {
      const uint64_t o = ((uint64_t)seg * n_rows + j0 + row) * k + q;
      const bool in = q < s_n[row];
      seg_key[o] = in ? s_key[e] : kKNone;
      seg_idx[o] = in ? s_idx[e] : 0u;
    }
  }
  if (threadIdx.x < TJ && j0 + threadIdx.x < j1) {
    seg_n[(uint64_t)seg * n_rows + j0 + threadIdx.x] = s_n[threadIdx.x];
    seg_drop[(uint64_t)seg * n_rows + j0 + threadIdx.x] = s_drop[threadIdx.x];
  }
}

// the grid of knnv_nearest_kernel.  tie_total: [n_rows], every column of a flagged row at tau that is not left out; tie_count,
// tie_first: [n_rows][n_classes], those of a class and the least index among them (0xFFFFFFFF: none).  class_of is trusted, every table
// access guarded
template <int KIND, int TY, int W>
__global__ __launch_bounds__(256, 1) void knnv_ties_kernel(const double *__restrict__ a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims,
                                                           const double *__restrict__ metric, double p, uint32_t n_ct, uint32_t tiles_per_seg,
                                                           const uint32_t *__restrict__ group_of, const uint32_t *__restrict__ class_of, uint32_t n_classes,
                                                           const uint64_t *__restrict__ m_tau, const uint32_t *__restrict__ m_flag, uint32_t *tie_total,
                                                           uint32_t *tie_count, uint32_t *tie_first) {
  using S = KnnShape<TY, W>;
  constexpr uint32_t TJ = S::TJ;
  __shared__ __attribute__((aligned(16))) double As[kKDC][W + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kKDC][TJ + 2];
  __shared__ double s_metric[kKDC];
  const uint32_t j0 = blockIdx.x * TJ, j1 = min(n_rows, j0 + TJ);
  if (!__syncthreads_or(threadIdx.x < TJ && j0 + threadIdx.x < j1 && m_flag[j0 + threadIdx.x] != 0)) return;  // (nearly every workgroup)
  uint32_t t_begin, t_end;
  knn_segment(n_ct, tiles_per_seg, &t_begin, &t_end);
  const uint32_t ti = (threadIdx.x % S::NCG) * 4, tj = (threadIdx.x / S::NCG) * TY;
  uint64_t tau[TY];
  bool fl[TY];
#pragma unroll
  for (int yy = 0; yy < TY; ++yy) {
    const uint32_t j = j0 + tj + yy;
    fl[yy] = j < j1 && m_flag[j] != 0;
    tau[yy] = fl[yy] ? m_tau[j] : kKNone;
  }
  KnnvLeftOut<TY> out;
  out.rows(group_of, first_row + j0 + tj, r1);
  knnv_tiles<KIND, TY, W>(a, r1, first_row, j0, j1, n_dims, metric, p, t_begin, t_end, As, Bs, s_metric, [&](uint32_t i0, uint32_t i1, double(&acc)[TY][4]) {
    out.columns(i0 + ti, i1);
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      if (!fl[yy]) continue;
      const uint32_t j = j0 + tj + yy;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t i = i0 + ti + x;
        if (i < i1 && d == d && !out.left_out(yy, x, i) && knn_key(d) == tau[yy]) {
          atomicAdd(tie_total + j, 1u);
          const uint32_t c = class_of[i];
          if (c < n_classes) {
            atomicAdd(tie_count + (uint64_t)j * n_classes + c, 1u);
            atomicMin(tie_first + (uint64_t)j * n_classes + c, i);
          }
        }
      }
    }
  });
}

// One list, many cuts: a block of 64 (one wavefront) a row.  The merged list holds the row's K nearest (fewer: everything), ascending by
// (key, index); tau_K is its last key.  For cut t, tau_t is the min(ks[t], n)-th key of the merged list, and the list at k = ks[t] is the
// merged entries with key <= tau_t -- a prefix.  A TIE GROUP BELOW tau_K LIES WHOLLY INSIDE THE MERGED LIST, because everything below
// tau_K is in it (the K smallest of a set hold all that is smaller than the K-th): nothing outside has to be looked at for such a cut,
// which is what makes one pass over the pairs enough.  Where tau_t == tau_K, and only there, the ties outside the merged list join:
// from the segments' lists for an unflagged row (the group's members behind the merged list's last index), from the tables for a flagged
// one (the whole group; the merged list then counts below tau_K alone, as in knn_vote_kernel).  Every cut at tau_K has the same list:
// it is voted once.
// The list is walked ONCE: s_rep[q] is the place of the first entry of q's class (the class's nearest member: the list is in order), and
// a running count s_cnt[s_rep[q]] is extended from cut to cut; after each cut the winner is taken over the places that stand for a
// class, by (count descending, first (key, index) ascending).  Integer sums and a strict order: the same bits whatever the lanes' order.
// LDS: 1,152 entries of 16 bytes as knn_vote_kernel has them, and 1 KiB of places and counts.
__global__ __launch_bounds__(64) void knn_vote_ks_kernel(const uint64_t *__restrict__ seg_key, const uint32_t *__restrict__ seg_idx, const uint32_t *__restrict__ seg_n,
                                                         uint32_t n_seg, uint32_t r2, uint32_t k, const uint64_t *__restrict__ m_key, const uint32_t *__restrict__ m_idx,
                                                         const uint32_t *__restrict__ m_n, const uint64_t *__restrict__ m_tau, const uint32_t *__restrict__ m_flag,
                                                         const uint32_t *__restrict__ class_of, uint32_t n_classes, const uint32_t *__restrict__ tie_total,
                                                         const uint32_t *__restrict__ tie_count, const uint32_t *__restrict__ tie_first, KnnKs ks,
                                                         uint32_t *__restrict__ out_class, uint32_t *__restrict__ out_votes, uint32_t *__restrict__ out_n,
                                                         double *__restrict__ out_first_dist) {
  __shared__ uint64_t s_k[kKVoteList];
  __shared__ uint32_t s_i[kKVoteList], s_c[kKVoteList];
  __shared__ uint32_t s_rep[kKMaxK], s_cnt[kKMaxK];
  __shared__ uint32_t s_nt;
  constexpr uint32_t kNoPlace = 0xFFFFFFFFu;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  auto reduce = [](KnnBest best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      KnnBest other;
      other.cnt = (uint32_t)__shfl_xor((int)best.cnt, o, 64);
      other.idx = (uint32_t)__shfl_xor((int)best.idx, o, 64);
      other.cls = (uint32_t)__shfl_xor((int)best.cls, o, 64);
      other.key = (uint64_t)__shfl_xor((unsigned long long)best.key, o, 64);
      if (knn_better(other, best)) best = other;
    }
    return best;
  };
  for (uint32_t row = blockIdx.x; row < r2; row += gridDim.x) {
    auto write = [&](uint32_t t, const KnnBest &best, uint32_t n_list) {
      if (threadIdx.x == 0) {
        const uint64_t o = (uint64_t)t * r2 + row;
        out_class[o] = best.cnt ? best.cls : KPOP_NO_CLASS;
        out_votes[o] = best.cnt;
        out_n[o] = n_list;
        if (out_first_dist) out_first_dist[o] = best.cnt ? knn_key_dist(best.key) : nan;
      }
    };
    const uint32_t nm = m_n[row];
    if (nm == 0) {  // no list: no distance of the row is a number, every column is left out, or the set is empty
      const KnnBest none = {0u, 0u, KPOP_NO_CLASS, kKNone};
      for (uint32_t t = 0; t < ks.n; ++t) write(t, none, 0u);
      continue;
    }
    const uint64_t tau_K = m_tau[row];
    const bool flagged = m_flag[row] != 0;
    __syncthreads();  // (the row before is done with the lists)
    if (threadIdx.x == 0) s_nt = 0;
    for (uint32_t q = threadIdx.x; q < nm; q += 64) {
      const uint32_t idx = m_idx[(uint64_t)row * k + q];
      s_k[q] = m_key[(uint64_t)row * k + q];
      s_i[q] = idx;
      s_c[q] = class_of[idx];
      s_cnt[q] = 0;
    }
    __syncthreads();
    // the place that stands for an entry's class; none for a class that is not below n_classes: it counts in out_n, votes for nobody
    for (uint32_t q = threadIdx.x; q < nm; q += 64) {
      const uint32_t c = s_c[q];
      uint32_t f = 0;
      while (s_c[f] != c) ++f;  // (f <= q)
      s_rep[q] = c < n_classes ? f : kNoPlace;
    }
    // the ties of tau_K that the segments' lists hold outside the merged list: behind slot kKMaxK, in any order (their order is the index)
    const uint32_t last_idx = s_i[nm - 1];
    if (!flagged)
      for (uint32_t e = threadIdx.x; e < n_seg * k; e += 64) {
        const uint32_t s = e / k, q = e % k;
        const uint64_t o = (uint64_t)s * r2 + row;
        if (q < seg_n[o] && seg_key[o * k + q] == tau_K) {
          const uint32_t idx = seg_idx[o * k + q];
          if (idx > last_idx) {
            const uint32_t slot = kKMaxK + atomicAdd(&s_nt, 1u);  // (at most kKMaxTies of them: knn_merge_kernel flags the row otherwise)
            s_k[slot] = tau_K;
            s_i[slot] = idx;
            s_c[slot] = class_of[idx];
          }
        }
      }
    __syncthreads();
    const uint32_t nt = s_nt;
    // the merged entries at or below a key: a prefix
    auto at_or_below = [&](uint64_t key) {
      uint32_t lo = 0, hi = nm;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_k[mid] <= key) lo = mid + 1;
        else hi = mid;
      }
      return lo;
    };
    uint32_t done = 0;  // the prefix already counted
    auto extend = [&](uint32_t end) {
      for (uint32_t q = done + threadIdx.x; q < end; q += 64) {
        const uint32_t f = s_rep[q];
        if (f != kNoPlace) atomicAdd(&s_cnt[f], 1u);
      }
      done = max(done, end);
      __syncthreads();
    };
    bool have_last = false;
    KnnBest last = {0u, 0u, KPOP_NO_CLASS, kKNone};
    uint32_t last_n = 0;
    for (uint32_t t = 0; t < ks.n; ++t) {
      const uint64_t tau = s_k[min(ks.k[t], nm) - 1];
      KnnBest best = {0u, 0u, KPOP_NO_CLASS, kKNone};
      if (tau != tau_K) {  // the group of tau is inside the merged list
        const uint32_t end = at_or_below(tau);
        extend(end);
        for (uint32_t q = threadIdx.x; q < end; q += 64) {
          if (s_rep[q] != q) continue;
          const KnnBest cand = {s_cnt[q], s_i[q], s_c[q], s_k[q]};
          if (knn_better(cand, best)) best = cand;
        }
        write(t, reduce(best), end);
        __syncthreads();  // (the counts are read before the next cut adds to them)
        continue;
      }
      if (!have_last) {
        have_last = true;
        // flagged: the merged list below tau_K, the whole group from the tables; unflagged: the merged list, the rest of the group
        // from the lists
        const uint32_t end = flagged ? at_or_below(tau_K - 1) : nm;  // (tau_K > 0: a key has its top bit set or is a negative number's complement)
        extend(end);
        for (uint32_t q = threadIdx.x; q < end; q += 64) {
          if (s_rep[q] != q) continue;
          const uint32_t c = s_c[q];
          uint32_t cnt = s_cnt[q];
          if (flagged) cnt += tie_count[(uint64_t)row * n_classes + c];
          else
            for (uint32_t e = 0; e < nt; ++e) cnt += s_c[kKMaxK + e] == c ? 1u : 0u;
          const KnnBest cand = {cnt, s_i[q], c, s_k[q]};
          if (knn_better(cand, best)) best = cand;
        }
        if (flagged) {  // the classes that only the tie group holds
          last_n = end + tie_total[row];
          for (uint32_t c = threadIdx.x; c < n_classes; c += 64) {
            const uint32_t tc = tie_count[(uint64_t)row * n_classes + c];
            if (tc == 0) continue;
            bool below = false;
            for (uint32_t f = 0; f < end; ++f) below = below || s_c[f] == c;
            if (below) continue;
            const KnnBest cand = {tc, tie_first[(uint64_t)row * n_classes + c], c, tau_K};
            if (knn_better(cand, best)) best = cand;
          }
        } else {  // the classes that only the ties outside the merged list hold: the first of them stands for its class
          last_n = nm + nt;
          for (uint32_t e = threadIdx.x; e < nt; e += 64) {
            const uint32_t c = s_c[kKMaxK + e], idx = s_i[kKMaxK + e];
            if (c >= n_classes) continue;
            bool inside = false;
            for (uint32_t f = 0; f < nm; ++f) inside = inside || s_c[f] == c;
            if (inside) continue;
            uint32_t cnt = 0;
            bool first = true;
            for (uint32_t f = 0; f < nt; ++f) {
              if (s_c[kKMaxK + f] != c) continue;
              ++cnt;
              if (s_i[kKMaxK + f] < idx) first = false;
            }
            if (!first) continue;
            const KnnBest cand = {cnt, idx, c, tau_K};
            if (knn_better(cand, best)) best = cand;
          }
        }
        last = reduce(best);
      }
      write(t, last, last_n);
    }
  }
}

// out_correct[t]: the rows of slice t whose class is their own (KPOP_NO_CLASS is never correct).  A block a slice; integers
__global__ __launch_bounds__(1024) void knn_correct_kernel(const uint32_t *__restrict__ out_class, const uint32_t *__restrict__ class_of, uint32_t first_row,
                                                           uint32_t n_rows, unsigned long long *__restrict__ out_correct) {
  __shared__ unsigned long long s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint32_t row = threadIdx.x; row < n_rows; row += 1024) {
    const uint32_t c = out_class[(uint64_t)blockIdx.x * n_rows + row];
    mine += (c != KPOP_NO_CLASS && c == class_of[first_row + row]) ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_sum, mine);
  __syncthreads();
  if (threadIdx.x == 0) out_correct[blockIdx.x] = s_sum;
}

// ks: not empty, strictly ascending, each in 1..128, at most 32 of them -> the cut points by value and K, the last
static int knn_check_ks(const uint32_t *ks, uint32_t n_ks, const char *who, KnnKs *out) {
  if (n_ks == 0 || !ks) KPOP_FAIL(KPOP_ERR_INVALID, "%s: no k", who);
  if (n_ks > kKMaxKs) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u values of k (at most %u)", who, n_ks, kKMaxKs);
  out->n = n_ks;
  for (uint32_t t = 0; t < kKMaxKs; ++t) out->k[t] = 0;
  for (uint32_t t = 0; t < n_ks; ++t) {
    if (ks[t] == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: k = 0", who);
    if (t && ks[t] <= ks[t - 1]) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the values of k are not strictly ascending (%u after %u)", who, ks[t], ks[t - 1]);
    if (ks[t] > (uint32_t)kKMaxK) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: k = %u (at most %d)", who, ks[t], kKMaxK);
    out->k[t] = ks[t];
  }
  return 0;
}

static void knn_vote_ks_launch(const KnnWork &w, uint32_t n_seg, uint32_t rows, uint32_t K, const uint32_t *d_class_of, uint32_t n_classes, const KnnKs &ks,
                               uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist, hipStream_t st) {
  knn_vote_ks_kernel<<<dim3(std::min(rows, 1u << 20)), dim3(64), 0, st>>>(w.seg_key, w.seg_idx, w.seg_n, n_seg, rows, K, w.m_key, w.m_idx, w.m_n, w.m_tau, w.m_flag,
                                                                         d_class_of, n_classes, w.tie_total, w.tie_count, w.tie_first, ks, d_out_class, d_out_votes,
                                                                         d_out_n, d_out_first_dist);
}

// the body of the many-k vote's entry points: enqueues only
static int vote_ks_dev(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2, const uint32_t *ks_host, uint32_t n_ks,
                       void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist, hipStream_t st, const char *who) {
  KnnKs ks;
  KPOP_TRY(knn_check_ks(ks_host, n_ks, who, &ks));
  const uint32_t K = ks.k[n_ks - 1];
  KPOP_TRY(knn_check_sizes(K, n_classes, who));
  if (r2 == 0) return KPOP_OK;
  if (!d_out_class || !d_out_votes || !d_out_n || !d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 && (!d_class_of || !d_m2)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  if (div_up(r2, 16) > 0x7FFFFFFFull) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u query rows", who, r2);
  const KnnWork w = knn_carve(d_work, r2, K, n_classes, D, rs->normalize != 0);
  uint32_t n_seg = 0;
  if (r1 == 0) {
    KPOP_HIP(hipMemsetAsync(w.m_n, 0, (uint64_t)r2 * 4, st));  // every list is empty
  } else {
    KPOP_HIP(hipMemsetAsync(reinterpret_cast<char *>(d_work) + w.tables_off, 0, w.tables_bytes, st));
    KPOP_HIP(hipMemsetAsync(w.tie_first, 0xFF, (uint64_t)r2 * n_classes * 4, st));
    const double *a = rs->rows, *b = d_m2;
    if (rs->normalize) {  // the set's quotients from its copy, the query rows' from the norms' pass: knn_dev's
      KPOP_TRY(rs->prepared(st));
      KPOP_TRY(rs->divided(st, &a));
      KPOP_TRY(refset_query_norms(rs, d_m2, r2, w.n2, w.b, st));
      b = w.b;
    }
    KPOP_TRY(knn_run_passes(rs->kind, a, r1, b, r2, D, rs->metric, rs->p, K, d_class_of, n_classes, w, &n_seg, st));
  }
  knn_vote_ks_launch(w, n_seg, r2, K, d_class_of, n_classes, ks, d_out_class, d_out_votes, d_out_n, d_out_first_dist, st);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

template <int KIND, int TY, int W>
static int knnv_passes(const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p, uint32_t k,
                       const uint32_t *group_of, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg_out, hipStream_t st) {
  constexpr uint32_t TJ = KnnShape<TY, W>::TJ;
  const uint32_t n_ct = div_up(r1, W), strips = div_up(n_rows, TJ);
  const uint32_t n_seg_max = std::max(1u, std::min(knn_max_segments(n_rows, TJ), n_ct));
  const uint32_t tiles_per_seg = div_up(n_ct, n_seg_max), n_seg = div_up(n_ct, tiles_per_seg);  // (no segment is empty)
  *n_seg_out = n_seg;
  const dim3 grid(strips, n_seg);
  knnv_nearest_kernel<KIND, TY, W><<<grid, dim3(256), 0, st>>>(a, r1, first_row, n_rows, n_dims, metric, p, k, n_ct, tiles_per_seg, group_of, w.seg_key, w.seg_idx,
                                                            w.seg_n, w.seg_drop);
  KPOP_LAUNCH_CHECK();
  KPOP_TRY(knn_run_merge(w, n_seg, n_rows, k, st));
  knnv_ties_kernel<KIND, TY, W><<<grid, dim3(256), 0, st>>>(a, r1, first_row, n_rows, n_dims, metric, p, n_ct, tiles_per_seg, group_of, class_of, n_classes, w.m_tau,
                                                         w.m_flag, w.tie_total, w.tie_count, w.tie_first);
  KPOP_LAUNCH_CHECK();
  return 0;
}

template <int KIND>
static int knnv_passes_of(const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p, uint32_t k,
                          const uint32_t *group_of, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg, hipStream_t st) {
  const uint32_t TJ = knn_strip_rows(k);
  if (TJ == 64) return knnv_passes<KIND, 4, 64>(a, r1, first_row, n_rows, n_dims, metric, p, k, group_of, class_of, n_classes, w, n_seg, st);
  if (TJ == 32) return knnv_passes<KIND, 2, 64>(a, r1, first_row, n_rows, n_dims, metric, p, k, group_of, class_of, n_classes, w, n_seg, st);
  return knnv_passes<KIND, 1, 64>(a, r1, first_row, n_rows, n_dims, metric, p, k, group_of, class_of, n_classes, w, n_seg, st);
}

// the body of the validation's entry points: enqueues only.  The workspace is the vote's without a query side
static int validate_dev(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const uint32_t *d_group_of, uint32_t first_row, uint32_t n_rows,
                        const uint32_t *ks_host, uint32_t n_ks, void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n,
                        double *d_out_first_dist, uint64_t *d_out_correct, hipStream_t st, const char *who) {
  KnnKs ks;
  KPOP_TRY(knn_check_ks(ks_host, n_ks, who, &ks));
  const uint32_t K = ks.k[n_ks - 1];
  KPOP_TRY(knn_check_sizes(K, n_classes, who));
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if ((uint64_t)first_row + n_rows > r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: rows %u .. %llu of a set of %u", who, first_row, (unsigned long long)first_row + n_rows, r1);
  if (!d_out_correct) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  if (n_rows == 0) {
    KPOP_HIP(hipMemsetAsync(d_out_correct, 0, (uint64_t)n_ks * 8, st));
    return KPOP_OK;
  }
  if (!d_out_class || !d_out_votes || !d_out_n || !d_work || !d_class_of) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const KnnWork w = knn_carve(d_work, n_rows, K, n_classes, D, false);
  KPOP_HIP(hipMemsetAsync(reinterpret_cast<char *>(d_work) + w.tables_off, 0, w.tables_bytes, st));
  KPOP_HIP(hipMemsetAsync(w.tie_first, 0xFF, (uint64_t)n_rows * n_classes * 4, st));
  const double *a = rs->rows;
  if (rs->normalize) {  // both operands the set's divided copy: clusters.hip's
    KPOP_TRY(rs->prepared(st));
    KPOP_TRY(rs->divided(st, &a));
  }
  uint32_t n_seg = 0;
  switch (rs->kind) {
    case KPOP_EUCLIDEAN:
      KPOP_TRY(knnv_passes_of<KPOP_EUCLIDEAN>(a, r1, first_row, n_rows, D, rs->metric, rs->p, K, d_group_of, d_class_of, n_classes, w, &n_seg, st));
      break;
    case KPOP_COSINE: KPOP_TRY(knnv_passes_of<KPOP_COSINE>(a, r1, first_row, n_rows, D, rs->metric, rs->p, K, d_group_of, d_class_of, n_classes, w, &n_seg, st)); break;
    default: KPOP_TRY(knnv_passes_of<KPOP_MINKOWSKI>(a, r1, first_row, n_rows, D, rs->metric, rs->p, K, d_group_of, d_class_of, n_classes, w, &n_seg, st)); break;
  }
  knn_vote_ks_launch(w, n_seg, n_rows, K, d_class_of, n_classes, ks, d_out_class, d_out_votes, d_out_n, d_out_first_dist, st);
  KPOP_LAUNCH_CHECK();
  knn_correct_kernel<<<dim3(n_ks), dim3(1024), 0, st>>>(d_out_class, d_class_of, first_row, n_rows, reinterpret_cast<unsigned long long *>(d_out_correct));
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

// the rows of a call of a host form: as many as keep the workspace bounded (a quarter of a GiB, or what 64 rows take) -- kpop_knn_vote's
// rule.  query_bytes: what a row's query side takes beside the lists and the tables
static uint32_t knn_rows_a_call(uint32_t rows, uint32_t K, uint32_t n_classes, uint32_t n_dims, bool normalize, uint32_t n_ks, uint64_t query_bytes) {
  const uint64_t per_row = knn_carve(nullptr, 1024, K, n_classes, n_dims, normalize).bytes / 1024 + query_bytes + (uint64_t)n_ks * 20 + 32;
  return (uint32_t)std::min<uint64_t>(rows, std::max<uint64_t>(64, (256ull << 20) / per_row));
}

// slices [n_ks][nr] of a call -> the caller's [n_ks][rows] at row j0
template <class T>
static int knn_slices_back(T *out, uint32_t rows, uint32_t j0, const DevBuf &from, uint32_t nr, uint32_t n_ks, hipStream_t st) {
  for (uint32_t t = 0; t < n_ks; ++t)
    KPOP_HIP(hipMemcpyAsync(out + (uint64_t)t * rows + j0, reinterpret_cast<const T *>(from.p) + (uint64_t)t * nr, (uint64_t)nr * sizeof(T), hipMemcpyDeviceToHost, st));
  return 0;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_knn_ks_vote_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k_max, uint32_t n_classes) {
  if (!rs) return 0;
  return knn_carve(nullptr, r2, k_max, n_classes, rs->n_dims, rs->normalize != 0).bytes;
}

extern "C" int kpop_dev_knn_ks_vote(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2, const uint32_t *ks,
                                    uint32_t n_ks, void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist,
                                    void *stream) {
  const char *who = "kpop_dev_knn_ks_vote";
  KPOP_TRY(refset_check_handle(rs, who));
  return vote_ks_dev(rs, d_class_of, n_classes, d_m2, r2, ks, n_ks, d_work, d_out_class, d_out_votes, d_out_n, d_out_first_dist, as_stream(stream), who);
}

extern "C" int kpop_knn_ks_vote(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const double *m2, uint32_t r2, const uint32_t *ks, uint32_t n_ks,
                                uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n, double *out_first_dist) {
  const char *who = "kpop_knn_ks_vote";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KnnKs cuts;
  KPOP_TRY(knn_check_ks(ks, n_ks, who, &cuts));
  const uint32_t K = cuts.k[n_ks - 1];
  KPOP_TRY(knn_check_sizes(K, n_classes, who));
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if ((r1 && !class_of) || (r2 && (!out_class || !out_votes || !out_n)) || (r1 && r2 && !m2)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  for (uint32_t i = 0; i < r1; ++i)
    if (class_of[i] >= n_classes) KPOP_FAIL(KPOP_ERR_INVALID, "%s: row %u has class %u of %u", who, i, class_of[i], n_classes);
  if (r2 == 0) return KPOP_OK;
  hipStream_t st = nullptr;
  const uint32_t chunk = knn_rows_a_call(r2, K, n_classes, D, rs->normalize != 0, n_ks, (uint64_t)D * 8);
  DevBuf dc, d2, dw, ocl, ovo, on, ofd;
  KPOP_TRY(dc.alloc((uint64_t)r1 * 4));
  KPOP_TRY(d2.alloc((uint64_t)chunk * D * 8));
  // (the last chunk may be cut into more segments than a whole one: the larger of the two workspaces)
  KPOP_TRY(dw.alloc(std::max(kpop_dev_knn_ks_vote_workspace_bytes(rs, chunk, K, n_classes),
                             kpop_dev_knn_ks_vote_workspace_bytes(rs, r2 % chunk ? r2 % chunk : chunk, K, n_classes))));
  KPOP_TRY(ocl.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(ovo.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(on.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(ofd.alloc((uint64_t)n_ks * chunk * 8));
  if (r1) KPOP_HIP(hipMemcpyAsync(dc.p, class_of, (uint64_t)r1 * 4, hipMemcpyHostToDevice, st));
  for (uint32_t j0 = 0; j0 < r2; j0 += chunk) {
    const uint32_t nr = std::min(chunk, r2 - j0);
    if (r1) KPOP_HIP(hipMemcpyAsync(d2.p, m2 + (uint64_t)j0 * D, (uint64_t)nr * D * 8, hipMemcpyHostToDevice, st));
    KPOP_TRY(vote_ks_dev(rs, dc.as<uint32_t>(), n_classes, d2.as<double>(), nr, ks, n_ks, dw.p, ocl.as<uint32_t>(), ovo.as<uint32_t>(), on.as<uint32_t>(),
                         ofd.as<double>(), st, who));
    KPOP_TRY(knn_slices_back(out_class, r2, j0, ocl, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_votes, r2, j0, ovo, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_n, r2, j0, on, nr, n_ks, st));
    if (out_first_dist) KPOP_TRY(knn_slices_back(out_first_dist, r2, j0, ofd, nr, n_ks, st));
    KPOP_HIP(hipStreamSynchronize(st));
  }
  return KPOP_OK;
}

extern "C" uint64_t kpop_dev_knn_validate_workspace_bytes(const kpop_refset *rs, uint32_t n_rows, uint32_t k_max, uint32_t n_classes) {
  if (!rs) return 0;
  return knn_carve(nullptr, n_rows, k_max, n_classes, rs->n_dims, false).bytes;
}

extern "C" int kpop_dev_knn_validate(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const uint32_t *d_group_of, uint32_t first_row,
                                     uint32_t n_rows, const uint32_t *ks, uint32_t n_ks, void *d_work, uint32_t *d_out_class, uint32_t *d_out_votes,
                                     uint32_t *d_out_n, double *d_out_first_dist, uint64_t *d_out_correct, void *stream) {
  const char *who = "kpop_dev_knn_validate";
  KPOP_TRY(refset_check_handle(rs, who));
  return validate_dev(rs, d_class_of, n_classes, d_group_of, first_row, n_rows, ks, n_ks, d_work, d_out_class, d_out_votes, d_out_n, d_out_first_dist, d_out_correct,
                      as_stream(stream), who);
}

extern "C" int kpop_knn_validate(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const uint32_t *group_of, const uint32_t *ks, uint32_t n_ks,
                                 uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n, double *out_first_dist, uint64_t *out_correct) {
  const char *who = "kpop_knn_validate";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KnnKs cuts;
  KPOP_TRY(knn_check_ks(ks, n_ks, who, &cuts));
  const uint32_t K = cuts.k[n_ks - 1];
  KPOP_TRY(knn_check_sizes(K, n_classes, who));
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (!out_correct || (r1 && (!class_of || !out_class || !out_votes || !out_n))) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  for (uint32_t i = 0; i < r1; ++i)
    if (class_of[i] >= n_classes) KPOP_FAIL(KPOP_ERR_INVALID, "%s: row %u has class %u of %u", who, i, class_of[i], n_classes);
  for (uint32_t t = 0; t < n_ks; ++t) out_correct[t] = 0;
  if (r1 == 0) return KPOP_OK;
  hipStream_t st = nullptr;
  // the set's rows in ranges that keep the workspace bounded; the query side of a range is the set's own (divided) rows: nothing a row
  const uint32_t chunk = knn_rows_a_call(r1, K, n_classes, D, false, n_ks, 0);
  DevBuf dc, dg, dw, ocl, ovo, on, ofd, oco;
  KPOP_TRY(dc.alloc((uint64_t)r1 * 4));
  if (group_of) KPOP_TRY(dg.alloc((uint64_t)r1 * 4));
  // (the last range may be cut into more segments than a whole one: the larger of the two workspaces)
  KPOP_TRY(dw.alloc(std::max(kpop_dev_knn_validate_workspace_bytes(rs, chunk, K, n_classes),
                             kpop_dev_knn_validate_workspace_bytes(rs, r1 % chunk ? r1 % chunk : chunk, K, n_classes))));
  KPOP_TRY(ocl.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(ovo.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(on.alloc((uint64_t)n_ks * chunk * 4));
  KPOP_TRY(ofd.alloc((uint64_t)n_ks * chunk * 8));
  KPOP_TRY(oco.alloc((uint64_t)kKMaxKs * 8));
  KPOP_HIP(hipMemcpyAsync(dc.p, class_of, (uint64_t)r1 * 4, hipMemcpyHostToDevice, st));
  if (group_of) KPOP_HIP(hipMemcpyAsync(dg.p, group_of, (uint64_t)r1 * 4, hipMemcpyHostToDevice, st));
  for (uint32_t j0 = 0; j0 < r1; j0 += chunk) {
    const uint32_t nr = std::min(chunk, r1 - j0);
    uint64_t correct[kKMaxKs];
    KPOP_TRY(validate_dev(rs, dc.as<uint32_t>(), n_classes, group_of ? dg.as<uint32_t>() : nullptr, j0, nr, ks, n_ks, dw.p, ocl.as<uint32_t>(), ovo.as<uint32_t>(),
                          on.as<uint32_t>(), ofd.as<double>(), oco.as<uint64_t>(), st, who));
    KPOP_TRY(knn_slices_back(out_class, r1, j0, ocl, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_votes, r1, j0, ovo, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_n, r1, j0, on, nr, n_ks, st));
    if (out_first_dist) KPOP_TRY(knn_slices_back(out_first_dist, r1, j0, ofd, nr, n_ks, st));
    KPOP_HIP(hipMemcpyAsync(correct, oco.p, (uint64_t)n_ks * 8, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipStreamSynchronize(st));
    for (uint32_t t = 0; t < n_ks; ++t) out_correct[t] += correct[t];
  }
  return KPOP_OK;
}

extern "C" int kpop_distance_knn_validate(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                          const uint32_t *class_of, uint32_t n_classes, const uint32_t *group_of, const uint32_t *ks, uint32_t n_ks,
                                          uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n, double *out_first_dist, uint64_t *out_correct) {
  kpop_refset *rs = nullptr;
  KPOP_TRY(kpop_refset_create(m, rows, n_dims, metric, kind, p, normalize, 0, &rs));
  const int rc = kpop_knn_validate(rs, class_of, n_classes, group_of, ks, n_ks, out_class, out_votes, out_n, out_first_dist, out_correct);
  const int rc_free = kpop_refset_free(rs);
  return rc ? rc : rc_free;
}
