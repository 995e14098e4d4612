// knn.hip -- the k-NN vote: classify query rows against a labelled resident set.
//
//   The list of query row j: the set rows whose distance to j is a number, ordered by (d with -0 taken as +0, index) ascending; its
//   first k, plus every further row whose distance equals the k-th one -- eff_len of summarize_distance_matrix_row
//   (lib/Matrix.ml:641-650): whole tie groups.  The vote (the reference's README.md:773-775): the class with the most members in the
//   list; among classes with equally many, the one whose nearest member comes first in the list's order.  d(j, i) is the reference
//   chain's distance (lib/Space.ml:182-205 with the adaptors of lib/Matrix.ml:243-250): the bits of distance_rowwise_kernel
//   (distance.hip), whatever kpop_tune says -- no setting is read here.  Neither the r2 x r1 matrix nor a list longer than k a row
//   is formed; every step is a function of the distances alone: the same bits on every run.
//
// Four launches, always the same four (the device form reads nothing back):
//   knn_nearest_kernel   the arithmetic of distance_rowwise_kernel, operation for operation (pair_tile.h).  A workgroup owns a
//                        strip of TJ query rows and walks the column tiles of its segment of the set, columns ascending.  Every row
//                        has in LDS the sorted list of its k smallest (key, index) so far and the list's bound, its k-th key.  A
//                        thread compares its 4 x TY finished distances with the bound; after the first tiles almost nothing passes.
//                        What passes is inserted by the row's wavefront, one candidate at a time, the lanes side by side over the
//                        list's slots (a row belongs to ONE wavefront: no other touches its list).  The k smallest of a set under a
//                        strict order do not depend on the order of arrival.  Beside each list a count of DROPPED TIES: the entries
//                        refused or evicted whose key equals the list's current k-th key, reset whenever that key changes.  The rows
//                        of a strip by k, so that the lists fit the LDS (KnnShape, knn_strip_rows); the columns in as many segments
//                        as make about kKBlocks workgroups with the strips, so that a few query rows still fill the chip.
//   knn_merge_kernel     per row: the segments' lists merged, tau = the k-th key (the largest, if there are fewer than k).  A
//                        segment's k-th key never lies below tau, so an entry equal to tau can only have been dropped while that
//                        segment's bound was tau -- and the bound stays there afterwards.  Hence: the tie group of tau is held whole
//                        by the segments' lists unless a segment whose final k-th key is tau reports dropped ties: the row is FLAGGED
//                        (also when the lists hold more entries at tau than knn_vote_kernel has room for: kKMaxTies).
//   knn_ties_kernel      the same tile loop; a workgroup returns at once unless one of its rows is flagged (the common case: no tie
//                        group longer than k slots hold).  For a flagged row every column with key == tau adds 1 to
//                        tie_count[row][class] and takes atomicMin of its index into tie_first[row][class]: sums and minima do not
//                        depend on the order, and all entries of a tie group share one distance, so their order is their index.
//   knn_vote_kernel      per row: the classes of the entries below tau are tallied; the tie group comes from the segments' lists
//                        (unflagged) or from the tables (flagged); the winner by (count descending, first (key, index) ascending).
// The chain makes no -0 (a sum of terms added to +0, its square root, half or power): a key gives back the distance's bits.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "distance_routes.h"
#include "knn_lists.h"
#include "pair_tile.h"
#include "refset.h"
#include "space_ops.h"

namespace kpop {

// (a row's list and its insertion, the shapes, the workspace and the limits: knn_lists.h, shared with knn_validate.hip)
// The two kernels over the pairs walk their tiles with the sweep of pair_tile.h.  a: the set's rows, b: the query rows, both as the chain
// reads them (divided by their rows' norms when the set normalises).  A workgroup's rows j0 .. j1 (at most TJ), its column tiles
// t_begin .. t_end of W rows of the set each; no thread is idle.

// Who is left out of a row's list.  The vote: nobody -- every call folds away.  The validation (knn_validate.hip), whose query rows are
// rows of the set: row j itself, or every row of j's group.  A thread knows its rows' groups (or their indices in the set) for the
// launch, the tile's four columns' groups for the tile.  left_out(yy, x, i): column i, the thread's x-th, is not a neighbour of its
// yy-th row
struct KnnNobodyLeftOut {
  __device__ __forceinline__ void rows(const uint32_t *, uint32_t, uint32_t) {}
  __device__ __forceinline__ void columns(uint32_t, uint32_t) {}
  __device__ __forceinline__ bool left_out(int, int, uint32_t) const { return false; }
};
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

// Strip blockIdx.x: query rows j0 .. j0 + TJ; segment blockIdx.y.  seg_key, seg_idx: [segment][r2][k], the list's first seg_n
// entries ascending; seg_drop: the dropped ties of the list's last key.  TJ k <= SLOTS (the launch sees to it).  Who: who is left out;
// group_of, first_row are read by KnnvLeftOut alone (the query rows are then rows first_row .. first_row + r2 of the set).  A column
// that is left out is refused before it can be inserted OR counted as a dropped tie: a row whose own index ties with its k-th key would
// otherwise flag itself.
template <int KIND, int TY, int W, class Who>
__global__ __launch_bounds__(256, 1) void knn_nearest_kernel(const double *__restrict__ a, uint32_t r1, const double *__restrict__ b, uint32_t r2, uint32_t n_dims,
                                                             const double *__restrict__ metric, double p, uint32_t k, uint32_t n_ct, uint32_t tiles_per_seg,
                                                             const uint32_t *__restrict__ group_of, uint32_t first_row, uint64_t *__restrict__ seg_key,
                                                             uint32_t *__restrict__ seg_idx, uint32_t *__restrict__ seg_n, uint32_t *__restrict__ seg_drop) {
  using S = KnnShape<TY, W>;
  constexpr uint32_t TJ = S::TJ;
  __shared__ __attribute__((aligned(16))) double As[kPairDC][W + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][TJ + 2];
  __shared__ double s_metric[kPairDC];
  __shared__ uint64_t s_key[S::SLOTS];
  __shared__ uint32_t s_idx[S::SLOTS];
  __shared__ uint64_t s_bound[TJ];
  __shared__ uint32_t s_n[TJ], s_drop[TJ], s_bidx[TJ];
  const uint32_t j0 = blockIdx.x * TJ, j1 = min(r2, j0 + TJ);  // (the grid has div_up(r2, TJ) strips: j0 < r2)
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
  Who out;
  out.rows(group_of, first_row + j0 + tj, r1);
  const PairTilesOf tiles{W, min(r1, t_end * W)};
  const PairRows set{a, r1}, query{b, r2};
  PairStage<W, TJ> stage;
  // (a function of its own and not the loop's text: written into the loop the insertion's compares come out if-converted otherwise and
  // the vote and the validation ran 1.5 to 2 % slower, profiles/pair_sweep_refactor.md, section 4)
  const auto epilogue = [&](uint32_t i0, uint32_t i1, double(&acc)[TY][4]) {
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
        const uint64_t key = distance_key(d);
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
  };
  PairTile cur = tiles.at(t_begin * W), nxt;
  for (pair_sweep_open(stage, set, cur, query, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = tiles.after(cur);
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, set, cur, nxt, query, j0, j1, n_dims, metric, p, ti, tj, true);
    epilogue(cur.i0, cur.i1, acc);
  }
  __syncthreads();
  const uint32_t seg = blockIdx.y;
  for (uint32_t e = threadIdx.x; e < TJ * k; e += 256) {
    const uint32_t row = e / k, q = e % k;
    if (j0 + row < j1) {
      const uint64_t o = ((uint64_t)seg * r2 + j0 + row) * k + q;
      const bool in = q < s_n[row];
      seg_key[o] = in ? s_key[e] : kKNone;
      seg_idx[o] = in ? s_idx[e] : 0u;
    }
  }
  if (threadIdx.x < TJ && j0 + threadIdx.x < j1) {
    seg_n[(uint64_t)seg * r2 + j0 + threadIdx.x] = s_n[threadIdx.x];
    seg_drop[(uint64_t)seg * r2 + j0 + threadIdx.x] = s_drop[threadIdx.x];
  }
}

// a block of 64 a row: every entry's place in the merged list is its place in its own segment's list plus its lower bounds in the
// others (the pairs of a row are all distinct: they differ in the index) -- within_merge_kernel's.  m_key, m_idx: [r2][k], the first
// m_n entries; m_tau: the last of them; m_flag: the tie group of tau is not whole in the segments' lists
__global__ __launch_bounds__(64) void knn_merge_kernel(const uint64_t *__restrict__ seg_key, const uint32_t *__restrict__ seg_idx, const uint32_t *__restrict__ seg_n,
                                                       const uint32_t *__restrict__ seg_drop, uint32_t n_seg, uint32_t r2, uint32_t k, uint64_t *__restrict__ m_key,
                                                       uint32_t *__restrict__ m_idx, uint32_t *__restrict__ m_n, uint64_t *__restrict__ m_tau, uint32_t *__restrict__ m_flag) {
  __shared__ uint64_t s_k[kKMaxK];
  __shared__ uint32_t s_i[kKMaxK];
  __shared__ uint32_t s_ties, s_total;
  __shared__ unsigned long long s_least;
  for (uint32_t row = blockIdx.x; row < r2; row += gridDim.x) {
    __syncthreads();  // (the row before has read s_k and the three words)
    if (threadIdx.x == 0) {
      s_ties = 0;
      s_total = 0;
      s_least = kKNone;
    }
    __syncthreads();
    // the lists' lengths in all, and the least k-th key of a full list: k entries lie at or below it, so nothing above it is among the
    // k smallest -- most of what the segments hold, and it is not looked at again
    for (uint32_t s = threadIdx.x; s < n_seg; s += 64) {
      const uint64_t o = (uint64_t)s * r2 + row;
      const uint32_t ns = seg_n[o];
      if (ns) atomicAdd(&s_total, ns);
      if (ns == k) atomicMin(&s_least, (unsigned long long)seg_key[o * k + k - 1]);
    }
    __syncthreads();
    const uint32_t nm = min(s_total, k);
    const uint64_t least = s_least;
    for (uint32_t e = threadIdx.x; e < n_seg * k; e += 64) {
      const uint32_t s = e / k, q = e % k;
      if (q >= seg_n[(uint64_t)s * r2 + row]) continue;
      const uint64_t base = ((uint64_t)s * r2 + row) * k;
      const uint64_t key = seg_key[base + q];
      if (key > least) continue;
      const uint32_t idx = seg_idx[base + q];
      uint32_t rank = q;
      for (uint32_t s2 = 0; s2 < n_seg && rank < k; ++s2) {
        if (s2 == s) continue;
        const uint64_t b2 = ((uint64_t)s2 * r2 + row) * k;
        uint32_t lo = 0, hi = seg_n[(uint64_t)s2 * r2 + row];
        while (lo < hi) {  // the first entry of the list that is not below (key, idx)
          const uint32_t mid = (lo + hi) >> 1;
          if (key_less(seg_key[b2 + mid], seg_idx[b2 + mid], key, idx)) lo = mid + 1;
          else hi = mid;
        }
        rank += lo;
      }
      if (rank < k) {
        s_k[rank] = key;
        s_i[rank] = idx;
      }
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < nm; q += 64) {
      m_key[(uint64_t)row * k + q] = s_k[q];
      m_idx[(uint64_t)row * k + q] = s_i[q];
    }
    const uint64_t tau = nm ? s_k[nm - 1] : kKNone;
    // the ties of tau that the lists hold: more than knn_vote_kernel has room for, and the tables take over
    uint32_t ties = 0;
    for (uint32_t e = threadIdx.x; e < n_seg * k; e += 64) {
      const uint64_t o = (uint64_t)(e / k) * r2 + row;
      ties += (e % k < seg_n[o] && seg_key[o * k + e % k] == tau) ? 1u : 0u;
    }
    if (ties) atomicAdd(&s_ties, ties);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t flag = (nm && s_ties > (uint32_t)kKMaxTies) ? 1u : 0u;
      if (nm == k)
        for (uint32_t s = 0; s < n_seg; ++s) {
          const uint64_t o = (uint64_t)s * r2 + row;
          if (seg_n[o] == k && seg_key[o * k + k - 1] == tau && seg_drop[o] > 0) flag = 1;
        }
      m_n[row] = nm;
      m_tau[row] = tau;
      m_flag[row] = flag;
    }
  }
}

// the grid of knn_nearest_kernel.  tie_total: [r2], every column of a flagged row at tau; tie_count, tie_first: [r2][n_classes], those
// of a class and the least index among them (0xFFFFFFFF: none), none of them left out.  class_of is trusted, every table access guarded
template <int KIND, int TY, int W, class Who>
__global__ __launch_bounds__(256, 1) void knn_ties_kernel(const double *__restrict__ a, uint32_t r1, const double *__restrict__ b, uint32_t r2, uint32_t n_dims,
                                                          const double *__restrict__ metric, double p, uint32_t n_ct, uint32_t tiles_per_seg,
                                                          const uint32_t *__restrict__ group_of, uint32_t first_row, const uint32_t *__restrict__ class_of,
                                                          uint32_t n_classes, const uint64_t *__restrict__ m_tau, const uint32_t *__restrict__ m_flag,
                                                          uint32_t *tie_total, uint32_t *tie_count, uint32_t *tie_first) {
  using S = KnnShape<TY, W>;
  constexpr uint32_t TJ = S::TJ;
  __shared__ __attribute__((aligned(16))) double As[kPairDC][W + 2];
  __shared__ __attribute__((aligned(16))) double Bs[kPairDC][TJ + 2];
  __shared__ double s_metric[kPairDC];
  const uint32_t j0 = blockIdx.x * TJ, j1 = min(r2, j0 + TJ);
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
  Who out;
  out.rows(group_of, first_row + j0 + tj, r1);
  const PairTilesOf tiles{W, min(r1, t_end * W)};
  const PairRows set{a, r1}, query{b, r2};
  PairStage<W, TJ> stage;
  PairTile cur = tiles.at(t_begin * W), nxt;
  for (pair_sweep_open(stage, set, cur, query, j0, j1, n_dims); cur.i0 < cur.i1; cur = nxt) {
    nxt = tiles.after(cur);
    double acc[TY][4];
    pair_sweep_tile<KIND>(stage, acc, As, Bs, s_metric, set, cur, nxt, query, j0, j1, n_dims, metric, p, ti, tj, true);
    const uint32_t i0 = cur.i0, i1 = cur.i1;
    out.columns(i0 + ti, i1);
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) {
      if (!fl[yy]) continue;
      const uint32_t j = j0 + tj + yy;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double d = scale_distance<KIND>(acc[yy][x], p);
        const uint32_t i = i0 + ti + x;
        if (i < i1 && d == d && !out.left_out(yy, x, i) && distance_key(d) == tau[yy]) {
          atomicAdd(tie_total + j, 1u);
          const uint32_t c = class_of[i];
          if (c < n_classes) {
            atomicAdd(tie_count + (uint64_t)j * n_classes + c, 1u);
            atomicMin(tie_first + (uint64_t)j * n_classes + c, i);
          }
        }
      }
    }
  }
}

// a block of 64 (one wavefront) a row
__global__ __launch_bounds__(64) void knn_vote_kernel(const uint64_t *__restrict__ seg_key, const uint32_t *__restrict__ seg_idx, const uint32_t *__restrict__ seg_n,
                                                      uint32_t n_seg, uint32_t r2, uint32_t k, const uint64_t *__restrict__ m_key, const uint32_t *__restrict__ m_idx,
                                                      const uint32_t *__restrict__ m_n, const uint64_t *__restrict__ m_tau, const uint32_t *__restrict__ m_flag,
                                                      const uint32_t *__restrict__ class_of, uint32_t n_classes, const uint32_t *__restrict__ tie_total,
                                                      const uint32_t *__restrict__ tie_count, const uint32_t *__restrict__ tie_first, uint32_t *__restrict__ out_class,
                                                      uint32_t *__restrict__ out_votes, uint32_t *__restrict__ out_n, double *__restrict__ out_first_dist) {
  __shared__ uint64_t s_k[kKVoteList];
  __shared__ uint32_t s_i[kKVoteList], s_c[kKVoteList];
  __shared__ uint32_t s_nb, s_nt;
  for (uint32_t row = blockIdx.x; row < r2; row += gridDim.x) {
    const uint32_t nm = m_n[row];
    if (nm == 0) {  // no distance of the row is a number (or the set is empty)
      if (threadIdx.x == 0) {
        out_class[row] = KPOP_NO_CLASS;
        out_votes[row] = 0;
        out_n[row] = 0;
        if (out_first_dist) out_first_dist[row] = __longlong_as_double(0x7FF8000000000000ll);
      }
      continue;
    }
    const uint64_t tau = m_tau[row];
    const bool flagged = m_flag[row] != 0;
    __syncthreads();  // (the row before is done with the lists)
    if (threadIdx.x == 0) {
      s_nb = 0;
      s_nt = 0;
    }
    __syncthreads();
    // the entries below tau: a prefix of the merged list, fewer than k
    for (uint32_t q = threadIdx.x; q < nm; q += 64) {
      const uint64_t key = m_key[(uint64_t)row * k + q];
      if (key < tau) {
        const uint32_t idx = m_idx[(uint64_t)row * k + q];
        s_k[q] = key;
        s_i[q] = idx;
        s_c[q] = class_of[idx];
        atomicAdd(&s_nb, 1u);
      }
    }
    // the tie group, when the segments' lists hold it whole: behind slot kKMaxK, in any order (its order is the index)
    if (!flagged)
      for (uint32_t e = threadIdx.x; e < n_seg * k; e += 64) {
        const uint32_t s = e / k, q = e % k;
        const uint64_t o = (uint64_t)s * r2 + row;
        if (q < seg_n[o] && seg_key[o * k + q] == tau) {
          const uint32_t slot = kKMaxK + atomicAdd(&s_nt, 1u);  // (at most kKMaxTies of them: knn_merge_kernel flags the row otherwise)
          const uint32_t idx = seg_idx[o * k + q];
          s_k[slot] = tau;
          s_i[slot] = idx;
          s_c[slot] = class_of[idx];
        }
      }
    __syncthreads();
    const uint32_t nb = s_nb, nt = s_nt, L = nb + nt;
    auto phys = [&](uint32_t e) { return e < nb ? e : kKMaxK + (e - nb); };
    KnnBest best = {0u, 0u, KPOP_NO_CLASS, kKNone};
    // an entry that is the first of its class stands for the class
    for (uint32_t e = threadIdx.x; e < L; e += 64) {
      const uint32_t pe = phys(e), c = s_c[pe];
      if (c >= n_classes) continue;  // counts in out_n, votes for nobody
      uint32_t cnt = 0;
      bool first = true;
      for (uint32_t f = 0; f < L; ++f) {
        const uint32_t pf = phys(f);
        if (s_c[pf] != c) continue;
        ++cnt;
        if (key_less(s_k[pf], s_i[pf], s_k[pe], s_i[pe])) first = false;
      }
      if (!first) continue;
      if (flagged) cnt += tie_count[(uint64_t)row * n_classes + c];
      const KnnBest cand = {cnt, s_i[pe], c, s_k[pe]};
      if (knn_better(cand, best)) best = cand;
    }
    uint32_t n_list = L;
    if (flagged) {  // the classes that only the tie group holds
      n_list = nb + tie_total[row];
      for (uint32_t c = threadIdx.x; c < n_classes; c += 64) {
        const uint32_t tc = tie_count[(uint64_t)row * n_classes + c];
        if (tc == 0) continue;
        bool below = false;
        for (uint32_t f = 0; f < nb; ++f) below = below || s_c[f] == c;
        if (below) continue;
        const KnnBest cand = {tc, tie_first[(uint64_t)row * n_classes + c], c, tau};
        if (knn_better(cand, best)) best = cand;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      KnnBest other;
      other.cnt = (uint32_t)__shfl_xor((int)best.cnt, o, 64);
      other.idx = (uint32_t)__shfl_xor((int)best.idx, o, 64);
      other.cls = (uint32_t)__shfl_xor((int)best.cls, o, 64);
      other.key = (uint64_t)__shfl_xor((unsigned long long)best.key, o, 64);
      if (knn_better(other, best)) best = other;
    }
    if (threadIdx.x == 0) {
      out_class[row] = best.cnt ? best.cls : KPOP_NO_CLASS;
      out_votes[row] = best.cnt;
      out_n[row] = n_list;
      if (out_first_dist) out_first_dist[row] = best.cnt ? key_f64(best.key) : __longlong_as_double(0x7FF8000000000000ll);
    }
  }
}

// the three passes over the pairs.  LEAVE_OUT: the query rows are rows first_row .. first_row + r2 of the set a, without the rows that
// group_of leaves out of each list (knn_validate.hip); otherwise the rows of b, and group_of and first_row are not read.  ties false:
// the first two alone -- the merged lists and their last keys, for a caller that wants the k-th key and not the k-th key's members
template <int KIND, int TY, int W, bool LEAVE_OUT>
static int knn_passes(const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k,
                      const uint32_t *group_of, uint32_t first_row, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg_out,
                      bool ties, hipStream_t st) {
  using Who = std::conditional_t<LEAVE_OUT, KnnvLeftOut<TY>, KnnNobodyLeftOut>;
  constexpr uint32_t TJ = KnnShape<TY, W>::TJ;
  const uint32_t n_ct = div_up(r1, W), strips = div_up(r2, TJ);
  const uint32_t n_seg_max = std::max(1u, std::min(knn_max_segments(r2, TJ), n_ct));
  const uint32_t tiles_per_seg = div_up(n_ct, n_seg_max), n_seg = div_up(n_ct, tiles_per_seg);  // (no segment is empty)
  *n_seg_out = n_seg;
  const dim3 grid(strips, n_seg);
  knn_nearest_kernel<KIND, TY, W, Who><<<grid, dim3(256), 0, st>>>(a, r1, b, r2, n_dims, metric, p, k, n_ct, tiles_per_seg, group_of, first_row, w.seg_key, w.seg_idx,
                                                                   w.seg_n, w.seg_drop);
  KPOP_LAUNCH_CHECK();
  knn_merge_kernel<<<dim3(std::min(r2, 1u << 20)), dim3(64), 0, st>>>(w.seg_key, w.seg_idx, w.seg_n, w.seg_drop, n_seg, r2, k, w.m_key, w.m_idx, w.m_n, w.m_tau, w.m_flag);
  KPOP_LAUNCH_CHECK();
  if (!ties) return 0;
  knn_ties_kernel<KIND, TY, W, Who><<<grid, dim3(256), 0, st>>>(a, r1, b, r2, n_dims, metric, p, n_ct, tiles_per_seg, group_of, first_row, class_of, n_classes, w.m_tau,
                                                                w.m_flag, w.tie_total, w.tie_count, w.tie_first);
  KPOP_LAUNCH_CHECK();
  return 0;
}

template <int KIND, bool LEAVE_OUT>
static int knn_passes_of(const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k,
                         const uint32_t *group_of, uint32_t first_row, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg,
                         bool ties, hipStream_t st) {
  const uint32_t TJ = knn_strip_rows(k);
  if (TJ == 64) return knn_passes<KIND, 4, 64, LEAVE_OUT>(a, r1, b, r2, n_dims, metric, p, k, group_of, first_row, class_of, n_classes, w, n_seg, ties, st);
  if (TJ == 32) return knn_passes<KIND, 2, 64, LEAVE_OUT>(a, r1, b, r2, n_dims, metric, p, k, group_of, first_row, class_of, n_classes, w, n_seg, ties, st);
  return knn_passes<KIND, 1, 64, LEAVE_OUT>(a, r1, b, r2, n_dims, metric, p, k, group_of, first_row, class_of, n_classes, w, n_seg, ties, st);
}

template <bool LEAVE_OUT>
static int knn_passes_of_kind(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k,
                              const uint32_t *group_of, uint32_t first_row, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg,
                              bool ties, hipStream_t st) {
  return by_kind(kind, [&](auto K) {
    return knn_passes_of<decltype(K)::value, LEAVE_OUT>(a, r1, b, r2, n_dims, metric, p, k, group_of, first_row, class_of, n_classes, w, n_seg, ties, st);
  });
}

// (knn_lists.h) the three passes as knn_dev launches them, and with rows left out: for knn_validate.hip
int knn_run_passes(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k,
                   const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg, hipStream_t st) {
  return knn_passes_of_kind<false>(kind, a, r1, b, r2, n_dims, metric, p, k, nullptr, 0, class_of, n_classes, w, n_seg, true, st);
}
int knn_run_leave_out_passes(int kind, const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p,
                             uint32_t k, const uint32_t *group_of, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg,
                             hipStream_t st) {
  return knn_passes_of_kind<true>(kind, a, r1, a + (uint64_t)first_row * n_dims, n_rows, n_dims, metric, p, k, group_of, first_row, class_of, n_classes, w, n_seg, true, st);
}
// (knn_lists.h) the leave-self-out lists alone: knn_nearest_kernel with every row left out of its own list, then knn_merge_kernel.
// w.m_n, w.m_tau hold every row's length and last key; no class array is read and no tie table written (reachability.hip)
int knn_run_leave_self_out_lists(int kind, const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p,
                                 uint32_t k, const KnnWork &w, uint32_t *n_seg, hipStream_t st) {
  return knn_passes_of_kind<true>(kind, a, r1, a + (uint64_t)first_row * n_dims, n_rows, n_dims, metric, p, k, nullptr, first_row, nullptr, 0, w, n_seg, false, st);
}

// (knn_lists.h) the same two passes for query rows b, nobody left out: w.m_n, w.m_tau again, for a caller that wants every query row's
// k-th key over the whole set (lof.hip).  r1 > 0
int knn_run_lists(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k, const KnnWork &w,
                  uint32_t *n_seg, hipStream_t st) {
  return knn_passes_of_kind<false>(kind, a, r1, b, r2, n_dims, metric, p, k, nullptr, 0, nullptr, 0, w, n_seg, false, st);
}

// the body of both entry points: enqueues only
static int knn_dev(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2, uint32_t k, void *d_work,
                   uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist, hipStream_t st, const char *who) {
  KPOP_TRY(knn_check_sizes(k, n_classes, who));
  if (r2 == 0) return KPOP_OK;
  if (!d_out_class || !d_out_votes || !d_out_n || !d_work) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if (r1 && (!d_class_of || !d_m2)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  if (div_up(r2, 16) > 0x7FFFFFFFull) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u query rows", who, r2);
  const KnnWork w = knn_carve(d_work, r2, k, n_classes, D, rs->normalize != 0);
  const uint32_t rows_grid = std::min(r2, 1u << 20);
  uint32_t n_seg = 0;
  if (r1 == 0) {
    KPOP_HIP(hipMemsetAsync(w.m_n, 0, (uint64_t)r2 * 4, st));  // every list is empty
  } else {
    KPOP_HIP(hipMemsetAsync(reinterpret_cast<char *>(d_work) + w.tables_off, 0, w.tables_bytes, st));
    KPOP_HIP(hipMemsetAsync(w.tie_first, 0xFF, (uint64_t)r2 * n_classes * 4, st));
    const double *a, *b = d_m2;
    KPOP_TRY(refset_chain_rows(rs, st, &a));
    if (rs->normalize) {  // the query rows' quotients from the norms' pass: prepare_operands' (distance.hip)
      KPOP_TRY(refset_query_norms(rs, d_m2, r2, w.n2, w.b, st));
      b = w.b;
    }
    KPOP_TRY(knn_run_passes(rs->kind, a, r1, b, r2, D, rs->metric, rs->p, k, d_class_of, n_classes, w, &n_seg, st));
  }
  knn_vote_kernel<<<dim3(rows_grid), dim3(64), 0, st>>>(w.seg_key, w.seg_idx, w.seg_n, n_seg, r2, k, w.m_key, w.m_idx, w.m_n, w.m_tau, w.m_flag, d_class_of, n_classes,
                                                        w.tie_total, w.tie_count, w.tie_first, d_out_class, d_out_votes, d_out_n, d_out_first_dist);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
}

}  // namespace kpop

using namespace kpop;

extern "C" uint64_t kpop_dev_knn_vote_workspace_bytes(const kpop_refset *rs, uint32_t r2, uint32_t k, uint32_t n_classes) {
  if (!rs) return 0;
  return knn_carve(nullptr, r2, k, n_classes, rs->n_dims, rs->normalize != 0).bytes;
}

extern "C" int kpop_dev_knn_vote(kpop_refset *rs, const uint32_t *d_class_of, uint32_t n_classes, const double *d_m2, uint32_t r2, uint32_t k, void *d_work,
                                 uint32_t *d_out_class, uint32_t *d_out_votes, uint32_t *d_out_n, double *d_out_first_dist, void *stream) {
  const char *who = "kpop_dev_knn_vote";
  KPOP_TRY(refset_check_handle(rs, who));
  return knn_dev(rs, d_class_of, n_classes, d_m2, r2, k, d_work, d_out_class, d_out_votes, d_out_n, d_out_first_dist, as_stream(stream), who);
}

extern "C" int kpop_knn_vote(kpop_refset *rs, const uint32_t *class_of, uint32_t n_classes, const double *m2, uint32_t r2, uint32_t k, uint32_t *out_class,
                             uint32_t *out_votes, uint32_t *out_n, double *out_first_dist) {
  const char *who = "kpop_knn_vote";
  KPOP_TRY(refset_check_handle(rs, who));
  ArenaScope scratch;
  KPOP_TRY(knn_check_sizes(k, n_classes, who));
  const uint32_t r1 = rs->r1, D = rs->n_dims;
  if ((r1 && !class_of) || (r2 && (!out_class || !out_votes || !out_n)) || (r1 && r2 && !m2)) KPOP_FAIL(KPOP_ERR_INVALID, "%s: null argument", who);
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, false, who));
  if (r2 == 0) return KPOP_OK;
  // the query rows in chunks that keep the workspace bounded (a quarter of a GiB, or what 64 rows take)
  const uint64_t per_row = knn_carve(nullptr, 1024, k, n_classes, D, rs->normalize != 0).bytes / 1024 + (uint64_t)D * 8 + 32;
  const uint32_t chunk = (uint32_t)std::min<uint64_t>(r2, std::max<uint64_t>(64, (256ull << 20) / per_row));
  HostCall h;
  const hipStream_t st = h.st;
  const uint32_t *dc = h.in(class_of, r1);
  double *d2 = h.dev<double>((uint64_t)chunk * D);
  // (the last chunk may be cut into more segments than a whole one: the larger of the two workspaces)
  void *dw = h.work(std::max(kpop_dev_knn_vote_workspace_bytes(rs, chunk, k, n_classes),
                             kpop_dev_knn_vote_workspace_bytes(rs, r2 % chunk ? r2 % chunk : chunk, k, n_classes)));
  uint32_t *ocl = h.dev<uint32_t>(chunk), *ovo = h.dev<uint32_t>(chunk), *on = h.dev<uint32_t>(chunk);
  double *ofd = out_first_dist ? h.dev<double>(chunk) : nullptr;
  KPOP_TRY(h.upload());
  for (uint32_t j0 = 0; j0 < r2; j0 += chunk) {
    const uint32_t nr = std::min(chunk, r2 - j0);
    if (r1) KPOP_HIP(hipMemcpyAsync(d2, m2 + (uint64_t)j0 * D, (uint64_t)nr * D * 8, hipMemcpyHostToDevice, st));
    KPOP_TRY(knn_dev(rs, dc, n_classes, d2, nr, k, dw, ocl, ovo, on, ofd, st, who));
    KPOP_HIP(hipMemcpyAsync(out_class + j0, ocl, (uint64_t)nr * 4, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipMemcpyAsync(out_votes + j0, ovo, (uint64_t)nr * 4, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipMemcpyAsync(out_n + j0, on, (uint64_t)nr * 4, hipMemcpyDeviceToHost, st));
    if (ofd) KPOP_HIP(hipMemcpyAsync(out_first_dist + j0, ofd, (uint64_t)nr * 8, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipStreamSynchronize(st));
  }
  return KPOP_OK;
}

extern "C" int kpop_distance_knn_vote(const double *m1, uint32_t r1, const uint32_t *class_of, uint32_t n_classes, const double *m2, uint32_t r2, uint32_t n_dims,
                                      const double *metric, int kind, double p, int normalize, uint32_t k, uint32_t *out_class, uint32_t *out_votes,
                                      uint32_t *out_n, double *out_first_dist) {
  return with_temporary_refset(m1, r1, n_dims, metric, kind, p, normalize,
                               [&](kpop_refset *rs) { return kpop_knn_vote(rs, class_of, n_classes, m2, r2, k, out_class, out_votes, out_n, out_first_dist); });
}
