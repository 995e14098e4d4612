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
//   knn_nearest_kernel   knn.hip's three passes over the pairs with KnnvLeftOut for "who is left out" (knn_run_leave_out_passes): a
//   knn_merge_kernel     column that is left out is refused before it can be inserted or counted as a dropped tie, and in the tie
//   knn_ties_kernel      tables.  The groups of a tile's four columns are loaded once a tile, those of a thread's rows once a launch.
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
        if (out_first_dist) out_first_dist[o] = best.cnt ? key_f64(best.key) : nan;
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
    const double *a, *b = d_m2;
    KPOP_TRY(refset_chain_rows(rs, st, &a));
    if (rs->normalize) {  // the query rows' quotients from the norms' pass: knn_dev's
      KPOP_TRY(refset_query_norms(rs, d_m2, r2, w.n2, w.b, st));
      b = w.b;
    }
    KPOP_TRY(knn_run_passes(rs->kind, a, r1, b, r2, D, rs->metric, rs->p, K, d_class_of, n_classes, w, &n_seg, st));
  }
  knn_vote_ks_launch(w, n_seg, r2, K, d_class_of, n_classes, ks, d_out_class, d_out_votes, d_out_n, d_out_first_dist, st);
  KPOP_LAUNCH_CHECK();
  return KPOP_OK;
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
  const double *a;  // both operands
  KPOP_TRY(refset_chain_rows(rs, st, &a));
  uint32_t n_seg = 0;
  KPOP_TRY(knn_run_leave_out_passes(rs->kind, a, r1, first_row, n_rows, D, rs->metric, rs->p, K, d_group_of, d_class_of, n_classes, w, &n_seg, st));
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
static int knn_slices_back(T *out, uint32_t rows, uint32_t j0, const T *from, uint32_t nr, uint32_t n_ks, hipStream_t st) {
  for (uint32_t t = 0; t < n_ks; ++t)
    KPOP_HIP(hipMemcpyAsync(out + (uint64_t)t * rows + j0, from + (uint64_t)t * nr, (uint64_t)nr * sizeof(T), hipMemcpyDeviceToHost, st));
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
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, false, who));
  if (r2 == 0) return KPOP_OK;
  const uint32_t chunk = knn_rows_a_call(r2, K, n_classes, D, rs->normalize != 0, n_ks, (uint64_t)D * 8);
  const uint64_t slices = (uint64_t)n_ks * chunk;
  HostCall h;
  const hipStream_t st = h.st;
  const uint32_t *dc = h.in(class_of, r1);
  double *d2 = h.dev<double>((uint64_t)chunk * D);
  // (the last chunk may be cut into more segments than a whole one: the larger of the two workspaces)
  void *dw = h.work(std::max(kpop_dev_knn_ks_vote_workspace_bytes(rs, chunk, K, n_classes),
                             kpop_dev_knn_ks_vote_workspace_bytes(rs, r2 % chunk ? r2 % chunk : chunk, K, n_classes)));
  uint32_t *ocl = h.dev<uint32_t>(slices), *ovo = h.dev<uint32_t>(slices), *on = h.dev<uint32_t>(slices);
  double *ofd = out_first_dist ? h.dev<double>(slices) : nullptr;
  KPOP_TRY(h.upload());
  for (uint32_t j0 = 0; j0 < r2; j0 += chunk) {
    const uint32_t nr = std::min(chunk, r2 - j0);
    if (r1) KPOP_HIP(hipMemcpyAsync(d2, m2 + (uint64_t)j0 * D, (uint64_t)nr * D * 8, hipMemcpyHostToDevice, st));
    KPOP_TRY(vote_ks_dev(rs, dc, n_classes, d2, nr, ks, n_ks, dw, ocl, ovo, on, ofd, st, who));
    KPOP_TRY(knn_slices_back(out_class, r2, j0, ocl, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_votes, r2, j0, ovo, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_n, r2, j0, on, nr, n_ks, st));
    if (ofd) KPOP_TRY(knn_slices_back(out_first_dist, r2, j0, ofd, nr, n_ks, st));
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
  KPOP_TRY(check_row_classes(class_of, r1, n_classes, false, who));
  for (uint32_t t = 0; t < n_ks; ++t) out_correct[t] = 0;
  if (r1 == 0) return KPOP_OK;
  // the set's rows in ranges that keep the workspace bounded; the query side of a range is the set's own (divided) rows: nothing a row
  const uint32_t chunk = knn_rows_a_call(r1, K, n_classes, D, false, n_ks, 0);
  const uint64_t slices = (uint64_t)n_ks * chunk;
  HostCall h;
  const hipStream_t st = h.st;
  const uint32_t *dc = h.in(class_of, r1), *dg = group_of ? h.in(group_of, r1) : nullptr;
  // (the last range may be cut into more segments than a whole one: the larger of the two workspaces)
  void *dw = h.work(std::max(kpop_dev_knn_validate_workspace_bytes(rs, chunk, K, n_classes),
                             kpop_dev_knn_validate_workspace_bytes(rs, r1 % chunk ? r1 % chunk : chunk, K, n_classes)));
  uint32_t *ocl = h.dev<uint32_t>(slices), *ovo = h.dev<uint32_t>(slices), *on = h.dev<uint32_t>(slices);
  double *ofd = out_first_dist ? h.dev<double>(slices) : nullptr;
  uint64_t *oco = h.dev<uint64_t>(kKMaxKs);
  KPOP_TRY(h.upload());
  for (uint32_t j0 = 0; j0 < r1; j0 += chunk) {
    const uint32_t nr = std::min(chunk, r1 - j0);
    uint64_t correct[kKMaxKs];
    KPOP_TRY(validate_dev(rs, dc, n_classes, dg, j0, nr, ks, n_ks, dw, ocl, ovo, on, ofd, oco, st, who));
    KPOP_TRY(knn_slices_back(out_class, r1, j0, ocl, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_votes, r1, j0, ovo, nr, n_ks, st));
    KPOP_TRY(knn_slices_back(out_n, r1, j0, on, nr, n_ks, st));
    if (ofd) KPOP_TRY(knn_slices_back(out_first_dist, r1, j0, ofd, nr, n_ks, st));
    KPOP_HIP(hipMemcpyAsync(correct, oco, (uint64_t)n_ks * 8, hipMemcpyDeviceToHost, st));
    KPOP_HIP(hipStreamSynchronize(st));
    for (uint32_t t = 0; t < n_ks; ++t) out_correct[t] += correct[t];
  }
  return KPOP_OK;
}

extern "C" int kpop_distance_knn_validate(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize,
                                          const uint32_t *class_of, uint32_t n_classes, const uint32_t *group_of, const uint32_t *ks, uint32_t n_ks,
                                          uint32_t *out_class, uint32_t *out_votes, uint32_t *out_n, double *out_first_dist, uint64_t *out_correct) {
  return with_temporary_refset(m, rows, n_dims, metric, kind, p, normalize, [&](kpop_refset *rs) {
    return kpop_knn_validate(rs, class_of, n_classes, group_of, ks, n_ks, out_class, out_votes, out_n, out_first_dist, out_correct);
  });
}
