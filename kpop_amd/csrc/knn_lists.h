// knn_lists.h -- what the k-NN vote (knn.hip) and the k-NN validation (knn_validate.hip) share: a row's sorted list in LDS and the
// insertion into it, the workgroup shapes, the workspace's layout and the limits (the keys and their order: space_ops.h).  The kernels
// that walk the pairs are knn.hip's; it launches them for knn_validate.hip too (knn_run_passes, knn_run_leave_out_passes).
#pragma once
#include <algorithm>

#include "common.h"
#include "refset_call.h"
#include "space_ops.h"

namespace kpop {

constexpr int kKMaxK = 128;
// a workgroup's shape: W columns (rows of the set) x TJ query rows, a thread 4 columns x TY rows
template <int TY, int W>
struct KnnShape {
  static constexpr uint32_t NCG = W / 4, NRG = 256 / NCG, TJ = TY * NRG;
  static constexpr uint32_t SLOTS = 2048;  // list slots of the workgroup: TJ k <= SLOTS, the whole within 64 KiB of LDS
};
constexpr int kKMaxSeg = 128, kKBlocks = 512;                // segments a strip at most; workgroups a launch aims at (two a CU)
constexpr int kKMaxTies = 1024;                              // listed ties of a row that knn_vote_kernel takes from the lists; more: the tables
constexpr int kKVoteList = kKMaxK + kKMaxTies;               // knn_vote_kernel: < k entries below tau, then the listed ties
constexpr uint64_t kKNone = ~0ull;                           // (no key: distance_key maps only a NaN's bits there, and a NaN is never a key)
constexpr uint32_t kKMaxClasses = 65535;
constexpr uint32_t kKMaxKs = 32;                             // the cut points of one list (knn_validate.hip)

// One candidate into a row's sorted list, by the whole wavefront that owns the row (every argument is the same in all 64 lanes).
// lk, li: the row's k slots; *np its length; *bp, *bip its bound (kKNone until the list is full, then its k-th key and index); *dp its
// dropped ties.
// A lane holds slots lane and lane + 64 (k <= 128).  The slots are read into registers before any is written, and the LDS serves a
// wavefront's accesses in the order it issued them: volatile keeps the compiler from moving them.
__device__ __forceinline__ void knn_insert(volatile uint64_t *lk, volatile uint32_t *li, volatile uint32_t *np, volatile uint64_t *bp, volatile uint32_t *bip,
                                           volatile uint32_t *dp, uint32_t k, uint64_t ck, uint32_t ci, uint32_t lane) {
  const uint32_t n = *np;
  uint64_t bk = 0;
  if (n == k) {
    bk = lk[k - 1];
    const uint32_t bi = li[k - 1];
    if (ck > bk) return;
    if (ck == bk && ci > bi) {  // refused, a tie of the k-th key
      if (lane == 0) *dp = *dp + 1;
      return;
    }
  }
  const uint32_t q0 = lane, q1 = lane + 64;
  const uint64_t e0k = q0 < n ? lk[q0] : 0, e1k = q1 < n ? lk[q1] : 0;
  const uint32_t e0i = q0 < n ? li[q0] : 0, e1i = q1 < n ? li[q1] : 0;
  const uint32_t pos = (uint32_t)__popcll(__ballot(q0 < n && key_less(e0k, e0i, ck, ci))) + (uint32_t)__popcll(__ballot(q1 < n && key_less(e1k, e1i, ck, ci)));
  // (pos <= n, and pos < k: a full list was entered only below its last entry)
  if (q0 < n && q0 >= pos && q0 + 1 < k) {
    lk[q0 + 1] = e0k;
    li[q0 + 1] = e0i;
  }
  if (q1 < n && q1 >= pos && q1 + 1 < k) {
    lk[q1 + 1] = e1k;
    li[q1 + 1] = e1i;
  }
  if (lane == 0) {
    lk[pos] = ck;
    li[pos] = ci;
  }
  if (n < k) {
    if (lane == 0) *np = n + 1;
    if (n + 1 == k) {
      const uint64_t nk = lk[k - 1];
      const uint32_t ni = li[k - 1];
      if (lane == 0) {
        *bp = nk;
        *bip = ni;
      }
    }
  } else {  // the old last entry, of key bk, was evicted
    const uint64_t nk = lk[k - 1];
    const uint32_t ni = li[k - 1];
    if (lane == 0) {
      *dp = (nk == bk) ? *dp + 1 : 0u;
      *bp = nk;
      *bip = ni;
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// the column tiles of a segment
__device__ __forceinline__ void knn_segment(uint32_t n_ct, uint32_t tiles_per_seg, uint32_t *t_begin, uint32_t *t_end) {
  *t_begin = min(n_ct, blockIdx.y * tiles_per_seg);
  *t_end = min(n_ct, *t_begin + tiles_per_seg);
}

struct KnnBest {
  uint32_t cnt, idx, cls;
  uint64_t key;
};
__device__ __forceinline__ bool knn_better(const KnnBest &x, const KnnBest &y) {  // more members; among equally many, the nearer first member
  return x.cnt > y.cnt || (x.cnt == y.cnt && x.cnt > 0 && key_less(x.key, x.idx, y.key, y.idx));
}

// the workspace, carved: the query rows' norms and divided copy, the segments' lists, the merged lists, the tie tables.  It depends on
// r2, k, n_classes, the set's n_dims and the constants above; not on r1
struct KnnWork {
  double *n2, *b;
  uint64_t *seg_key, *m_key, *m_tau;
  uint32_t *seg_idx, *seg_n, *seg_drop, *m_idx, *m_n, *m_flag, *tie_total, *tie_count, *tie_first;
  uint64_t tables_off, tables_bytes, bytes;
};

// the rows of a strip by k, so that their lists fit the workgroup's slots: 64 columns x 64, 32 or 16 rows, a thread 4 x 4, 2 or 1.
// (The choice moves no bit: a pair's chain is one thread's either way.  rowwise_block's 32 columns x 256 rows, a thread 4 x 8, was
// tried for k <= 6 against long sets and measured slower here -- profiles/knn_vote.md -- and is not built.)
static uint32_t knn_strip_rows(uint32_t k) { return k <= 2048 / 64 ? 64u : k <= 2048 / 32 ? 32u : 16u; }
// the segments the columns are cut into at most: as many as make kKBlocks workgroups with the strips of r2 query rows (forest.hip's
// reason: a few query rows still fill the chip).  By r2 and k alone, so that the workspace does not depend on the set
static uint32_t knn_max_segments(uint32_t r2, uint32_t strip_rows) {
  return std::max(1u, std::min<uint32_t>(kKMaxSeg, div_up(kKBlocks, std::max(1u, div_up(r2, strip_rows)))));
}

static KnnWork knn_carve(void *work, uint32_t r2, uint32_t k, uint32_t n_classes, uint32_t n_dims, bool normalize) {
  Carver c(work);
  const uint64_t n = r2, lists = n * k, segs = knn_max_segments(r2, knn_strip_rows(k));
  KnnWork w;
  w.n2 = c.take<double>(normalize ? n * 8 : 0);
  w.b = c.take<double>(normalize ? n * n_dims * 8 : 0);
  w.seg_key = c.take<uint64_t>(lists * 8 * segs);
  w.seg_idx = c.take<uint32_t>(lists * 4 * segs);
  w.seg_n = c.take<uint32_t>(n * 4 * segs);
  w.seg_drop = c.take<uint32_t>(n * 4 * segs);
  w.m_key = c.take<uint64_t>(lists * 8);
  w.m_idx = c.take<uint32_t>(lists * 4);
  w.m_tau = c.take<uint64_t>(n * 8);
  w.m_n = c.take<uint32_t>(n * 4);
  w.m_flag = c.take<uint32_t>(n * 4);
  w.tables_off = c.off;
  w.tie_total = c.take<uint32_t>(n * 4);
  w.tie_count = c.take<uint32_t>(n * n_classes * 4);
  w.tables_bytes = c.off - w.tables_off;  // (zeroes)
  w.tie_first = c.take<uint32_t>(n * n_classes * 4);  // (ones)
  w.bytes = c.off + 256;
  return w;
}

static inline int knn_check_sizes(uint32_t k, uint32_t n_classes, const char *who) {
  if (k == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: k = 0", who);
  if (k > (uint32_t)kKMaxK) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: k = %u (at most %d)", who, k, kKMaxK);
  if (n_classes == 0) KPOP_FAIL(KPOP_ERR_INVALID, "%s: no classes", who);
  if (n_classes > kKMaxClasses) KPOP_FAIL(KPOP_ERR_UNSUPPORTED, "%s: %u classes (at most %u)", who, n_classes, kKMaxClasses);
  return 0;
}

// knn.hip: the three passes over the pairs -- knn_nearest_kernel, knn_merge_kernel, knn_ties_kernel -- for the set's kind.  The second
// form takes rows first_row .. first_row + n_rows of the set a itself as the query rows and leaves out of each row's list the row
// (group_of == NULL) or its whole group (knn_validate.hip).  Both enqueue only
int knn_run_passes(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k,
                   const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg, hipStream_t st);
int knn_run_leave_out_passes(int kind, const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p,
                             uint32_t k, const uint32_t *group_of, const uint32_t *class_of, uint32_t n_classes, const KnnWork &w, uint32_t *n_seg,
                             hipStream_t st);
// the first two of them alone, every row left out of its own list: w.m_n, w.m_tau are each row's length and last (k-th) key.  No
// class array, no tie table: the tie pass settles WHICH rows share the k-th key, never its value (reachability.hip's core distances)
int knn_run_leave_self_out_lists(int kind, const double *a, uint32_t r1, uint32_t first_row, uint32_t n_rows, uint32_t n_dims, const double *metric, double p,
                                 uint32_t k, const KnnWork &w, uint32_t *n_seg, hipStream_t st);
// the same two for query rows b with nobody left out: every query row's k-th key over the whole set (lof.hip's query form).  r1 > 0
int knn_run_lists(int kind, const double *a, uint32_t r1, const double *b, uint32_t r2, uint32_t n_dims, const double *metric, double p, uint32_t k, const KnnWork &w,
                  uint32_t *n_seg, hipStream_t st);

// reachability.hip: every row's core distance at min_pts (in 1 .. kKMaxK + 1, checked by the caller; r1 > 0) into d_core[r1], the set
// walked in slabs whose lists are d_work's core_workspace_bytes.  Enqueues only.  lof.hip's k-distances are these at min_pts = k + 1
uint64_t core_workspace_bytes(uint32_t r1, uint32_t min_pts, uint32_t n_dims);
int core_dev(kpop_refset *rs, uint32_t min_pts, void *d_work, double *d_core, hipStream_t st);

}  // namespace kpop
