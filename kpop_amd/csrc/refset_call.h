// refset_call.h -- the host side of a call on a resident set, once: what within.hip, clusters.hip, representatives.hip, dbscan.hip,
// forest.hip, reachability.hip, knn.hip, knn_validate.hip, silhouette.hip, farthest_first.hip and kmedoids.hip do around their kernels,
// and the host-buffer forms of refset.hip with them: the set's rows as the chain reads them, the workspace carved, the one-shot form,
// the argument checks that several entry points share, and -- host_call.h -- the device side of a host-buffer call (HostCall).
#pragma once
#include "common.h"
#include "host_call.h"
#include "refset.h"

namespace kpop {

// the set's rows as the chain reads them: divided by their norms when the set normalises (its own copy, built on first use)
static inline int refset_chain_rows(kpop_refset *rs, hipStream_t st, const double **a) {
  *a = rs->rows;
  if (rs->normalize) {
    KPOP_TRY(rs->prepared(st));
    KPOP_TRY(rs->divided(st, a));
  }
  return 0;
}

// a caller's workspace, carved: every piece starts at a multiple of 256 bytes.  base may be null: off is then the size alone
struct Carver {
  char *base;
  uint64_t off;
  explicit Carver(void *work) : base(reinterpret_cast<char *>(work)), off(0) {}
  template <class T>
  T *take(uint64_t bytes) {
    char *q = base + off;
    off += (bytes + 255) & ~255ull;
    return reinterpret_cast<T *>(q);
  }
};

// the one-shot form of a call: a set made of m for f(rs) alone
template <class F>
static int with_temporary_refset(const double *m, uint32_t rows, uint32_t n_dims, const double *metric, int kind, double p, int normalize, F &&f) {
  kpop_refset *rs = nullptr;
  KPOP_TRY(kpop_refset_create(m, rows, n_dims, metric, kind, p, normalize, 0, &rs));
  const int rc = f(rs);
  const int rc_free = kpop_refset_free(rs);
  return rc ? rc : rc_free;
}

// what an earlier call returned and this one takes back through known_rows: an entry is no larger than its row and names a row that
// stands for itself (a label: the smallest index of its component).  name: the array's; noun: "a label", "an entry"
static inline int check_known_prefix(const uint32_t *x, uint32_t known_rows, const char *who, const char *name, const char *noun) {
  for (uint32_t i = 0; i < known_rows; ++i)
    if (x[i] > i || x[x[i]] != x[i])
      KPOP_FAIL(KPOP_ERR_INVALID, "%s: %s[%u] = %u is not %s this call returns (%s[i] <= i, %s[%s[i]] == %s[i])", who, name, i, x[i], noun, name, name, name, name);
  return 0;
}

// a radius or a threshold of a host form: any number, none that is not one
static inline int check_distance_is_a_number(double d, const char *who) {
  if (d != d) KPOP_FAIL(KPOP_ERR_INVALID, "%s: the distance is not a number", who);
  return 0;
}

// a class for every row of a labelled set.  or_none: KPOP_NO_CLASS is a row's class too, and leaves the row out
static inline int check_row_classes(const uint32_t *class_of, uint32_t r1, uint32_t n_classes, bool or_none, const char *who) {
  for (uint32_t i = 0; i < r1; ++i) {
    if (class_of[i] < n_classes || (or_none && class_of[i] == KPOP_NO_CLASS)) continue;
    if (or_none) KPOP_FAIL(KPOP_ERR_INVALID, "%s: row %u has class %u of %u (KPOP_NO_CLASS leaves a row out)", who, i, class_of[i], n_classes);
    KPOP_FAIL(KPOP_ERR_INVALID, "%s: row %u has class %u of %u", who, i, class_of[i], n_classes);
  }
  return 0;
}

// n distinct rows of a set of r1.  name: the array's; noun: what a repeated entry is called ("seed", "row")
static inline int check_distinct_rows(const uint32_t *x, uint32_t n, uint32_t r1, const char *who, const char *name, const char *noun) {
  std::vector<bool> seen(r1, false);
  for (uint32_t t = 0; t < n; ++t) {
    if (x[t] >= r1) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %s[%u] = %u in a set of %u rows", who, name, t, x[t], r1);
    if (seen[x[t]]) KPOP_FAIL(KPOP_ERR_INVALID, "%s: %s[%u] = %u is a repeated %s", who, name, t, x[t], noun);
    seen[x[t]] = true;
  }
  return 0;
}

}  // namespace kpop
