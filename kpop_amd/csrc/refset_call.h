// refset_call.h -- the host side of a call on a resident set, once: what within.hip, clusters.hip, forest.hip, knn.hip,
// knn_validate.hip, representatives.hip and dbscan.hip do around their kernels.
#pragma once
#include "common.h"
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

}  // namespace kpop
