/* c_lof.c -- the local outlier factor from a plain C99 host: does a row belong to the database at all?  (kpop_lof, kpop_lof_score:
 * the distances of Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, never formed.)  The worked case of INTEGRATION.md 6n: eleven
 * rows on a line, all values small binary fractions, so every distance is exact -- a grid whose interior scores exactly 1, an outlier,
 * a clump of k + 1 copies (lrd +inf, lof 1) and the row beside it (lof +inf); then four query rows scored against the set as it
 * stands.  k = 2.  Built and run by tests/test_gpu_lof_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_lof.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_lof
 * Exits non-zero on any mismatch with what it expects. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "kpop_hip.h"

#define CHECK(call)                                                                  \
  do {                                                                               \
    int rc_ = (call);                                                                \
    if (rc_ != 0) {                                                                  \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, kpop_last_error());      \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

#define D 3
#define ROWS 11
#define QUERIES 4
#define K 2

static void print_counts(const char *what, const uint32_t *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) printf(" %u", v[i]);
  printf("\n");
}

static void print_doubles(const char *what, const double *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}

static int differ(const double *got, const double *want, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (got[i] != want[i]) return 1;
  return 0;
}

static void fill(double *m, const double *x, int n) { /* dimension 0 of the rows; the other dimensions are zero */
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < D; ++c) m[i * D + c] = c == 0 ? x[i] : 0.0;
}

int main(void) {
  const double x[ROWS] = {0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, -3.0, 2.0, 2.0, 2.0};
  const double q[QUERIES] = {0.625, -1.0, 2.0, 100.0};
  const double want_kdist[ROWS] = {0.5, 0.25, 0.25, 0.25, 0.25, 0.25, 0.5, 3.25, 0.0, 0.0, 0.0};
  const uint32_t want_n[ROWS] = {2, 2, 2, 2, 2, 2, 5, 2, 2, 2, 2};
  const double want_lrd[ROWS] = {2.6666666666666665, 2.6666666666666665, 4.0, 4.0, 4.0, 2.6666666666666665, 2.2222222222222223, 0.32, INFINITY, INFINITY, INFINITY};
  const double want_lof[ROWS] = {1.25, 1.25, 0.83333333333333326, 1.0, 0.83333333333333326, 1.1666666666666667, INFINITY, 8.3333333333333321, 1.0, 1.0, 1.0};
  const double want_q_kdist[QUERIES] = {0.125, 1.25, 0.0, 98.0};
  const uint32_t want_q_n[QUERIES] = {2, 2, 3, 3};
  const double want_q_lrd[QUERIES] = {4.0, 0.88888888888888884, INFINITY, 0.01020408163265306};
  const double want_q_lof[QUERIES] = {1.0, 3.0, 1.0, INFINITY};
  double rows[ROWS * D], queries[QUERIES * D], metric[D];
  fill(rows, x, ROWS);
  fill(queries, q, QUERIES);
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* the set, every row against the others */
  double kdist[ROWS], lrd[ROWS], lof[ROWS], core[ROWS];
  uint32_t n_neigh[ROWS];
  CHECK(kpop_lof(rs, K, kdist, n_neigh, lrd, lof));
  print_doubles("kdist", kdist, ROWS);
  print_counts("n_neigh", n_neigh, ROWS);
  print_doubles("lrd", lrd, ROWS);
  print_doubles("lof", lof, ROWS);
  int bad = differ(kdist, want_kdist, ROWS) || differ(lrd, want_lrd, ROWS) || differ(lof, want_lof, ROWS);
  for (int i = 0; i < ROWS && !bad; ++i) bad = n_neigh[i] != want_n[i];
  /* the k-distances are the core distances at min_pts = k + 1 */
  CHECK(kpop_core_distances(rs, K + 1, core));
  printf("kdist is core_distances(k + 1): %s\n", differ(kdist, core, ROWS) ? "NO" : "yes");
  bad = bad || differ(kdist, core, ROWS);
  /* four query rows against the set as it stands */
  double q_kdist[QUERIES], q_lrd[QUERIES], q_lof[QUERIES];
  uint32_t q_n[QUERIES];
  CHECK(kpop_lof_score(rs, K, kdist, lrd, queries, QUERIES, q_kdist, q_n, q_lrd, q_lof));
  print_doubles("query kdist", q_kdist, QUERIES);
  print_counts("query n_neigh", q_n, QUERIES);
  print_doubles("query lrd", q_lrd, QUERIES);
  print_doubles("query lof", q_lof, QUERIES);
  bad = bad || differ(q_kdist, want_q_kdist, QUERIES) || differ(q_lrd, want_q_lrd, QUERIES) || differ(q_lof, want_q_lof, QUERIES);
  for (int i = 0; i < QUERIES && !bad; ++i) bad = q_n[i] != want_q_n[i];
  /* without keeping a set, the factors alone */
  double again[ROWS];
  CHECK(kpop_distance_lof(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, K, NULL, NULL, NULL, again));
  printf("without a set: %s\n", differ(again, lof, ROWS) ? "a DIFFERENT result" : "the same result");
  bad = bad || differ(again, lof, ROWS);
  /* k = 0 and k = 129 are refused */
  const int rc0 = kpop_lof(rs, 0, NULL, NULL, NULL, lof), rc129 = kpop_lof(rs, 129, NULL, NULL, NULL, lof);
  printf("k = 0: %d, k = 129: %d\n", rc0, rc129);
  bad = bad || rc0 != KPOP_ERR_INVALID || rc129 != KPOP_ERR_UNSUPPORTED;
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return bad ? 1 : 0;
}
