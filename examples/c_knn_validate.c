/* c_knn_validate.c -- how good is a labelled set as a k-NN classifier, and at which k?  From a plain C99 host: every row of a resident
 * set classified by its neighbours among the OTHER rows (kpop_knn_validate: the neighbour list of Matrix.summarize_distance_matrix_row,
 * lib/Matrix.ml:641-650, without the row itself or without its whole group, and the vote that the reference's README takes with awk), at
 * a ladder of k from one pass over the pairs; the README measures accuracy by a hold-out run instead (README.md:1077-1085).
 * Built and run by tests/test_gpu_knn_validate_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_knn_validate.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_knn_validate
 * Prints the accuracy for each k, leave-one-out and with groups of three rows left out together, the rows' votes at one k, and the
 * ladders that are refused. */
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

#define D 4
#define ROWS 10
#define CLASSES 3
#define N_KS 4

/* row i, dimension c: small exact binary fractions */
static double ref_value(int i, int c) { return (double)((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (c == i % D ? 0.5 : 0.0); }

static const char *status(int rc) { return rc == KPOP_ERR_INVALID ? "invalid" : rc == KPOP_ERR_UNSUPPORTED ? "unsupported" : rc == 0 ? "accepted" : "?"; }

static int validate(kpop_refset *rs, const uint32_t *class_of, const uint32_t *group_of, const uint32_t *ks, int rows_at) {
  uint32_t cls[N_KS * ROWS], votes[N_KS * ROWS], n[N_KS * ROWS];
  double first[N_KS * ROWS];
  uint64_t correct[N_KS];
  CHECK(kpop_knn_validate(rs, class_of, CLASSES, group_of, ks, N_KS, cls, votes, n, first, correct));
  for (int t = 0; t < N_KS; ++t) printf("k = %u: %llu of %d correct\n", ks[t], (unsigned long long)correct[t], ROWS);
  if (rows_at < 0) return 0;
  for (int j = 0; j < ROWS; ++j) {
    const int o = rows_at * ROWS + j;
    if (cls[o] == KPOP_NO_CLASS) printf("row %d (class %u): no class\n", j, class_of[j]);
    else printf("row %d (class %u): class %u with %u of %u, nearest at %.15g\n", j, class_of[j], cls[o], votes[o], n[o], first[o]);
  }
  return 0;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], metric[D];
  uint32_t class_of[ROWS], group_of[ROWS];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  const uint32_t ks[N_KS] = {1, 3, 5, 8};
  for (int i = 0; i < ROWS; ++i) {
    class_of[i] = (uint32_t)(i % CLASSES);
    group_of[i] = (uint32_t)(i / 3);
    for (int c = 0; c < D; ++c) rows[i * D + c] = ref_value(i == ROWS - 1 ? 2 : i, c); /* the last row IS row 2: a duplicate stays a neighbour */
  }
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 1, 0, &rs));
  printf("leave-one-out\n");
  if (validate(rs, class_of, NULL, ks, 1)) return 1; /* the rows at k = 3 */
  printf("groups of three\n");
  if (validate(rs, class_of, group_of, ks, -1)) return 1;
  /* the ladders that are refused */
  uint32_t cls[N_KS * ROWS], votes[N_KS * ROWS], n[N_KS * ROWS];
  uint64_t correct[N_KS];
  const uint32_t descending[2] = {3, 1}, zero[2] = {0, 2}, beyond[2] = {5, 129};
  printf("ks = 3, 1: %s\n", status(kpop_knn_validate(rs, class_of, CLASSES, NULL, descending, 2, cls, votes, n, NULL, correct)));
  printf("ks = 0, 2: %s\n", status(kpop_knn_validate(rs, class_of, CLASSES, NULL, zero, 2, cls, votes, n, NULL, correct)));
  printf("no k: %s\n", status(kpop_knn_validate(rs, class_of, CLASSES, NULL, ks, 0, cls, votes, n, NULL, correct)));
  printf("ks = 5, 129: %s\n", status(kpop_knn_validate(rs, class_of, CLASSES, NULL, beyond, 2, cls, votes, n, NULL, correct)));
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return 0;
}
