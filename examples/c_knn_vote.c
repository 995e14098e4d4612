/* c_knn_vote.c -- the k-NN classifier from a plain C99 host: a class for each query row from its k nearest rows of a labelled resident
 * set (kpop_knn_vote: the neighbour list of Matrix.summarize_distance_matrix_row, lib/Matrix.ml:641-650, and the vote that the
 * reference's README takes over it with awk).  The labels travel with the call; three numbers and a distance a query row come back.
 * Built and run by tests/test_gpu_knn_vote_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_knn_vote.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_knn_vote
 * Prints, per k and query row, the class, its votes, the length of the list and the distance of the class's nearest member. */
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
#define ROWS 9
#define QUERIES 3
#define CLASSES 3

/* reference row i, dimension c: small exact binary fractions, no two rows alike */
static double ref_value(int i, int c) { return (double)((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (c == i % D ? 0.5 : 0.0); }

static int vote(kpop_refset *rs, const uint32_t *class_of, const double *q, uint32_t k) {
  uint32_t cls[QUERIES], votes[QUERIES], n[QUERIES];
  double first[QUERIES];
  CHECK(kpop_knn_vote(rs, class_of, CLASSES, q, QUERIES, k, cls, votes, n, first));
  printf("k = %u\n", k);
  for (int j = 0; j < QUERIES; ++j) {
    if (cls[j] == KPOP_NO_CLASS) printf("query %d: no class\n", j);
    else printf("query %d: class %u with %u of %u, nearest at %.15g\n", j, cls[j], votes[j], n[j], first[j]);
  }
  return 0;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], queries[QUERIES * D], metric[D];
  uint32_t class_of[ROWS];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  for (int i = 0; i < ROWS; ++i) {
    class_of[i] = (uint32_t)(i % CLASSES);
    for (int c = 0; c < D; ++c) rows[i * D + c] = ref_value(i, c);
  }
  for (int j = 0; j < QUERIES; ++j)
    for (int c = 0; c < D; ++c) queries[j * D + c] = j == 2 ? ref_value(4, c) : ref_value(j + 1, c) + (double)(c + 1) / 16.0; /* query 2 IS row 4 */
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 1, 0, &rs));
  if (vote(rs, class_of, queries, 1)) return 1;   /* the nearest class */
  if (vote(rs, class_of, queries, 5)) return 1;   /* the README's classifier */
  if (vote(rs, class_of, queries, 128)) return 1; /* more than the set holds: everybody votes */
  /* without the distances; a k beyond the limit is refused */
  uint32_t cls[QUERIES], votes[QUERIES], n[QUERIES];
  CHECK(kpop_knn_vote(rs, class_of, CLASSES, queries, QUERIES, 3, cls, votes, n, NULL));
  printf("k = 3, classes alone:");
  for (int j = 0; j < QUERIES; ++j) printf(" %u", cls[j]);
  printf("\n");
  printf("k = 129: %s\n", kpop_knn_vote(rs, class_of, CLASSES, queries, QUERIES, 129, cls, votes, n, NULL) == KPOP_ERR_UNSUPPORTED ? "unsupported" : "?");
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return 0;
}
