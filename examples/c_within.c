/* c_within.c -- a range query from a plain C99 host: every row of a resident set within a distance of each query row
 * (kpop_neighbours_within: the neighbour list of Matrix.summarize_distance_matrix_row, lib/Matrix.ml:632-690, cut at a distance
 * instead of a count).  The lists' total size is not known beforehand: the program starts with room for two entries, and when the
 * call answers KPOP_ERR_CAPACITY it reads the total out of the offsets -- they are always complete -- grows its buffers and asks
 * again.  Built and run by tests/test_gpu_within_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_within.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_within
 * Prints, per threshold and query row, the row's list in ascending (distance, index) order, deterministically. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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

/* reference row i, dimension c: small exact binary fractions, no two rows alike */
static double ref_value(int i, int c) { return (double)((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (c == i % D ? 0.5 : 0.0); }

static int query(kpop_refset *rs, const double *q, double max_distance) {
  uint64_t offsets[QUERIES + 1], capacity = 2;
  uint32_t *idx = malloc(capacity * sizeof *idx);
  double *dist = malloc(capacity * sizeof *dist);
  int rc, calls = 0;
  if (!idx || !dist) return 1;
  for (;;) {
    rc = kpop_neighbours_within(rs, q, QUERIES, max_distance, capacity, offsets, idx, dist);
    ++calls;
    if (rc != KPOP_ERR_CAPACITY) break;
    capacity = offsets[QUERIES]; /* exact, whatever the room was */
    free(idx);
    free(dist);
    idx = malloc(capacity * sizeof *idx);
    dist = malloc(capacity * sizeof *dist);
    if (!idx || !dist) return 1;
  }
  CHECK(rc);
  printf("within %.15g: %llu neighbours in %d call%s\n", max_distance, (unsigned long long)offsets[QUERIES], calls, calls == 1 ? "" : "s");
  for (int j = 0; j < QUERIES; ++j) {
    printf("query %d:", j);
    for (uint64_t k = offsets[j]; k < offsets[j + 1]; ++k) printf(" %u at %.15g", idx[k], dist[k]);
    printf("\n");
  }
  free(idx);
  free(dist);
  return 0;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], queries[QUERIES * D], metric[D];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = ref_value(i, c);
  for (int j = 0; j < QUERIES; ++j)
    for (int c = 0; c < D; ++c) queries[j * D + c] = j == 2 ? ref_value(4, c) : ref_value(j + 1, c) + (double)(c + 1) / 16.0; /* query 2 IS row 4 */
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 1, 0, &rs));
  if (query(rs, queries, 0.0)) return 1;   /* exact duplicates */
  if (query(rs, queries, 0.5)) return 1;   /* a neighbourhood */
  if (query(rs, queries, 1e300)) return 1; /* everything, sorted */
  /* count only: no lists, no capacity */
  uint64_t offsets[QUERIES + 1];
  CHECK(kpop_neighbours_within(rs, queries, QUERIES, 0.25, 0, offsets, NULL, NULL));
  printf("count within 0.25:");
  for (int j = 0; j < QUERIES; ++j) printf(" %llu", (unsigned long long)(offsets[j + 1] - offsets[j]));
  printf("\n");
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return 0;
}
