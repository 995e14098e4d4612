/* c_refset.c -- a resident reference set from a plain C99 host: the register of Matrix.summarize_rowwise (lib/Matrix.ml:691-766)
 * prepared once with kpop_refset_create, queried twice, grown with kpop_refset_append and queried again -- what a binding does
 * when one register answers many batches.  Built and run by tests/test_gpu_refset_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_refset.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_refset
 * Prints, per query row, the mean distance and the two nearest reference rows, deterministically. */
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
#define ROWS 6   /* in the set at first */
#define MORE 3   /* appended later */
#define QUERIES 2
#define NB 2

/* reference row i, dimension c: small exact binary fractions, no two rows alike */
static double ref_value(int i, int c) { return (double)((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (c == i % D ? 0.5 : 0.0); }

static int query(kpop_refset *rs, const char *what, const double *q) {
  double stats[4 * QUERIES], dist[NB * QUERIES], z[NB * QUERIES];
  uint32_t n[QUERIES], idx[NB * QUERIES], r1 = 0;
  CHECK(kpop_refset_info(rs, &r1, NULL, NULL, NULL));
  CHECK(kpop_refset_distance_summary(rs, q, QUERIES, NB, NB, stats, n, idx, dist, z));
  for (int j = 0; j < QUERIES; ++j)
    printf("%s: %u rows, query %d: mean %.15g nearest %u at %.15g then %u at %.15g\n", what, r1, j, stats[4 * j], idx[NB * j], dist[NB * j],
           idx[NB * j + 1], dist[NB * j + 1]);
  return 0;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[(ROWS + MORE) * D], queries[2][QUERIES * D], metric[D];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  for (int i = 0; i < ROWS + MORE; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = ref_value(i, c);
  for (int b = 0; b < 2; ++b)
    for (int j = 0; j < QUERIES; ++j)
      for (int c = 0; c < D; ++c) queries[b][j * D + c] = ref_value(2 * b + j + 1, c) + (double)(c + 1 + b) / 16.0;
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 1, ROWS + MORE, &rs));
  if (query(rs, "first", queries[0])) return 1;
  if (query(rs, "second", queries[1])) return 1;
  CHECK(kpop_refset_append(rs, rows + ROWS * D, MORE));
  if (query(rs, "grown", queries[1])) return 1;
  /* the set is full: one more row is refused and changes nothing */
  const int rc = kpop_refset_append(rs, rows, 1);
  uint32_t r1 = 0, cap = 0;
  uint64_t bytes = 0;
  CHECK(kpop_refset_info(rs, &r1, NULL, &cap, &bytes));
  printf("full: append returned %d, %u of %u rows, %s\n", rc, r1, cap, bytes > 0 ? "device memory reported" : "NO device memory reported");
  /* every distance of the second batch, as kpop_distance_rowwise would give them */
  double all[QUERIES * (ROWS + MORE)];
  CHECK(kpop_refset_distance_rowwise(rs, queries[1], QUERIES, all));
  for (int j = 0; j < QUERIES; ++j) {
    printf("distances %d:", j);
    for (int i = 0; i < ROWS + MORE; ++i) printf(" %.15g", all[j * (ROWS + MORE) + i]);
    printf("\n");
  }
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return 0;
}
