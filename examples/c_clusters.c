/* c_clusters.c -- clusters at a distance from a plain C99 host: the connected components of the graph that joins two rows of a
 * resident set when they lie within a distance of each other (kpop_clusters_within: the distances of Matrix.get_distance_rowwise,
 * lib/Matrix.ml:191-266, of the set against itself, never formed).  The set is made with room to grow, clustered, given more rows
 * -- one of them between two clusters -- and clustered again from the labels it had: only the pairs with a new row in them are
 * examined, and the answer is the from-scratch one.  Built and run by tests/test_gpu_clusters_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_clusters.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_clusters
 * Prints, per step, the number of clusters and the largest clusters' sizes with their labels, deterministically. */
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
#define ROWS 24
#define MORE 8
#define TOP 3
#define MAX_DISTANCE 0.375

/* row i, dimension c: group i % 5 sits at (2 g, g, 0, -g); inside a group the rows step by 1/8 along dimension i % D -- small exact
   binary fractions */
static double row_value(int i, int c) {
  const int g = i % 5;
  const double centre = c == 0 ? 2.0 * g : c == 1 ? g : c == 2 ? 0.0 : -g;
  return centre + (c == i % D ? (double)(i / 5) / 8.0 : 0.0);
}

/* the rows appended: seven steps of an eighth from group 0's centre to group 1's (a bridge), and one row far from everything */
static double more_value(int k, int c) {
  if (k == MORE - 1) return c == 3 ? 40.0 : 0.0;
  return (c == 0 ? 2.0 : c == 1 ? 1.0 : c == 2 ? 0.0 : -1.0) * (double)(k + 1) / 8.0;
}

static int report(const char *what, const uint32_t *labels, uint32_t rows, uint32_t n_clusters) {
  uint32_t *size = calloc(rows, sizeof *size);
  if (!size) return 1;
  for (uint32_t i = 0; i < rows; ++i) ++size[labels[i]];
  printf("%s: %u rows in %u clusters; largest:", what, rows, n_clusters);
  for (int t = 0; t < TOP; ++t) { /* by size, then by label */
    uint32_t best = rows;
    for (uint32_t i = 0; i < rows; ++i)
      if (size[i] && (best == rows || size[i] > size[best])) best = i;
    if (best == rows) break;
    printf(" %u rows under label %u;", size[best], best);
    size[best] = 0;
  }
  printf("\n");
  free(size);
  return 0;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], more[MORE * D], metric[D];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = row_value(i, c);
  for (int k = 0; k < MORE; ++k)
    for (int c = 0; c < D; ++c) more[k * D + c] = more_value(k, c);
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, ROWS + MORE, &rs));
  uint32_t labels[ROWS + MORE], again[ROWS + MORE], n_clusters = 0, n_again = 0;
  CHECK(kpop_clusters_within(rs, MAX_DISTANCE, 0, labels, &n_clusters));
  if (report("created", labels, ROWS, n_clusters)) return 1;
  /* the set grows: labels[0 .. ROWS) are what the call above returned, at the same distance */
  CHECK(kpop_refset_append(rs, more, MORE));
  CHECK(kpop_clusters_within(rs, MAX_DISTANCE, ROWS, labels, &n_clusters));
  if (report("grown", labels, ROWS + MORE, n_clusters)) return 1;
  /* from scratch: the same labels */
  CHECK(kpop_clusters_within(rs, MAX_DISTANCE, 0, again, &n_again));
  int same = n_again == n_clusters;
  for (int i = 0; i < ROWS + MORE; ++i) same = same && again[i] == labels[i];
  printf("from scratch: %s\n", same ? "the same labels" : "DIFFERENT labels");
  printf("labels:");
  for (int i = 0; i < ROWS + MORE; ++i) printf(" %u", labels[i]);
  printf("\n");
  /* without keeping a set */
  CHECK(kpop_distance_clusters(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 1e300, again, &n_again));
  if (report("everything joined", again, ROWS, n_again)) return 1;
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return same ? 0 : 1;
}
