/* c_dbscan.c -- DBSCAN on a resident set from a plain C99 host: core rows, border rows and noise (kpop_dbscan: the distances of
 * Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, of the set against itself, never formed).  Ten rows on a line, all values
 * small binary fractions, so every distance is exact: two clusters of four core rows each, a border row that lies at exactly eps
 * from a core row of either -- it goes to the one with the smaller row index and joins nothing --, and a row far from everything,
 * which is noise.  First without keeping a set (kpop_distance_dbscan), then on a resident set (kpop_dbscan), which must say the
 * same.  Built and run by tests/test_gpu_dbscan_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_dbscan.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_dbscan
 * Prints the labels, the core rows, the degrees and the counts; exits non-zero on any mismatch with what it expects. */
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
#define ROWS 10
#define EPS 0.375
#define MIN_PTS 4

static void print_row(const char *what, const uint32_t *v, int n) {
  printf("%s:", what);
  for (int i = 0; i < n; ++i) {
    if (v[i] == KPOP_NOISE) printf(" noise");
    else printf(" %u", v[i]);
  }
  printf("\n");
}

static int differ(const uint32_t *a, const uint32_t *b, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i] != b[i]) return 1;
  return 0;
}

int main(void) {
  /* dimension 0 of the rows; the other dimensions are zero.  Row 7 lies at 0.375 from row 9 (a core row of the cluster under
     label 0) and from row 3 (of the cluster under label 3) */
  const double x[ROWS] = {0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375};
  const uint32_t want_labels[ROWS] = {0, 0, 0, 3, 3, 3, 3, 3, KPOP_NOISE, 0};
  const uint32_t want_core_of[ROWS] = {0, 1, 2, 3, 4, 5, 6, 3, KPOP_NOISE, 9};
  const uint32_t want_degree[ROWS] = {4, 4, 4, 5, 4, 4, 4, 3, 1, 5};
  const uint32_t want_counts[3] = {2, 8, 1};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  /* without keeping a set */
  uint32_t labels[ROWS], core_of[ROWS], degree[ROWS], counts[3];
  CHECK(kpop_distance_dbscan(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, EPS, MIN_PTS, labels, core_of, degree, counts));
  print_row("labels", labels, ROWS);
  print_row("core_of", core_of, ROWS);
  print_row("degree", degree, ROWS);
  printf("counts: %u clusters, %u core rows, %u noise rows\n", counts[0], counts[1], counts[2]);
  int bad = differ(labels, want_labels, ROWS) || differ(core_of, want_core_of, ROWS) || differ(degree, want_degree, ROWS) ||
            differ(counts, want_counts, 3);
  /* on a resident set; the core rows and the degrees need not be asked for */
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  uint32_t again[ROWS], again_counts[3];
  CHECK(kpop_dbscan(rs, EPS, MIN_PTS, again, NULL, NULL, again_counts));
  const int same = !differ(again, labels, ROWS) && !differ(again_counts, counts, 3);
  printf("resident set: %s\n", same ? "the same labels" : "DIFFERENT labels");
  /* the border row joins nothing: counted as a core row (min_pts = 3) it makes one cluster of the two */
  CHECK(kpop_dbscan(rs, EPS, 3, again, NULL, NULL, again_counts));
  print_row("labels at min_pts 3", again, ROWS);
  printf("counts at min_pts 3: %u clusters, %u core rows, %u noise rows\n", again_counts[0], again_counts[1], again_counts[2]);
  bad = bad || again_counts[0] != 1 || again_counts[1] != 9 || again_counts[2] != 1;
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return (bad || !same) ? 1 : 0;
}
