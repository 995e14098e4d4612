/* c_silhouette.c -- the silhouette and the medoids of a labelled resident set from a plain C99 host (kpop_silhouette: the distances
 * of Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, of the set against itself, never formed).  The ten rows of c_dbscan.c, all
 * values small binary fractions, so every distance and every sum is exact; the labels are kpop_dbscan's at eps = .375, min_pts = 4
 * made dense: class 0 is rows 0, 1, 2, 9, class 1 rows 3 to 7, and row 8, the noise row, is left out (KPOP_NOISE == KPOP_NO_CLASS).
 * Row 7, the border row, lies as far from its own cluster as from the other: its silhouette is exactly 0.  First on a resident set
 * (kpop_dbscan, then kpop_silhouette), then without keeping a set (kpop_distance_silhouette), which must say the same, then the
 * means by class (kpop_silhouette_summary).  Built and run by tests/test_gpu_silhouette_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_silhouette.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_silhouette
 * Prints a line a row, a line a class and the means; exits non-zero on any mismatch with what it expects. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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
#define CLASSES 2
#define EPS 0.375
#define MIN_PTS 4

int main(void) {
  const double x[ROWS] = {0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375};
  const double want_own[ROWS] = {0.25, 1.0 / 6, 1.0 / 6, 0.28125, 0.25, 0.28125, 0.375, 0.5625, 0.0, 0.25};
  const double want_other[ROWS] = {1.2, 1.075, 0.95, 0.9375, 1.0625, 1.1875, 1.3125, 0.5625, 0.0, 0.825};
  const uint32_t want_medoid[CLASSES] = {1, 4};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* the labels of kpop_dbscan (the smallest core row of a cluster, or KPOP_NOISE) as classes 0, 1, ... in ascending label order */
  uint32_t labels[ROWS], counts[3], class_of[ROWS], label_of_class[ROWS], n_classes = 0;
  CHECK(kpop_dbscan(rs, EPS, MIN_PTS, labels, NULL, NULL, counts));
  for (uint32_t l = 0; l < ROWS; ++l) {
    int used = 0;
    for (int i = 0; i < ROWS; ++i) used = used || labels[i] == l;
    if (used) label_of_class[n_classes++] = l;
  }
  for (int i = 0; i < ROWS; ++i) {
    class_of[i] = KPOP_NO_CLASS;
    for (uint32_t c = 0; c < n_classes; ++c)
      if (labels[i] == label_of_class[c]) class_of[i] = c;
  }
  printf("classes: %u\n", n_classes);
  int bad = n_classes != CLASSES;
  double own[ROWS], other[ROWS], sil[ROWS], medoid_mean[CLASSES];
  uint32_t other_class[ROWS], class_rows[CLASSES], medoid[CLASSES];
  CHECK(kpop_silhouette(rs, class_of, CLASSES, own, other, other_class, sil, class_rows, medoid, medoid_mean));
  for (int i = 0; i < ROWS; ++i) {
    if (class_of[i] == KPOP_NO_CLASS) {
      printf("row %d: left out\n", i);
      bad = bad || own[i] == own[i] || other[i] == other[i] || sil[i] == sil[i] || other_class[i] != KPOP_NO_CLASS;
      continue;
    }
    printf("row %d: class %u own %.17g other %.17g (class %u) silhouette %.17g\n", i, class_of[i], own[i], other[i], other_class[i], sil[i]);
    bad = bad || own[i] != want_own[i] || other[i] != want_other[i] || other_class[i] != 1 - class_of[i];
  }
  bad = bad || sil[7] != 0.0 || sil[3] != 0.7 || sil[0] != 19.0 / 24;
  for (int c = 0; c < CLASSES; ++c) {
    printf("class %d: %u rows, medoid row %u at %.17g\n", c, class_rows[c], medoid[c], medoid_mean[c]);
    bad = bad || medoid[c] != want_medoid[c] || medoid_mean[c] != want_own[want_medoid[c]];
  }
  bad = bad || class_rows[0] != 4 || class_rows[1] != 5;
  /* without keeping a set; the means alone (every output may be NULL) */
  double own2[ROWS], other2[ROWS], sil2[ROWS];
  CHECK(kpop_distance_silhouette(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, class_of, CLASSES, own2, other2, NULL, sil2, NULL, NULL, NULL));
  const int same = !memcmp(own, own2, sizeof own) && !memcmp(other, other2, sizeof other) && !memcmp(sil, sil2, sizeof sil);
  printf("without a set: %s\n", same ? "the same bits" : "DIFFERENT bits");
  /* the means, summed in row order: host arithmetic */
  double class_mean[CLASSES], overall;
  CHECK(kpop_silhouette_summary(ROWS, class_of, CLASSES, sil, class_mean, &overall));
  printf("mean silhouette: class 0 %.17g, class 1 %.17g, all rows %.17g\n", class_mean[0], class_mean[1], overall);
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return (bad || !same) ? 1 : 0;
}
