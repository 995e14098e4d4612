/* c_class_linkage.c -- the distances between every two classes of a labelled resident set, and the classes' tree, from a plain C99
 * host (kpop_class_linkage: the distances of Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, of the set against itself, never
 * formed; kpop_class_tree: host arithmetic).  The ten rows of INTEGRATION.md section 6o on a line, all values small binary fractions,
 * so every distance and every sum is exact: three classes of three rows, row 8 left out, class 3 empty.  First on a resident set, then
 * without keeping one (kpop_distance_class_linkage), which must say the same, then the three trees.  Built and run by
 * tests/test_gpu_class_linkage_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_class_linkage.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_class_linkage
 * Prints a line a class pair and a line a merge; exits non-zero on any mismatch with what it expects. */
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
#define CLASSES 4

int main(void) {
  const double x[ROWS] = {0.0, 4.0, 0.5, 10.0, 1.0, 4.5, 11.0, 6.0, 2.0, 13.0};
  const uint32_t class_of[ROWS] = {0, 1, 0, 2, 0, 1, 2, 1, KPOP_NO_CLASS, 2};
  /* the upper triangle of the classes that have rows: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) */
  const double want_mean[6] = {2.0 / 3, 39.0 / 9, 97.5 / 9, 4.0 / 3, 6.5, 2.0};
  const double want_min[6] = {0.5, 3.0, 9.0, 0.5, 4.0, 1.0}, want_max[6] = {1.0, 6.0, 13.0, 2.0, 9.0, 3.0};
  const uint32_t want_i[6] = {0, 1, 3, 1, 3, 3}, want_j[6] = {2, 4, 4, 5, 7, 6};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  uint32_t class_rows[CLASSES], min_i[CLASSES * CLASSES], min_j[CLASSES * CLASSES];
  double mean[CLASSES * CLASSES], lo[CLASSES * CLASSES], hi[CLASSES * CLASSES];
  CHECK(kpop_class_linkage(rs, class_of, CLASSES, class_rows, mean, lo, hi, min_i, min_j));
  printf("class_rows:");
  for (int c = 0; c < CLASSES; ++c) printf(" %u", class_rows[c]);
  printf("\n");
  int bad = class_rows[0] != 3 || class_rows[1] != 3 || class_rows[2] != 3 || class_rows[3] != 0, k = 0;
  for (int a = 0; a < CLASSES; ++a)
    for (int b = a; b < CLASSES; ++b) {
      const int e = a * CLASSES + b, t = b * CLASSES + a;
      /* symmetric bit for bit (a NaN has the declared bits in both halves) */
      bad = bad || memcmp(&mean[e], &mean[t], 8) || memcmp(&lo[e], &lo[t], 8) || memcmp(&hi[e], &hi[t], 8) || min_i[e] != min_i[t] || min_j[e] != min_j[t];
      if (b == 3) {
        bad = bad || mean[e] == mean[e] || lo[e] == lo[e] || hi[e] == hi[e] || min_i[e] != KPOP_NO_CLASS || min_j[e] != KPOP_NO_CLASS;
        continue;
      }
      printf("classes %d %d: mean %.17g min %.17g (rows %u %u) max %.17g\n", a, b, mean[e], lo[e], min_i[e], min_j[e], hi[e]);
      bad = bad || mean[e] != want_mean[k] || lo[e] != want_min[k] || hi[e] != want_max[k] || min_i[e] != want_i[k] || min_j[e] != want_j[k];
      ++k;
    }
  printf("class 3: empty\n");
  /* without keeping a set; the means alone (every output may be NULL) */
  double mean2[CLASSES * CLASSES];
  CHECK(kpop_distance_class_linkage(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, class_of, CLASSES, NULL, mean2, NULL, NULL, NULL, NULL));
  const int same = !memcmp(mean, mean2, sizeof mean);
  printf("without a set: %s\n", same ? "the same bits" : "DIFFERENT bits");
  /* the trees: host arithmetic.  Merge t makes node CLASSES + t */
  const char *names[3] = {"single", "complete", "average"};
  const double *tables[3] = {lo, hi, mean};
  const int linkages[3] = {KPOP_LINK_SINGLE, KPOP_LINK_COMPLETE, KPOP_LINK_AVERAGE};
  const double want_h[3][2] = {{3.0, 4.0}, {6.0, 13.0}, {39.0 / 9, (3.0 * (97.5 / 9) + 3.0 * 6.5) / 6.0}};
  for (int l = 0; l < 3; ++l) {
    uint32_t n_merges = 0, left[CLASSES - 1], right[CLASSES - 1], size[CLASSES - 1];
    double height[CLASSES - 1];
    CHECK(kpop_class_tree(CLASSES, class_rows, tables[l], linkages[l], &n_merges, left, right, height, size));
    bad = bad || n_merges != 2;
    for (uint32_t t = 0; t < n_merges; ++t) {
      printf("%s merge %u: nodes %u %u -> node %u at %.17g, %u rows\n", names[l], t, left[t], right[t], CLASSES + t, height[t], size[t]);
      bad = bad || height[t] != want_h[l][t];
    }
    bad = bad || left[0] != 0 || right[0] != 1 || size[0] != 6 || left[1] != 2 || right[1] != 4 || size[1] != 9;
  }
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return (bad || !same) ? 1 : 0;
}
