/* c_density_peaks.c -- density peaks from a plain C99 host: clusters when neither a radius nor a count is known, and the nearest
 * better row for any score.  (kpop_density_peaks, kpop_density_peaks_cut: the distances of Matrix.get_distance_rowwise,
 * lib/Matrix.ml:191-266, never formed.)  The worked case of INTEGRATION.md 6p: nine rows on a line, all values small binary fractions,
 * so every distance is exact -- a tight lineage of five rows, a second one of three, and a row far from both.  eps = 0.5.  One call
 * gives density, delta and parent; the cut is then made twice on the host, after a look at the decision graph, and once more by the
 * library in the call itself.  Built and run by tests/test_gpu_density_peaks_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_density_peaks.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_density_peaks
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
#define ROWS 9
#define EPS 0.5

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

static int differ_u32(const uint32_t *got, const uint32_t *want, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (got[i] != want[i]) return 1;
  return 0;
}

int main(void) {
  const double x[ROWS] = {0.0, 0.5, 1.0, 1.5, 10.0, 10.5, 11.0, 30.0, 0.75};
  const double want_density[ROWS] = {2, 4, 4, 2, 2, 3, 2, 1, 3};
  const double want_delta[ROWS] = {0.5, INFINITY, 0.5, 0.5, 0.5, 9.5, 0.5, 19.0, 0.25};
  const uint32_t want_parent[ROWS] = {1, 1, 1, 2, 5, 2, 5, 6, 1};
  const uint32_t want_loose[ROWS] = {1, 1, 1, 1, 5, 5, 5, 7, 1}; /* min_density = -inf, min_delta = 2 */
  const uint32_t want_dense[ROWS] = {1, 1, 1, 1, 5, 5, 5, 5, 1}; /* min_density = 2, min_delta = 2: the far row is no centre */
  const uint32_t want_loose_counts[3] = {3, 1, 0}, want_dense_counts[3] = {2, 1, 0};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0; /* dimension 0; the other dimensions are zero */
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* one pass: the decision graph, no cut yet */
  double density[ROWS], delta[ROWS];
  uint32_t parent[ROWS], labels[ROWS], counts[3];
  CHECK(kpop_density_peaks(rs, EPS, NULL, -INFINITY, INFINITY, density, delta, parent, NULL, NULL));
  print_doubles("density", density, ROWS);
  print_doubles("delta", delta, ROWS);
  print_counts("parent", parent, ROWS);
  int bad = differ(density, want_density, ROWS) || differ(delta, want_delta, ROWS) || differ_u32(parent, want_parent, ROWS);
  /* the cut on the host, at thresholds chosen after the pass */
  CHECK(kpop_density_peaks_cut(ROWS, density, delta, parent, -INFINITY, 2.0, labels, counts));
  print_counts("labels at (-inf, 2)", labels, ROWS);
  print_counts("counts at (-inf, 2)", counts, 3);
  bad = bad || differ_u32(labels, want_loose, ROWS) || differ_u32(counts, want_loose_counts, 3);
  CHECK(kpop_density_peaks_cut(ROWS, density, delta, parent, 2.0, 2.0, labels, counts));
  print_counts("labels at (2, 2)", labels, ROWS);
  print_counts("counts at (2, 2)", counts, 3);
  bad = bad || differ_u32(labels, want_dense, ROWS) || differ_u32(counts, want_dense_counts, 3);
  /* the same cut made by the call itself, with the densities handed back in: eps is then not read */
  uint32_t again[ROWS], again_counts[3];
  CHECK(kpop_density_peaks(rs, NAN, density, 2.0, 2.0, NULL, NULL, NULL, again, again_counts));
  const int same = !differ_u32(again, labels, ROWS) && !differ_u32(again_counts, counts, 3);
  printf("the cut in the call: %s\n", same ? "the same labels" : "DIFFERENT labels");
  bad = bad || !same;
  /* without keeping a set */
  double delta2[ROWS];
  uint32_t parent2[ROWS];
  CHECK(kpop_distance_density_peaks(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, EPS, NULL, -INFINITY, INFINITY, NULL, delta2, parent2, NULL, NULL));
  const int same2 = !differ(delta2, delta, ROWS) && !differ_u32(parent2, parent, ROWS);
  printf("without a set: %s\n", same2 ? "the same result" : "a DIFFERENT result");
  bad = bad || !same2;
  /* no density and no radius, a threshold that is not a number, a parent that ranks below its child: refused */
  parent2[1] = 0; /* row 0 (density 2) above row 1 (density 4) */
  const int rc_eps = kpop_density_peaks(rs, NAN, NULL, -INFINITY, 1.0, NULL, delta2, NULL, NULL, NULL);
  const int rc_nan = kpop_density_peaks(rs, EPS, NULL, -INFINITY, NAN, NULL, delta2, NULL, NULL, NULL);
  const int rc_cut = kpop_density_peaks_cut(ROWS, density, delta, parent2, -INFINITY, 2.0, labels, counts);
  printf("no eps: %d, a NaN threshold: %d, a parent below its child: %d\n", rc_eps, rc_nan, rc_cut);
  bad = bad || rc_eps != KPOP_ERR_INVALID || rc_nan != KPOP_ERR_INVALID || rc_cut != KPOP_ERR_INVALID;
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return bad ? 1 : 0;
}
