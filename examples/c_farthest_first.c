/* c_farthest_first.c -- the farthest-first traversal of a resident set from a plain C99 host: k diverse rows for every k
 * (kpop_farthest_first: the distances of Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, of the set against itself, never
 * formed).  The ten rows of c_dbscan.c on a line, all values small binary fractions, so every distance is exact.  The full order
 * with its radii and parents; then the same from its first three picks as seeds, which must agree; then a cover at a radius of
 * 0.375: the picks made before the radius fell to it, and the pick that stands for every row.  Built and run by
 * tests/test_gpu_farthest_first_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_farthest_first.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_farthest_first
 * Exits non-zero on any mismatch with what it expects. */
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
#define COVER_RADIUS 0.375

static void print_rows(const char *what, const uint32_t *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) {
    if (v[i] == KPOP_NOISE) printf(" none");
    else printf(" %u", v[i]);
  }
  printf("\n");
}

static void print_radii(const char *what, const double *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}

int main(void) {
  /* dimension 0 of the rows; the other dimensions are zero.  Row 7 lies at 0.75 from rows 0 and 6: the tie keeps the earlier pick */
  const double x[ROWS] = {0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375};
  const uint32_t want_pick[ROWS] = {0, 8, 6, 7, 3, 9, 1, 2, 4, 5};
  const uint32_t want_parent[ROWS] = {KPOP_NOISE, 0, 0, 0, 6, 0, 0, 9, 3, 6};
  const uint32_t want_rep_of[ROWS] = {0, 0, 0, 6, 6, 6, 6, 7, 8, 0};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* every row, in farthest-first order */
  uint32_t n_picks = 0, pick[ROWS], parent[ROWS], rep_of[ROWS];
  double radius[ROWS], rep_dist[ROWS];
  CHECK(kpop_farthest_first(rs, ROWS, -1.0, NULL, 0, &n_picks, pick, radius, parent, NULL, NULL, NULL));
  print_rows("pick", pick, n_picks);
  print_radii("pick_radius", radius, n_picks);
  print_rows("pick_parent", parent, n_picks);
  int bad = n_picks != ROWS;
  for (uint32_t t = 0; t < n_picks && !bad; ++t) bad = pick[t] != want_pick[t] || parent[t] != want_parent[t];
  /* from the first three picks as seeds: the same traversal */
  uint32_t n_again = 0, again[ROWS], again_parent[ROWS];
  double again_radius[ROWS];
  CHECK(kpop_farthest_first(rs, ROWS, -1.0, pick, 3, &n_again, again, again_radius, again_parent, NULL, NULL, NULL));
  int same = n_again == n_picks;
  for (uint32_t t = 0; t < n_picks && same; ++t) same = again[t] == pick[t] && again_radius[t] == radius[t] && again_parent[t] == parent[t];
  printf("from three seeds: %s\n", same ? "the same picks" : "DIFFERENT picks");
  /* a cover at a radius, without keeping a set: the traversal stops before the first pick whose radius is within it */
  CHECK(kpop_distance_farthest_first(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, ROWS, COVER_RADIUS, NULL, 0, &n_again, again, NULL, NULL, rep_of,
                                     rep_dist, NULL));
  print_rows("pick at 0.375", again, n_again);
  print_rows("rep_of", rep_of, ROWS);
  print_radii("rep_dist", rep_dist, ROWS);
  bad = bad || n_again != 4;
  for (int i = 0; i < ROWS && !bad; ++i) bad = rep_of[i] != want_rep_of[i] || rep_dist[i] > COVER_RADIUS;
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return (bad || !same) ? 1 : 0;
}
