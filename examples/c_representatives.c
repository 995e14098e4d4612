/* c_representatives.c -- representatives at a distance from a plain C99 host: a resident set is thinned to one row per neighbourhood
 * of a radius (kpop_representatives_within: the greedy cover in row order over the distances of Matrix.get_distance_rowwise,
 * lib/Matrix.ml:191-266, of the set against itself, never formed), every dropped row remembering the kept row that stands for it.
 * The set is made with room to grow, thinned, given more rows, and thinned again from the result it had: only the new rows are
 * examined, against the representatives, and the answer is the from-scratch one.  Built and run by
 * tests/test_gpu_representatives_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_representatives.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_representatives
 * Prints, per step, the representatives; then every row's representative and its distance, deterministically. */
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
#define MAX_DISTANCE 0.375

/* row i, dimension c: group i % 5 sits at (2 g, g, 0, -g); inside a group the rows step by 1/8 along dimension i % D -- small exact
   binary fractions */
static double row_value(int i, int c) {
  const int g = i % 5;
  const double centre = c == 0 ? 2.0 * g : c == 1 ? g : c == 2 ? 0.0 : -g;
  return centre + (c == i % D ? (double)(i / 5) / 8.0 : 0.0);
}

/* the rows appended: seven steps of an eighth from group 0's centre towards group 1's (some within reach of a representative, some
   not), and one row far from everything */
static double more_value(int k, int c) {
  if (k == MORE - 1) return c == 3 ? 40.0 : 0.0;
  return (c == 0 ? 2.0 : c == 1 ? 1.0 : c == 2 ? 0.0 : -1.0) * (double)(k + 1) / 8.0;
}

static void report(const char *what, const uint32_t *rep_of, uint32_t rows, uint32_t n_reps) {
  printf("%s: %u rows, %u representatives:", what, rows, n_reps);
  for (uint32_t i = 0; i < rows; ++i)
    if (rep_of[i] == i) printf(" %u", i);
  printf("\n");
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
  uint32_t rep_of[ROWS + MORE], again_of[ROWS + MORE], n_reps = 0, n_again = 0;
  double rep_dist[ROWS + MORE], again_dist[ROWS + MORE];
  CHECK(kpop_representatives_within(rs, MAX_DISTANCE, 0, rep_of, rep_dist, &n_reps));
  report("created", rep_of, ROWS, n_reps);
  /* the set grows: rep_of[0 .. ROWS) are what the call above returned, at the same distance; rep_dist[0 .. ROWS) stays as it is */
  CHECK(kpop_refset_append(rs, more, MORE));
  CHECK(kpop_representatives_within(rs, MAX_DISTANCE, ROWS, rep_of, rep_dist, &n_reps));
  report("grown", rep_of, ROWS + MORE, n_reps);
  /* from scratch: the same result */
  CHECK(kpop_representatives_within(rs, MAX_DISTANCE, 0, again_of, again_dist, &n_again));
  int same = n_again == n_reps;
  for (int i = 0; i < ROWS + MORE; ++i) same = same && again_of[i] == rep_of[i] && again_dist[i] == rep_dist[i];
  printf("from scratch: %s\n", same ? "the same result" : "a DIFFERENT result");
  printf("rep_of:");
  for (int i = 0; i < ROWS + MORE; ++i) printf(" %u", rep_of[i]);
  printf("\nrep_dist:");
  for (int i = 0; i < ROWS + MORE; ++i) printf(" %.17g", rep_dist[i]);
  printf("\n");
  /* without keeping a set, and without the distances */
  CHECK(kpop_distance_representatives(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 1e300, again_of, NULL, &n_again));
  report("one neighbourhood", again_of, ROWS, n_again);
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return same ? 0 : 1;
}
