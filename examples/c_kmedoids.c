/* c_kmedoids.c -- k-medoids on a resident set from a plain C99 host: three groups around three real rows (kpop_kmedoids: the
 * distances of Matrix.get_distance_rowwise, lib/Matrix.ml:191-266, of the set against itself, never formed).  The ten rows of
 * c_farthest_first.c on a line, all values small binary fractions, so every distance and every sum is exact.  The first three
 * farthest-first picks are the initial medoids (the k-centre seeding); then the plain assignment to them (max_iter = 0), the run
 * to convergence, and the same run continued from the first round's medoids, which must agree.  Built and run by
 * tests/test_gpu_kmedoids_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_kmedoids.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_kmedoids
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
#define K 3
#define MAX_ITER 10

static void print_rows(const char *what, const uint32_t *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) {
    if (v[i] == KPOP_NO_CLASS) printf(" none");
    else printf(" %u", v[i]);
  }
  printf("\n");
}

static void print_doubles(const char *what, const double *v, uint32_t n) {
  printf("%s:", what);
  for (uint32_t i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}

int main(void) {
  /* dimension 0 of the rows; the other dimensions are zero */
  const double x[ROWS] = {0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375};
  const uint32_t want_init[K] = {0, 8, 6}, want_medoid[K] = {2, 8, 4}; /* row 4 on a tie with row 5 */
  const uint32_t want_class[ROWS] = {0, 0, 0, 2, 2, 2, 2, 0, 1, 0};
  const double want_dist[ROWS] = {0.25, 0.125, 0.0, 0.125, 0.0, 0.125, 0.25, 0.5, 0.0, 0.125};
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? x[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  CHECK(kpop_init(0));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  uint32_t n_picks = 0, init[K];
  CHECK(kpop_farthest_first(rs, K, -1.0, NULL, 0, &n_picks, init, NULL, NULL, NULL, NULL, NULL));
  print_rows("init", init, n_picks);
  int bad = n_picks != K;
  for (uint32_t c = 0; c < K && !bad; ++c) bad = init[c] != want_init[c];
  /* the plain assignment to the three picks */
  uint32_t medoid[K], class_of[ROWS], class_rows[K], n_iter = 0;
  double dist[ROWS], own_mean[ROWS], cost[MAX_ITER + 1];
  int converged = 0;
  CHECK(kpop_kmedoids(rs, K, init, 0, medoid, class_of, dist, own_mean, class_rows, cost, &n_iter, &converged));
  print_rows("class_of, round 0", class_of, ROWS);
  print_doubles("own_mean, round 0", own_mean, ROWS);
  printf("cost[0] = %.17g, a fixed point: %s\n", cost[0], converged ? "yes" : "no");
  bad = bad || n_iter != 0 || converged || cost[0] != 2.25;
  /* to convergence */
  CHECK(kpop_kmedoids(rs, K, init, MAX_ITER, medoid, class_of, dist, own_mean, class_rows, cost, &n_iter, &converged));
  print_rows("medoid", medoid, K);
  print_rows("class_of", class_of, ROWS);
  print_doubles("dist", dist, ROWS);
  print_rows("class_rows", class_rows, K);
  print_doubles("cost", cost, n_iter + 1);
  printf("n_iter = %u, converged = %d\n", n_iter, converged);
  bad = bad || n_iter != 1 || !converged || cost[1] != 1.5 || cost[2] == cost[2]; /* (past n_iter: NaN) */
  for (uint32_t c = 0; c < K && !bad; ++c) bad = medoid[c] != want_medoid[c];
  for (int i = 0; i < ROWS && !bad; ++i) bad = class_of[i] != want_class[i] || dist[i] != want_dist[i];
  /* one round, then the rest from its medoids, without keeping a set: the same result */
  uint32_t first[K], again[K], again_class[ROWS], n_first = 0, n_again = 0;
  double again_dist[ROWS];
  int conv_first = 0, conv_again = 0;
  CHECK(kpop_distance_kmedoids(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, K, init, 1, first, NULL, NULL, NULL, NULL, NULL, &n_first, &conv_first));
  CHECK(kpop_distance_kmedoids(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, K, first, MAX_ITER - 1, again, again_class, again_dist, NULL, NULL, NULL, &n_again,
                               &conv_again));
  int same = n_first + n_again == n_iter && conv_again == converged;
  for (uint32_t c = 0; c < K && same; ++c) same = again[c] == medoid[c];
  for (int i = 0; i < ROWS && same; ++i) same = again_class[i] == class_of[i] && again_dist[i] == dist[i];
  printf("continued from the first round: %s\n", same ? "the same result" : "a DIFFERENT result");
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  if (bad) fprintf(stderr, "the result is not the expected one\n");
  return (bad || !same) ? 1 : 0;
}
