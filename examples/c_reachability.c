/* c_reachability.c -- the mutual-reachability forest of a resident set from a plain C99 host: DBSCAN at every radius.  The worked
 * case of INTEGRATION.md 6j -- ten rows whose only non-zero coordinate is 0, .125, .25, 1.125, 1.25, 1.375, 1.5, .75, 5, .375, under the
 * distances of Matrix.get_distance_rowwise (lib/Matrix.ml:191-266) of the set against itself, euclidean, a metric of ones, not
 * normalised, min_pts = 4: every row's core distance and the minimum spanning forest under max(d, core_i, core_j)
 * (kpop_reachability_tree).  One forest answers every radius: it is cut at two of them on the host (kpop_reachability_cut: no GPU
 * work), and at each the core rows' labels are compared with what kpop_dbscan finds there with its passes over all pairs.
 * Built and run by tests/test_gpu_reachability_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_reachability.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_reachability
 * Prints the core distances, the forest's edges in their order, the two cuts and the argument errors, deterministically. */
#include <math.h>
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

#define D 3
#define ROWS 10
#define MIN_PTS 4

static const double X[ROWS] = {0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375};

/* the forest cut at T on the host, and the core rows' labels against kpop_dbscan(T, MIN_PTS): 1 when they agree */
static int cut_and_compare(kpop_refset *rs, uint32_t n_edges, const uint32_t *edge_i, const uint32_t *edge_j, const double *edge_dist, const double *core_dist,
                           double T) {
  uint32_t cut[ROWS], counts[3], labels[ROWS], core_of[ROWS], degree[ROWS], db_counts[3];
  if (kpop_reachability_cut(ROWS, n_edges, edge_i, edge_j, edge_dist, core_dist, T, cut, counts) != 0) return 0;
  printf("cut at %g: %u clusters, %u core rows, %u noise rows; labels:", T, counts[0], counts[1], counts[2]);
  for (int i = 0; i < ROWS; ++i) {
    if (cut[i] == KPOP_NOISE) printf(" -");
    else printf(" %u", cut[i]);
  }
  printf("\n");
  if (kpop_dbscan(rs, T, MIN_PTS, labels, core_of, degree, db_counts) != 0) return 0;
  int same = counts[0] == db_counts[0] && counts[1] == db_counts[1];
  for (int i = 0; i < ROWS; ++i) {
    const int core = degree[i] >= MIN_PTS;
    same = same && core == (core_dist[i] <= T) && (core ? cut[i] == labels[i] : cut[i] == KPOP_NOISE);
  }
  printf("the cut at %g and kpop_dbscan at %g: %s\n", T, T, same ? "the same labels on the core rows" : "DIFFERENT labels");
  return same;
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], metric[D];
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = c == 0 ? X[i] : 0.0;
  for (int c = 0; c < D; ++c) metric[c] = 1.0;
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* the core distances alone, then the whole forest: every pair whose weight is a number is an edge of the graph */
  double core_dist[ROWS], core_again[ROWS], edge_dist[ROWS - 1];
  uint32_t edge_i[ROWS - 1], edge_j[ROWS - 1], labels[ROWS], n_edges = 0;
  CHECK(kpop_core_distances(rs, MIN_PTS, core_dist));
  printf("core distances at min_pts = %d:", MIN_PTS);
  for (int i = 0; i < ROWS; ++i) printf(" %.17g", core_dist[i]);
  printf("\n");
  CHECK(kpop_reachability_tree(rs, MIN_PTS, INFINITY, &n_edges, edge_i, edge_j, edge_dist, core_again, labels));
  int same = 1;
  for (int i = 0; i < ROWS; ++i) same = same && core_again[i] == core_dist[i] && labels[i] == 0;
  printf("forest: %u edges on %d rows\n", n_edges, ROWS);
  for (uint32_t e = 0; e < n_edges; ++e) printf("edge %u: %u - %u at %.17g\n", e, edge_i[e], edge_j[e], edge_dist[e]);
  /* two cuts of the one forest, on the host, each against the passes over all pairs */
  same = cut_and_compare(rs, n_edges, edge_i, edge_j, edge_dist, core_dist, 0.25) && same;
  same = cut_and_compare(rs, n_edges, edge_i, edge_j, edge_dist, core_dist, 0.375) && same;
  /* what the calls refuse */
  uint32_t counts[3];
  printf("min_pts = 0: %d\n", kpop_core_distances(rs, 0, core_again));
  printf("min_pts = 130: %d\n", kpop_reachability_tree(rs, 130, INFINITY, &n_edges, edge_i, edge_j, edge_dist, core_again, labels));
  printf("max_distance = NaN: %d\n", kpop_reachability_tree(rs, MIN_PTS, NAN, &n_edges, edge_i, edge_j, edge_dist, core_again, labels));
  printf("no room for the edges: %d\n", kpop_reachability_tree(rs, MIN_PTS, INFINITY, &n_edges, NULL, NULL, NULL, core_again, labels));
  printf("a cut without core distances: %d\n", kpop_reachability_cut(ROWS, 0, NULL, NULL, NULL, NULL, 0.25, labels, counts));
  printf("a cut at NaN: %d\n", kpop_reachability_cut(ROWS, 0, NULL, NULL, NULL, core_dist, NAN, labels, counts));
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return same ? 0 : 1;
}
