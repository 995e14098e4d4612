/* c_forest.c -- the single-linkage tree of a resident set from a plain C99 host: the minimum spanning forest of the graph on the
 * set's rows under the distances of Matrix.get_distance_rowwise (lib/Matrix.ml:191-266) of the set against itself, never formed
 * (kpop_spanning_forest).  One forest answers every threshold: it is cut at two distances on the host (kpop_forest_cut: no GPU
 * work), and the second cut is compared with what kpop_clusters_within finds at that distance with a pass over all pairs.
 * Built and run by tests/test_gpu_forest_c.py:
 *     gcc -O2 -std=c99 -Iinclude examples/c_forest.c -Lkpop_amd -lkpop_hip -Wl,-rpath,$PWD/kpop_amd -lm -o c_forest
 * Prints the forest's edges in their order, the two cuts' labels, and whether the second equals the clusters, deterministically. */
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

#define D 4
#define GROUPED 24
#define ROWS 32
#define CUT_A 0.25
#define CUT_B 0.375

/* row i, dimension c.  The first 24 rows: group i % 5 sits at (2 g, g, 0, -g); inside a group the rows step by 1/8 along
   dimension i % D.  Then seven steps of an eighth from group 0's centre to group 1's (a bridge), and one row far from everything:
   small exact binary fractions, and many equal distances */
static double row_value(int i, int c) {
  if (i == ROWS - 1) return c == 3 ? 40.0 : 0.0;
  if (i >= GROUPED) return (c == 0 ? 2.0 : c == 1 ? 1.0 : c == 2 ? 0.0 : -1.0) * (double)(i - GROUPED + 1) / 8.0;
  const int g = i % 5;
  const double centre = c == 0 ? 2.0 * g : c == 1 ? g : c == 2 ? 0.0 : -g;
  return centre + (c == i % D ? (double)(i / 5) / 8.0 : 0.0);
}

static void print_labels(const char *what, const uint32_t *labels, uint32_t n_clusters) {
  printf("%s: %u clusters; labels:", what, n_clusters);
  for (int i = 0; i < ROWS; ++i) printf(" %u", labels[i]);
  printf("\n");
}

int main(void) {
  CHECK(kpop_init(0));
  double rows[ROWS * D], metric[D];
  const double inertia[D] = {0.4, 0.3, 0.2, 0.1};
  for (int i = 0; i < ROWS; ++i)
    for (int c = 0; c < D; ++c) rows[i * D + c] = row_value(i, c);
  CHECK(kpop_metric_compute(KPOP_METRIC_POWERS, inertia, D, 1.0, 1.0, 2.0, metric));
  kpop_refset *rs = NULL;
  CHECK(kpop_refset_create(rows, ROWS, D, metric, KPOP_EUCLIDEAN, 2.0, 0, 0, &rs));
  /* the whole tree: every pair whose distance is a number is an edge of the graph */
  uint32_t edge_i[ROWS - 1], edge_j[ROWS - 1], labels[ROWS], n_edges = 0;
  double edge_dist[ROWS - 1];
  CHECK(kpop_spanning_forest(rs, INFINITY, &n_edges, edge_i, edge_j, edge_dist, labels));
  printf("forest: %u edges on %d rows\n", n_edges, ROWS);
  for (uint32_t e = 0; e < n_edges; ++e) printf("edge %u: %u - %u at %.17g\n", e, edge_i[e], edge_j[e], edge_dist[e]);
  /* two cuts of the one forest, on the host */
  uint32_t cut_a[ROWS], cut_b[ROWS], n_a = 0, n_b = 0;
  CHECK(kpop_forest_cut(ROWS, n_edges, edge_i, edge_j, edge_dist, CUT_A, cut_a, &n_a));
  print_labels("cut at 0.25", cut_a, n_a);
  CHECK(kpop_forest_cut(ROWS, n_edges, edge_i, edge_j, edge_dist, CUT_B, cut_b, &n_b));
  print_labels("cut at 0.375", cut_b, n_b);
  /* the same clusters, from a pass over all pairs */
  uint32_t clusters[ROWS], n_clusters = 0;
  CHECK(kpop_clusters_within(rs, CUT_B, 0, clusters, &n_clusters));
  int same = n_clusters == n_b;
  for (int i = 0; i < ROWS; ++i) same = same && clusters[i] == cut_b[i];
  printf("the cut at 0.375 and kpop_clusters_within at 0.375: %s\n", same ? "the same labels" : "DIFFERENT labels");
  CHECK(kpop_refset_free(rs));
  CHECK(kpop_shutdown());
  return same ? 0 : 1;
}
