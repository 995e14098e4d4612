// forest_rounds.h -- the Boruvka rounds of forest.hip for another caller: reachability.hip runs them under the mutual-reachability
// weight.  The kernels, the workspace and the two sorts stay forest.hip's own, one body each; this is the way in (as knn_lists.h
// is knn.hip's for knn_validate.hip).
#pragma once
#include "common.h"
#include "refset.h"

namespace kpop {

// the bytes forest_dev carves out of d_work for a set of r1 rows: kpop_dev_spanning_forest_workspace_bytes
uint64_t forest_workspace_bytes(uint32_t r1);

// The minimum spanning forest of the set under the order (weight, i, j), capped at max_distance: what kpop_dev_spanning_forest
// documents.  d_core == NULL: an edge weighs its distance.  d_core[r1] set: it weighs max(d, d_core[i], d_core[j]), and a NaN among
// the three is no edge.  host_reads: after a round, wait for the word that says what it added and stop at zero; otherwise enqueues
// only, ceil(log2 r1) gated rounds.  who: the entry point, for the messages
int forest_dev(kpop_refset *rs, const double *d_core, double max_distance, void *d_work, uint32_t *d_n_edges, uint32_t *d_edge_i, uint32_t *d_edge_j,
               double *d_edge_dist, uint32_t *d_labels, hipStream_t st, bool host_reads, const char *who);

}  // namespace kpop
