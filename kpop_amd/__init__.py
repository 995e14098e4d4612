"""kpop_amd -- KPop's count -> twist -> distance hot path on AMD MI355X (gfx950).

The product is libkpop_hip.so (hand-written HIP kernels behind the C ABI of
include/kpop_hip.h); this package is the thin host-side mirror of the
reference's interface for that path.  Importing it does not touch the GPU;
`init(device)` does, and fails loudly when no GPU or no library is present.
"""
from .api import (check, COSINE, DNA_DS, DNA_SS, PROTEIN, EUCLIDEAN, METRIC_FLAT, METRIC_POWERS, MINKOWSKI, KPopError,  # noqa: F401
                  Twister, ca, count_reads, device_count, distance_rowwise, distance_summary, embeddings, init, summarize_distances,
                  metric_compute, parse_distance, splits_gaps, counter_stats, counter_combine, counter_transform, counter_distill, DISTILL_ROW_NAMES, COMBINE_MEAN,
                  COMBINE_MEDIAN, TRANSF_BINARY, TRANSF_POWER, TRANSF_CLR, TRANSF_PSEUDO, Pipeline, host_empty, init_devices, use_device,
                  device_slots, OUT_TWISTED, OUT_DISTANCES, OUT_SUMMARY, Sharded, shard_bounds, sharded_distance_rowwise,
                  sharded_distance_summary, RefSet, dev_refset_workspace_bytes, dev_refset_distance_rowwise, dev_refset_distance_summary,
                  dev_neighbours_within_workspace_bytes, dev_neighbours_within, distance_within, dev_clusters_within_workspace_bytes,
                  dev_clusters_within, distance_clusters, dev_spanning_forest_workspace_bytes, dev_spanning_forest, distance_spanning_forest,
                  forest_cut, NO_CLASS, dev_knn_vote_workspace_bytes, dev_knn_vote, distance_knn_vote, dev_knn_vote_ks_workspace_bytes,
                  dev_knn_vote_ks, dev_knn_validate_workspace_bytes, dev_knn_validate, distance_knn_validate, confusion_matrix,
                  dev_representatives_within_workspace_bytes, dev_representatives_within, distance_representatives, NOISE,
                  dev_dbscan_workspace_bytes, dev_dbscan, distance_dbscan, dev_core_distances_workspace_bytes, dev_core_distances,
                  dev_reachability_forest_workspace_bytes, dev_reachability_forest, distance_reachability_forest, reachability_cut,
                  Silhouette, dev_silhouette_workspace_bytes, dev_silhouette, distance_silhouette, silhouette_summary, dense_labels,
                  ClassLinkage, dev_class_linkage_workspace_bytes, dev_class_linkage, distance_class_linkage, ClassTree, class_tree, class_tree_newick,
                  LINK_SINGLE, LINK_COMPLETE, LINK_AVERAGE,
                  FarthestFirst, dev_farthest_first_workspace_bytes, dev_farthest_first, distance_farthest_first,
                  KMedoids, dev_kmedoids_workspace_bytes, dev_kmedoids, distance_kmedoids,
                  Lof, dev_lof_workspace_bytes, dev_lof, dev_lof_score_workspace_bytes, dev_lof_score, distance_lof,
                  DensityPeaks, dev_density_peaks_workspace_bytes, dev_density_peaks, distance_density_peaks, density_peaks_cut)

__all__ = ["init", "device_count", "count_reads", "Twister", "ca", "metric_compute", "distance_rowwise",
           "distance_summary", "embeddings", "splits_gaps", "summarize_distances", "parse_distance", "KPopError", "DNA_DS", "DNA_SS", "PROTEIN", "EUCLIDEAN", "COSINE",
           "MINKOWSKI", "METRIC_FLAT", "METRIC_POWERS", "counter_stats", "counter_combine", "counter_transform", "counter_distill", "DISTILL_ROW_NAMES",
           "COMBINE_MEAN", "COMBINE_MEDIAN", "TRANSF_BINARY", "TRANSF_POWER", "TRANSF_CLR", "TRANSF_PSEUDO", "Pipeline", "host_empty",
           "init_devices", "use_device", "device_slots", "OUT_TWISTED", "OUT_DISTANCES", "OUT_SUMMARY", "Sharded", "shard_bounds",
           "sharded_distance_rowwise", "sharded_distance_summary", "RefSet", "dev_refset_workspace_bytes",
           "dev_refset_distance_rowwise", "dev_refset_distance_summary", "dev_neighbours_within_workspace_bytes",
           "dev_neighbours_within", "distance_within", "dev_clusters_within_workspace_bytes", "dev_clusters_within",
           "distance_clusters", "dev_spanning_forest_workspace_bytes", "dev_spanning_forest", "distance_spanning_forest", "forest_cut",
           "NO_CLASS", "dev_knn_vote_workspace_bytes", "dev_knn_vote", "distance_knn_vote", "dev_knn_vote_ks_workspace_bytes", "dev_knn_vote_ks",
           "dev_knn_validate_workspace_bytes", "dev_knn_validate", "distance_knn_validate", "confusion_matrix",
           "dev_representatives_within_workspace_bytes", "dev_representatives_within", "distance_representatives", "NOISE",
           "dev_dbscan_workspace_bytes", "dev_dbscan", "distance_dbscan", "dev_core_distances_workspace_bytes", "dev_core_distances",
           "dev_reachability_forest_workspace_bytes", "dev_reachability_forest", "distance_reachability_forest", "reachability_cut",
           "Silhouette", "dev_silhouette_workspace_bytes", "dev_silhouette", "distance_silhouette", "silhouette_summary", "dense_labels",
           "ClassLinkage", "dev_class_linkage_workspace_bytes", "dev_class_linkage", "distance_class_linkage", "ClassTree", "class_tree", "class_tree_newick",
           "LINK_SINGLE", "LINK_COMPLETE", "LINK_AVERAGE",
           "FarthestFirst", "dev_farthest_first_workspace_bytes", "dev_farthest_first", "distance_farthest_first",
           "KMedoids", "dev_kmedoids_workspace_bytes", "dev_kmedoids", "distance_kmedoids",
           "Lof", "dev_lof_workspace_bytes", "dev_lof", "dev_lof_score_workspace_bytes", "dev_lof_score", "distance_lof",
           "DensityPeaks", "dev_density_peaks_workspace_bytes", "dev_density_peaks", "distance_density_peaks", "density_peaks_cut"]
