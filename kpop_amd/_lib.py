"""ctypes binding of libkpop_hip.so -- the C ABI declared in include/kpop_hip.h.

There is no CPU fallback: if the shared library is missing, or no GPU is
visible when kpop_init() runs, the caller gets an exception.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KPOP_HIP_LIB", os.path.join(_HERE, "libkpop_hip.so"))  # the override is for A/B runs of two builds

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
vp = C.c_void_p


class PipelineConfig(C.Structure):
    """kpop_pipeline_config (include/kpop_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("content", C.c_int), ("normalize_counts", C.c_int), ("kind", C.c_int),
                ("p", C.c_double), ("normalize_distances", C.c_int), ("outputs", C.c_int), ("keep_at_most", C.c_uint32),
                ("max_neighbours", C.c_uint32), ("chunk_reads", C.c_uint32), ("depth", C.c_uint32),
                ("chunk_bases", C.c_uint64), ("record_timeline", C.c_int)]


class PipelineOutputs(C.Structure):
    """kpop_pipeline_outputs (include/kpop_hip.h)"""
    _fields_ = [("twisted", vp), ("distances", vp), ("stats", vp), ("n_neighbours", vp), ("nb_index", vp),
                ("nb_distance", vp), ("nb_z", vp)]


# name -> (restype, argtypes); mirrors include/kpop_hip.h one to one
SIGNATURES = {
    "kpop_init": (C.c_int, [C.c_int]),
    "kpop_init_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "kpop_use_device": (C.c_int, [C.c_int]),
    "kpop_device_slots": (C.c_int, []),
    "kpop_host_alloc": (C.c_int, [C.POINTER(vp), C.c_uint64]),
    "kpop_host_free": (C.c_int, [vp]),
    "kpop_host_register": (C.c_int, [vp, C.c_uint64]),
    "kpop_host_unregister": (C.c_int, [vp]),
    "kpop_pipeline_create": (C.c_int, [vp, f64p, C.c_uint32, f64p, C.POINTER(PipelineConfig), C.POINTER(vp)]),
    "kpop_pipeline_submit": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(PipelineOutputs), u64p]),
    "kpop_pipeline_submit_packed": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.POINTER(PipelineOutputs), u64p]),
    "kpop_pipeline_collect": (C.c_int, [vp, C.c_uint64]),
    "kpop_packed_code_words": (C.c_uint64, [C.c_uint64]),
    "kpop_packed_mask_words": (C.c_uint64, [C.c_uint64]),
    "kpop_pack_bases": (C.c_int, [vp, C.c_uint64, vp, vp, C.c_int]),
    "kpop_count_twist_packed": (C.c_int, [vp, vp, vp, u64p, C.c_uint32, C.c_int, C.c_int, f64p]),
    "kpop_dev_unpack_bases": (C.c_int, [vp, vp, C.c_uint64, vp, vp]),
    "kpop_dev_count_twist_packed": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_int, vp, vp]),
    "kpop_pipeline_run": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(PipelineOutputs)]),
    "kpop_pipeline_stats": (C.c_int, [vp, u32p, C.POINTER(C.c_int), u32p]),
    "kpop_pipeline_timeline": (C.c_int, [vp, C.c_uint32, f64p, u32p]),
    "kpop_pipeline_destroy": (C.c_int, [vp]),
    "kpop_dev_workspace_reserve_stream": (C.c_int, [C.c_uint64, vp]),
    "kpop_shard_bounds": (C.c_int, [C.c_uint64, C.c_int, C.c_int, u64p, u64p]),
    "kpop_twister_replicate": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    "kpop_sharded_create": (C.c_int, [vp, f64p, C.c_uint32, f64p, C.POINTER(PipelineConfig), C.POINTER(vp)]),
    "kpop_sharded_slots": (C.c_int, [vp]),
    "kpop_sharded_run": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(PipelineOutputs)]),
    "kpop_sharded_spectra_twist": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, f64p]),
    "kpop_sharded_resident_step": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), u32p, u64p, C.c_uint32, C.c_int, C.c_int]),
    "kpop_sharded_resident_buffers": (C.c_int, [vp, C.c_int, C.POINTER(vp), u64p, u64p, C.POINTER(vp)]),
    "kpop_sharded_timings": (C.c_int, [vp, C.c_int, f64p, f64p]),
    "kpop_sharded_chunk_timings": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "kpop_sharded_all_vs_all_summary": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u64p, u64p, f64p, u32p,
                                                  u32p, f64p, f64p]),
    "kpop_sharded_destroy": (C.c_int, [vp]),
    "kpop_sharded_distance_rowwise": (C.c_int, [f64p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double,
                                                C.c_int, f64p]),
    "kpop_sharded_distance_summary": (C.c_int, [f64p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double,
                                                C.c_int, C.c_uint32, C.c_uint32, f64p, u32p, u32p, f64p, f64p]),
    "kpop_shutdown": (C.c_int, []),
    "kpop_device_count": (C.c_int, []),
    "kpop_last_error": (C.c_char_p, []),
    "kpop_version": (C.c_char_p, []),
    "kpop_synchronize": (C.c_int, [vp]),
    "kpop_tune": (C.c_int, [C.c_char_p, C.c_int]),
    "kpop_debug_counters": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "kpop_debug_summary_fallbacks": (C.c_int, [C.POINTER(C.c_uint64)]),
    "kpop_dev_malloc": (C.c_int, [C.POINTER(vp), C.c_uint64]),
    "kpop_dev_free": (C.c_int, [vp]),
    "kpop_memcpy_h2d": (C.c_int, [vp, vp, C.c_uint64]),
    "kpop_memcpy_d2h": (C.c_int, [vp, vp, C.c_uint64]),
    "kpop_dev_memset": (C.c_int, [vp, C.c_int, C.c_uint64]),
    "kpop_count_reads": (C.c_int, [u8p, u64p, C.c_uint32, C.c_int, C.c_int, C.c_int, u64p, u32p, u64p,
                                   C.c_uint64]),
    "kpop_twister_load": (C.c_int, [f64p, C.c_uint64, C.c_uint32, u64p, C.c_int, C.POINTER(vp)]),
    "kpop_twister_synth": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.POINTER(vp)]),
    "kpop_twister_synth_slice": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                           C.POINTER(vp)]),
    "kpop_twister_set_count_k": (C.c_int, [vp, C.c_int]),
    "kpop_twister_free": (C.c_int, [vp]),
    "kpop_twister_info": (C.c_int, [vp, u64p, u32p, C.POINTER(C.c_int), u64p]),
    "kpop_twister_direct_bytes": (C.c_int, [vp, u64p]),
    "kpop_twist": (C.c_int, [vp, u64p, f64p, u64p, C.c_uint32, C.c_int, f64p]),
    "kpop_count_twist": (C.c_int, [vp, u8p, u64p, C.c_uint32, C.c_int, C.c_int, f64p]),
    "kpop_spectra_twist": (C.c_int, [vp, u8p, u64p, C.c_uint32, C.c_int, C.c_int, C.c_int, f64p]),
    "kpop_ca": (C.c_int, [f64p, C.c_uint64, C.c_uint32, C.c_int, u32p, f64p, f64p, f64p]),
    "kpop_debug_ca": (C.c_int, [C.POINTER(C.c_uint64)]),
    "kpop_metric_compute": (C.c_int, [C.c_int, f64p, C.c_uint32, C.c_double, C.c_double, C.c_double, f64p]),
    "kpop_distance_rowwise": (C.c_int, [f64p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int,
                                        C.c_double, C.c_int, f64p]),
    "kpop_distance_summary": (C.c_int, [f64p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int,
                                        C.c_double, C.c_int, C.c_uint32, C.c_uint32, f64p, u32p, u32p, f64p,
                                        f64p]),
    "kpop_embeddings": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, f64p]),
    "kpop_splits_gaps": (C.c_int, [f64p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, f64p, u32p, u32p, u32p]),
    "kpop_summarize_distances": (C.c_int, [f64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f64p, u32p, u32p, f64p,
                                           f64p]),
    "kpop_dev_summarize_distances": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp,
                                               vp]),
    "kpop_counter_stats": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64, C.c_double, C.c_double, f64p, f64p]),
    "kpop_counter_combine": (C.c_int, [C.POINTER(vp), C.c_uint64, u32p, C.c_uint32, f64p, C.c_int, vp, f64p]),
    "kpop_counter_transform": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64, C.c_int, C.c_double, C.c_double, f64p,
                                         C.c_int, f64p]),
    "kpop_counter_distill": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64, u32p, C.c_uint32, f64p, f64p]),
    "kpop_dev_counter_distill_workspace_bytes": (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint32]),
    "kpop_dev_counter_distill": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, C.c_uint32, vp, vp, f64p, vp]),
    "kpop_debug_distill_clocks": (C.c_int, [f64p]),
    "kpop_dev_counter_ld": (C.c_uint64, [C.c_uint64]),
    "kpop_dev_counter_workspace_bytes": (C.c_uint64, [C.c_uint32, C.c_uint64]),
    "kpop_dev_counter_stats": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, C.c_double, vp, vp, vp, vp]),
    "kpop_dev_counter_combine": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, C.c_double,
                                           C.c_int, vp, vp, vp, vp]),
    "kpop_dev_counter_transform": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_double, C.c_double,
                                             vp, C.c_int, vp, vp]),
    "kpop_dev_division_probe": (C.c_int, [vp, vp, C.c_uint64, vp, vp, vp]),
    "kpop_dev_synth_reads": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp, vp]),
    "kpop_dev_count_reads_scratch_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_int]),
    "kpop_dev_count_reads": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "kpop_dev_workspace_reserve": (C.c_int, [C.c_uint64]),
    "kpop_dev_count_twist": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_int, vp, vp]),
    "kpop_dev_twist": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_int, vp, vp]),
    "kpop_dev_ca_workspace_bytes": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "kpop_dev_ca": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.c_int, vp, u32p, vp, vp, vp, vp]),
    "kpop_dev_table_row_sums": (C.c_int, [vp, C.c_uint64, C.c_uint32, vp, vp]),
    "kpop_dev_table_col_sums": (C.c_int, [vp, C.c_uint64, C.c_uint32, vp, vp]),
    "kpop_dev_table_gather_rows": (C.c_int, [vp, C.c_uint32, vp, C.c_uint64, vp, vp]),
    "kpop_dev_twist_dense_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_twist_dense": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_int, vp, vp, vp]),
    "kpop_dev_count_twist_dense_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_count_twist_dense": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp]),
    "kpop_dev_twist_dense_sorted": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_int, vp, vp, vp]),
    "kpop_dev_distance_workspace_bytes": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "kpop_dev_distance_rowwise": (C.c_int, [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_int,
                                            C.c_double, C.c_int, vp, vp, vp]),
    "kpop_dev_row_norms": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, vp, vp]),
    "kpop_dev_distance_rowwise_norms": (C.c_int, [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_int, vp, vp,
                                                  vp]),
    "kpop_dev_distance_summary": (C.c_int, [vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, C.c_int,
                                            C.c_double, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp,
                                            vp, vp]),
    "kpop_refset_create": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32, C.POINTER(vp)]),
    "kpop_dev_refset_wrap": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_int, vp, C.POINTER(vp)]),
    "kpop_refset_append": (C.c_int, [vp, f64p, C.c_uint32]),
    "kpop_refset_info": (C.c_int, [vp, u32p, u32p, u32p, u64p]),
    "kpop_refset_free": (C.c_int, [vp]),
    "kpop_refset_distance_rowwise": (C.c_int, [vp, f64p, C.c_uint32, f64p]),
    "kpop_refset_distance_summary": (C.c_int, [vp, f64p, C.c_uint32, C.c_uint32, C.c_uint32, f64p, u32p, u32p, f64p, f64p]),
    "kpop_dev_refset_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_refset_distance_rowwise": (C.c_int, [vp, vp, C.c_uint32, vp, vp, vp]),
    "kpop_dev_refset_distance_summary": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_neighbours_within": (C.c_int, [vp, f64p, C.c_uint32, C.c_double, C.c_uint64, u64p, u32p, f64p]),
    "kpop_dev_neighbours_within_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint64]),
    "kpop_dev_neighbours_within": (C.c_int, [vp, vp, C.c_uint32, C.c_double, C.c_uint64, vp, vp, vp, vp, vp]),
    "kpop_distance_within": (C.c_int, [f64p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_uint64,
                                       u64p, u32p, f64p]),
    "kpop_clusters_within": (C.c_int, [vp, C.c_double, C.c_uint32, u32p, u32p]),
    "kpop_dev_clusters_within_workspace_bytes": (C.c_uint64, [vp]),
    "kpop_dev_clusters_within": (C.c_int, [vp, C.c_double, C.c_uint32, vp, vp, vp, vp]),
    "kpop_distance_clusters": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, u32p, u32p]),
    "kpop_spanning_forest": (C.c_int, [vp, C.c_double, u32p, u32p, u32p, f64p, u32p]),
    "kpop_dev_spanning_forest_workspace_bytes": (C.c_uint64, [vp]),
    "kpop_dev_spanning_forest": (C.c_int, [vp, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_spanning_forest": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, u32p, u32p, u32p, f64p,
                                                u32p]),
    "kpop_forest_cut": (C.c_int, [C.c_uint32, C.c_uint32, u32p, u32p, f64p, C.c_double, u32p, u32p]),
    # the k-NN vote (knn.hip)
    "kpop_knn_vote": (C.c_int, [vp, u32p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, u32p, u32p, u32p, f64p]),
    "kpop_dev_knn_vote_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kpop_dev_knn_vote": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_knn_vote": (C.c_int, [f64p, C.c_uint32, u32p, C.c_uint32, f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32,
                                         u32p, u32p, u32p, f64p]),
    # k-NN validation: many k in one pass, leave-out votes (knn_validate.hip)
    "kpop_knn_ks_vote": (C.c_int, [vp, u32p, C.c_uint32, f64p, C.c_uint32, u32p, C.c_uint32, u32p, u32p, u32p, f64p]),
    "kpop_dev_knn_ks_vote_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kpop_dev_knn_ks_vote": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, u32p, C.c_uint32, vp, vp, vp, vp, vp, vp]),
    "kpop_knn_validate": (C.c_int, [vp, u32p, C.c_uint32, u32p, u32p, C.c_uint32, u32p, u32p, u32p, f64p, u64p]),
    "kpop_dev_knn_validate_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32, C.c_uint32]),
    "kpop_dev_knn_validate": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, u32p, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_knn_validate": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, u32p, C.c_uint32, u32p, u32p, C.c_uint32,
                                             u32p, u32p, u32p, f64p, u64p]),
    # representatives at a distance: the greedy cover in row order (representatives.hip)
    "kpop_representatives_within": (C.c_int, [vp, C.c_double, C.c_uint32, u32p, f64p, u32p]),
    "kpop_dev_representatives_within_workspace_bytes": (C.c_uint64, [vp]),
    "kpop_dev_representatives_within": (C.c_int, [vp, C.c_double, C.c_uint32, vp, vp, vp, vp, vp]),
    "kpop_distance_representatives": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, u32p, f64p, u32p]),
    # DBSCAN on a resident set: core rows, border rows and noise (dbscan.hip)
    "kpop_dbscan": (C.c_int, [vp, C.c_double, C.c_uint32, u32p, u32p, u32p, u32p]),
    "kpop_dev_dbscan_workspace_bytes": (C.c_uint64, [vp]),
    "kpop_dev_dbscan": (C.c_int, [vp, C.c_double, C.c_uint32, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_dbscan": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_uint32, u32p, u32p, u32p, u32p]),
    # the mutual-reachability tree: core distances, the forest under max(d, core_i, core_j), its cut (reachability.hip)
    "kpop_core_distances": (C.c_int, [vp, C.c_uint32, f64p]),
    "kpop_dev_core_distances_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_core_distances": (C.c_int, [vp, C.c_uint32, vp, vp, vp]),
    "kpop_reachability_tree": (C.c_int, [vp, C.c_uint32, C.c_double, u32p, u32p, u32p, f64p, f64p, u32p]),
    "kpop_dev_reachability_tree_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_reachability_tree": (C.c_int, [vp, C.c_uint32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_reachability_tree": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32, C.c_double, u32p, u32p, u32p,
                                                  f64p, f64p, u32p]),
    "kpop_reachability_cut": (C.c_int, [C.c_uint32, C.c_uint32, u32p, u32p, f64p, f64p, C.c_double, u32p, u32p]),
    # the silhouette and the medoids of a labelled set (silhouette.hip)
    "kpop_silhouette": (C.c_int, [vp, u32p, C.c_uint32, f64p, f64p, u32p, f64p, u32p, u32p, f64p]),
    "kpop_dev_silhouette_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_silhouette": (C.c_int, [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_silhouette": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, u32p, C.c_uint32, f64p, f64p, u32p, f64p, u32p,
                                           u32p, f64p]),
    "kpop_silhouette_summary": (C.c_int, [C.c_uint32, u32p, C.c_uint32, f64p, f64p, f64p]),
    # the distances between every two classes of a labelled set, and the classes' tree (class_linkage.hip)
    "kpop_class_linkage": (C.c_int, [vp, u32p, C.c_uint32, u32p, f64p, f64p, f64p, u32p, u32p]),
    "kpop_dev_class_linkage_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_class_linkage": (C.c_int, [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_class_linkage": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, u32p, C.c_uint32, u32p, f64p, f64p, f64p, u32p,
                                              u32p]),
    "kpop_class_tree": (C.c_int, [C.c_uint32, u32p, f64p, C.c_int, u32p, u32p, u32p, f64p, u32p]),
    # the farthest-first traversal: k diverse rows for every k (farthest_first.hip)
    "kpop_farthest_first": (C.c_int, [vp, C.c_uint32, C.c_double, u32p, C.c_uint32, u32p, u32p, f64p, u32p, u32p, f64p, u32p]),
    "kpop_dev_farthest_first_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_farthest_first": (C.c_int, [vp, C.c_uint32, C.c_double, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_farthest_first": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32, C.c_double, u32p, C.c_uint32, u32p,
                                               u32p, f64p, u32p, u32p, f64p, u32p]),
    # k-medoids: clusters when a count is known (kmedoids.hip)
    "kpop_kmedoids": (C.c_int, [vp, C.c_uint32, u32p, C.c_uint32, u32p, u32p, f64p, f64p, u32p, f64p, u32p, C.POINTER(C.c_int)]),
    "kpop_dev_kmedoids_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
    "kpop_dev_kmedoids": (C.c_int, [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_kmedoids": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32, u32p, C.c_uint32, u32p, u32p, f64p, f64p,
                                         u32p, f64p, u32p, C.POINTER(C.c_int)]),
    # the local outlier factor of a set, and of query rows against it (lof.hip)
    "kpop_lof": (C.c_int, [vp, C.c_uint32, f64p, u32p, f64p, f64p]),
    "kpop_dev_lof_workspace_bytes": (C.c_uint64, [vp, C.c_uint32]),
    "kpop_dev_lof": (C.c_int, [vp, C.c_uint32, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_lof": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_uint32, f64p, u32p, f64p, f64p]),
    "kpop_lof_score": (C.c_int, [vp, C.c_uint32, f64p, f64p, f64p, C.c_uint32, f64p, u32p, f64p, f64p]),
    "kpop_dev_lof_score_workspace_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
    "kpop_dev_lof_score": (C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]),
    # density peaks: every row's nearest denser row, their forest and its cut (density_peaks.hip)
    "kpop_density_peaks": (C.c_int, [vp, C.c_double, f64p, C.c_double, C.c_double, f64p, f64p, u32p, u32p, u32p]),
    "kpop_dev_density_peaks_workspace_bytes": (C.c_uint64, [vp]),
    "kpop_dev_density_peaks": (C.c_int, [vp, C.c_double, vp, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
    "kpop_distance_density_peaks": (C.c_int, [f64p, C.c_uint32, C.c_uint32, f64p, C.c_int, C.c_double, C.c_int, C.c_double, f64p, C.c_double, C.c_double, f64p, f64p,
                                              u32p, u32p, u32p]),
    "kpop_density_peaks_cut": (C.c_int, [C.c_uint32, f64p, f64p, u32p, C.c_double, C.c_double, u32p, u32p]),
}


class KPopError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libkpop_hip: %s (status %d)" % (msg, code))
        self.code = code


_lib = None


def load():
    """dlopen libkpop_hip.so and declare every symbol of include/kpop_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C kpop_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own HIP/HSA runtime.  Two runtimes in one process do not both see the
    # GPU, and whichever is loaded first wins, so when torch is installed let its copy be the process's runtime
    # (libkpop_hip.so only needs libamdhip64.so.7 by SONAME).  Stand-alone users (the C++ CLIs) get /opt/rocm's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if "KPOP_HIP_LIB" in os.environ and not hasattr(lib, name):
            continue  # an older build under A/B comparison
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise KPopError(rc, load().kpop_last_error().decode("utf-8", "replace"))
