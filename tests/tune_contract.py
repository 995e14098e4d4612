"""The contract of kpop_tune (include/kpop_hip.h), as data: one row for every key the library accepts.

A helper module, no tests in it: tests/test_tune_contract.py holds the table to the sources (the chain of kpop_tune in
kpop_amd/csrc/runtime.hip, the initialisers of Context in kpop_amd/csrc/common.h, the header's comment) without a GPU, and
tests/test_gpu_tune_contract.py holds the kernels to the table.

A row:
  default     the initialiser of Context::tune_<key>, kpop_amd/csrc/common.h (the line in the comment beside it)
  values      every accepted value of a small domain; both ends and one inside for a range
  rejected    one or two values just outside
  effect      what a setting may do to results, read from the code it selects (the lines in the comment):
                "bits"    every setting gives the default's bits
                "order"   another order of additions: equal to the reference within the project's tolerance (1e-12 of the
                          result's scale), not bit for bit
                "approx"  the documented matrix-core approximations and what selects between them: within the bound the header
                          states (distances <= 1e-12 relative; a summary's medians, MADs and neighbour lists bit for bit, its mean
                          and standard deviation sums of approximate values)
                "none"    instrumentation that never touches results
  covered_by  the test file that sets every value of `values`
"""
import contextlib

NEW = "test_gpu_tune_contract.py"


def _row(default, values, rejected, effect, covered_by):
    return {"default": default, "values": tuple(values), "rejected": tuple(rejected), "effect": effect, "covered_by": covered_by}


KNOBS = {
    # count_twist.hip wave_gather_rows* (:157-290): a dimension's sum is one ascending chain of __dadd_rn(__dmul_rn()) whatever U
    # (the lane groups of the packed forms take rows g, g + G, ... for U = 8 and 16 alike); the rows past the last are +0.0 * 0.0
    "unroll": _row(8, (8, 16), (4, 32), "bits", NEW),                                   # common.h:105
    # the same chains, the loads' kind alone: count_twist.hip:173, 206, 236, 270 (reads), :778 (streaming), :1516 (residual rows)
    "nt": _row(2, (0, 1, 2), (3, -1), "bits", NEW),                                     # common.h:106
    # count_twist.hip:744-800: a segment's four wavefronts take every fourth run of 64 windows and their sums are added, then
    # the segments' in order (:1586-1597) -- where a segment ends decides which windows meet in which partial sum
    "seg": _row(0, (0, 64, 1024, 16384), (63, 100, 16448), "order", NEW),               # common.h:107
    # count_twist.hip:1693-1696, 1708, 1763: the launch's dynamic LDS, which no kernel reads
    "ldspad": _row(0, (0, 16384), (65537, -1), "bits", NEW),                            # common.h:108
    # development switches (common.h:109-119; "results may be WRONG when the low ones are set"): listed, not held to anything
    "dbg": _row(0, (0,), (), "none", "test_gpu_distance.py"),                           # common.h:120
    # count_twist.hip:1862 (tile route), :2185 (dense image), :2304 (kpop_twist's contraction): sums on the matrix cores
    "dense": _row(2, (0, 1, 2), (3, -1), "order", NEW),                                 # common.h:121
    # count_twist.hip:1046-1050, 1149-1210: a chunk of 32 sequences has other seeds, hence another consensus set, other rows on
    # the matrix cores and others on the residual lists
    "tileg": _row(64, (32, 64), (48, 16), "order", NEW),                                # common.h:122
    # count_twist.hip:1741, 1947-1973: tile_pipe.h's kernel or count_twist_tile_kernel, each with its own order of the set's rows
    "tilepipe": _row(1, (0, 1), (2, -1), "order", NEW),                                 # common.h:123
    # count_twist.hip:1744: the three-stage form multiplies and gathers in the exchanging kernel's order (up to 64 dimensions)
    "tilewide": _row(0, (0, 1), (2, -1), "bits", "test_gpu_twist.py"),                  # common.h:124
    # count_twist.hip:1831-1845: sub-batches of sequences are other groups of 64, hence other consensus sets
    "tilecap_mb": _row(0, (0, 40), (-1,), "order", "test_gpu_twist.py"),                # common.h:125
    # count_twist.hip:1957, tile_pipe.h:821-827: s_setprio of the MFMA wavefronts from the low two bits; bit 2 travels to the
    # kernel (bit 7 of its switches) and nothing there reads it
    "pipeprio": _row(1, range(8), (8, -1), "bits", NEW),                                # common.h:126
    # integer spectra: sort_count.hip, every path counts the same windows
    "blocksort": _row(1, (0, 1), (2, -1), "bits", "test_gpu_count.py"),                 # common.h:127
    "hist": _row(1, (0, 1), (2, -1), "bits", "test_gpu_count.py"),                      # common.h:128
    "histguess": _row(1, (0, 1), (2, -1), "bits", "test_gpu_count.py"),                 # common.h:129
    # count_twist.hip:250-290: with rows missing the hashes without a row stay in the list (adding +0.0), so the rows are dealt
    # to the lane groups differently: another grouping of the same additions (a complete twister: the same bits)
    "direct": _row(2, (0, 1, 2), (3, -1), "order", "test_gpu_twist.py"),                # common.h:130
    # class_set.hip: the tiled kernel's chain a pair
    "class_set": _row(1, (0, 1, 2), (3, -1), "bits", "test_gpu_class_set_distance.py"),  # common.h:131
    # distance_mfma.hip: the refinement finds the same candidates in the lists or in the rows
    "summary_mfma_lists": _row(1, (0, 1), (2, -1), "bits", "test_gpu_distance.py"),     # common.h:132
    "distance_mfma": _row(1, (0, 1), (2, -1), "approx", "test_gpu_distance.py"),        # common.h:133
    "summary_mfma": _row(1, (0, 1, 2), (3, -1), "approx", "test_gpu_distance.py"),      # common.h:134
    # summary_large.hip: batches of query rows, each row's results its own
    "summary_lanes": _row(1, (1, 2), (0, 3), "bits", "test_gpu_distance.py"),           # common.h:135
    # which rows go to the exact fall-back (their mean and standard deviation are then exact sums, not approximate ones)
    "summary_sample": _row(1, (0, 1), (2, -1), "approx", "test_gpu_distance.py"),       # common.h:136
    "summary_rawref": _row(1, (0, 1), (2, -1), "approx", "test_gpu_distance.py"),       # common.h:137
    "summary_pass": _row(1, (0, 1), (2, -1), "approx", "test_gpu_distance.py"),         # common.h:138
    "summary_audit": _row(0, (0, 1), (2, -1), "none", "test_gpu_distance.py"),          # common.h:139
    # medians, MADs and neighbour lists are order statistics (exact in every mode); mean and standard deviation are summed per mode
    "summary2": _row(1, (0, 1, 2, 3), (4, -1), "approx", "test_gpu_distance.py"),       # common.h:141
    # distill.hip: a k-mer's statistics are its own, whichever band it is in
    "distill_band": _row(0, (0, 128, 1700), (-1,), "bits", "test_gpu_distill.py"),      # common.h:142
    "distill_clock": _row(0, (0, 1), (2, -1), "none", NEW),                             # common.h:143
    "histlds": _row(1, (0, 1, 2, 3, 4), (5, -1), "bits", "test_gpu_count.py"),          # common.h:148
}


@contextlib.contextmanager
def tuned(**knobs):
    """with tuned(unroll=16, nt=1): the knobs at these values, every one of them back at its default afterwards -- also when the
    block fails, or when one of the settings is refused (the knobs are process-wide: runtime.hip, "a knob holds for every device slot")"""
    from kpop_amd import api
    try:
        for key, value in knobs.items():
            api.tune(key, value)
        yield
    finally:
        for key in knobs:
            api.tune(key, KNOBS[key]["default"])
