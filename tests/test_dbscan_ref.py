"""CPU tests of DBSCAN on a resident set (kpop_dbscan, include/kpop_hip.h): the numpy reference
(tests/dbscan_ref.py) on the hand-made case of the declared semantics and on its edge values, and the boundary -- the header declares
the four functions with the lines of the reference they stand on, the library exports them, the Python table binds them, the package
offers them, and the kernels are built from their own file."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import NOISE, check_invariants, dbscan_ref

FUNCTIONS = ["kpop_dbscan", "kpop_dev_dbscan_workspace_bytes", "kpop_dev_dbscan", "kpop_distance_dbscan"]
KERNELS = ["dbscan_degree_kernel", "dbscan_classify_kernel", "dbscan_union_kernel", "dbscan_border_kernel", "dbscan_finalize_kernel"]

# ten rows of three dimensions, dimension 0 below and the rest zero; euclidean, a metric of ones, not normalised.  Every value is
# dyadic, so every distance is exact: row 7 lies at exactly 0.375 from row 9 (cluster 0) and from row 3 (cluster 3)
HAND_X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
HAND_EPS, HAND_MIN_PTS = 0.375, 4
HAND_OTHER_ORDER = [1.125, 1.25, 1.375, 1.5, 0.75, 0.0, 0.125, 0.25, 0.375, 5.0]


def hand_rows(xs):
    m = np.zeros((len(xs), 3))
    m[:, 0] = xs
    return m


def euclidean(m):
    """the chain restated for a metric of ones: the root of the sum, over the dimensions ascending, of the squared differences"""
    diff = m[:, None, :] - m[None, :, :]
    acc = np.zeros(diff.shape[:2])
    for c in range(m.shape[1]):
        acc = acc + diff[:, :, c] * diff[:, :, c] * 1.0
    return np.sqrt(acc)


def test_the_hand_made_case():
    D = euclidean(hand_rows(HAND_X))
    assert D[7, 3] == 0.375 and D[9, 7] == 0.375 and D[7, 2] == 0.5
    labels, core_of, degree, counts = dbscan_ref(D, HAND_EPS, HAND_MIN_PTS)
    assert degree.tolist() == [4, 4, 4, 5, 4, 4, 4, 3, 1, 5]
    assert labels.tolist() == [0, 0, 0, 3, 3, 3, 3, 3, NOISE, 0]
    assert core_of.tolist() == [0, 1, 2, 3, 4, 5, 6, 3, NOISE, 9]  # row 7: the smaller index wins, although label 0 is smaller
    assert counts.tolist() == [2, 8, 1]
    check_invariants(labels, core_of, degree, counts, HAND_MIN_PTS)
    # the border row joins nothing: with it counted as a core row (min_pts = 3) the two clusters become one
    assert dbscan_ref(D, HAND_EPS, 3)[3].tolist() == [1, 9, 1]


def test_the_hand_made_case_in_another_order():
    labels, core_of, degree, counts = dbscan_ref(euclidean(hand_rows(HAND_OTHER_ORDER)), HAND_EPS, HAND_MIN_PTS)
    assert labels.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, NOISE]
    assert core_of[4] == 0 and degree[4] == 3  # the border row: at 0.375 from row 0 and from row 8, the smaller index
    assert counts.tolist() == [2, 8, 1]
    check_invariants(labels, core_of, degree, counts, HAND_MIN_PTS)


def test_a_border_label_may_exceed_its_index():
    # row 0 is a border row of the cluster of rows 1 .. 4
    D = euclidean(hand_rows([0.0, 0.375, 0.5, 0.625, 0.75]))
    labels, core_of, degree, counts = dbscan_ref(D, 0.375, 4)
    assert degree.tolist() == [2, 5, 4, 4, 4] and labels.tolist() == [1, 1, 1, 1, 1] and core_of.tolist() == [1, 1, 2, 3, 4]
    check_invariants(labels, core_of, degree, counts, 4)


def test_only_the_lower_triangle_is_read():
    D = euclidean(hand_rows(HAND_X))
    want = dbscan_ref(D, HAND_EPS, HAND_MIN_PTS)
    spoiled = np.tril(D, -1) + np.triu(np.full(D.shape, np.nan))
    for got, w in zip(dbscan_ref(spoiled, HAND_EPS, HAND_MIN_PTS), want):
        assert np.array_equal(got, w)


def test_edge_values():
    from clusters_ref import clusters_ref
    D = euclidean(hand_rows(HAND_X))
    n = len(HAND_X)
    with pytest.raises(ValueError):
        dbscan_ref(D, float("nan"), 2)
    with pytest.raises(ValueError):
        dbscan_ref(D, 0.375, 0)
    # eps < 0: every degree is 1
    labels, core_of, degree, counts = dbscan_ref(D, -1.0, 1)
    assert degree.tolist() == [1] * n and labels.tolist() == list(range(n)) and counts.tolist() == [n, n, 0]
    labels, core_of, degree, counts = dbscan_ref(D, -1.0, 2)
    assert labels.tolist() == [NOISE] * n and core_of.tolist() == [NOISE] * n and counts.tolist() == [0, 0, n]
    # min_pts > r1: all noise, whatever eps
    assert dbscan_ref(D, float("inf"), n + 1)[3].tolist() == [0, 0, n]
    assert dbscan_ref(D, float("inf"), n)[3].tolist() == [1, n, 0]
    # min_pts = 1: the clusters at that distance, no noise; min_pts = 2: a singleton is noise, every other component keeps its label
    for eps in (0.125, 0.375, 0.5):
        single = clusters_ref(D, eps)[0]
        one = dbscan_ref(D, eps, 1)
        assert np.array_equal(one[0], single) and one[3][2] == 0 and one[3][1] == n
        two = dbscan_ref(D, eps, 2)
        alone = np.bincount(single, minlength=n)[single] == 1
        assert np.array_equal(two[0], np.where(alone, NOISE, single).astype(np.uint32))
    # a NaN distance is within nothing: a row of NaNs has degree 1; +inf is a number at eps = +inf
    bad = np.array(D)
    bad[4, :] = bad[:, 4] = np.nan
    bad[8, 0] = bad[0, 8] = np.inf
    labels, core_of, degree, counts = dbscan_ref(bad, float("inf"), 2)
    assert degree[4] == 1 and labels[4] == NOISE and degree[8] == n - 1 and counts.tolist() == [1, n - 1, 1]
    # an empty set
    assert dbscan_ref(np.zeros((0, 0)), 1.0, 1)[3].tolist() == [0, 0, 0]


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*dbscan[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_representatives(") < code.index("kpop_dbscan(")  # the block after the representatives
    assert re.search(r"#define\s+KPOP_NOISE\s+0xFFFFFFFFu", code)
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands on, as its neighbours do
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment or "lib/Space.ml:" in comment, name


def test_python_surface():
    import kpop_amd
    for name in ("distance_dbscan", "dev_dbscan_workspace_bytes", "dev_dbscan", "NOISE"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert kpop_amd.NOISE == NOISE == 0xFFFFFFFF
    assert callable(kpop_amd.RefSet.dbscan)


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "dbscan.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "dbscan.hip")).read()
    for kernel in KERNELS:
        assert "void " + kernel in src
