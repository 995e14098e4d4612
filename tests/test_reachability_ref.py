"""CPU tests of the mutual-reachability forest (kpop_reachability_tree, include/kpop_hip.h): the numpy reference
(tests/reachability_ref.py) on the worked case of the declared semantics, number for number; its relations to what exists -- with
min_pts = 1 it is forest_ref, its cut is dbscan_ref on the core rows with every other row alone (DBSCAN*), a capped forest is a prefix
of the uncapped one -- on rows full of ties, with and without a NaN row; the boundary (the header declares the eight functions with
their citations, the library exports them, the Python table binds them, the package offers them, the kernels are built from their own
file and the rounds stay forest.hip's); and kpop_reachability_cut -- host arithmetic alone -- through the library, without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import NOISE, dbscan_ref
from forest_ref import cut_ref, forest_ref
from reachability_ref import core_ref, reach_matrix, reachability_cut_ref, reachability_forest_ref
from test_gpu_forest import clustered_rows

FUNCTIONS = ["kpop_core_distances", "kpop_dev_core_distances_workspace_bytes", "kpop_dev_core_distances", "kpop_reachability_tree",
             "kpop_dev_reachability_tree_workspace_bytes", "kpop_dev_reachability_tree", "kpop_distance_reachability_tree", "kpop_reachability_cut"]
ERR_INVALID = -1
INF = float("inf")
MIN_PTS = [1, 2, 4, 5, 12, 130, 131]

# the ten rows of INTEGRATION.md 6i (tests/test_dbscan_ref.py): the only coordinate that is not zero; every value dyadic
HAND_X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
WORKED = {
    4: ([.375, .25, .25, .375, .25, .25, .375, .5, 3.75, .375],
        [(1, 2, .25), (4, 5, .25), (0, 1, .375), (0, 9, .375), (3, 4, .375), (3, 6, .375), (2, 7, .5), (3, 7, .5), (4, 8, 3.75)]),
    3: ([.25, .125, .125, .25, .125, .125, .25, .375, 3.625, .25],
        [(1, 2, .125), (4, 5, .125), (0, 1, .25), (1, 9, .25), (3, 4, .25), (4, 6, .25), (3, 7, .375), (7, 9, .375), (5, 8, 3.625)]),
}


def euclidean(m):
    """the chain restated for a metric of ones: the root of the sum, over the dimensions ascending, of the squared differences"""
    acc = np.zeros((m.shape[0], m.shape[0]))
    for c in range(m.shape[1]):
        diff = m[:, None, c] - m[None, :, c]
        acc = acc + diff * diff
    return np.sqrt(acc)


def hand_matrix():
    return np.abs(np.subtract.outer(np.array(HAND_X), np.array(HAND_X)))


def edges(forest):
    return list(zip(forest[0].tolist(), forest[1].tolist(), forest[2].tolist()))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("min_pts", [4, 3])
def test_the_worked_case(min_pts):
    D = hand_matrix()
    core, forest = WORKED[min_pts]
    assert core_ref(D, min_pts).tolist() == core
    ei, ej, ed, got_core, labels = reachability_forest_ref(D, min_pts)
    assert got_core.tolist() == core and edges((ei, ej, ed)) == forest and not labels.any()
    assert ei.dtype == ej.dtype == labels.dtype == np.uint32 and ed.dtype == got_core.dtype == np.float64
    assert len(np.unique(ed)) < len(ed)  # ties, which the strict order (mr, i, j) settles
    if min_pts == 4:
        # the cut at .375: rows 0, 1, 2, 9 and rows 3 .. 6; rows 7 (6i's border row) and 8 are not core here: DBSCAN*
        labels, counts = reachability_cut_ref(10, ei, ej, ed, got_core, .375)
        assert labels.tolist() == [0, 0, 0, 3, 3, 3, 3, NOISE, NOISE, 0] and counts.tolist() == [2, 8, 2]
        assert cut_ref(10, ei, ej, ed, .375)[0].tolist() == [0, 0, 0, 3, 3, 3, 3, 7, 8, 0]
        want = dbscan_ref(D, .375, 4)
        assert want[0].tolist() == [0, 0, 0, 3, 3, 3, 3, 3, NOISE, 0] and want[3].tolist()[:2] == counts.tolist()[:2]
        # the cut at .25: the pairs {1, 2} and {4, 5} only
        labels, counts = reachability_cut_ref(10, ei, ej, ed, got_core, .25)
        assert labels.tolist() == [NOISE, 1, 1, NOISE, 4, 4, NOISE, NOISE, NOISE, NOISE] and counts.tolist() == [2, 4, 6]


def test_core_ref_edge_values():
    D = hand_matrix()
    assert same_bits(core_ref(D, 1), np.zeros(10))
    assert core_ref(D, 10).tolist() == [5.0, 4.875, 4.75, 3.875, 3.75, 3.625, 3.5, 4.25, 5.0, 4.625]  # the farthest other row
    assert np.isnan(core_ref(D, 11)).all()  # min_pts > r1
    with pytest.raises(ValueError):
        core_ref(D, 0)
    # a row of NaNs: its own core distance is NaN for min_pts >= 2, +0 for 1, and the others' lists simply lack it; +inf is a number
    bad = np.array(D)
    bad[4, :] = bad[:, 4] = np.nan
    bad[8, 0] = bad[0, 8] = INF
    assert same_bits(core_ref(bad, 1), np.zeros(10))
    core = core_ref(bad, 9)  # eight others is all a row has left
    assert np.isnan(core[4]) and core[0] == INF and core[8] == INF and np.isfinite(np.delete(core, [0, 4, 8])).all()
    assert np.isnan(core_ref(bad, 10)).all()
    # a zero is written as +0, whatever its sign in the matrix
    Z = np.array([[0.0, 0.0], [-0.0, 0.0]])
    assert same_bits(core_ref(Z, 2), np.zeros(2))
    # only the lower triangle is read
    spoiled = np.tril(D, -1) + np.triu(np.full(D.shape, np.nan))
    assert same_bits(core_ref(spoiled, 4), core_ref(D, 4))
    assert all(np.array_equal(a, b) for a, b in zip(reachability_forest_ref(spoiled, 4), reachability_forest_ref(D, 4)))
    # an empty set
    assert [len(a) for a in reachability_forest_ref(np.zeros((0, 0)), 3)] == [0] * 5


_rows = {}


def matrices():
    """clustered_rows(130, 9) with and without a NaN row: made once, never changed"""
    if not _rows:
        m = clustered_rows(130, 9)
        bad = np.array(m)
        bad[20, 4] = np.nan
        for name, rows in (("plain", m), ("a NaN row", bad)):
            D = euclidean(rows)
            D.setflags(write=False)
            _rows[name] = D
    return _rows


@pytest.mark.parametrize("min_pts", MIN_PTS)
@pytest.mark.parametrize("name", ["plain", "a NaN row"])
def test_relations_to_what_exists(name, min_pts):
    D = matrices()[name]
    n = D.shape[0]
    low = D[np.tril_indices(n, -1)]
    ei, ej, ed, core, labels = reachability_forest_ref(D, min_pts)
    # the defining relation with 6i: core <= eps iff degree >= min_pts -- for eps >= 0, and for min_pts >= 2 below zero too (at
    # min_pts = 1 a row is its own neighbour at distance +0, which no negative eps reaches although its degree is 1)
    thresholds = [float(np.nanquantile(low, q)) for q in (0.01, 0.05, 0.2, 0.6)]
    for T in thresholds + [INF, 0.0] + ([-1.0] if min_pts > 1 else []):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(core <= T, dbscan_ref(D, T, min_pts)[2] >= min_pts), (name, min_pts, T)
    # 1. min_pts = 1: the single-linkage tree
    if min_pts == 1:
        assert same_bits(core, np.zeros(n))
        assert all(np.array_equal(a, b) for a, b in zip((ei, ej, ed, labels), forest_ref(D, INF)))
    if min_pts > n:
        assert np.isnan(core).all() and len(ei) == 0 and np.array_equal(labels, np.arange(n))
        return
    if min_pts > 1 and name == "a NaN row":
        assert np.isnan(core[20]) and not np.any(ei == 20) and not np.any(ej == 20) and labels[20] == 20
    assert np.all(ed >= np.maximum(core[ei], core[ej]))
    if 2 <= min_pts <= 12:  # full of ties: the chain's equal steps give its inner rows one core distance
        assert len(np.unique(ed)) < len(ed) - 10
    for T in thresholds:
        # 2. the cut is DBSCAN*: dbscan's labels on the core rows, every other row alone
        got = cut_ref(n, ei, ej, ed, T)[0]
        want, _, degree, counts = dbscan_ref(D, T, min_pts)
        is_core = degree >= min_pts
        assert np.array_equal(got[is_core], want[is_core]), (name, min_pts, T)
        assert np.array_equal(got[~is_core], np.arange(n)[~is_core]), (name, min_pts, T)
        assert np.all(np.bincount(got, minlength=n)[got[~is_core]] == 1), (name, min_pts, T)
        rl, rc = reachability_cut_ref(n, ei, ej, ed, core, T)
        assert np.array_equal(rl[is_core], want[is_core]) and np.all(rl[~is_core] == NOISE) and rc.tolist()[:2] == counts.tolist()[:2]
        assert rc[2] == n - rc[1]
        # 3. a forest capped at T is the prefix of the uncapped one up to the last edge within T
        ci, cj, cd, ccore, clabels = reachability_forest_ref(D, min_pts, T)
        keep = ed <= T
        assert np.array_equal(ci, ei[keep]) and np.array_equal(cj, ej[keep]) and np.array_equal(cd, ed[keep]), (name, min_pts, T)
        assert same_bits(ccore, core) and np.array_equal(clabels, got)
    assert len(reachability_forest_ref(D, min_pts, -1.0)[0]) == 0
    with pytest.raises(ValueError):
        reachability_forest_ref(D, min_pts, float("nan"))


def test_reach_matrix_hands_a_nan_on():
    D = hand_matrix()
    core = core_ref(D, 4)
    core[2] = np.nan
    M = reach_matrix(D, core)
    assert np.isnan(M[2]).all() and np.isnan(M[:, 2]).all() and np.isnan(np.diag(M)).all()
    rest = np.delete(np.delete(M, 2, 0), 2, 1)
    assert np.isfinite(rest[~np.eye(9, dtype=bool)]).all() and np.array_equal(M[1, 0], 0.375)


def test_header_declares_and_library_exports_the_eight_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*(?:reachability|core_distances)[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_dbscan(") < code.index("kpop_core_distances(")  # the block after DBSCAN's
    for name in FUNCTIONS:  # no name that the forest's, the DBSCAN's or the sets' name tests would count
        assert "forest" not in name and "dbscan" not in name and "clusters" not in name and not re.match(r"kpop_(dev_)?refset_", name)
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
    for name in ("dev_core_distances_workspace_bytes", "dev_core_distances", "dev_reachability_forest_workspace_bytes", "dev_reachability_forest",
                 "distance_reachability_forest", "reachability_cut"):
        assert callable(getattr(kpop_amd, name)) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.core_distances) and callable(kpop_amd.RefSet.reachability_forest)


def test_the_kernels_are_built_from_their_own_file():
    csrc = os.path.join(ROOT, "kpop_amd", "csrc")
    assert "reachability.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "reachability.hip")).read()
    for kernel in ("reach_core_kernel", "reach_fill_kernel"):
        assert "void " + kernel in src
    assert "asm" not in re.sub(r"//.*", "", src)  # plain HIP C++ throughout
    # the rounds and the lists are reused, not copied: one body each, where they were, reached through the two headers
    forest = open(os.path.join(csrc, "forest.hip")).read()
    knn = open(os.path.join(csrc, "knn.hip")).read()
    for kernel in ("forest_nearest_kernel", "forest_row_min_kernel", "forest_comp_edge_kernel", "forest_link_kernel", "forest_flatten_kernel",
                   "forest_tile_labels_kernel", "forest_write_kernel"):
        assert forest.count("void " + kernel + "(") == 1 and kernel not in re.sub(r"//.*", "", src)
    for kernel in ("knn_nearest_kernel", "knn_merge_kernel"):
        assert knn.count("void " + kernel + "(") == 1 and kernel not in re.sub(r"//.*", "", src)
    assert "ForestDistanceWeight" in forest and "ForestReachWeight" in forest
    assert "forest_dev(" in src and '#include "forest_rounds.h"' in src and '#include "forest_rounds.h"' in forest
    assert "knn_run_leave_self_out_lists(" in src and "knn_run_leave_self_out_lists(" in knn
    assert "knn_ties_kernel" not in src  # the tie pass settles who is a member, never the k-th key: not run here


def raw_cut(r1, ei, ej, ed, core, T, null=()):
    from kpop_amd import _lib
    ei, ej = np.ascontiguousarray(ei, dtype=np.uint32), np.ascontiguousarray(ej, dtype=np.uint32)
    ed, core = np.ascontiguousarray(ed, dtype=np.float64), np.ascontiguousarray(core, dtype=np.float64)
    labels = np.full(max(r1, 1), 12345, dtype=np.uint32)
    counts = np.full(3, 12345, dtype=np.uint32)
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    pointer = lambda a, ty, name: a.ctypes.data_as(ty) if len(a) and name not in null else None
    rc = _lib.load().kpop_reachability_cut(r1, len(ei), pointer(ei, u32p, "ei"), pointer(ej, u32p, "ej"), pointer(ed, f64p, "ed"), pointer(core, f64p, "core"), T,
                                           pointer(labels, u32p, "labels"), pointer(counts, u32p, "counts"))
    return rc, labels[:r1], counts


def check_cut(r1, ei, ej, ed, core, T):
    import kpop_amd
    want = reachability_cut_ref(r1, ei, ej, ed, core, T)
    rc, labels, counts = raw_cut(r1, ei, ej, ed, core, T)
    assert rc == 0
    assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[1]), (r1, T)
    got = kpop_amd.reachability_cut(r1, ei, ej, ed, core, T)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (r1, T)


def test_reachability_cut_runs_without_a_gpu():
    rng = np.random.RandomState(11)
    # reachability forests, cut at every weight, between the weights and at both infinities
    for name, D in matrices().items():
        for min_pts in (1, 4, 12, 131):
            ei, ej, ed, core, _ = reachability_forest_ref(D, min_pts)
            values = np.unique(ed)
            for T in list(values[::7]) + list((values[1:] + values[:-1])[::11] / 2) + [INF, -INF, 0.0, -1.0]:
                check_cut(D.shape[0], ei, ej, ed, core, float(T))
    ei, ej, ed, core, _ = reachability_forest_ref(hand_matrix(), 4)
    for T in (.25, .375, .5, 3.75, INF):
        check_cut(10, ei, ej, ed, core, T)
    # edge lists that are no forests, core distances that belong to nothing: cycles, repeated edges, NaNs, any order
    for n, n_edges in ((6, 15), (50, 200), (50, 20)):
        ei = rng.randint(0, n - 1, size=n_edges)
        ej = ei + 1 + (rng.randint(0, n, size=n_edges) % (n - 1 - ei))
        ed = rng.randint(0, 5, size=n_edges).astype(np.float64)
        ed[::7] = np.nan
        core = rng.randint(0, 5, size=n).astype(np.float64)
        core[::5] = np.nan
        core[1] = INF
        for T in (-INF, 0.0, 1.0, 2.5, 4.0, INF):
            check_cut(n, ei, ej, ed, core, T)
    # no edges; no rows
    check_cut(5, [], [], [], [0.0, 1.0, np.nan, 2.0, 0.5], 1.0)
    check_cut(0, [], [], [], [], 1.0)
    rc, _, counts = raw_cut(0, [], [], [], [], 1.0, null=("labels",))
    assert rc == 0 and counts.tolist() == [0, 0, 0]


def test_reachability_cut_refuses():
    import kpop_amd
    core = [0.0, 0.0, 0.0, 0.0]
    assert raw_cut(4, [0], [1], [1.0], core, float("nan"))[0] == ERR_INVALID
    assert raw_cut(4, [0, 2], [1, 2], [1.0, 1.0], core, 2.0)[0] == ERR_INVALID  # i == j
    assert raw_cut(4, [0, 3], [1, 2], [1.0, 1.0], core, 2.0)[0] == ERR_INVALID  # i > j
    assert raw_cut(4, [0, 2], [1, 4], [1.0, 1.0], core, 2.0)[0] == ERR_INVALID  # j == r1
    assert raw_cut(4, [0, 2], [1, 4], [1.0, 9.0], core, 2.0)[0] == ERR_INVALID  # ... even beyond the cut
    assert raw_cut(0, [0], [1], [1.0], [], 2.0)[0] == ERR_INVALID
    for name in ("core", "labels", "counts", "ei", "ej", "ed"):
        assert raw_cut(4, [0], [1], [1.0], core, 2.0, null=(name,))[0] == ERR_INVALID, name
    assert raw_cut(4, [0], [1], [1.0], core, 2.0)[0] == 0
    with pytest.raises(kpop_amd.KPopError) as e:
        kpop_amd.reachability_cut(4, [0], [1], [1.0], core, float("nan"))
    assert e.value.code == ERR_INVALID
    with pytest.raises(kpop_amd.KPopError) as e:
        kpop_amd.reachability_cut(4, [1], [1], [1.0], core, 1.0)
    assert e.value.code == ERR_INVALID
    with pytest.raises(ValueError):
        kpop_amd.reachability_cut(4, [0], [1], [1.0], core[:3], 1.0)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    rs.info = lambda: {"r1": 2, "n_dims": 3}
    with pytest.raises(kpop_amd.KPopError):
        rs.core_distances(2)
    with pytest.raises(kpop_amd.KPopError):
        rs.reachability_forest(2)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_reachability_forest(np.ones((2, 3)), np.ones(3), min_pts=2)
