"""CPU tests of the boundary of the single-linkage tree: include/kpop_hip.h declares the five functions, after the clusters, with the
lines of the reference they stand on; the library exports them, the Python table binds them, the package offers them; and
kpop_forest_cut -- host arithmetic alone -- runs here, without a GPU and without kpop_init, against tests/forest_ref.py's cut_ref."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from forest_ref import cut_ref, forest_ref

FUNCTIONS = ["kpop_spanning_forest", "kpop_dev_spanning_forest_workspace_bytes", "kpop_dev_spanning_forest", "kpop_distance_spanning_forest",
             "kpop_forest_cut"]
ERR_INVALID = -1
INF = float("inf")


def test_header_declares_and_library_exports_the_five_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*forest[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    for name in FUNCTIONS:  # a block of their own after the clusters; and no name that the clusters' or the sets' name tests would count
        assert code.index("kpop_distance_clusters(") < code.index(name + "(")
        assert "clusters" not in name and not re.match(r"kpop_(dev_)?refset_", name)
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
    for name in ("distance_spanning_forest", "dev_spanning_forest_workspace_bytes", "dev_spanning_forest", "forest_cut"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.spanning_forest)


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "forest.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "forest.hip")).read()
    for kernel in ("forest_nearest_kernel", "forest_row_min_kernel", "forest_comp_edge_kernel", "forest_link_kernel", "forest_flatten_kernel"):
        assert "void " + kernel in src


def raw_cut(r1, ei, ej, ed, T, null_labels=False):
    from kpop_amd import _lib
    ei, ej = np.ascontiguousarray(ei, dtype=np.uint32), np.ascontiguousarray(ej, dtype=np.uint32)
    ed = np.ascontiguousarray(ed, dtype=np.float64)
    labels = np.full(max(r1, 1), 12345, dtype=np.uint32)
    n = C.c_uint32(12345)
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    pointer = lambda a, ty: a.ctypes.data_as(ty) if len(a) else None
    rc = _lib.load().kpop_forest_cut(r1, len(ei), pointer(ei, u32p), pointer(ej, u32p), pointer(ed, f64p), T,
                                     None if null_labels else labels.ctypes.data_as(u32p), C.byref(n))
    return rc, labels[:r1], n.value


def check_cut(r1, ei, ej, ed, T):
    import kpop_amd
    want = cut_ref(r1, ei, ej, ed, T)
    rc, labels, n = raw_cut(r1, ei, ej, ed, T)
    assert rc == 0
    assert np.array_equal(labels, want[0]) and n == want[1], (r1, T)
    got = kpop_amd.forest_cut(r1, ei, ej, ed, T)
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]) and got[1] == want[1], (r1, T)


def test_forest_cut_runs_without_a_gpu():
    rng = np.random.RandomState(5)
    # forests, cut at every value, between the values and at both infinities
    for n in (1, 2, 9, 120):
        D = np.tril(rng.randint(1, 7, size=(n, n)).astype(np.float64) / 4.0, -1)
        if n > 5:
            D[n // 2, :] = np.nan
            D[:, n // 2] = np.nan
            D[n - 1, :n - 1] = INF
        for cap in (INF, 1.0):
            ei, ej, ed, _ = forest_ref(D, cap)
            values = np.unique(ed[np.isfinite(ed)])
            for T in list(values) + list((values[1:] + values[:-1]) / 2) + [INF, -INF, 0.0, -1.0]:
                check_cut(n, ei, ej, ed, float(T))
    # edge lists that are no forests: cycles, repeated edges, NaN distances, any order
    for n, n_edges in ((6, 15), (50, 200), (50, 20)):
        ei = rng.randint(0, n - 1, size=n_edges)
        ej = ei + 1 + (rng.randint(0, n, size=n_edges) % (n - 1 - ei))
        ed = rng.randint(0, 5, size=n_edges).astype(np.float64)
        ed[::7] = np.nan
        for T in (-INF, 0.0, 1.0, 2.5, 4.0, INF):
            check_cut(n, ei, ej, ed, T)
    # no edges; no rows
    check_cut(5, [], [], [], 1.0)
    check_cut(0, [], [], [], 1.0)
    rc, _, n = raw_cut(0, [], [], [], 1.0, null_labels=True)
    assert rc == 0 and n == 0


def test_forest_cut_refuses():
    import kpop_amd
    assert raw_cut(4, [0], [1], [1.0], float("nan"))[0] == ERR_INVALID
    assert raw_cut(4, [0, 2], [1, 2], [1.0, 1.0], 2.0)[0] == ERR_INVALID  # i == j
    assert raw_cut(4, [0, 3], [1, 2], [1.0, 1.0], 2.0)[0] == ERR_INVALID  # i > j
    assert raw_cut(4, [0, 2], [1, 4], [1.0, 1.0], 2.0)[0] == ERR_INVALID  # j == r1
    assert raw_cut(4, [0, 2], [1, 4], [1.0, 9.0], 2.0)[0] == ERR_INVALID  # ... even beyond the cut
    assert raw_cut(0, [0], [1], [1.0], 2.0)[0] == ERR_INVALID
    with pytest.raises(kpop_amd.KPopError) as e:
        kpop_amd.forest_cut(4, [0], [1], [1.0], float("nan"))
    assert e.value.code == ERR_INVALID
    with pytest.raises(kpop_amd.KPopError) as e:
        kpop_amd.forest_cut(4, [1], [1], [1.0], 1.0)
    assert e.value.code == ERR_INVALID
