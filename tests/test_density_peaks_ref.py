"""tests/density_peaks_ref.py held to INTEGRATION.md section 6p: the worked case value for value, the closed form of the GPU tests' deep
chain against brute force, the properties that need no GPU, and the boundary -- include/kpop_hip.h declares the five functions with the
lines of the reference they stand on, the library exports them, the Python table binds them, the package offers them; and
kpop_density_peaks_cut, which is host arithmetic alone, against the reference through ctypes on a machine without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from density_peaks_ref import (INF, NOISE, QNAN_BITS, chain_case, components_within, cut_ref, degree_density, density_peaks_ref, parents_ref, ranks_above,
                               same_bits)

# the worked case of INTEGRATION.md 6p: nine rows on a line, euclidean, flat metric, no normalising, eps = 0.5; every distance exact
HAND_X = [0, 0.5, 1, 1.5, 10, 10.5, 11, 30, 0.75]
HAND_EPS = 0.5
HAND_DENSITY = [2, 4, 4, 2, 2, 3, 2, 1, 3]
HAND_DELTA = [0.5, INF, 0.5, 0.5, 0.5, 9.5, 0.5, 19, 0.25]
HAND_PARENT = [1, 1, 1, 2, 5, 2, 5, 6, 1]
HAND_CUTS = (((-INF, 2.0), [1, 1, 1, 1, 5, 5, 5, 7, 1], [3, 1, 0]), ((2.0, 2.0), [1, 1, 1, 1, 5, 5, 5, 5, 1], [2, 1, 0]))

FUNCTIONS = ["kpop_density_peaks", "kpop_dev_density_peaks_workspace_bytes", "kpop_dev_density_peaks", "kpop_distance_density_peaks", "kpop_density_peaks_cut"]
ERR_INVALID, ERR_NOT_INIT = -1, -5


def line(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(np.subtract.outer(x, x))


def random_forest(rng, r, left_out=0):
    """a forest by the definition's own rule -- a parent ranks above its child -- with densities full of ties"""
    density = rng.randint(0, 6, size=r).astype(np.float64)
    out = rng.choice(r, size=left_out, replace=False) if left_out else np.zeros(0, dtype=np.int64)
    density[out] = np.nan
    parent, delta = np.arange(r, dtype=np.uint32), np.full(r, INF)
    for j in range(r):
        if np.isnan(density[j]):
            parent[j], delta[j] = NOISE, np.nan
            continue
        above = [i for i in range(r) if not np.isnan(density[i]) and ranks_above(density, i, j)]
        if above and rng.rand() < 0.9:
            parent[j], delta[j] = above[rng.randint(len(above))], rng.randint(0, 8) / 4.0
    return density, delta, parent


def test_the_worked_case():
    D = line(HAND_X)
    assert degree_density(D, HAND_EPS).tolist() == HAND_DENSITY
    got = density_peaks_ref(D, eps=HAND_EPS)
    assert got.density.tolist() == HAND_DENSITY and got.delta.tolist() == HAND_DELTA and got.parent.tolist() == HAND_PARENT
    assert got.labels is None and got.counts is None and got.parent.dtype == np.uint32
    for (min_density, min_delta), labels, counts in HAND_CUTS:
        cut = density_peaks_ref(D, eps=HAND_EPS, min_density=min_density, min_delta=min_delta)
        assert cut.labels.tolist() == labels and cut.counts.tolist() == counts
        assert np.array_equal(cut.labels[cut.labels], cut.labels)
    # re-derived: row 8 (0.75) sees rows 1 and 2 at 0.25, both denser -- the smaller index; row 5's only denser rows are the left
    # lineage's, the nearest row 2 at 9.5; row 7 (30) follows row 6 although every row is denser: row 6 is the nearest
    assert D[8, 1] == D[8, 2] == 0.25 and D[5, 2] == 9.5 and D[7, 6] == 19


def test_the_closed_form_of_the_chain():
    r = 1000
    pos, density, delta, parent = chain_case(r, 7)
    rows = np.zeros((r, 3))
    rows[:, 0] = pos
    D = np.sqrt(((rows[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2))
    want_delta, want_parent = parents_ref(D, density)
    assert same_bits(delta, want_delta) and np.array_equal(parent, want_parent)
    root = int(np.flatnonzero(pos == r // 3)[0])
    labels, counts = cut_ref(density, delta, parent, -INF, INF)
    assert np.all(labels == root) and counts.tolist() == [1, 1, 0]
    labels, counts = cut_ref(density, delta, parent, -INF, 0.5)
    assert np.array_equal(labels, np.arange(r)) and counts.tolist() == [r, 1, 0]


def test_a_parent_ranks_above_its_child():
    rng = np.random.RandomState(11)
    for r in (1, 2, 17, 120):
        x = rng.randint(0, 40, size=(r, 2)) / 4.0  # ties of distance, and copies
        D = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
        for density in (degree_density(D, 1.0), rng.randint(0, 4, size=r).astype(np.float64), rng.standard_normal(r)):
            got = density_peaks_ref(D, density=density, min_delta=0.75)
            roots = 0
            for j in range(r):
                i = int(got.parent[j])
                if i == j:
                    roots += 1
                    assert got.delta[j] == INF
                else:
                    assert ranks_above(density, i, j) and got.delta[j] == D[j, i]
            assert roots >= 1 and got.counts[1] == roots and got.counts[2] == 0
            top = max(range(r), key=lambda i: (density[i], -i))
            assert got.parent[top] == top


def test_the_cut_refines_the_graph_at_eps():
    rng = np.random.RandomState(5)
    x = np.concatenate([rng.standard_normal((60, 2)) * 0.3, rng.standard_normal((40, 2)) * 1.5 + 6.0])
    D = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    for eps in (0.2, 0.6, 2.0):
        got = density_peaks_ref(D, eps=eps, min_delta=eps)
        comp = components_within(D, eps)
        assert np.array_equal(comp[got.labels], comp)  # rows j and labels[j] in one component
        nearest = np.where(np.eye(len(x), dtype=bool), INF, D).min(axis=1)
        assert np.all(got.delta >= nearest)


def test_the_conventions():
    D = line([0, 1, 2, 4])
    # a NaN density: left out, nobody's candidate
    got = density_peaks_ref(D, density=[1, np.nan, 1, 3], min_delta=INF)
    assert got.delta.view(np.uint64)[1] == QNAN_BITS and got.parent[1] == NOISE and got.labels[1] == NOISE
    assert got.parent.tolist() == [3, NOISE, 0, 3] and got.delta.tolist()[::2] == [4, 2] and got.counts.tolist() == [1, 1, 1]
    # -0 equals +0: rows 0 and 1 tie, the smaller index above; +-inf are numbers
    got = density_peaks_ref(D, density=[-0.0, 0.0, -INF, INF])
    assert got.parent.tolist() == [3, 0, 1, 3] and got.delta.tolist() == [4, 1, 1, INF]
    # a row with a NaN in it: all its distances NaNs, a root; and nobody's parent
    E = D.copy()
    E[3, :] = E[:, 3] = np.nan
    got = density_peaks_ref(E, density=[1, 2, 3, 9], min_delta=INF)
    assert got.parent.tolist() == [1, 2, 2, 3] and got.counts.tolist() == [2, 2, 0] and got.labels.tolist() == [2, 2, 2, 3]
    # a negative eps: every degree 1, the rank is the row order: the nearest row of smaller index
    got = density_peaks_ref(line([5, 1, 2, 4.5]), eps=-1.0)
    assert got.density.tolist() == [1] * 4 and got.parent.tolist() == [0, 0, 1, 0] and got.delta.tolist() == [INF, 4, 1, 0.5]
    # -0 distances are written as +0
    Z = -np.zeros((2, 2))
    got = density_peaks_ref(Z, density=[1, 1])
    assert got.delta[1] == 0 and not np.signbit(got.delta[1])
    # no rows, one row
    assert len(density_peaks_ref(np.zeros((0, 0)), eps=1.0, min_delta=1.0).labels) == 0
    got = density_peaks_ref(np.zeros((1, 1)), eps=1.0, min_delta=1.0)
    assert got.parent.tolist() == [0] and got.delta.tolist() == [INF] and got.counts.tolist() == [1, 1, 0]


def cut_through_ctypes(density, delta, parent, min_density, min_delta, want_labels=True):
    from kpop_amd import _lib
    lib = _lib.load()
    density, delta = np.ascontiguousarray(density, dtype=np.float64), np.ascontiguousarray(delta, dtype=np.float64)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    r = len(parent)
    labels, counts = np.full(max(r, 1), 12345, dtype=np.uint32), np.full(3, 12345, dtype=np.uint32)
    f64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    pad = np.zeros(1)
    rc = lib.kpop_density_peaks_cut(r, (density if r else pad).ctypes.data_as(f64p), (delta if r else pad).ctypes.data_as(f64p),
                                    (parent if r else np.zeros(1, dtype=np.uint32)).ctypes.data_as(u32p), min_density, min_delta,
                                    labels.ctypes.data_as(u32p) if want_labels else None, counts.ctypes.data_as(u32p))
    return rc, labels[:r], counts


def test_the_cut_in_the_library_needs_no_gpu():
    """kpop_density_peaks_cut is host arithmetic: no GPU, no kpop_init.  (On the commit before this call existed the library has no
    such symbol.)"""
    import kpop_amd
    rng = np.random.RandomState(3)
    for r, left_out in ((0, 0), (1, 0), (2, 0), (30, 0), (200, 0), (200, 9), (5000, 40)):
        density, delta, parent = random_forest(rng, r, left_out) if r <= 200 else chain_forest(rng, r, left_out)
        for min_density, min_delta in ((-INF, INF), (-INF, 0.5), (2.0, 0.5), (INF, -INF), (-INF, -INF), (3.0, 1.25)):
            want_labels, want_counts = cut_ref(density, delta, parent, min_density, min_delta)
            rc, labels, counts = cut_through_ctypes(density, delta, parent, min_density, min_delta)
            assert rc == 0 and np.array_equal(labels, want_labels) and np.array_equal(counts, want_counts), (r, min_density, min_delta)
            assert counts[2] == left_out and np.all(labels[np.isnan(density)] == NOISE)
            keep = labels != NOISE
            assert np.array_equal(labels[labels[keep]], labels[keep])
            again, again_counts = kpop_amd.density_peaks_cut(density, delta, parent, min_density, min_delta)
            assert np.array_equal(again, want_labels) and np.array_equal(again_counts, want_counts)
    # counts alone
    density, delta, parent = random_forest(rng, 20)
    rc, _, counts = cut_through_ctypes(density, delta, parent, -INF, 0.5, want_labels=False)
    assert rc == 0 and np.array_equal(counts, cut_ref(density, delta, parent, -INF, 0.5)[1])
    # the worked case
    for (min_density, min_delta), labels, counts in HAND_CUTS:
        rc, got, n = cut_through_ctypes(HAND_DENSITY, HAND_DELTA, HAND_PARENT, min_density, min_delta)
        assert rc == 0 and got.tolist() == labels and n.tolist() == counts


def chain_forest(rng, r, left_out):
    """a long forest, deep chains in it, built in O(r): a row's parent is the row before it in a shuffled order, the densities falling
    along the order; every 97th row a root"""
    order = rng.permutation(r)
    density, delta, parent = np.zeros(r), rng.randint(0, 8, size=r) / 4.0, np.arange(r, dtype=np.uint32)
    density[order] = -np.arange(r, dtype=np.float64)
    parent[order[1:]] = order[:-1]
    roots = order[::97]
    parent[roots], delta[roots] = roots, INF
    out = order[rng.choice(r // 97, size=left_out, replace=False) * 97 + 96]  # (the last row of a chain: nobody's parent)
    density[out], delta[out], parent[out] = np.nan, np.nan, NOISE
    return density, delta, parent


def test_what_the_cut_refuses():
    density, delta = np.array([3.0, 2.0, 2.0, 1.0]), np.array([INF, 1.0, 1.0, 1.0])
    good = [0, 0, 1, 2]
    assert cut_through_ctypes(density, delta, good, -INF, 1.0)[0] == 0
    for min_density, min_delta in ((np.nan, 1.0), (0.0, np.nan)):
        rc, labels, counts = cut_through_ctypes(density, delta, good, min_density, min_delta)
        assert rc == ERR_INVALID and np.all(labels == 12345) and np.all(counts == 12345)  # nothing is written
    for bad in ([0, 3, 1, 2],    # a parent of lower density
                [0, 2, 1, 2],    # an equal density and a LARGER index: ranks below
                [0, 0, 1, 4],    # a parent = r1
                [0, 0, 1, 77],   # a parent beyond r1
                [1, 0, 1, 2]):   # the top of the order under somebody: with [1] -> 0 a cycle
        rc, labels, counts = cut_through_ctypes(density, delta, bad, -INF, 1.0)
        assert rc == ERR_INVALID and np.all(labels == 12345) and np.all(counts == 12345), bad
    # a NaN density ranks above nobody and below nobody: it may only be left out or stand alone
    assert cut_through_ctypes([np.nan, 1.0], [1.0, INF], [1, 1], -INF, 1.0)[0] == ERR_INVALID
    assert cut_through_ctypes([1.0, np.nan], [INF, 1.0], [0, 0], -INF, 1.0)[0] == ERR_INVALID
    assert cut_through_ctypes([1.0, np.nan], [INF, np.nan], [0, NOISE], -INF, 1.0)[0] == 0
    import kpop_amd
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.density_peaks_cut(density, delta, [0, 3, 1, 2], -INF, 1.0)
    with pytest.raises(ValueError):
        kpop_amd.density_peaks_cut(density, delta[:3], good)


def test_header_declares_and_library_exports_the_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*density_peaks[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_dev_lof_score(") < code.index("kpop_density_peaks(")  # the block after the local outlier factor
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Space.ml:182-205" in comment or "lib/Matrix.ml:191-266" in comment, name  # which lines of the reference it stands on


def test_python_surface():
    import kpop_amd
    for name in ("DensityPeaks", "distance_density_peaks", "dev_density_peaks_workspace_bytes", "dev_density_peaks", "density_peaks_cut"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.density_peaks)
    assert kpop_amd.DensityPeaks._fields == ("density", "delta", "parent", "labels", "counts")
    with pytest.raises(ValueError):
        kpop_amd.distance_density_peaks(np.zeros((3, 2)), np.ones(3), eps=1.0)
    with pytest.raises(ValueError):
        kpop_amd.distance_density_peaks(np.zeros((3, 2)), np.ones(2), density=np.ones(4))


def test_the_kernels_are_built_from_their_own_file():
    csrc = os.path.join(ROOT, "kpop_amd", "csrc")
    assert "density_peaks.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "density_peaks.hip")).read()
    code = re.sub(r"//.*", "", src)
    for kernel in ("density_peaks_sweep_kernel", "density_peaks_key_kernel", "density_peaks_merge_kernel", "density_peaks_flags_kernel",
                   "density_peaks_jump_kernel", "density_peaks_degree_kernel"):
        assert "void " + kernel in src
    assert "asm" not in code  # plain HIP C++ throughout
    # one sweep body over gathered rows: its steps and the chain stand in pair_tile.h and not here; the lanes meet in the shared tree
    assert src.count("pair_sweep_tile<KIND>(") == 1 and "pair_sweep_open(" in src and "PairRowsAt" in code and "key_at_min" in code
    assert "stage.store(" not in src and "pair_accumulate<" not in src and "__dsub_rn(av[" not in src
    assert "atomicMin" not in code and "unsafeAtomic" not in code  # a row owns its minimum: the only atomics are integer counts
    # the sort and the degree pass are reused, not copied
    assert "radix_sort_pairs_u64(" in code and "dbscan_degree_dev(" in code and "dbscan_degree_kernel" not in code
    assert "int dbscan_degree_dev(" in open(os.path.join(csrc, "dbscan.hip")).read()
    assert "int dbscan_degree_dev(" in open(os.path.join(csrc, "self_tile.h")).read()


def test_refusals_made_on_the_host():
    """no handle: refused on the host -- KPOP_ERR_NOT_INIT where nothing has initialised the library, KPOP_ERR_INVALID where something
    has -- and the workspace size of no set is 0.  Neither needs a GPU"""
    from kpop_amd import _lib
    lib = _lib.load()
    f64, u32 = (C.c_double * 4)(), (C.c_uint32 * 4)()
    refused = (ERR_INVALID, ERR_NOT_INIT)
    assert lib.kpop_density_peaks(None, 1.0, None, -INF, 1.0, f64, f64, u32, u32, u32) in refused
    assert lib.kpop_dev_density_peaks(None, 1.0, None, -INF, 1.0, None, None, None, None, None, None, None) in refused
    assert lib.kpop_dev_density_peaks_workspace_bytes(None) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    rs.info = lambda: {"r1": 2, "n_dims": 3}
    with pytest.raises(kpop_amd.KPopError):
        rs.density_peaks(eps=1.0)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_density_peaks(np.ones((2, 3)), np.ones(3), eps=1.0)
