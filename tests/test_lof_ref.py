"""tests/lof_ref.py held to INTEGRATION.md section 6n: the worked case value for value, the properties that need no GPU, and the
boundary -- include/kpop_hip.h declares the seven functions with the lines of the reference they stand on, the library exports them, the
Python table binds them, the package offers them, and the refusals that are decided on the host are made without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from lof_ref import INF, QNAN_BITS, U, k_distance, lof_ref, lof_score_ref, neighbourhood_max, same_bits

# the worked case of INTEGRATION.md 6n: one-dimensional rows, euclidean, flat metric, no normalising, k = 2; every distance exact
HAND_X = [0, .25, .5, .75, 1, 1.25, 1.5, -3, 2, 2, 2]
HAND_K = 2
HAND_KDIST = [.5, .25, .25, .25, .25, .25, .5, 3.25, 0, 0, 0]
HAND_N = [2, 2, 2, 2, 2, 2, 5, 2, 2, 2, 2]
HAND_LRD = [2.6666666666666665, 2.6666666666666665, 4, 4, 4, 2.6666666666666665, 2.2222222222222223, 0.32, INF, INF, INF]
HAND_LOF = [1.25, 1.25, 0.83333333333333326, 1, 0.83333333333333326, 1.1666666666666667, INF, 8.3333333333333321, 1, 1, 1]
HAND_Q = [0.625, -1, 2, 100]
HAND_Q_KDIST = [.125, 1.25, 0, 98]
HAND_Q_N = [2, 2, 3, 3]
HAND_Q_LRD = [4, 0.88888888888888884, INF, 0.01020408163265306]
HAND_Q_LOF = [1, 3, 1, INF]

FUNCTIONS = ["kpop_lof", "kpop_dev_lof_workspace_bytes", "kpop_dev_lof", "kpop_distance_lof", "kpop_lof_score", "kpop_dev_lof_score_workspace_bytes",
             "kpop_dev_lof_score"]
ERR_INVALID, ERR_NOT_INIT = -1, -5


def line(x, y=None):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(np.subtract.outer(x if y is None else np.asarray(y, dtype=np.float64), x))


def check_hand(got, kdist, n, lrd, lof):
    assert got.kdist.tolist() == kdist and got.n_neigh.tolist() == n and got.lrd.tolist() == lrd and got.lof.tolist() == lof
    assert not np.any(np.signbit(got.kdist)) and got.n_neigh.dtype == np.uint32


def test_the_worked_case():
    want = lof_ref(line(HAND_X), HAND_K)
    check_hand(want, HAND_KDIST, HAND_N, HAND_LRD, HAND_LOF)
    check_hand(lof_score_ref(line(HAND_X, HAND_Q), HAND_K, want.kdist, want.lrd), HAND_Q_KDIST, HAND_Q_N, HAND_Q_LRD, HAND_Q_LOF)


def test_an_equally_spaced_line():
    """a row whose neighbours are all interior -- they and their own neighbours have the grid's k-distance, which holds from h = k / 2
    positions off either end -- has the density of each of them: exactly 1"""
    for r, k in ((40, 2), (40, 4), (41, 6), (9, 2)):
        got = lof_ref(line(np.arange(r) * 0.25), k)
        h = k // 2
        assert np.all(got.kdist[h:r - h] == h * 0.25) and np.all(got.n_neigh[h:r - h] == k)
        inner = np.arange(3 * h, r - 3 * h)  # a row, its neighbours (h to each side) and theirs: 3 h from the ends at least
        assert len(inner) and np.all(got.lof[inner] == 1.0), (r, k)
        assert got.lof[0] > 1.0


def test_a_permutation_of_the_rows():
    """the neighbourhood is the whole tie group: kdist and n_neigh permute exactly; lrd is one rounding of an exact sum's quotient on
    both sides (the reference's sums are exactly rounded), so it permutes exactly too, and lof with it -- held to the GPU tests' bound"""
    rng = np.random.RandomState(4)
    x = rng.randint(0, 64, size=60) / 8.0  # ties, and copies
    D = line(x)
    for k in (1, 3, 7):
        got = lof_ref(D, k)
        perm = rng.permutation(len(x))
        moved = lof_ref(D[np.ix_(perm, perm)], k)
        assert same_bits(moved.kdist, got.kdist[perm]) and np.array_equal(moved.n_neigh, got.n_neigh[perm])
        assert same_bits(moved.lrd, got.lrd[perm])
        bound = 4 * (neighbourhood_max(got.n_neigh) + 2) * U
        a, b = moved.lof, got.lof[perm]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
        ok = np.isfinite(b)
        assert np.all(np.abs(a[ok] - b[ok]) <= bound * b[ok])


def test_fewer_rows_than_neighbours():
    for r, k in ((1, 1), (3, 3), (3, 128), (0, 5)):
        got = lof_ref(line(np.arange(r)), k)
        for a in (got.kdist, got.lrd, got.lof):
            assert len(a) == r and np.all(a.view(np.uint64) == QNAN_BITS)
        assert not got.n_neigh.any()
    got = lof_score_ref(line([0, 1], [5, 6, 7]), 3, [1.0, 1.0], [1.0, 1.0])
    assert np.all(np.isnan(got.kdist)) and not got.n_neigh.any() and np.all(got.lof.view(np.uint64) == QNAN_BITS)
    for bad in (0, 129, 1.5):
        with pytest.raises(ValueError):
            lof_ref(line([0, 1, 2]), bad)


def test_a_row_holding_a_nan():
    """row 4's distances are NaNs both ways: it has no neighbours, and it is in nobody's neighbourhood"""
    x = np.array([0, 1, 2, 4, 0, 8, 9.5])
    D = line(x)
    D[4, :] = D[:, 4] = np.nan
    got = lof_ref(D, 2)
    keep = [0, 1, 2, 3, 5, 6]
    want = lof_ref(D[np.ix_(keep, keep)], 2)
    for a in (got.kdist, got.lrd, got.lof):
        assert a.view(np.uint64)[4] == QNAN_BITS
    assert got.n_neigh[4] == 0
    for a, b in zip(got, want):
        assert same_bits(a[keep].astype(np.float64), b.astype(np.float64))
    assert k_distance([np.nan, 3.0, -0.0, INF], 1) == 0.0 and not np.signbit(k_distance([-0.0], 1))
    assert k_distance([np.nan, 3.0, INF], 2) == INF and np.isnan(k_distance([np.nan, 3.0, INF], 3))


def test_the_conventions():
    # a clump of k + 1 copies: lrd +inf, lof 1.0; the row beside it: lof +inf
    got = lof_ref(line([5, 5, 5, 6]), 2)
    assert got.lrd[:3].tolist() == [INF] * 3 and got.lof[:3].tolist() == [1.0] * 3 and got.lof[3] == INF and got.n_neigh.tolist() == [2, 2, 2, 3]
    # an infinite distance is a number: S1 = +inf gives lrd 0, and 0 / 0 a NaN with the declared bits
    D = line([0, 1, 2])
    D[2, :2] = D[:2, 2] = INF
    got = lof_ref(D, 2)
    assert got.kdist.tolist() == [INF] * 3 and got.lrd.tolist() == [0.0] * 3 and np.all(got.lof.view(np.uint64) == QNAN_BITS)
    # a NaN k-distance of a neighbour poisons the sum it is in
    D = line([0, 1, 2, 3])
    D[3, 1:3] = D[1:3, 3] = np.nan  # row 3 has one numeric distance: no 2-distance; row 0 has it within its own
    got = lof_ref(D, 2)
    assert np.isnan(got.kdist[3]) and got.n_neigh[3] == 0
    got = lof_ref(D, 3)
    assert got.kdist[0] == 3.0 and got.n_neigh[0] == 3 and np.isnan(got.lrd[0]) and np.isnan(got.lof[0])


def test_header_declares_and_library_exports_the_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*lof[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_kmedoids(") < code.index("kpop_lof(")  # the block after k-medoids
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Space.ml:182-205" in comment or "lib/Matrix.ml:191-266" in comment, name  # which lines of the reference it stands on


def test_python_surface():
    import kpop_amd
    for name in ("Lof", "distance_lof", "dev_lof_workspace_bytes", "dev_lof", "dev_lof_score_workspace_bytes", "dev_lof_score"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.lof) and callable(kpop_amd.RefSet.lof_score)
    assert kpop_amd.Lof._fields == ("kdist", "n_neigh", "lrd", "lof")
    with pytest.raises(ValueError):
        kpop_amd.distance_lof(np.zeros((3, 2)), np.ones(3))
    with pytest.raises(ValueError):
        kpop_amd.distance_lof(np.zeros((3, 2)), np.ones(2), k=-1)


def test_the_kernels_are_built_from_their_own_file():
    csrc = os.path.join(ROOT, "kpop_amd", "csrc")
    assert "lof.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "lof.hip")).read()
    code = re.sub(r"//.*", "", src)
    for kernel in ("lof_pass_kernel", "lof_rows_kernel", "lof_kdist_kernel", "lof_fill_kernel"):
        assert "void " + kernel in src
    assert "asm" not in code  # plain HIP C++ throughout
    # one sweep body: its steps and the chain stand in pair_tile.h and not here; the lanes meet in the shared tree
    assert src.count("pair_sweep_tile<KIND>(") == 1 and "pair_sweep_open(" in src and "PairTilesOf" in src and "reduce_row_lanes" in src
    assert "stage.store(" not in src and "pair_accumulate<" not in src and "__dsub_rn(av[" not in src
    assert "atomicAdd" not in code and "unsafeAtomicAdd" not in code  # no atomic at all, so no floating-point one
    # the k-distances are the core distances' and the k-NN passes': reused through the header, not copied
    assert "core_dev(" in code and "knn_run_lists(" in code and "knn_nearest_kernel" not in code and "knn_merge_kernel" not in code
    assert "knn_run_leave_self_out_lists" not in code  # (the slab loop stays in reachability.hip)
    knn = open(os.path.join(csrc, "knn.hip")).read()
    assert "int knn_run_lists(" in knn and "int knn_run_lists(" in open(os.path.join(csrc, "knn_lists.h")).read()


def test_refusals_made_on_the_host():
    """no handle: refused on the host -- KPOP_ERR_NOT_INIT where nothing has initialised the library, KPOP_ERR_INVALID where something
    has -- and the workspace sizes of no set are 0.  Neither needs a GPU"""
    from kpop_amd import _lib
    lib = _lib.load()
    f64, u32 = (C.c_double * 4)(), (C.c_uint32 * 4)()
    refused = (ERR_INVALID, ERR_NOT_INIT)
    assert lib.kpop_lof(None, 2, f64, u32, f64, f64) in refused
    assert lib.kpop_lof_score(None, 2, f64, f64, f64, 1, f64, u32, f64, f64) in refused
    assert lib.kpop_dev_lof(None, 2, None, None, None, None, None, None) in refused
    assert lib.kpop_dev_lof_score(None, 2, None, None, None, 1, None, None, None, None, None, None) in refused
    assert lib.kpop_dev_lof_workspace_bytes(None, 2) == 0 and lib.kpop_dev_lof_score_workspace_bytes(None, 4, 2) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    rs.info = lambda: {"r1": 2, "n_dims": 3}
    with pytest.raises(kpop_amd.KPopError):
        rs.lof(1)
    with pytest.raises(kpop_amd.KPopError):
        rs.lof_score(np.ones((1, 3)), 1, np.ones(2), np.ones(2))
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_lof(np.ones((2, 3)), np.ones(3), k=1)
