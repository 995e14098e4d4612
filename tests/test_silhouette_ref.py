"""The reference of the silhouette and the medoids (tests/silhouette_ref.py) on the worked case of INTEGRATION.md 6k, the ABI of the
block, and the parts of it that need no GPU: kpop_silhouette_summary and dense_labels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import NOISE, dbscan_ref
from silhouette_ref import NO_CLASS, same_bits, silhouette_ref, summary_ref

FUNCTIONS = ["kpop_silhouette", "kpop_dev_silhouette_workspace_bytes", "kpop_dev_silhouette", "kpop_distance_silhouette", "kpop_silhouette_summary"]
KERNELS = ["silhouette_keys_kernel", "silhouette_tiles_kernel", "silhouette_pass_kernel", "silhouette_rows_kernel", "silhouette_medoid_kernel",
           "silhouette_classes_kernel"]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3

# the ten rows of INTEGRATION.md 6i, kpop_dbscan's labels at eps = .375, min_pts = 4 made dense
HAND_X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
HAND_CLASS = [0, 0, 0, 1, 1, 1, 1, 1, NO_CLASS, 0]
HAND_OWN = [0.25, 1 / 6, 1 / 6, 0.28125, 0.25, 0.28125, 0.375, 0.5625, None, 0.25]
HAND_OTHER = [1.2, 1.075, 0.95, 0.9375, 1.0625, 1.1875, 1.3125, 0.5625, None, 0.825]


def euclidean_line(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


def test_the_worked_case():
    D = euclidean_line(HAND_X)
    labels = dbscan_ref(D, 0.375, 4)[0]
    import kpop_amd
    class_of, n_classes, label_of_class = kpop_amd.dense_labels(labels)
    assert class_of.tolist() == HAND_CLASS and n_classes == 2 and label_of_class.tolist() == [0, 3]
    own, other, ocls, sil, class_rows, medoid, medoid_mean = silhouette_ref(D, class_of, n_classes)
    for j in range(10):
        if HAND_OWN[j] is None:
            assert np.isnan(own[j]) and np.isnan(other[j]) and ocls[j] == NO_CLASS and np.isnan(sil[j])
        else:
            assert own[j] == HAND_OWN[j] and other[j] == HAND_OTHER[j], j  # every distance and sum is exact: bit for bit
            assert ocls[j] == 1 - HAND_CLASS[j]
    assert sil[7] == 0.0 and not np.signbit(sil[7])  # the border row
    assert sil[3] == 0.7 and sil[0] == 19 / 24
    assert class_rows.tolist() == [4, 5]
    assert medoid.tolist() == [1, 4]  # row 1 on a tie with row 2
    assert medoid_mean.tolist() == [1 / 6, 0.25]


def test_special_cases_of_the_reference():
    D = euclidean_line([0.0, 1.0, 1.0, 3.0, 7.0])
    # a class of one row: own +0, silhouette +0; an empty class; a row left out
    own, other, ocls, sil, class_rows, medoid, medoid_mean = silhouette_ref(D, [0, 1, 1, 3, NO_CLASS], 4)
    assert own.tolist()[:4] == [0.0, 0.0, 0.0, 0.0] and sil[0] == 0.0 and sil[3] == 0.0
    assert other.tolist()[:4] == [1.0, 1.0, 1.0, 2.0] and ocls.tolist() == [1, 0, 0, 1, NO_CLASS]
    assert np.isnan(sil[4]) and class_rows.tolist() == [1, 2, 0, 1]
    assert medoid.tolist() == [0, 1, NO_CLASS, 3] and np.isnan(medoid_mean[2])
    assert sil[1] == 1.0  # (1 - 0) / 1
    # one class alone: no other class
    own, other, ocls, sil, _, medoid, _ = silhouette_ref(D, [0] * 5, 1)
    assert np.all(np.isnan(other)) and np.all(ocls == NO_CLASS) and np.all(np.isnan(sil)) and medoid.tolist() == [1]
    # a tie for the other class goes to the smaller class; duplicates of two classes: 0 / 0
    own, other, ocls, sil, _, _, _ = silhouette_ref(euclidean_line([0.0, -1.0, 1.0, 0.0, 0.0]), [0, 2, 1, 0, 3], 4)
    assert ocls[0] == 3 and other[0] == 0.0 and np.isnan(sil[0])  # class 3 lies on row 0: own 0, other 0
    assert ocls[4] == 0 and ocls[1] == 0 and ocls[2] == 0
    own, other, ocls, sil, _, _, _ = silhouette_ref(euclidean_line([0.0, -1.0, 1.0]), [0, 2, 1], 3)
    assert ocls[0] == 1 and other[0] == 1.0  # classes 1 and 2 both at 1
    # a NaN distance poisons the sums it is in, and a NaN mean is never the least
    bad = euclidean_line([0.0, 1.0, 2.0, 5.0, 6.0, 9.0])
    bad[2, :] = bad[:, 2] = np.nan
    own, other, ocls, sil, _, medoid, _ = silhouette_ref(bad, [0, 0, 0, 1, 1, 2], 3)
    assert np.all(np.isnan(own[:3])) and medoid[0] == NO_CLASS  # every sum of class 0 holds the row
    assert ocls[3] == 2 and other[3] == 4.0 and ocls[5] == 1  # class 0's mean is a NaN: class 2 is the least
    assert np.isnan(other[2]) and ocls[2] == NO_CLASS  # the row itself: every mean a NaN


def test_header_declares_and_library_exports_the_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*silhouette[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_reachability_cut(") < code.index("kpop_silhouette(")  # the block after the reachability tree
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Space.ml:182-205" in comment, name  # every declaration says which lines of the reference it stands on


def test_python_surface():
    import kpop_amd
    for name in ("distance_silhouette", "dev_silhouette_workspace_bytes", "dev_silhouette", "silhouette_summary", "dense_labels", "Silhouette"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.silhouette)
    assert kpop_amd.Silhouette._fields == ("own_mean", "other_mean", "other_class", "silhouette", "class_rows", "medoid", "medoid_mean")


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "silhouette.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "silhouette.hip")).read()
    for kernel in KERNELS:
        assert kernel in src
    assert "PairRowsAt" in src and "pair_sweep_tile<KIND>(" in src and "reduce_row_lanes" in src  # columns gathered, the sweep of pair_tile.h
    assert "load_indexed" not in src and "stage.store(" not in src and "pair_accumulate<" not in src
    assert "radix_sort_pairs_u64" in src and "exclusive_scan" in src
    assert "atomicAdd(double" not in src and "unsafeAtomicAdd" not in src  # no floating-point atomic


def test_summary_against_the_reference():
    import kpop_amd
    rng = np.random.RandomState(11)
    r1, n_classes = 257, 6
    class_of = rng.randint(0, n_classes - 1, size=r1).astype(np.uint32)  # class 5 is empty
    class_of[class_of == 2] = 4
    class_of[rng.rand(r1) < 0.1] = NO_CLASS
    # values whose sum depends on the order: magnitudes over 2^60
    sil = rng.uniform(-1, 1, size=r1) * 2.0 ** rng.randint(-30, 30, size=r1)
    assert sum(sil[::-1].tolist()) != sum(sil.tolist())
    want_mean, want_all = summary_ref(class_of, n_classes, sil)
    got_mean, got_all = kpop_amd.silhouette_summary(class_of, sil, n_classes)
    assert same_bits(got_mean, want_mean) and same_bits([got_all], [want_all])
    assert np.isnan(got_mean[2]) and np.isnan(got_mean[5]) and not np.isnan(got_mean[4])
    # the values of the rows left out are not read into any sum
    spoiled = np.where(class_of == NO_CLASS, np.nan, sil)
    got_mean2, got_all2 = kpop_amd.silhouette_summary(class_of, spoiled, n_classes)
    assert same_bits(got_mean2, want_mean) and same_bits([got_all2], [want_all])
    # a NaN entry poisons its class and the overall mean, and nothing else
    k = int(np.flatnonzero(class_of == 1)[3])
    poisoned = np.array(sil)
    poisoned[k] = np.nan
    got_mean3, got_all3 = kpop_amd.silhouette_summary(class_of, poisoned, n_classes)
    assert np.isnan(got_mean3[1]) and np.isnan(got_all3)
    keep = np.arange(n_classes) != 1
    assert same_bits(got_mean3[keep], want_mean[keep])
    # n_classes from the labels; nothing at all; every row left out
    assert same_bits(kpop_amd.silhouette_summary(class_of, sil)[0], want_mean[:5])
    mean, overall = kpop_amd.silhouette_summary(np.zeros(0, dtype=np.uint32), np.zeros(0), 3)
    assert np.all(np.isnan(mean)) and len(mean) == 3 and np.isnan(overall)
    mean, overall = kpop_amd.silhouette_summary(np.full(4, NO_CLASS, dtype=np.uint32), np.ones(4), 2)
    assert np.all(np.isnan(mean)) and np.isnan(overall)


def test_summary_errors():
    import kpop_amd
    from kpop_amd import _lib
    lib = _lib.load()
    cls = np.array([0, 1, NO_CLASS], dtype=np.uint32)
    sil = np.array([0.5, -0.5, np.nan])
    for n_classes, code in ((0, ERR_INVALID), (65536, ERR_UNSUPPORTED), (1, ERR_INVALID)):  # (1: row 1 has class 1 of 1)
        with pytest.raises(kpop_amd.KPopError) as e:
            kpop_amd.silhouette_summary(cls, sil, n_classes)
        assert e.value.code == code and "kpop_silhouette_summary" in str(e.value)
    assert kpop_amd.silhouette_summary(cls, sil, 65535)[1] == 0.0
    u32, f64 = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    mean, overall = np.zeros(2), C.c_double()
    assert lib.kpop_silhouette_summary(3, u32(cls), 2, f64(sil), f64(mean), C.byref(overall)) == 0
    assert lib.kpop_silhouette_summary(3, None, 2, f64(sil), f64(mean), C.byref(overall)) == ERR_INVALID
    assert lib.kpop_silhouette_summary(3, u32(cls), 2, None, f64(mean), C.byref(overall)) == ERR_INVALID
    assert lib.kpop_silhouette_summary(3, u32(cls), 2, f64(sil), None, C.byref(overall)) == ERR_INVALID
    assert lib.kpop_silhouette_summary(3, u32(cls), 2, f64(sil), f64(mean), None) == ERR_INVALID
    assert lib.kpop_silhouette_summary(0, None, 2, None, f64(mean), C.byref(overall)) == 0  # no row: nothing is read


def test_dense_labels():
    import kpop_amd
    assert kpop_amd.NO_CLASS == kpop_amd.NOISE == NO_CLASS == NOISE
    rng = np.random.RandomState(5)
    x = np.concatenate([rng.randint(0, 8, size=40) * 4.0 + rng.randint(0, 3, size=40) * 0.125, [100.0, 200.0]])
    D = euclidean_line(x)
    labels = dbscan_ref(D, 0.375, 3)[0]
    assert np.any(labels == NOISE) and len(np.unique(labels)) > 3
    class_of, n_classes, label_of_class = kpop_amd.dense_labels(labels)
    assert class_of.dtype == np.uint32 and label_of_class.dtype == np.uint32
    assert n_classes == len(label_of_class) == len(np.unique(labels[labels != NOISE]))
    assert np.all(np.diff(label_of_class.astype(np.int64)) > 0)  # ascending label order
    assert np.array_equal(class_of == NO_CLASS, labels == NOISE)
    kept = labels != NOISE
    assert np.array_equal(label_of_class[class_of[kept]], labels[kept])
    assert set(class_of[kept].tolist()) == set(range(n_classes))
    # every row noise, and no row at all
    class_of, n_classes, label_of_class = kpop_amd.dense_labels(np.full(3, NOISE, dtype=np.uint32))
    assert class_of.tolist() == [NO_CLASS] * 3 and n_classes == 0 and len(label_of_class) == 0
    class_of, n_classes, label_of_class = kpop_amd.dense_labels(np.zeros(0, dtype=np.uint32))
    assert len(class_of) == 0 and n_classes == 0
    with pytest.raises(ValueError):
        kpop_amd.dense_labels(np.array([[0, 1]]))
    with pytest.raises(ValueError):
        kpop_amd.dense_labels(np.array([-1, 0]))
