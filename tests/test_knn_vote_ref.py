"""CPU tests of the k-NN vote: the numpy reference the GPU tests compare with (tests/knn_vote_ref.py) on the worked case of
INTEGRATION.md section 6f and on the README's row, and the boundary -- the header declares the four functions, the library exports them,
the Python table binds them, the kernels are built from their own file, and without a GPU a call fails (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from knn_vote_ref import NO_CLASS, knn_lists, knn_vote_ref

FUNCTIONS = ["kpop_knn_vote", "kpop_dev_knn_vote_workspace_bytes", "kpop_dev_knn_vote", "kpop_distance_knn_vote"]

nan, inf = float("nan"), float("inf")
D = np.array([[0.5, 0.25, 2.0, 0.25, 1.0],
              [0.0, 3.0, -0.0, 1.5, 0.0],
              [nan, 1.0, inf, 0.75, nan],
              [nan, nan, nan, nan, nan]])
CLASS_OF = np.array([4, 7, 7, 4, 9])
NO = NO_CLASS
WORKED = {1: ([7, 4, 4, NO], [1, 1, 1, 0], [2, 3, 1, 0], [0.25, 0.0, 0.75, nan]),
          2: ([7, 4, 4, NO], [1, 1, 1, 0], [2, 3, 2, 0], [0.25, 0.0, 0.75, nan]),
          3: ([4, 4, 7, NO], [2, 1, 2, 0], [3, 3, 3, 0], [0.25, 0.0, 1.0, nan]),
          5: ([7, 4, 7, NO], [2, 2, 2, 0], [5, 5, 3, 0], [0.25, 0.0, 1.0, nan])}


@pytest.mark.parametrize("k", sorted(WORKED))
def test_the_worked_case(k):
    """row 0, k = 1: columns 1 and 3 tie at 0.25, the group is listed whole, classes 7 and 4 have one vote each and 7 appears first; row 0,
    k = 5: two votes each, 7 first; row 1: -0 beside +0, ordered by column; row 2: a NaN is never listed, +inf is; row 3: nothing"""
    cls, votes, n, first = knn_vote_ref(D, CLASS_OF, k)
    assert cls.dtype == votes.dtype == n.dtype == np.uint32 and first.dtype == np.float64
    want = WORKED[k]
    assert cls.tolist() == want[0]
    assert votes.tolist() == want[1]
    assert n.tolist() == want[2]
    assert np.array_equal(first.view(np.uint64), np.array(want[3]).view(np.uint64))
    assert not np.signbit(first[1])  # the nearest member of class 4 in row 1 is column 0, the +0


def test_the_lists_of_the_worked_case():
    assert [l.tolist() for l in knn_lists(D, 1)] == [[1, 3], [0, 2, 4], [3], []]
    assert [l.tolist() for l in knn_lists(D, 3)] == [[1, 3, 0], [0, 2, 4], [3, 1, 2], []]
    assert [l.tolist() for l in knn_lists(D, 128)] == [[1, 3, 0, 4, 2], [0, 2, 4, 3, 1], [3, 1, 2], []]
    with pytest.raises(ValueError):
        knn_lists(D, 0)
    # a class that is not below n_classes counts in n and votes for nobody
    cls, votes, n, first = knn_vote_ref(D, CLASS_OF, 5, n_classes=8)
    assert cls.tolist() == [7, 4, 7, NO] and votes.tolist() == [2, 2, 2, 0] and n.tolist() == [5, 5, 3, 0]
    cls, votes, n, first = knn_vote_ref(D, CLASS_OF, 1, n_classes=4)
    assert cls.tolist() == [NO] * 4 and votes.tolist() == [0] * 4 and n.tolist() == [2, 3, 1, 0] and np.isnan(first).all()


def test_reference_on_the_readme_row():
    """the ten distances of README.md:645-649 with k = 2: the list is the summary line's two neighbours; every neighbour its own class,
    so the winner is the first neighbour"""
    kat = load_golden("readme_kat.json")
    row = np.array([[float(x) for x in kat["distance_row_text"]]])
    assert kat["keep_at_most"] == 2
    (cols,) = knn_lists(row, 2)
    want = kat["summary_line"].split("\t")
    assert ['"%s"' % kat["distance_header"][i] for i in cols] == [want[5], want[8]]
    assert row[0, cols].tolist() == [float(want[6]), float(want[9])]
    cls, votes, n, first = knn_vote_ref(row, np.arange(10), 2)
    assert '"%s"' % kat["distance_header"][int(cls[0])] == want[5]
    assert (int(votes[0]), int(n[0]), float(first[0])) == (1, 2, float(want[6]))


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*knn_vote[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_forest_cut(") < code.index("kpop_knn_vote(")  # the block after the single-linkage tree
    assert re.search(r"#define\s+KPOP_NO_CLASS\s+0xFFFFFFFFu", code)
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands on, as its neighbours do
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment, name
    # the other families stay what they are
    assert not any(re.match(r"kpop_(dev_)?refset_", name) or "clusters" in name or "forest" in name for name in FUNCTIONS)


def test_python_surface():
    import kpop_amd
    for name in ("dev_knn_vote_workspace_bytes", "dev_knn_vote", "distance_knn_vote"):
        assert callable(getattr(kpop_amd, name)) and name in kpop_amd.__all__
    assert kpop_amd.NO_CLASS == NO_CLASS and "NO_CLASS" in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.knn_vote)


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "knn.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "knn.hip")).read()
    for kernel in ("knn_nearest_kernel", "knn_merge_kernel", "knn_ties_kernel", "knn_vote_kernel"):
        assert "void " + kernel in src
    assert "asm" not in re.sub(r"//.*", "", src)  # plain HIP C++ throughout


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    rs.info = lambda: {"r1": 2, "n_dims": 3}
    with pytest.raises(kpop_amd.KPopError):
        rs.knn_vote(np.ones((2, 3)), [0, 1], k=1)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_knn_vote(np.ones((2, 3)), [0, 1], np.ones((2, 3)), np.ones(3), k=1)
