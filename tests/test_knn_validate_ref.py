"""CPU tests of the k-NN validation: the numpy reference the GPU tests compare with (tests/knn_validate_ref.py) on the worked case of
INTEGRATION.md section 6g, the accuracy bookkeeping (confusion_matrix), and the boundary -- the header declares the functions with their
citations, the library exports them, the Python table binds them, the kernels are built from their own file, the vote's kernels are
where they were, and without a GPU a call fails (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from knn_validate_ref import knn_validate_ref, leave_out
from knn_vote_ref import NO_CLASS, knn_vote_ref

FUNCTIONS = ["kpop_knn_ks_vote", "kpop_dev_knn_ks_vote_workspace_bytes", "kpop_dev_knn_ks_vote", "kpop_knn_validate",
             "kpop_dev_knn_validate_workspace_bytes", "kpop_dev_knn_validate", "kpop_distance_knn_validate"]

nan = float("nan")
NO = NO_CLASS
X = np.array([0.0, 1.0, 1.0, 3.0, 10.0, nan])
CLASS_OF = np.array([0, 1, 0, 1, 1, 0])
D = np.abs(X[:, None] - X[None, :])
FIRST = [1.0, 0.0, 0.0, 2.0, 7.0, nan]
WORKED = {1: ([1, 0, 1, 1, 1, NO], [1, 1, 1, 1, 1, 0], [2, 1, 1, 2, 1, 0], 2),
          2: ([1, 0, 1, 1, 1, NO], [1, 2, 1, 1, 2, 0], [2, 2, 2, 2, 3, 0], 2),
          4: ([1, 0, 1, 1, 1, NO], [3, 2, 3, 2, 2, 0], [4, 4, 4, 4, 4, 0], 2)}


def test_the_worked_case():
    """leave-one-out over 1-D points 0, 1, 1, 3, 10, NaN.  Row 0, k = 1: rows 1 and 2 tie at 1, the group is listed whole, a vote each and
    class 1 (row 1) comes first.  Rows 1 and 2 are duplicates: each lists the other at 0 and NOT itself.  Row 3, k = 1: rows 1 and 2 at 2.
    Row 4, k = 2: row 3 at 7, then rows 1 and 2 tie at 9.  Row 5 holds a NaN: no list, and it is in nobody's"""
    ks = sorted(WORKED)
    cls, votes, n, first, correct = knn_validate_ref(D, CLASS_OF, ks)
    assert cls.dtype == votes.dtype == n.dtype == np.uint32 and first.dtype == np.float64 and correct.dtype == np.uint64
    for t, k in enumerate(ks):
        want = WORKED[k]
        assert cls[t].tolist() == want[0], k
        assert votes[t].tolist() == want[1], k
        assert n[t].tolist() == want[2], k
        assert np.array_equal(first[t].view(np.uint64), np.array(FIRST).view(np.uint64)), k
        assert int(correct[t]) == want[3], k
    # slice t is the vote over the matrix without what is left out
    E = leave_out(D)
    assert np.isnan(np.diag(E)).all() and np.array_equal(np.isnan(E[:5, :5]), np.eye(5, dtype=bool))
    for t, k in enumerate(ks):
        for a, b in zip((cls[t], votes[t], n[t]), knn_vote_ref(E, CLASS_OF, k)[:3]):
            assert np.array_equal(a, b)


def test_groups():
    # rows 1 and 2 (the duplicates) in one group: neither lists the other any more
    group_of = np.array([0, 1, 1, 2, 3, 4])
    cls, votes, n, first, correct = knn_validate_ref(D, CLASS_OF, (1,), group_of)
    assert cls[0].tolist() == [1, 0, 0, 1, 1, NO] and n[0].tolist() == [2, 1, 1, 2, 1, 0] and first[0][:5].tolist() == [1.0, 1.0, 1.0, 2.0, 7.0]
    assert int(correct[0]) == 3  # rows 2, 3 and 4
    # the same group in another spelling
    again = knn_validate_ref(D, CLASS_OF, (1,), np.array([7, 0, 0, 9, 3, 4]))
    assert all(np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
               for a, b in zip(again, (cls, votes, n, first, correct)))
    # a group for every row is leave-one-out
    alone = knn_validate_ref(D, CLASS_OF, (1, 2, 4), np.arange(6))
    loo = knn_validate_ref(D, CLASS_OF, (1, 2, 4))
    assert all(np.array_equal(a[~np.isnan(a)] if a.dtype == np.float64 else a, b[~np.isnan(b)] if b.dtype == np.float64 else b) for a, b in zip(alone, loo))
    # the whole set in one group: nobody has a list
    cls, votes, n, first, correct = knn_validate_ref(D, CLASS_OF, (1, 4), np.zeros(6, dtype=np.uint32))
    assert np.all(cls == NO) and not votes.any() and not n.any() and np.isnan(first).all() and correct.tolist() == [0, 0]
    # a set of one row
    cls, votes, n, first, correct = knn_validate_ref(np.zeros((1, 1)), [0], (1,))
    assert cls.tolist() == [[NO]] and n.tolist() == [[0]] and correct.tolist() == [0]


def test_confusion_matrix():
    import kpop_amd
    cls, votes, n, first, correct = knn_validate_ref(D, CLASS_OF, (1, 2, 4))
    for t in range(3):
        M = kpop_amd.confusion_matrix(CLASS_OF, cls[t], 2)
        assert M.shape == (2, 3) and M.sum() == 6 and M.trace() == int(correct[t])
        assert M.tolist() == [[0, 2, 1], [1, 2, 0]]  # rows: the true class; the last column: NO_CLASS (row 5)
    assert kpop_amd.confusion_matrix([], [], 3).tolist() == [[0] * 4] * 3
    for bad in (([0, 2], [0, 0], 2), ([0, 1], [0, 5], 2), ([0, 1], [0], 2)):
        with pytest.raises(ValueError):
            kpop_amd.confusion_matrix(*bad)


def test_header_declares_and_library_exports_the_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*knn_(?:ks_vote|validate)[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_knn_vote(") < code.index("kpop_knn_ks_vote(")  # the block after the vote's
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands on, as its neighbours do
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment, name


def test_python_surface():
    import kpop_amd
    for name in ("dev_knn_vote_ks_workspace_bytes", "dev_knn_vote_ks", "dev_knn_validate_workspace_bytes", "dev_knn_validate", "distance_knn_validate",
                 "confusion_matrix"):
        assert callable(getattr(kpop_amd, name)) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.knn_vote_ks) and callable(kpop_amd.RefSet.knn_validate)


def test_the_kernels_are_built_from_their_own_file():
    csrc = os.path.join(ROOT, "kpop_amd", "csrc")
    assert "knn_validate.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "knn_validate.hip")).read()
    for kernel in ("knn_vote_ks_kernel", "knn_correct_kernel"):
        assert "void " + kernel in src
    assert "asm" not in re.sub(r"//.*", "", src)  # plain HIP C++ throughout
    # the kernels that walk the pairs, the merge and the vote stay in knn.hip, one body each for the vote and the leave-out votes
    # (a "who is left out" policy), and are launched from there alone
    vote = open(os.path.join(csrc, "knn.hip")).read()
    for kernel in ("knn_nearest_kernel", "knn_merge_kernel", "knn_ties_kernel", "knn_vote_kernel"):
        assert vote.count("void " + kernel + "(") == 1 and "void " + kernel not in src
        assert kernel + "<" not in src  # neither launched nor instantiated in this translation unit
    assert "KnnvLeftOut" in vote and "KnnNobodyLeftOut" in vote
    assert "knn_run_leave_out_passes(" in src and "knn_run_passes(" in src
    # one tile loop: the reference chain's line stands in pair_tile.h and in neither k-NN file
    assert "__dsub_rn(av[" not in src and "__dsub_rn(av[" not in vote and '#include "pair_tile.h"' in vote
    assert "__dsub_rn(av[" in open(os.path.join(csrc, "pair_tile.h")).read()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    rs.info = lambda: {"r1": 2, "n_dims": 3}
    with pytest.raises(kpop_amd.KPopError):
        rs.knn_vote_ks(np.ones((2, 3)), [0, 1], (1, 2))
    with pytest.raises(kpop_amd.KPopError):
        rs.knn_validate([0, 1], ks=(1,))
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_knn_validate(np.ones((2, 3)), [0, 1], np.ones(3), ks=(1,))
