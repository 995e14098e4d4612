"""CPU tests of the range query: the numpy reference the GPU tests compare with (tests/within_ref.py), and the boundary -- the header
declares the four functions, the library exports them, the Python table binds them, and without a GPU a query fails (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from within_ref import rows_of, within_ref

FUNCTIONS = ["kpop_neighbours_within", "kpop_dev_neighbours_within_workspace_bytes", "kpop_dev_neighbours_within", "kpop_distance_within"]


def test_reference_by_hand():
    """3 x 5: a tie (row 0: columns 1 and 3), a -0 beside a +0 (row 1: ordered by column, the sign kept), a NaN (row 2: never a hit)"""
    nan, inf = float("nan"), float("inf")
    D = np.array([[0.5, 0.25, 2.0, 0.25, 1.0],
                  [0.0, 3.0, -0.0, 1.5, 0.0],
                  [nan, 1.0, inf, 0.75, nan]])
    offsets, idx, dist = within_ref(D, 1.0)
    assert offsets.dtype == np.uint64 and idx.dtype == np.uint32 and dist.dtype == np.float64
    assert offsets.tolist() == [0, 4, 7, 9]
    assert idx.tolist() == [1, 3, 0, 4, 0, 2, 4, 3, 1]
    assert dist.tolist() == [0.25, 0.25, 0.5, 1.0, 0.0, 0.0, 0.0, 0.75, 1.0]
    assert np.signbit(dist[4:7]).tolist() == [False, True, False]  # the distances keep their bits
    # the inclusive boundary, an empty result, everything that is a number
    assert within_ref(D, 0.25)[0].tolist() == [0, 2, 5, 5] and within_ref(D, 0.25)[1].tolist() == [1, 3, 0, 2, 4]
    assert within_ref(D, -1.0)[0].tolist() == [0, 0, 0, 0] and within_ref(D, -1.0)[1].size == 0
    assert within_ref(D, 0.0)[1].tolist() == [0, 2, 4]  # -0 <= 0
    full = within_ref(D, inf)
    assert full[0].tolist() == [0, 5, 10, 13] and full[1][10:].tolist() == [3, 1, 2]
    assert within_ref(np.zeros((0, 5)), 1.0)[0].tolist() == [0] and within_ref(np.zeros((2, 0)), 1.0)[0].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        within_ref(D, nan)


def test_reference_on_the_readme_row():
    """the ten distances of README.md:645-649: cut between the 2nd and the 3rd smallest, the list is the summary row's two neighbours"""
    kat = load_golden("readme_kat.json")
    row = np.array([[float(x) for x in kat["distance_row_text"]]])
    by_distance = np.sort(row[0])
    T = (by_distance[1] + by_distance[2]) / 2
    (idx, dist), = rows_of(within_ref(row, T))
    want = kat["summary_line"].split("\t")
    assert ['"%s"' % kat["distance_header"][i] for i in idx] == [want[5], want[8]]
    assert dist.tolist() == [float(want[6]), float(want[9])]


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, code), "include/kpop_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands in for
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment, name
    assert not any(re.match(r"kpop_(dev_)?refset_", name) for name in FUNCTIONS)  # (that family stays its ten functions)


def test_python_surface():
    import kpop_amd
    for name in ("dev_neighbours_within_workspace_bytes", "dev_neighbours_within", "distance_within"):
        assert callable(getattr(kpop_amd, name)) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.within)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    rs = kpop_amd.RefSet.__new__(kpop_amd.RefSet)  # (a set cannot be made without a GPU: the call on no set at all)
    rs._h, rs._keep = None, None
    with pytest.raises(kpop_amd.KPopError):
        rs.within(np.ones((2, 3)), 1.0)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_within(np.ones((2, 3)), np.ones((2, 3)), np.ones(3), 1.0)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_within(np.ones((2, 3)), np.ones((2, 3)), np.ones(3), 1.0, capacity=4)
