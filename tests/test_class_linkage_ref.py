"""CPU tests of the class linkage's declared semantics: the worked case against both references of
tests/class_linkage_ref.py, the line reference against the matrix reference, and kpop_class_tree -- host arithmetic inside the library,
no GPU -- against the reference tree: merges, ties, empty classes, forests, the error codes, monotone heights, what an average-linkage
height is, and the Newick strings."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from class_linkage_ref import (LINK_AVERAGE, LINK_COMPLETE, LINK_SINGLE, NAMES, NO_CLASS, QNAN_BITS, class_linkage_ref, class_tree_ref, leaves_under,
                               line_linkage_ref, same_bits)
from conftest import ROOT

LINKAGES = (LINK_SINGLE, LINK_COMPLETE, LINK_AVERAGE)
ERR_INVALID, ERR_UNSUPPORTED = -1, -3

# ten rows on a line, three classes of three rows, row 8 left out, class 3 empty
HAND_X = [0.0, 4.0, 0.5, 10.0, 1.0, 4.5, 11.0, 6.0, 2.0, 13.0]
HAND_CLASS = [0, 1, 0, 2, 0, 1, 2, 1, NO_CLASS, 2]
HAND_N = 4
HAND_ROWS = [3, 3, 3, 0]
N = float("nan")
HAND_MEAN = [[2 / 3, 39 / 9, 97.5 / 9, N], [39 / 9, 4 / 3, 6.5, N], [97.5 / 9, 6.5, 2.0, N], [N, N, N, N]]
HAND_MIN = [[0.5, 3.0, 9.0, N], [3.0, 0.5, 4.0, N], [9.0, 4.0, 1.0, N], [N, N, N, N]]
HAND_MAX = [[1.0, 6.0, 13.0, N], [6.0, 2.0, 9.0, N], [13.0, 9.0, 3.0, N], [N, N, N, N]]
X = NO_CLASS
HAND_MIN_I = [[0, 1, 3, X], [1, 1, 3, X], [3, 3, 3, X], [X, X, X, X]]
HAND_MIN_J = [[2, 4, 4, X], [4, 5, 7, X], [4, 7, 6, X], [X, X, X, X]]
# the trees: (left, right, height, size) a merge; class 3 is no leaf, merge t makes node 4 + t
HAND_TREES = {LINK_SINGLE: ([0, 2], [1, 4], [3.0, 4.0], [6, 9]), LINK_COMPLETE: ([0, 2], [1, 4], [6.0, 13.0], [6, 9]),
              LINK_AVERAGE: ([0, 2], [1, 4], [39 / 9, (3.0 * (97.5 / 9) + 3.0 * 6.5) / 6.0], [6, 9])}


def line_matrix(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(np.subtract.outer(x, x))


def check_tables(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name)
        if w.dtype == np.float64:
            assert same_bits(g, w), (what, name, g, w)
        else:
            assert np.array_equal(g, w), (what, name, g, w)


def check_tree(got, want, what):
    for name, g, w in zip(("left", "right", "height", "size"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g, w)
        if name == "height":
            assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), np.ascontiguousarray(w, dtype=np.float64).view(np.uint64)), (what, name, g, w)
        else:
            assert g.dtype == np.uint32 and np.array_equal(g, w), (what, name, g, w)


def test_the_worked_case_in_both_references():
    hand = (np.array(HAND_ROWS, dtype=np.uint32), np.array(HAND_MEAN), np.array(HAND_MIN), np.array(HAND_MAX), np.array(HAND_MIN_I, dtype=np.uint32),
            np.array(HAND_MIN_J, dtype=np.uint32))
    by_matrix = class_linkage_ref(line_matrix(HAND_X), HAND_CLASS, HAND_N)
    by_line = line_linkage_ref(HAND_X, HAND_CLASS, HAND_N)
    check_tables(by_matrix, hand, "the matrix reference")
    check_tables(by_line, hand, "the line reference")
    for t in by_matrix[1:4]:  # the declared NaN, not any NaN
        assert np.all(t[3].view(np.uint64) == QNAN_BITS) and np.all(t[:, 3].view(np.uint64) == QNAN_BITS)


def test_the_worked_case_trees():
    import kpop_amd
    tables = class_linkage_ref(line_matrix(HAND_X), HAND_CLASS, HAND_N)
    for linkage, table in ((LINK_SINGLE, tables[2]), (LINK_COMPLETE, tables[3]), (LINK_AVERAGE, tables[1])):
        want = HAND_TREES[linkage]
        check_tree(class_tree_ref(tables[0], table, linkage), want, ("reference", linkage))
        got = kpop_amd.class_tree(tables[0], table, linkage)
        assert isinstance(got, kpop_amd.ClassTree) and got._fields == ("left", "right", "height", "size")
        check_tree(got, want, ("library", linkage))
    # UPGMA's root: the mean over the 18 pairs of a row of classes 0 and 1 and a row of class 2
    assert abs(HAND_TREES[LINK_AVERAGE][2][1] - 156 / 18) <= 4 * 2.0 ** -53 * 156 / 18


def test_line_reference_against_matrix_reference():
    rng = np.random.RandomState(6)
    for n, n_classes, below in ((200, 5, 8192), (200, 7, 24), (60, 9, 8192)):  # (below 24: duplicates, ties in every least pair)
        x = rng.randint(0, below, size=n) / 8.0
        class_of = rng.choice(np.array(list(range(n_classes - 1)) + [NO_CLASS], dtype=np.uint32), size=n)  # (the last class stays empty)
        check_tables(line_linkage_ref(x, class_of, n_classes), class_linkage_ref(line_matrix(x), class_of, n_classes), (n, n_classes, below))


def random_table(rng, n):
    d = rng.uniform(0.5, 9.0, size=(n, n))
    d = np.triu(d, 1)
    return d + d.T


@pytest.mark.parametrize("n_classes", [2, 3, 17, 200])
def test_tree_against_reference(n_classes):
    import kpop_amd
    rng = np.random.RandomState(n_classes)
    rows = rng.randint(1, 40, size=n_classes).astype(np.uint32)
    d = random_table(rng, n_classes)
    for linkage in LINKAGES:
        got = kpop_amd.class_tree(rows, d, linkage)
        check_tree(got, class_tree_ref(rows, d, linkage), (n_classes, linkage))
        assert len(got.left) == n_classes - 1 and got.size[-1] == rows.sum()
        assert np.all(got.left < got.right) and np.all(np.diff(got.height) >= 0)  # reducible: monotone heights
        # only the entries a < b are read: the lower triangle and the diagonal may hold anything
        junk = np.triu(d, 1) + np.tril(np.full((n_classes, n_classes), np.nan))
        check_tree(kpop_amd.class_tree(rows, junk, linkage), got, (n_classes, linkage, "upper triangle alone"))


def test_tree_ties_empty_classes_and_forests():
    import kpop_amd
    # every distance the same: the lower ids win, the new node has the highest id
    d = np.full((4, 4), 2.0)
    for linkage in LINKAGES:
        got = kpop_amd.class_tree([1, 1, 1, 1], d, linkage)
        check_tree(got, class_tree_ref([1, 1, 1, 1], d, linkage), linkage)
        assert got.height.tolist() == [2.0] * 3 and got.left.tolist() == [0, 2, 4] and got.right.tolist() == [1, 3, 5] and got.size.tolist() == [2, 2, 4]
    # a tie between (1, 2) and (0, 3): the lower first id wins; -0 is +0, so (0, 3) at -0 ties with (1, 2) at +0 and still wins
    d = np.array([[0, 5, 5, -0.0], [5, 0, 0.0, 5], [5, 0.0, 0, 5], [-0.0, 5, 5, 0]])
    got = kpop_amd.class_tree([2, 1, 1, 3], d, LINK_SINGLE)
    assert got.left.tolist() == [0, 1, 4] and got.right.tolist() == [3, 2, 5] and got.size.tolist() == [5, 2, 7]
    assert got.height.tolist() == [0.0, 0.0, 5.0] and not np.signbit(got.height[0])
    check_tree(got, class_tree_ref([2, 1, 1, 3], d, LINK_SINGLE), "signed zeros")
    # empty classes are no leaves: their entries (NaN here, as kpop_class_linkage writes them) are never read
    rng = np.random.RandomState(4)
    d = random_table(rng, 6)
    rows = np.array([3, 0, 2, 0, 0, 7], dtype=np.uint32)
    d[rows == 0, :] = np.nan
    d[:, rows == 0] = np.nan
    for linkage in LINKAGES:
        got = kpop_amd.class_tree(rows, d, linkage)
        check_tree(got, class_tree_ref(rows, d, linkage), ("empty classes", linkage))
        assert len(got.left) == 2 and set(got.left.tolist() + got.right.tolist()) == {0, 2, 5, 6} and got.size[-1] == 12
    # a NaN between two groups: the merges stop, a forest of two roots; NaN poisons what it is merged into
    d = np.array([[0, 1.0, N, N], [1.0, 0, N, N], [N, N, 0, 3.0], [N, N, 3.0, 0]])
    for linkage in LINKAGES:
        got = kpop_amd.class_tree([1, 2, 3, 4], d, linkage)
        check_tree(got, ([0, 2], [1, 3], [1.0, 3.0], [3, 7]), ("forest", linkage))
    d = np.array([[0, 1.0, 2.0], [1.0, 0, N], [2.0, N, 0]])
    for linkage in LINKAGES:
        got = kpop_amd.class_tree([1, 1, 1], d, linkage)
        check_tree(got, ([0], [1], [1.0], [2]), ("a NaN operand", linkage))
        check_tree(got, class_tree_ref([1, 1, 1], d, linkage), ("a NaN operand, reference", linkage))
    # every distance a NaN; one class; one class with rows among several
    assert len(kpop_amd.class_tree([1, 1], np.full((2, 2), N), LINK_AVERAGE).left) == 0
    assert len(kpop_amd.class_tree([5], np.zeros((1, 1)), LINK_SINGLE).left) == 0
    assert len(kpop_amd.class_tree([0, 5, 0], np.zeros((3, 3)), LINK_COMPLETE).left) == 0


def raw_tree(n_classes, rows, dist, linkage, outs=True):
    from kpop_amd import _lib
    n = max(n_classes, 2) - 1
    left, right, size = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    height = np.zeros(n)
    n_merges = C.c_uint32(77)
    u32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    f64 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    if outs:
        return _lib.load().kpop_class_tree(n_classes, u32(rows), f64(dist), linkage, C.byref(n_merges), u32(left), u32(right), f64(height), u32(size)), n_merges.value
    return _lib.load().kpop_class_tree(n_classes, u32(rows), f64(dist), linkage, C.byref(n_merges), None, None, None, None), n_merges.value


def test_tree_arguments():
    import kpop_amd
    rows, d = np.array([1, 2, 3], dtype=np.uint32), random_table(np.random.RandomState(1), 3)
    assert raw_tree(3, rows, d, LINK_AVERAGE) == (0, 2)
    for linkage in (-1, 3, 99):
        assert raw_tree(3, rows, d, linkage)[0] == ERR_INVALID
        with pytest.raises(kpop_amd.KPopError) as e:
            kpop_amd.class_tree(rows, d, linkage)
        assert e.value.code == ERR_INVALID and "kpop_class_tree" in str(e.value)
    assert raw_tree(0, rows, d, LINK_SINGLE)[0] == ERR_INVALID
    assert raw_tree(4097, rows, d, LINK_SINGLE)[0] == ERR_UNSUPPORTED
    assert raw_tree(3, None, d, LINK_SINGLE)[0] == ERR_INVALID and raw_tree(3, rows, None, LINK_SINGLE)[0] == ERR_INVALID
    assert raw_tree(3, rows, d, LINK_SINGLE, outs=False)[0] == ERR_INVALID
    assert raw_tree(1, rows, d, LINK_SINGLE, outs=False) == (0, 0)  # one class: nothing to write
    from kpop_amd import _lib
    assert _lib.load().kpop_class_tree(3, rows.ctypes.data_as(C.POINTER(C.c_uint32)), d.ctypes.data_as(C.POINTER(C.c_double)), 0, None, None, None, None,
                                       None) == ERR_INVALID
    with pytest.raises(ValueError):
        kpop_amd.class_tree(rows, d[:2], LINK_SINGLE)
    with pytest.raises(kpop_amd.KPopError) as e:
        kpop_amd.class_tree(np.zeros(0, dtype=np.uint32), np.zeros((0, 0)), LINK_SINGLE)
    assert e.value.code == ERR_INVALID


def test_average_heights_are_means_over_row_pairs():
    """UPGMA over classes weighted by their rows is UPGMA over the rows' cross pairs: a node's height is the mean of d over the pairs of a
    row under its left and a row under its right child.  Each Lance-Williams level adds the rounding of a weighted mean of two values
    that carry their own (four roundings, none amplified: every term is positive), on top of the two of a table entry -- well inside
    (N + 2) 2^-53 relative a level, N the pairs under the node; at the first level the height IS the table's entry"""
    import kpop_amd
    rng = np.random.RandomState(12)
    r1, n_classes = 160, 11
    pts = rng.normal(size=(r1, 3)) + 6.0 * rng.normal(size=(n_classes, 3))[rng.randint(0, n_classes, size=r1)]
    D = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    class_of = rng.randint(0, n_classes, size=r1).astype(np.uint32)
    rows, mean = class_linkage_ref(D, class_of, n_classes)[:2]
    tree = kpop_amd.class_tree(rows, mean, LINK_AVERAGE)
    assert len(tree.left) == n_classes - 1
    under = leaves_under(tree.left, tree.right, n_classes)
    level = {c: 0 for c in range(n_classes)}
    for t, (a, b) in enumerate(zip(tree.left, tree.right)):
        level[n_classes + t] = 1 + max(level[int(a)], level[int(b)])
        ia, ib = np.flatnonzero(np.isin(class_of, under[int(a)])), np.flatnonzero(np.isin(class_of, under[int(b)]))
        n_pairs = len(ia) * len(ib)
        want = math.fsum(D[np.ix_(ia, ib)].ravel()) / n_pairs
        bound = level[n_classes + t] * (n_pairs + 2) * 2.0 ** -53
        assert abs(tree.height[t] - want) <= bound * want, (t, tree.height[t], want, bound)
        assert tree.size[t] == len(ia) + len(ib)
    assert np.all(np.diff(tree.height) >= 0)


def test_newick():
    import kpop_amd
    tree = kpop_amd.ClassTree(np.array([0, 2], dtype=np.uint32), np.array([1, 4], dtype=np.uint32), np.array([3.0, 4.5]), np.array([6, 9], dtype=np.uint32))
    assert kpop_amd.class_tree_newick(tree, 4) == ["(2:4.5,(0:3.0,1:3.0):1.5);"]  # (the left child, the lower id, first)
    assert kpop_amd.class_tree_newick(tree, 4, names=["a", "b", "c", "d"]) == ["(c:4.5,(a:3.0,b:3.0):1.5);"]
    # a forest: a string a root, in ascending node id; a class that no merge names is not written
    forest = kpop_amd.ClassTree(np.array([0, 2], dtype=np.uint32), np.array([1, 3], dtype=np.uint32), np.array([1.0, 0.25]), np.array([3, 7], dtype=np.uint32))
    assert kpop_amd.class_tree_newick(forest, 5) == ["(0:1.0,1:1.0);", "(2:0.25,3:0.25);"]
    assert kpop_amd.class_tree_newick(kpop_amd.ClassTree(*[np.zeros(0)] * 4), 3) == []
    # the worked case's UPGMA tree
    tables = class_linkage_ref(line_matrix(HAND_X), HAND_CLASS, HAND_N)
    upgma = kpop_amd.class_tree(tables[0], tables[1], LINK_AVERAGE)
    h0, h1 = HAND_TREES[LINK_AVERAGE][2]
    assert kpop_amd.class_tree_newick(upgma, HAND_N) == ["(2:%r,(0:%r,1:%r):%r);" % (h1, h0, h0, h1 - h0)]
    # a chain as deep as the class limit allows: merge t >= 1 joins class t + 1 to the node before
    n = 4096
    chain = kpop_amd.ClassTree(np.array([0] + list(range(2, n)), dtype=np.uint32), np.array([1] + list(range(n, 2 * n - 2)), dtype=np.uint32),
                               np.arange(1, n, dtype=np.float64), np.arange(2, n + 1, dtype=np.uint32))
    (text,) = kpop_amd.class_tree_newick(chain, n)
    assert text.count("(") == n - 1 and text.startswith("(%d:%r,(" % (n - 1, float(n - 1))) and text.endswith("(0:1.0,1:1.0)" + ":1.0)" * (n - 2) + ";")
    with pytest.raises(ValueError):
        kpop_amd.class_tree_newick(kpop_amd.ClassTree([3], [1], [1.0], [2]), 4)
    with pytest.raises(ValueError):
        kpop_amd.class_tree_newick(tree, 4, names=["a"])


NEW_FUNCTIONS = ("kpop_class_linkage", "kpop_dev_class_linkage_workspace_bytes", "kpop_dev_class_linkage", "kpop_distance_class_linkage", "kpop_class_tree")


def test_surface():
    import kpop_amd
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for k, name in enumerate(("KPOP_LINK_SINGLE", "KPOP_LINK_COMPLETE", "KPOP_LINK_AVERAGE")):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, k), code), name
    assert (kpop_amd.LINK_SINGLE, kpop_amd.LINK_COMPLETE, kpop_amd.LINK_AVERAGE) == (LINK_SINGLE, LINK_COMPLETE, LINK_AVERAGE) == (0, 1, 2)
    for name in ("ClassLinkage", "distance_class_linkage", "dev_class_linkage_workspace_bytes", "dev_class_linkage", "ClassTree", "class_tree",
                 "class_tree_newick"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__, name
    assert callable(kpop_amd.RefSet.class_linkage)
    assert kpop_amd.ClassLinkage._fields == NAMES and kpop_amd.ClassTree._fields == ("left", "right", "height", "size")
