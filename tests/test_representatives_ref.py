"""CPU tests of the representatives at a distance: the numpy reference (tests/representatives_ref.py) on
hand-made matrices, the claim that the section's invariants determine the result, and the boundary -- include/kpop_hip.h declares the
four functions with the lines of the reference they stand on, the library exports them, the Python table binds them, and the package
offers them (as tests/test_clusters_abi.py does for the clusters)."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from representatives_ref import check_invariants, representatives_ref

FUNCTIONS = ["kpop_representatives_within", "kpop_dev_representatives_within_workspace_bytes", "kpop_dev_representatives_within",
             "kpop_distance_representatives"]
NAN, INF = float("nan"), float("inf")


def lower(entries, r):
    """a matrix with D[j, i] = entries[(j, i)] below the diagonal and a value nobody may read (-7, a hit at every threshold used
    here) on and above it"""
    D = np.full((r, r), -7.0)
    for j in range(r):
        for i in range(j):
            D[j, i] = entries.get((j, i), 9.0)
    return D


def test_the_nearest_earlier_representative_is_not_the_first():
    # rows 0 and 1 apart; row 2 within T of both, nearer to 1
    D = lower({(1, 0): 5.0, (2, 0): 0.9, (2, 1): 0.4}, 3)
    rep_of, rep_dist, n = representatives_ref(D, 1.0)
    assert rep_of.tolist() == [0, 1, 1] and rep_dist.tolist() == [0.0, 0.0, 0.4] and n == 2
    assert rep_of.dtype == np.uint32 and rep_dist.dtype == np.float64


def test_a_later_representative_is_nearer_but_ineligible():
    # row 1 is within T of row 0 at 0.9; row 2 is a representative and lies at 0.1 of row 1: row 1 stays with row 0
    D = lower({(1, 0): 0.9, (2, 0): 5.0, (2, 1): 0.1}, 3)
    rep_of, rep_dist, n = representatives_ref(D, 1.0)
    assert rep_of.tolist() == [0, 0, 2] and rep_dist.tolist() == [0.0, 0.9, 0.0] and n == 2


def test_ties_go_to_the_smaller_index():
    D = lower({(1, 0): 5.0, (2, 0): 5.0, (2, 1): 5.0, (3, 0): 9.0, (3, 1): 0.5, (3, 2): 0.5}, 4)
    rep_of, rep_dist, n = representatives_ref(D, 1.0)
    assert rep_of.tolist() == [0, 1, 2, 1] and rep_dist[3] == 0.5 and n == 3


def test_minus_zero():
    # -0 is taken as +0 in the order (so the tie goes to the smaller index) and written as +0
    D = lower({(1, 0): 5.0, (2, 0): 0.0, (2, 1): -0.0, (3, 0): 5.0, (3, 1): -0.0}, 4)
    rep_of, rep_dist, n = representatives_ref(D, 0.0)
    assert rep_of.tolist() == [0, 1, 0, 1] and n == 2
    assert not np.signbit(rep_dist).any() and rep_dist.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_thresholds_negative_zero_and_infinite():
    D = lower({(1, 0): 0.0, (2, 0): 3.0, (2, 1): 3.0, (3, 0): INF, (3, 1): INF, (3, 2): 4.0, (4, 0): INF, (4, 1): NAN, (4, 2): INF}, 5)
    rep_of, rep_dist, n = representatives_ref(D, -1.0)
    assert rep_of.tolist() == [0, 1, 2, 3, 4] and n == 5 and not rep_dist.any()
    rep_of, rep_dist, n = representatives_ref(D, 0.0)
    assert rep_of.tolist() == [0, 0, 2, 3, 4] and n == 4
    # +inf: a row is a representative iff its distance to every earlier representative is NaN; an infinite distance is a hit
    rep_of, rep_dist, n = representatives_ref(D, INF)
    assert rep_of.tolist() == [0, 0, 0, 0, 0] and n == 1 and rep_dist.tolist() == [0.0, 0.0, 3.0, INF, INF]
    with pytest.raises(ValueError):
        representatives_ref(D, NAN)


def test_a_nan_row_stands_for_itself_alone():
    e = {(j, i): 0.5 for j in range(5) for i in range(j)}
    for k in range(5):
        if k != 2:
            e[(max(k, 2), min(k, 2))] = NAN
    D = lower(e, 5)
    for T in (1.0, INF):
        rep_of, rep_dist, n = representatives_ref(D, T)
        assert rep_of.tolist() == [0, 0, 2, 0, 0] and n == 2 and rep_dist.tolist() == [0.0, 0.5, 0.0, 0.5, 0.5]


def random_matrix(rng, r, levels):
    """a symmetric matrix over a few levels, so that ties and chains are common; a NaN here and there"""
    D = rng.choice(levels, size=(r, r))
    D = np.tril(D, -1)
    D = D + D.T
    return D


def test_known_equals_from_scratch_for_every_prefix_length():
    rng = np.random.RandomState(6)
    for trial in range(20):
        r = 12
        D = random_matrix(rng, r, [0.0, 0.25, 0.5, 1.0, 2.0, NAN])
        for T in (0.25, 0.5, 1.0):
            want = representatives_ref(D, T)
            for n in range(r + 1):
                first = representatives_ref(D[:n, :n], T)
                assert np.array_equal(first[0], want[0][:n])  # the prefix property
                got = representatives_ref(D, T, known=first[0])
                assert np.array_equal(got[0], want[0]) and got[2] == want[2]
                assert np.array_equal(got[1], want[1])


def test_the_lower_triangle_alone_is_read():
    rng = np.random.RandomState(7)
    D = random_matrix(rng, 9, [0.25, 0.5, 1.0, 2.0])
    E = np.tril(D, -1) + np.triu(np.full((9, 9), -7.0))
    for T in (0.25, 0.5, 1.0):
        a, b = representatives_ref(D, T), representatives_ref(E, T)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_the_invariants_determine_the_result():
    """section 6h: any rep_of that satisfies the invariants is the reference's -- by brute force over every candidate (rep_of[i] one of
    0 .. i: 720 of them on 6 rows)"""
    rng = np.random.RandomState(8)
    cases = 0
    for trial in range(6):
        D = random_matrix(rng, 6, [0.0, 0.5, 1.0, 2.0, 3.0] + ([NAN] if trial % 2 else []))
        for T in (0.5, 1.0, 2.0):
            want = representatives_ref(D, T)[0]
            found = [c for c in itertools.product(*[range(i + 1) for i in range(6)]) if check_invariants(D, T, np.array(c))]
            assert found == [tuple(want.tolist())], (trial, T, found, want)
            cases += 1 < int(np.sum(want == np.arange(6))) < 6
    assert cases >= 5  # not all of them trivial


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*representatives[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_knn_validate(") < code.index("kpop_representatives_within(")  # the block after the k-NN validation
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands on, as its neighbours do
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment or "lib/Space.ml:" in comment, name
    # the names stay out of the other blocks' searches
    for name in FUNCTIONS:
        assert not re.search(r"clusters|forest|knn_vote|knn_(ks_vote|validate)|kpop_(dev_)?refset_", name)


def test_python_surface():
    import kpop_amd
    for name in ("distance_representatives", "dev_representatives_within_workspace_bytes", "dev_representatives_within"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.representatives)


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "representatives.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "representatives.hip")).read()
    for kernel in ("representatives_cover_kernel", "representatives_row_min_kernel", "representatives_hits_kernel", "representatives_resolve_kernel"):
        assert "void " + kernel in src
    # no tune key of its own, and none read
    assert "tune" not in re.sub(r"//.*", "", src)
