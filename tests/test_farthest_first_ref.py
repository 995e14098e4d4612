"""CPU tests of the farthest-first traversal: the numpy reference (tests/farthest_first_ref.py) on the
section's worked case and on random matrices held to the section's properties, the edge values, and the boundary -- include/kpop_hip.h
declares the four functions with the lines of the reference they stand on, the library exports them, the Python table binds them, and
the package offers them (as tests/test_representatives_ref.py does for the representatives)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from farthest_first_ref import NOISE, farthest_first_ref

FUNCTIONS = ["kpop_farthest_first", "kpop_dev_farthest_first_workspace_bytes", "kpop_dev_farthest_first", "kpop_distance_farthest_first"]
NAN, INF = float("nan"), float("inf")
X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]  # the ten rows of section 6i


def line_matrix(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_the_worked_case():
    D = line_matrix(X)
    got = farthest_first_ref(D)
    assert got.pick.tolist() == [0, 8, 6, 7, 3, 9, 1, 2, 4, 5]
    assert got.pick_radius.tolist() == [INF, 5.0, 1.5, 0.75, 0.375, 0.375, 0.125, 0.125, 0.125, 0.125]
    assert got.pick_parent.tolist() == [NOISE, 0, 0, 0, 6, 0, 0, 9, 3, 6]
    assert got.rep_of.tolist() == list(range(10)) and not got.rep_dist.any()
    assert got.pick.dtype == np.uint32 and got.pick_radius.dtype == np.float64 and got.pick_parent.dtype == np.uint32
    assert got.rep_of.dtype == np.uint32 and got.rep_dist.dtype == np.float64
    # row 7 lies at exactly .75 from rows 0 and 6: the tie keeps the earlier pick; rows 3 and 9 tie at .375: the smaller row goes first
    cut = farthest_first_ref(D, cover_radius=0.375)
    assert cut.pick.tolist() == [0, 8, 6, 7] and cut.pick_radius.tolist() == [INF, 5.0, 1.5, 0.75]
    assert cut.rep_of.tolist() == [0, 0, 0, 6, 6, 6, 6, 7, 8, 0]
    assert cut.rep_dist.tolist() == [0.0, 0.125, 0.25, 0.375, 0.25, 0.125, 0.0, 0.0, 0.0, 0.375]
    # from the first three picks as seeds: the same run
    assert same(farthest_first_ref(D, seeds=got.pick[:3]), got)
    # other seeds: another run, and the seeds' radii need not fall
    other = farthest_first_ref(D, max_picks=4, seeds=[1, 8, 2])
    assert other.pick.tolist() == [1, 8, 2, 6] and other.pick_radius.tolist() == [INF, 4.875, 0.125, 1.25]
    assert other.pick_parent.tolist() == [NOISE, 1, 1, 2]


def random_matrix(rng, r, levels, nan_rows=()):
    """a symmetric matrix over a few levels, so that ties are common; whole rows and columns of NaN"""
    D = rng.choice(levels, size=(r, r))
    D = np.tril(D, -1)
    D = D + D.T
    for i in nan_rows:
        D[i, :] = NAN
        D[:, i] = NAN
    np.fill_diagonal(D, -7.0)  # (nobody reads it)
    return D


LEVELS = [0.0, -0.0, 0.25, 0.5, 0.5, 1.0, 2.0, INF]


def cases():
    rng = np.random.RandomState(12)
    for trial in range(24):
        r = int(rng.randint(2, 15))
        nan_rows = [] if trial % 3 == 0 else list(rng.choice(r, size=min(r - 1, trial % 3), replace=False))
        levels = LEVELS + ([NAN] if trial % 4 == 3 else [])
        yield trial, random_matrix(rng, r, levels, nan_rows), nan_rows


def test_property_1_the_radii_fall():
    for trial, D, _ in cases():
        for seeds in ([], [D.shape[0] - 1], [1, 0]):
            got = farthest_first_ref(D, seeds=seeds)
            tail = got.pick_radius[max(len(seeds), 1):]
            assert np.all(tail[1:] <= tail[:-1]), (trial, seeds)
            assert got.pick_radius[0] == INF and got.pick_parent[0] == NOISE
            assert sorted(got.pick.tolist()) == list(range(D.shape[0]))  # the full order is a permutation
            assert not np.signbit(got.pick_radius).any() and not np.signbit(got.rep_dist).any()


def test_property_2_prefix():
    for trial, D, _ in cases():
        full = farthest_first_ref(D)
        for k in range(D.shape[0] + 1):
            got = farthest_first_ref(D, max_picks=k)
            assert same(got[:3], [x[:k] for x in full[:3]]), (trial, k)


def test_property_3_continuation():
    for trial, D, _ in cases():
        full = farthest_first_ref(D)
        for k in range(D.shape[0] + 1):
            assert same(farthest_first_ref(D, seeds=full.pick[:k]), full), (trial, k)
        # over a grown set: the old picks as seeds, then on
        r = D.shape[0]
        if r > 4:
            old = farthest_first_ref(D[:r - 2, :r - 2])
            grown = farthest_first_ref(D, seeds=old.pick)
            assert np.array_equal(grown.pick[:r - 2], old.pick) and sorted(grown.pick[r - 2:].tolist()) == [r - 2, r - 1]


def test_property_4_cover_and_packing():
    for trial, D, nan_rows in cases():
        for R in (0.0, 0.25, 0.5, 1.0, 2.0):
            for seeds in ([], [D.shape[0] - 1]):
                got = farthest_first_ref(D, cover_radius=R, seeds=seeds)
                assert np.all((got.rep_dist <= R) | (got.rep_dist == INF)), (trial, R)
                assert np.all(got.pick_radius[len(seeds):] > R), (trial, R)
                free = got.pick[len(seeds):]
                with np.errstate(invalid="ignore"):
                    for a in range(len(got.pick)):
                        for b in free[free != got.pick[a]]:
                            assert not D[b, got.pick[a]] <= R, (trial, R, a, b)
                # maximal: a row that was not picked lies within R of a pick, or has no distance that is a number to any pick
                left = np.setdiff1d(np.arange(D.shape[0]), got.pick)
                for i in left:
                    d = D[i, got.pick]
                    assert np.nanmin(d) <= R if np.any(d == d) else got.rep_of[i] == NOISE, (trial, R, i)


def test_property_5_the_nearest_pick_and_the_first_of_them():
    for trial, D, _ in cases():
        for k in (1, 2, 5):
            got = farthest_first_ref(D, max_picks=k)
            picked = np.zeros(D.shape[0], dtype=bool)
            picked[got.pick] = True
            for i in np.flatnonzero(~picked):
                d = D[i, got.pick] + 0.0
                if not np.any(d == d):
                    assert got.rep_of[i] == NOISE and got.rep_dist[i] == INF
                    continue
                least = np.nanmin(d)
                if least == INF:  # (an infinite distance is a number, but it is not strictly less than the +inf a row starts with)
                    assert got.rep_of[i] == NOISE and got.rep_dist[i] == INF
                    continue
                assert got.rep_dist[i] == least and got.rep_of[i] == got.pick[np.flatnonzero(d == least)[0]], (trial, k, i)
            assert np.array_equal(got.rep_of[picked], np.flatnonzero(picked)) and not got.rep_dist[picked].any()


def test_a_nan_row_is_picked_when_its_index_comes_up():
    e = line_matrix([0.0, 1.0, 3.0, 7.0, 7.5])
    e[2, :] = NAN
    e[:, 2] = NAN
    got = farthest_first_ref(e)
    # row 0; then the only row still at +inf, row 2, which nothing covers; then 4, 1, 3
    assert got.pick.tolist() == [0, 2, 4, 1, 3] and got.pick_radius.tolist() == [INF, INF, 7.5, 1.0, 0.5]
    assert got.pick_parent.tolist() == [NOISE, NOISE, 0, 0, 4]
    cut = farthest_first_ref(e, cover_radius=1.0, seeds=[0])
    assert cut.pick.tolist() == [0, 2, 4] and cut.rep_of.tolist() == [0, 0, 2, 4, 4]


def test_cover_radius_values():
    D = line_matrix(X)
    assert same(farthest_first_ref(D, cover_radius=-1.0), farthest_first_ref(D))
    zero = farthest_first_ref(D, cover_radius=0.0)
    assert len(zero.pick) == 10
    dup = line_matrix(X + [0.25])
    zero = farthest_first_ref(dup, cover_radius=0.0)
    assert len(zero.pick) == 10 and zero.rep_of[10] == 2 and zero.rep_dist[10] == 0.0
    assert same(farthest_first_ref(dup, cover_radius=-0.0), zero)
    # +inf: the first pick's own cover distance is +inf, so without a seed nothing is picked
    none = farthest_first_ref(D, cover_radius=INF)
    assert len(none.pick) == 0 and np.all(none.rep_of == NOISE) and np.all(none.rep_dist == INF)
    one = farthest_first_ref(D, cover_radius=INF, seeds=[4])
    assert one.pick.tolist() == [4] and one.rep_of.tolist() == [4] * 10
    with pytest.raises(ValueError):
        farthest_first_ref(D, cover_radius=NAN)


def test_max_picks_values():
    D = line_matrix(X)
    none = farthest_first_ref(D, max_picks=0)
    assert len(none.pick) == 0 and np.all(none.rep_of == NOISE) and np.all(none.rep_dist == INF)
    one = farthest_first_ref(D, max_picks=1)
    assert one.pick.tolist() == [0] and one.rep_of.tolist() == [0] * 10 and np.array_equal(one.rep_dist, np.array(X))
    assert same(farthest_first_ref(D, max_picks=10), farthest_first_ref(D, max_picks=1000))
    empty = farthest_first_ref(np.zeros((0, 0)), max_picks=5)
    assert len(empty.pick) == 0 and len(empty.rep_of) == 0


def test_seeds_that_are_refused():
    D = line_matrix(X)
    for seeds, max_picks in (([1, 1], 10), ([10], 10), ([-1], 10), ([0, 1, 2], 2)):
        with pytest.raises(ValueError):
            farthest_first_ref(D, max_picks=max_picks, seeds=seeds)


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*farthest_first[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_silhouette_summary(") < min(code.index(name + "(") for name in FUNCTIONS)  # the block after the silhouette
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
        assert not re.search(r"representatives|forest|clusters|dbscan|reachability|core_distances|silhouette|knn|within|kpop_(dev_)?refset_", name)


def test_python_surface():
    import kpop_amd
    from kpop_amd import api
    for name in ("FarthestFirst", "distance_farthest_first", "dev_farthest_first_workspace_bytes", "dev_farthest_first"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__ and hasattr(api, name)
    assert callable(kpop_amd.RefSet.farthest_first)
    assert kpop_amd.FarthestFirst._fields == ("pick", "pick_radius", "pick_parent", "rep_of", "rep_dist", "n_passes")


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "farthest_first.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "farthest_first.hip")).read()
    for kernel in ("farthest_first_pass_kernel", "farthest_first_resolve_kernel"):
        assert "void " + kernel in src
    code = re.sub(r"//.*", "", src)
    assert "tune" not in code and "asm" not in code and "atomic" not in code  # no knob, no inline assembly, no atomics
