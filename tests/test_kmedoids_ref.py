"""tests/kmedoids_ref.py held to INTEGRATION.md section 6m: the worked case value for value, the properties that do not need the GPU
(consistency, continuation, the cost never increasing, renumbering) on random dyadic 1-D sets -- every distance and every sum exact --
and the argument errors; and the ABI of the block.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from kmedoids_ref import NO_CLASS, assign_ref, cost_ref, kmedoids_ref, own_means_ref, update_ref

WORKED = [0, .125, .25, 1.125, 1.25, 1.375, 1.5, .75, 5, .375]  # the ten rows of section 6i, their first coordinate


def line(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, fields=("medoid", "class_of", "dist", "own_mean", "class_rows", "converged")):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            if x.dtype == np.float64:
                if not (np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(bits(x[~np.isnan(x)]), bits(y[~np.isnan(y)]))):
                    return False
            elif not np.array_equal(x, y):
                return False
        elif x != y:
            return False
    return True


def dyadic_sets(n_sets, seed):
    """1-D sets of up to 200 rows on a grid of 1/64 in clumps: every distance and every sum of up to 200 of them is exact"""
    rng = np.random.RandomState(seed)
    for _ in range(n_sets):
        r = int(rng.randint(1, 201))
        centres = rng.randint(0, 64, size=max(1, r // 12)) * 4.0
        x = centres[rng.randint(len(centres), size=r)] + rng.randint(-32, 33, size=r) / 64.0
        k = int(rng.randint(1, min(r, 12) + 1))
        init = rng.permutation(r)[:k]
        yield x, init


def test_worked_case():
    """Section 6m's worked case.  Round 1 finds the medoids 2, 8, 4 a fixed point -- the labelling did not move, so neither do the means --
    and the loop compares before it looks at max_iter: max_iter = 1 already reports converged, as max_iter = 0 from 2, 8, 4 does
    (continuation, property 3, needs the two to agree)."""
    D = line(WORKED)
    init = [0, 8, 6]
    L, d = assign_ref(D, init)
    assert L.tolist() == [0, 0, 0, 2, 2, 2, 2, 0, 1, 0]
    assert cost_ref(L, d) == 2.25
    own, rows = own_means_ref(D, L, 3)
    assert rows.tolist() == [5, 1, 4]
    assert [own[m] for m in (2, 8, 4)] == [.25, 0.0, 1 / 6]  # round 0's own means of the rows the update takes: the least of their classes
    assert own[0] == .375 and own[6] == .25
    run0 = kmedoids_ref(D, init, 0)
    assert run0.medoid.tolist() == init and run0.n_iter == 0 and not run0.converged and run0.cost.tolist() == [2.25]
    assert update_ref(run0.own_mean, run0.class_of, init) == [2, 8, 4]  # row 4 on a tie with row 5
    assert run0.own_mean[4] == run0.own_mean[5]
    run1 = kmedoids_ref(D, init, 1)
    assert run1.medoid.tolist() == [2, 8, 4] and run1.n_iter == 1 and run1.converged
    assert kmedoids_ref(D, [2, 8, 4], 0).converged
    assert run1.class_of.tolist() == L.tolist()
    assert run1.dist.tolist() == [.25, .125, 0, .125, 0, .125, .25, .5, 0, .125]
    assert run1.cost.tolist() == [2.25, 1.5]
    for max_iter in (2, 3, 100):
        run = kmedoids_ref(D, init, max_iter)
        assert run.n_iter == 1 and run.converged and same(run, run1, ("medoid", "class_of", "dist", "own_mean", "class_rows"))
        assert run.cost.tolist() == [2.25, 1.5]


def test_consistency_and_cost():
    """properties 2 and 4: what is returned is the assignment to medoid[] and that labelling's means; cost never increases, bit for bit"""
    worst = 0
    for x, init in dyadic_sets(60, 1):
        D = line(x)
        got = kmedoids_ref(D, init, 100)
        assert got.converged
        worst = max(worst, got.n_iter)
        L, d = assign_ref(D, got.medoid)
        own, rows = own_means_ref(D, L, len(init))
        assert np.array_equal(L, got.class_of) and np.array_equal(bits(d), bits(got.dist))
        assert np.array_equal(bits(own), bits(got.own_mean)) and np.array_equal(rows, got.class_rows)
        assert update_ref(own, L, got.medoid.tolist()) == got.medoid.tolist()  # a fixed point
        assert len(got.cost) == got.n_iter + 1 and np.all(got.cost[1:] <= got.cost[:-1]), got.cost
        assert got.cost[-1] == math.fsum(got.dist)
        assert np.all(got.class_of[got.medoid] == np.arange(len(init))) and not got.dist[got.medoid].any() and rows.min() >= 1
    assert worst <= 100


def test_continuation():
    """property 3: a rounds, then b rounds from its medoid[], is a + b rounds; the cost is the first run's followed by the second's from 1"""
    for x, init in dyadic_sets(40, 2):
        D = line(x)
        full = kmedoids_ref(D, init, 100)
        for a in range(0, full.n_iter + 2):
            first = kmedoids_ref(D, init, a)
            for b in (0, 1, 100):
                second = kmedoids_ref(D, first.medoid, b)
                whole = kmedoids_ref(D, init, a + b)
                assert same(second, whole), (a, b)
                assert np.array_equal(bits(np.concatenate([first.cost, second.cost[1:]])), bits(whole.cost)), (a, b)
                assert first.n_iter + second.n_iter == whole.n_iter


def test_renumbering():
    """property 6: permuting init permutes medoid / class_rows and relabels class_of; dist keeps its bits, own_mean too where no row is
    equidistant from two medoids"""
    rng = np.random.RandomState(3)
    for x, init in dyadic_sets(40, 4):
        D = line(x)
        k = len(init)
        perm = rng.permutation(k)
        for max_iter in (0, 1, 100):
            a, b = kmedoids_ref(D, init, max_iter), kmedoids_ref(D, np.asarray(init)[perm], max_iter)
            # an assignment tie anywhere along either run moves a row with the numbering: such a case says nothing
            tie = False
            for run in (a, b):
                for t in range(run.n_iter + 1):
                    M = kmedoids_ref(D, init if run is a else np.asarray(init)[perm], t).medoid
                    d = np.sort(D[:, M], axis=1)
                    rest = np.setdiff1d(np.arange(len(x)), M)
                    tie |= k > 1 and bool(np.any(d[rest, 0] == d[rest, 1]))
            if tie:
                assert max_iter > 0 or np.array_equal(bits(a.dist), bits(b.dist))  # dist keeps its bits whatever the ties
                continue
            assert np.array_equal(a.medoid[perm], b.medoid) and np.array_equal(a.class_rows[perm], b.class_rows)
            inv = np.empty(k, dtype=np.int64)
            inv[perm] = np.arange(k)
            assert np.array_equal(inv[a.class_of], b.class_of)
            assert np.array_equal(bits(a.dist), bits(b.dist)) and np.array_equal(bits(a.own_mean), bits(b.own_mean))
            assert a.n_iter == b.n_iter and a.converged == b.converged and np.array_equal(bits(a.cost), bits(b.cost))


def test_left_out_and_duplicates():
    D = line([0, 1, 1, 3, 7, 0]).copy()
    D[4, :] = D[:, 4] = np.nan  # row 4 has no distance that is a number
    got = kmedoids_ref(D, [1, 2], 0)  # row 2 is a duplicate of row 1 and a medoid itself: it keeps its own position
    assert got.class_of.tolist() == [0, 0, 1, 0, NO_CLASS, 0] and got.class_rows.tolist() == [4, 1]
    assert got.dist[4] == np.inf and np.isnan(got.own_mean[4]) and got.own_mean[2] == 0.0
    assert got.cost[-1] == math.fsum(got.dist[[0, 1, 2, 3, 5]])
    alone = kmedoids_ref(D, [4, 0], 5)  # a NaN row as a medoid: a class of one
    assert alone.class_of[4] == 0 and alone.class_rows[0] == 1 and alone.medoid[0] == 4 and alone.dist[4] == 0.0


def test_arguments():
    D = line([0, 1, 2, 3])
    for init in ([], [0, 1, 2, 3, 0], [4], [1, 1], None):
        with pytest.raises(ValueError):
            kmedoids_ref(D, init, 3)
    everyone = kmedoids_ref(D, [3, 2, 1, 0], 3)  # k == r: all singletons, a fixed point at once
    assert everyone.converged and everyone.n_iter == 0 and everyone.class_of.tolist() == [3, 2, 1, 0] and not everyone.dist.any()
    assert everyone.cost.tolist() == [0.0] and not everyone.own_mean.any()


FUNCTIONS = ["kpop_kmedoids", "kpop_dev_kmedoids_workspace_bytes", "kpop_dev_kmedoids", "kpop_distance_kmedoids"]
KERNELS = ["kmedoids_assign_kernel", "kmedoids_merge_kernel", "kmedoids_cost_kernel", "kmedoids_own_kernel", "kmedoids_rows_kernel", "kmedoids_medoid_kernel",
           "kmedoids_update_kernel", "kmedoids_finish_kernel"]


def test_header_declares_and_library_exports_the_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*kmedoids[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_farthest_first(") < code.index("kpop_kmedoids(")  # the block after the farthest-first traversal
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Space.ml:182-205" in comment or "lib/Matrix.ml:191-266" in comment, name  # which lines of the reference it stands on


def test_python_surface():
    import kpop_amd
    for name in ("distance_kmedoids", "dev_kmedoids_workspace_bytes", "dev_kmedoids", "KMedoids"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.kmedoids)
    assert kpop_amd.KMedoids._fields == ("medoid", "class_of", "dist", "own_mean", "class_rows", "cost", "n_iter", "converged")
    for bad in ([[0, 1]], [-1], [2 ** 32]):
        with pytest.raises(ValueError):
            kpop_amd.distance_kmedoids(np.zeros((3, 2)), np.ones(2), bad)
    with pytest.raises(ValueError):
        kpop_amd.distance_kmedoids(np.zeros((3, 2)), np.ones(2), [0], max_iter=-1)


def test_the_kernels_are_built_from_their_own_file():
    csrc = os.path.join(ROOT, "kpop_amd", "csrc")
    assert "kmedoids.hip" in open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "kmedoids.hip")).read()
    for kernel in KERNELS:
        assert kernel in src
    # gathered operands through the sweep of pair_tile.h, both kernels: its steps and the chain stand there and not here
    assert src.count("pair_sweep_tile<KIND>(") >= 2 and src.count("PairRowsAt") >= 2 and "reduce_row_lanes" in src
    assert "load_indexed" not in src and "stage.store(" not in src and "pair_accumulate<" not in src
    assert "pair_accumulate<KIND>(" in open(os.path.join(csrc, "pair_tile.h")).read()
    assert "atomicAdd(double" not in src and "unsafeAtomicAdd" not in src  # no floating-point atomic
    # the grouping is written once: both files take it from the header
    for name in ("kmedoids.hip", "silhouette.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "class_tiles.h"' in text and "class_tiles_group(" in text and "__global__ __launch_bounds__(256) void silhouette_keys_kernel" not in text
