"""CPU tests of the numpy reference of the single-linkage tree (tests/forest_ref.py): on small graphs full of ties it finds the least
spanning forest of an exhaustive enumeration, on larger ones what Kruskal's algorithm finds, and cutting its forest at any threshold
gives the clusters at that threshold (tests/clusters_ref.py)."""
import itertools

import numpy as np
import pytest

from clusters_ref import clusters_ref
from forest_ref import cut_ref, forest_ref

INF = float("inf")


def symmetric(lower):
    """a full matrix from its lower triangle; the upper one is poisoned, to show that nobody reads it"""
    D = np.tril(lower, -1)
    return D + np.triu(np.full(D.shape, -7.0), 0)


def tied_matrix(n, seed, top=3):
    rng = np.random.RandomState(seed)
    return symmetric(rng.randint(1, top + 1, size=(n, n)).astype(np.float64))


def allowed_edges(D, max_distance):
    n = D.shape[0]
    with np.errstate(invalid="ignore"):
        return [(float(D[j, i]) + 0.0, i, j) for i in range(n) for j in range(i + 1, n) if D[j, i] <= max_distance]


def kruskal(D, max_distance):
    """the second, independent algorithm: the edges in the order, each kept iff it joins two trees"""
    n = D.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    kept = []
    for d, i, j in sorted(allowed_edges(D, max_distance)):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.append((d, i, j))
    return kept


def exhaustive(D, max_distance):
    """of all spanning forests -- acyclic sets of n - (components) allowed edges -- the one whose sorted list of keys is least"""
    n = D.shape[0]
    edges = sorted(allowed_edges(D, max_distance))
    size = len(kruskal(D, max_distance))  # (n - the number of components: every spanning forest has as many edges)
    best = None
    for subset in itertools.combinations(edges, size):  # (subsets of a sorted list come sorted, and in lexicographic order)
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for _, i, j in subset:
            a, b = find(i), find(j)
            if a == b:
                break
            parent[a] = b
        else:
            best = subset
            break  # the first acyclic one is the least
    return list(best)


def as_list(forest):
    ei, ej, ed, _ = forest
    return list(zip(ed.tolist(), ei.tolist(), ej.tolist()))


def check_forest(forest, n):
    ei, ej, ed, labels = forest
    assert ei.dtype == np.uint32 and ej.dtype == np.uint32 and ed.dtype == np.float64 and labels.dtype == np.uint32
    assert len(ei) == len(ej) == len(ed) and labels.shape == (n,)
    assert np.all(ei < ej)
    assert as_list(forest) == sorted(as_list(forest))
    assert len(ei) == n - int(np.sum(labels == np.arange(n)))
    assert not np.any(np.signbit(ed))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_the_least_forest_of_an_exhaustive_enumeration(n):
    for seed in range(12 if n < 7 else 4):
        D = tied_matrix(n, 100 * n + seed)
        for max_distance in (INF, 2.0, 1.0, 0.5):
            got = forest_ref(D, max_distance)
            check_forest(got, n)
            assert as_list(got) == exhaustive(D, max_distance), (n, seed, max_distance)


@pytest.mark.parametrize("n", [2, 17, 64, 200])
def test_kruskal_and_prim_agree(n):
    rng = np.random.RandomState(n)
    cases = [("tied", tied_matrix(n, n, top=5)), ("random", symmetric(rng.uniform(size=(n, n)))),
             ("zeros", symmetric(np.where(rng.uniform(size=(n, n)) < 0.3, -0.0, rng.randint(0, 3, size=(n, n)).astype(np.float64))))]
    withnan = symmetric(rng.randint(1, 6, size=(n, n)).astype(np.float64))
    withnan[n // 2, :] = np.nan
    withnan[:, n // 2] = np.nan
    withnan[n - 1, 0] = INF
    cases.append(("nan and inf", withnan))
    for name, D in cases:
        values = np.unique(D[np.tril_indices(n, -1)])
        values = values[np.isfinite(values)]
        some = [float(values[len(values) // 2]), float(values[0])] if len(values) else []
        for max_distance in [INF, -1.0] + some:
            got = forest_ref(D, max_distance)
            check_forest(got, n)
            assert as_list(got) == kruskal(D, max_distance), (name, n, max_distance)
            want_labels = clusters_ref(D, max_distance)
            assert np.array_equal(got[3], want_labels[0]), (name, n, max_distance)
    assert len(forest_ref(cases[0][1], -1.0)[0]) == 0
    with pytest.raises(ValueError):
        forest_ref(cases[0][1], float("nan"))


@pytest.mark.parametrize("n", [1, 9, 60])
def test_the_cut_of_the_forest_is_the_clusters(n):
    rng = np.random.RandomState(7 * n)
    plain = tied_matrix(n, n, top=6) / 4.0
    withnan = np.array(plain)
    withnan[n // 3, :] = np.nan
    withnan[:, n // 3] = np.nan
    spread = symmetric(np.round(rng.uniform(size=(n, n)), 2))
    for name, D in (("tied", plain), ("a NaN row", withnan), ("random", spread)):
        ei, ej, ed, labels = forest_ref(D, INF)
        values = np.unique(D[np.tril_indices(n, -1)])
        values = values[np.isfinite(values)]
        thresholds = list(values) + list((values[1:] + values[:-1]) / 2) + [-1.0, INF]  # every value (the inclusive tie), the midpoints
        for T in thresholds:
            got = cut_ref(n, ei, ej, ed, T)
            want = clusters_ref(D, T)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (name, n, T)
        # a forest with a cap: its own cuts below the cap
        if len(values):
            cap = float(values[len(values) // 2])
            ci, cj, cd, clabels = forest_ref(D, cap)
            assert np.all(cd <= cap)
            assert np.array_equal(clabels, clusters_ref(D, cap)[0])
            for T in [v for v in thresholds if v <= cap]:
                assert np.array_equal(cut_ref(n, ci, cj, cd, T)[0], clusters_ref(D, T)[0]), (name, n, T, "capped")
    if n == 60:
        assert withnan_is_alone(forest_ref(withnan, INF), n // 3)


def withnan_is_alone(forest, row):
    ei, ej, _, labels = forest
    return labels[row] == row and int(np.sum(labels == row)) == 1 and not np.any(ei == row) and not np.any(ej == row)


def test_cut_ref_takes_any_edge_list():
    # a cycle and a repeated edge: not a forest
    labels, n = cut_ref(6, [0, 1, 0, 0, 4], [1, 2, 2, 1, 5], [1.0, 1.0, 3.0, 0.5, 2.0], 1.0)
    assert labels.tolist() == [0, 0, 0, 3, 4, 5] and n == 4
    labels, n = cut_ref(6, [0, 1, 0, 0, 4], [1, 2, 2, 1, 5], [1.0, 1.0, 3.0, 0.5, np.nan], INF)
    assert labels.tolist() == [0, 0, 0, 3, 4, 5] and n == 4
    assert cut_ref(0, [], [], [], 1.0)[1] == 0
    with pytest.raises(ValueError):
        cut_ref(3, [1], [1], [0.0], 1.0)
    with pytest.raises(ValueError):
        cut_ref(3, [0], [3], [0.0], 1.0)
    with pytest.raises(ValueError):
        cut_ref(3, [0], [1], [0.0], float("nan"))
