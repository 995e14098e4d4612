"""Density peaks over a given distance matrix and density array, by brute force: INTEGRATION.md section 6p written down and nothing
else (kpop_density_peaks, kpop_density_peaks_cut, include/kpop_hip.h).

D the r x r matrix of the set against itself (the diagonal is never read), density one f64 a row.  A row whose density is a NaN is
LEFT OUT: delta the quiet NaN 0x7FF8000000000000, parent and label NOISE, nobody's candidate.  Row i RANKS ABOVE row j iff
density[i] > density[j], or they are equal and i < j (-0 equals +0).  parent[j] is the least, under (D[j, i] with -0 as +0, i), of the
rows i that rank above j and whose D[j, i] is a number, delta[j] that distance; none: parent[j] = j and delta[j] = +inf, a ROOT.
The cut walks the parents: row j is a CENTRE iff it is a root or delta[j] > min_delta and density[j] >= min_density; labels[j] = j for
a centre, else labels[parent[j]]; counts = (centres, roots, rows left out)."""
import collections

import numpy as np

DensityPeaks = collections.namedtuple("DensityPeaks", "density delta parent labels counts")
NOISE = 0xFFFFFFFF
INF = float("inf")
QNAN_BITS = 0x7FF8000000000000
QNAN = np.array([QNAN_BITS], dtype=np.uint64).view(np.float64)[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def degree_density(D, eps):
    """dbscan's degree at eps as doubles: 1 + the other rows within eps (a NaN is within nothing)"""
    D = np.asarray(D, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        within = D <= eps
    np.fill_diagonal(within, False)
    return (1 + within.sum(axis=1)).astype(np.float64)


def ranks_above(density, i, j):
    """row i ranks above row j (both densities numbers)"""
    return density[i] > density[j] or (density[i] == density[j] and i < j)


def parents_ref(D, density):
    """-> (delta f64 [r], parent u32 [r]) by the definition, a row at a time"""
    D, density = np.asarray(D, dtype=np.float64), np.asarray(density, dtype=np.float64)
    r = len(density)
    assert D.shape == (r, r)
    delta, parent = np.full(r, INF), np.arange(r, dtype=np.uint32)
    idx = np.arange(r)
    kept = ~np.isnan(density)
    for j in range(r):
        if not kept[j]:
            delta[j], parent[j] = QNAN, NOISE
            continue
        with np.errstate(invalid="ignore"):
            above = kept & ((density > density[j]) | ((density == density[j]) & (idx < j)))
        cand = np.flatnonzero(above & ~np.isnan(D[j]))
        if not len(cand):
            continue
        d = D[j, cand] + 0.0  # (-0 + 0 is +0)
        best = cand[d == d.min()].min()  # ties of distance go to the smaller row index
        delta[j], parent[j] = D[j, best] + 0.0, best
    return delta, parent


def cut_ref(density, delta, parent, min_density=-INF, min_delta=INF):
    """-> (labels u32 [r], counts u32 [3]) by walking the parents"""
    r = len(parent)
    labels, counts = np.zeros(r, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    centre = np.zeros(r, dtype=bool)
    for j in range(r):
        if parent[j] == NOISE:
            counts[2] += 1
            continue
        root = parent[j] == j
        centre[j] = root or (delta[j] > min_delta and density[j] >= min_density)
        counts[0] += centre[j]
        counts[1] += root
    for j in range(r):
        at, steps = j, 0
        while parent[at] != NOISE and not centre[at]:
            at, steps = int(parent[at]), steps + 1
            assert steps <= r, "a cycle"
        labels[j] = NOISE if parent[at] == NOISE else at
    return labels, counts


def density_peaks_ref(D, density=None, eps=None, min_density=-INF, min_delta=None):
    """what RefSet.density_peaks returns, from the matrix"""
    density = degree_density(D, eps) if density is None else np.array(density, dtype=np.float64)
    delta, parent = parents_ref(D, density)
    labels, counts = cut_ref(density, delta, parent, min_density, min_delta) if min_delta is not None else (None, None)
    return DensityPeaks(density, delta, parent, labels, counts)


def components_within(D, eps):
    """the connected components of the graph at eps -> the smallest row index of each row's component"""
    D = np.asarray(D, dtype=np.float64)
    r = len(D)
    label = np.arange(r)
    with np.errstate(invalid="ignore"):
        within = D <= eps
    seen = np.zeros(r, dtype=bool)
    for s in range(r):
        if seen[s]:
            continue
        stack, seen[s] = [s], True
        while stack:
            a = stack.pop()
            label[a] = s
            for b in np.flatnonzero(within[a] & ~seen):
                if b != a:
                    seen[b] = True
                    stack.append(int(b))
    return label


def chain_case(r, seed):
    """the deep chain of the tests: row i at pos[i] of a seeded permutation, density -(pos - c)^2, c = r // 3 -> (pos, density, delta,
    parent) in closed form: delta 1 everywhere but at the root, the parent one step toward c, the row at c the one root"""
    pos = np.random.RandomState(seed).permutation(r)
    c = r // 3
    density = -((pos - c).astype(np.float64) ** 2)
    row_at = np.empty(r, dtype=np.int64)
    row_at[pos] = np.arange(r)
    toward = pos + np.where(pos < c, 1, -1)
    toward[pos == c] = c
    parent = row_at[toward].astype(np.uint32)
    delta = np.where(pos == c, INF, 1.0)
    return pos, density, delta, parent
