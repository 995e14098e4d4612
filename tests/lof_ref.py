"""The local outlier factor over a given distance matrix, in plain Python with math.fsum: INTEGRATION.md section 6n written down and
nothing else (kpop_lof, kpop_lof_score, include/kpop_hip.h).

Set form, D the r x r matrix of the set against itself (the diagonal is never read): kdist[j] the k-th least of the numbers among
D[j, i], i != j (a sort; -0 taken as +0; NaN when there are fewer than k); N(j) every i != j with D[j, i] <= kdist[j]; lrd[j] =
|N| / fsum(max(D[j, i], kdist[i])), ONE division; lof[j] = (fsum(lrd[i]) / |N|) / lrd[j], TWO divisions, inf / inf being 1.0.  Query
form, E the r2 x r1 matrix of the query rows against the set: the same with nothing left out and the set's kdist and lrd passed in.
A NaN term makes its sum a NaN; a row without neighbours gets NaN, 0, NaN, NaN; every NaN returned is the quiet NaN
0x7FF8000000000000 and every zero +0."""
import collections
import math

import numpy as np

Lof = collections.namedtuple("Lof", "kdist n_neigh lrd lof")
NAN = float("nan")
INF = float("inf")
QNAN_BITS = 0x7FF8000000000000
U = 2.0 ** -53


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def neighbourhood_max(n_neigh):
    """the n of the tests' bounds: the longest neighbourhood of the case (0 for no rows)"""
    return int(np.max(n_neigh)) if len(n_neigh) else 0


def _div(a, b):
    """IEEE division: x / 0 is an infinity, 0 / 0 and inf / inf a NaN"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sum(terms):
    """the exactly rounded sum; a NaN term poisons it, an infinity makes it one"""
    terms = list(terms)
    if any(t != t for t in terms):
        return NAN
    if any(t == INF for t in terms):
        return INF
    return math.fsum(terms)


def _clean(x):
    if x != x:
        return NAN
    return 0.0 if x == 0.0 else x


def _check(k):
    if int(k) != k or not 1 <= k <= 128:
        raise ValueError("k in 1 .. 128")
    return int(k)


def k_distance(row, k):
    """the k-th least of the numbers of a row of distances, NaN when there are fewer"""
    numbers = sorted(abs(float(d)) if d == 0 else float(d) for d in row if d == d)
    return numbers[k - 1] if len(numbers) >= k else NAN


def _density(dist, others, kd, col_kdist):
    """one row: its distances dist[i] to the columns `others`, its own k-distance -> (its neighbourhood, lrd)"""
    members = [i for i in others if dist[i] <= kd]  # (a NaN on either side compares false)
    if not members:
        return members, NAN
    s1 = _sum(NAN if col_kdist[i] != col_kdist[i] else max(float(dist[i]), float(col_kdist[i])) for i in members)
    return members, _clean(_div(len(members), s1))


def _factor(members, lrd, col_lrd):
    if not members:
        return NAN
    mean = _div(_sum(float(col_lrd[i]) for i in members), len(members))
    return 1.0 if mean == INF and lrd == INF else _clean(_div(mean, lrd))


def lof_ref(D, k):
    """the set form over the square matrix D -> Lof"""
    k = _check(k)
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    assert D.shape == (r, r)
    others = [[i for i in range(r) if i != j] for j in range(r)]
    kdist = np.array([k_distance(D[j, others[j]], k) for j in range(r)], dtype=np.float64).reshape(r)
    hoods, lrd = [None] * r, np.full(r, NAN)
    for j in range(r):
        hoods[j], lrd[j] = _density(D[j], others[j], kdist[j], kdist)
    n_neigh = np.array([len(h) for h in hoods], dtype=np.uint32).reshape(r)
    lof = np.array([_factor(hoods[j], lrd[j], lrd) for j in range(r)], dtype=np.float64).reshape(r)
    return Lof(kdist, n_neigh, lrd, lof)


def lof_score_ref(E, k, set_kdist, set_lrd):
    """the query form over E[r2, r1], the set's kdist and lrd at the same k -> Lof, one entry a query row"""
    k = _check(k)
    E = np.asarray(E, dtype=np.float64)
    r2, r1 = E.shape
    set_kdist, set_lrd = np.asarray(set_kdist, dtype=np.float64), np.asarray(set_lrd, dtype=np.float64)
    assert set_kdist.shape == (r1,) and set_lrd.shape == (r1,)
    kdist, n_neigh, lrd, lof = np.full(r2, NAN), np.zeros(r2, dtype=np.uint32), np.full(r2, NAN), np.full(r2, NAN)
    for q in range(r2):
        kdist[q] = k_distance(E[q], k)
        hood, lrd[q] = _density(E[q], range(r1), kdist[q], set_kdist)
        n_neigh[q], lof[q] = len(hood), _factor(hood, lrd[q], set_lrd)
    return Lof(kdist, n_neigh, lrd, lof)


def lof_rows_ref(E, rows, k, set_kdist, set_lrd):
    """the set form for a few rows of a long set: E[s] the distances of row rows[s] to every row of the set, the row itself left out;
    the neighbours' k-distances and densities are taken from set_kdist and set_lrd -> Lof, one entry a row of `rows`"""
    k = _check(k)
    E = np.asarray(E, dtype=np.float64)
    n, r1 = E.shape
    assert len(rows) == n
    kdist, n_neigh, lrd, lof = np.full(n, NAN), np.zeros(n, dtype=np.uint32), np.full(n, NAN), np.full(n, NAN)
    for s, j in enumerate(rows):
        others = [i for i in range(r1) if i != j]
        kdist[s] = k_distance(E[s, others], k)
        hood, lrd[s] = _density(E[s], others, kdist[s], set_kdist)
        n_neigh[s], lof[s] = len(hood), _factor(hood, lrd[s], set_lrd)
    return Lof(kdist, n_neigh, lrd, lof)
