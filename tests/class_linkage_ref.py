"""The distances between every two classes of a labelled set and the classes' tree, restated (kpop_class_linkage and
kpop_class_tree, include/kpop_hip.h).  Test infrastructure: numpy and math.fsum, nothing of the product.

class_linkage_ref works over a given r1 x r1 matrix D, D[j, i] the distance of rows i and j: every sum of distances is math.fsum's --
the exact sum, rounded once -- and a mean is that sum divided once.  line_linkage_ref is the exact reference for rows on a line with
dyadic coordinates: sums, minima and maxima between classes from sorted values and integer prefix sums in O(n log n), so that a long
set needs no quadratic matrix.  class_tree_ref is the agglomeration as a plain O(n^3) loop with the declared arithmetic in the declared
order."""
import math

import numpy as np

NO_CLASS = 0xFFFFFFFF
QNAN_BITS = 0x7FF8000000000000
QNAN = float(np.array([QNAN_BITS], dtype=np.uint64).view(np.float64)[0])
LINK_SINGLE, LINK_COMPLETE, LINK_AVERAGE = 0, 1, 2
NAMES = ("class_rows", "mean_dist", "min_dist", "max_dist", "min_i", "min_j")


def members_of(class_of, n_classes):
    class_of = np.asarray(class_of, dtype=np.int64)
    return [np.flatnonzero(class_of == c) for c in range(n_classes)]


def empty_tables(n_classes):
    return (np.zeros(n_classes, dtype=np.uint32), np.full((n_classes, n_classes), QNAN), np.full((n_classes, n_classes), QNAN),
            np.full((n_classes, n_classes), QNAN), np.full((n_classes, n_classes), NO_CLASS, dtype=np.uint32),
            np.full((n_classes, n_classes), NO_CLASS, dtype=np.uint32))


def pairs_of(members, a, b):
    """P(a, b) as two index arrays i < j (natural row indices)"""
    if a == b:
        k, l = np.triu_indices(len(members[a]), 1)
        return members[a][k], members[a][l]
    i, j = np.meshgrid(members[a], members[b], indexing="ij")
    i, j = i.ravel(), j.ravel()
    return np.minimum(i, j), np.maximum(i, j)


def class_linkage_ref(D, class_of, n_classes):
    """the six arrays of kpop_class_linkage over the r1 x r1 matrix D"""
    r1 = len(class_of)
    D = np.asarray(D, dtype=np.float64).reshape(r1, r1)
    members = members_of(class_of, n_classes)
    rows, mean, lo, hi, mi, mj = empty_tables(n_classes)
    rows[:] = [len(x) for x in members]
    for a in range(n_classes):
        for b in range(a, n_classes):
            i, j = pairs_of(members, a, b)
            if len(i) == 0:
                continue
            d = D[j, i]
            mean[a, b] = mean[b, a] = math.fsum(d) / len(d)  # (fsum of a NaN is a NaN)
            ok = d == d
            if not ok.any():
                continue
            d, i, j = d[ok] + 0.0, i[ok], j[ok]  # (-0 + 0 is +0)
            k = np.lexsort((j, i, d))[0]
            lo[a, b] = lo[b, a] = d[k]
            hi[a, b] = hi[b, a] = d.max()
            mi[a, b] = mi[b, a] = i[k]
            mj[a, b] = mj[b, a] = j[k]
    return rows, mean, lo, hi, mi, mj


def _first_rows(values, rows):
    """the distinct values ascending, and the two smallest rows that hold each (the second: -1 where there is one row alone)"""
    order = np.lexsort((rows, values))
    v, r = values[order], rows[order]
    first = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    second = first + 1
    has = (second < len(v)) & (v[np.minimum(second, len(v) - 1)] == v[first])
    return v[first], r[first], np.where(has, r[np.minimum(second, len(v) - 1)], -1)


def _least_pair(xa, ra, xb, rb, d, same):
    """the least (i, j) among the pairs of a row of (xa, ra) and a row of (xb, rb) at distance exactly d; same: both are one class"""
    ub, fb, sb = _first_rows(xb, rb)
    best = None
    for target in ((xa - d, xa + d) if d else (xa,)):
        pos = np.minimum(np.searchsorted(ub, target), len(ub) - 1)
        hit = ub[pos] == target
        c = fb[pos]
        if same and d == 0:  # the partner is another row: the second where the first is the row itself
            c = np.where(c == ra, sb[pos], c)
            hit &= c >= 0
        if hit.any():
            i, j = np.minimum(ra[hit], c[hit]), np.maximum(ra[hit], c[hit])
            k = np.lexsort((j, i))[0]
            cand = (int(i[k]), int(j[k]))
            best = cand if best is None or cand < best else best
    return best


def line_linkage_ref(x, class_of, n_classes, scale=8):
    """the six arrays for rows on a line at x, every x a multiple of 1 / scale (a power of two), d(i, j) = |x_i - x_j|: integers
    throughout, so every sum is exact whatever its length, and one rounding in the division of a mean"""
    xi = np.round(np.asarray(x, dtype=np.float64) * scale).astype(np.int64)
    assert np.array_equal(xi / float(scale), np.asarray(x, dtype=np.float64))
    members = members_of(class_of, n_classes)
    rows, mean, lo, hi, mi, mj = empty_tables(n_classes)
    rows[:] = [len(m) for m in members]
    srt = [np.sort(xi[m]) for m in members]
    pre = [np.concatenate([[0], np.cumsum(s)]) for s in srt]
    for a in range(n_classes):
        for b in range(a, n_classes):
            na, nb = len(srt[a]), len(srt[b])
            n_pairs = na * (na - 1) // 2 if a == b else na * nb
            if n_pairs == 0:
                continue
            # the sum over v of a of the sum over u of b of |v - u|: u below v counts v - u, u above u - v
            k = np.searchsorted(srt[b], srt[a], side="left")
            total = int(np.sum(srt[a] * k - pre[b][k]) + np.sum((pre[b][nb] - pre[b][k]) - srt[a] * (nb - k)))
            if a == b:
                total //= 2
                d_min = int(np.min(np.diff(srt[a])))
                d_max = int(srt[a][-1] - srt[a][0])
            else:
                below = srt[b][np.maximum(k - 1, 0)]
                above = srt[b][np.minimum(k, nb - 1)]
                d_min = int(min(np.min(np.abs(srt[a] - below)), np.min(np.abs(srt[a] - above))))
                d_max = int(max(srt[a][-1] - srt[b][0], srt[b][-1] - srt[a][0]))
            assert total < 2 ** 53
            mean[a, b] = mean[b, a] = (total / float(scale)) / n_pairs
            lo[a, b] = lo[b, a] = d_min / float(scale)
            hi[a, b] = hi[b, a] = d_max / float(scale)
            mi[a, b], mj[a, b] = _least_pair(xi[members[a]], members[a], xi[members[b]], members[b], d_min, a == b)
            mi[b, a], mj[b, a] = mi[a, b], mj[a, b]
    return rows, mean, lo, hi, mi, mj


def class_tree_ref(class_rows, dist, linkage):
    """kpop_class_tree: left, right, height, size.  Every step scans every pair of live nodes for the least under (distance with -0 as
    +0, lower id, higher id); a NaN is never the least; the new node's distances in the declared arithmetic, x the left node"""
    n_classes = len(class_rows)
    dist = np.asarray(dist, dtype=np.float64).reshape(n_classes, n_classes)
    size = {c: int(class_rows[c]) for c in range(n_classes) if class_rows[c]}
    d = {(a, b): float(dist[a, b]) for a in size for b in size if a < b}
    left, right, height, sizes = [], [], [], []
    t = 0
    while len(size) > 1:
        cand = [(v + 0.0, a, b) for (a, b), v in d.items() if v == v]
        if not cand:
            break
        h, x, y = min(cand)
        node = n_classes + t
        nx, ny = float(size[x]), float(size[y])
        for z in list(size):
            if z in (x, y):
                continue
            dx, dy = d.pop((min(x, z), max(x, z))), d.pop((min(y, z), max(y, z)))
            if dx != dx or dy != dy:
                v = float("nan")
            elif linkage == LINK_SINGLE:
                v = min(dx, dy)
            elif linkage == LINK_COMPLETE:
                v = max(dx, dy)
            else:
                v = (nx * dx + ny * dy) / (nx + ny)
            d[(z, node)] = v
        del d[(x, y)]
        size[node] = size.pop(x) + size.pop(y)
        left.append(x)
        right.append(y)
        height.append(h)
        sizes.append(size[node])
        t += 1
    return (np.array(left, dtype=np.uint32), np.array(right, dtype=np.uint32), np.array(height, dtype=np.float64), np.array(sizes, dtype=np.uint32))


def leaves_under(left, right, n_classes):
    """the classes under every node of a tree, by node id"""
    under = {c: [c] for c in range(n_classes)}
    for t, (a, b) in enumerate(zip(left, right)):
        under[n_classes + t] = under[int(a)] + under[int(b)]
    return under


def same_bits(a, b):
    """bit for bit where the values are numbers (+0 is not -0), a NaN where the other holds a NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
