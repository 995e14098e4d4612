"""The silhouette and the medoids of a labelled set, restated over a given distance matrix (kpop_silhouette,
include/kpop_hip.h).  Test infrastructure: numpy and math.fsum, nothing of the product.

D[k, i] is the distance of row rows[k] to row i of the set.  Every sum of distances is math.fsum's: the exact sum, rounded once; a
mean is that sum divided once.  Tie-breaks and special cases are the declared ones."""
import math

import numpy as np

NO_CLASS = 0xFFFFFFFF
NAN = float("nan")


def members_of(class_of, n_classes):
    class_of = np.asarray(class_of, dtype=np.int64)
    return [np.flatnonzero(class_of == c) for c in range(n_classes)]


def silhouette_value(own, other, n_c):
    """(other - own) / max(own, other) as IEEE arithmetic gives it, a zero as +0; +0 for a row alone in its class"""
    if n_c == 1:
        return 0.0
    own, other = np.float64(own), np.float64(other)
    with np.errstate(all="ignore"):
        s = float((other - own) / (own if own > other else other))
    return 0.0 if s == 0.0 else s


def rows_ref(D, rows, class_of, n_classes):
    """own_mean, other_mean, other_class, silhouette of the set's rows `rows`, D[k] the distances of rows[k] to every row of the set"""
    D = np.asarray(D, dtype=np.float64)
    class_of = np.asarray(class_of, dtype=np.int64)
    members = members_of(class_of, n_classes)
    n = len(rows)
    own, other, sil = np.full(n, NAN), np.full(n, NAN), np.full(n, NAN)
    ocls = np.full(n, NO_CLASS, dtype=np.uint32)
    for k, j in enumerate(rows):
        c = int(class_of[j])
        if c == NO_CLASS:
            continue
        assert 0 <= c < n_classes
        best, best_c = NAN, NO_CLASS
        for cc in range(n_classes):
            idx = members[cc]
            if len(idx) == 0:
                continue
            if cc == c:
                idx = idx[idx != j]
                own[k] = math.fsum(D[k, idx]) / len(idx) if len(idx) else 0.0
                continue
            mean = math.fsum(D[k, idx]) / len(idx)
            if mean == mean and (best_c == NO_CLASS or mean < best):  # ascending classes: a tie stays with the smaller
                best, best_c = mean, cc
        other[k], ocls[k] = best, best_c
        sil[k] = silhouette_value(own[k], other[k], len(members[c]))
    return own, other, ocls, sil


def medoids_ref(own, class_of, n_classes):
    """class_rows, medoid, medoid_mean from every row's own_mean"""
    members = members_of(class_of, n_classes)
    class_rows = np.array([len(x) for x in members], dtype=np.uint32).reshape(n_classes)
    medoid = np.full(n_classes, NO_CLASS, dtype=np.uint32)
    medoid_mean = np.full(n_classes, NAN)
    for c, idx in enumerate(members):
        cand = [(own[i] + 0.0, int(i)) for i in idx if own[i] == own[i]]  # (-0 + 0 is +0)
        if cand:
            medoid[c] = min(cand)[1]
            medoid_mean[c] = own[medoid[c]]
    return class_rows, medoid, medoid_mean


def silhouette_ref(D, class_of, n_classes):
    """the seven arrays of kpop_silhouette over the r1 x r1 matrix D"""
    r1 = len(class_of)
    D = np.asarray(D, dtype=np.float64).reshape(r1, r1)
    own, other, ocls, sil = rows_ref(D, range(r1), class_of, n_classes)
    return (own, other, ocls, sil) + medoids_ref(own, class_of, n_classes)


def second_least_other(D, rows, class_of, n_classes):
    """for the tests' margins: the two least means to another class of each row of `rows` (inf where there is none)"""
    class_of = np.asarray(class_of, dtype=np.int64)
    members = members_of(class_of, n_classes)
    out = np.full((len(rows), 2), np.inf)
    for k, j in enumerate(rows):
        if class_of[j] == NO_CLASS:
            continue
        means = sorted(math.fsum(D[k, idx]) / len(idx) for cc, idx in enumerate(members) if len(idx) and cc != class_of[j])
        means = [x for x in means if x == x][:2]
        out[k, :len(means)] = means
    return out


def summary_ref(class_of, n_classes, silhouette):
    """kpop_silhouette_summary: both means summed in ascending row order"""
    sums, rows = [0.0] * n_classes, [0] * n_classes
    total, n = 0.0, 0
    for c, s in zip(class_of, silhouette):
        c = int(c)
        if c == NO_CLASS:
            continue
        sums[c] += float(s)
        rows[c] += 1
        total += float(s)
        n += 1
    class_mean = np.array([sums[c] / rows[c] if rows[c] else NAN for c in range(n_classes)], dtype=np.float64).reshape(n_classes)
    return class_mean, (total / n if n else NAN)


def same_bits(a, b):
    """bit for bit where the values are numbers (+0 is not -0), a NaN where the other holds a NaN (the payload of a NaN that
    arithmetic made -- 0/0, a NaN distance -- is the processor's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
