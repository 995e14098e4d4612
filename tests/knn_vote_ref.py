"""numpy reference of the k-NN vote (kpop_knn_vote, include/kpop_hip.h): from an r2 x r1 distance matrix,
the classes of its columns and k to the four outputs.  Row j's list: the columns whose distance is a number, in ascending (distance,
column) order with -0 ordered as +0; its first k, plus every further one whose distance equals the k-th (lib/Matrix.ml:641-650: whole
tie groups).  The vote: the class with the most members in the list; among classes with equally many, the one that appears first in it.
Written from the declared semantics, not from the kernels."""
import numpy as np

NO_CLASS = 0xFFFFFFFF


def knn_lists(D, k):
    """-> [the columns of row j's list, in the list's order]"""
    D = np.asarray(D, dtype=np.float64)
    k = int(k)
    if k < 1:
        raise ValueError("k is at least 1")
    lists = []
    for row in D:
        cols = np.nonzero(~np.isnan(row))[0]
        cols = cols[np.lexsort((cols, row[cols] + 0.0))]  # (x + 0.0: -0 becomes +0 in the key alone)
        n = min(k, len(cols))
        while 0 < n < len(cols) and row[cols[n]] == row[cols[n - 1]]:
            n += 1
        lists.append(cols[:n])
    return lists


def vote(cols, dists, class_of, n_classes=None):
    """one list -> (class, votes, n, first); a column whose class is not below n_classes counts in n and votes for nobody"""
    count, first = {}, {}
    for pos, i in enumerate(cols):
        c = int(class_of[i])
        if n_classes is not None and c >= n_classes:
            continue
        count[c] = count.get(c, 0) + 1
        first.setdefault(c, pos)
    if not count:
        return NO_CLASS, 0, len(cols), float("nan")
    best = min(count, key=lambda c: (-count[c], first[c]))
    return best, count[best], len(cols), dists[first[best]]


def knn_vote_ref(D, class_of, k, n_classes=None, lists=None):
    """-> (cls u32, votes u32, n u32, first f64), one entry a row of D; first keeps the distance's bits.  lists: knn_lists(D, k), when
    the caller votes over them more than once"""
    D = np.asarray(D, dtype=np.float64)
    class_of = np.asarray(class_of)
    assert D.ndim == 2 and class_of.shape == (D.shape[1],)
    r2 = D.shape[0]
    cls, votes, n = (np.zeros(r2, dtype=np.uint32) for _ in range(3))
    first = np.zeros(r2, dtype=np.float64)
    for j, cols in enumerate(knn_lists(D, k) if lists is None else lists):
        cls[j], votes[j], n[j], first[j] = vote(cols, D[j, cols], class_of, n_classes)
    return cls, votes, n, first


def same_votes(got, want, what=""):
    """the four arrays bit for bit (a NaN is numpy's quiet one on both sides)"""
    for q, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, q, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (what, "output %d" % q, "rows", bad[:8].tolist(), a[bad[:8]].tolist(), b[bad[:8]].tolist())
