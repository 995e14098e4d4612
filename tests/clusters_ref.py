"""numpy reference of the clusters at a distance (kpop_clusters_within, include/kpop_hip.h): from a square matrix of distances and a
threshold to every row's label.  Rows i < j are joined iff D[j, i] <= T -- the LOWER triangle alone is read, the diagonal never, and a
NaN compares false: it joins nothing.  A row's label is the smallest row index of its connected component.  A plain union-find that
hooks the larger root under the smaller one, row by row; no scipy."""
import numpy as np


def clusters_ref(D, T, known=None):
    """-> (labels u32 [n], n_clusters).  known: the labels of the first len(known) rows from an earlier run at the same T; the pairs of
    two such rows are not looked at"""
    D = np.asarray(D, dtype=np.float64)
    T = float(T)
    if T != T:
        raise ValueError("the threshold is not a number")
    n = D.shape[0]
    assert D.shape == (n, n)
    parent = np.arange(n, dtype=np.int64)
    first = 0
    if known is not None:
        first = len(known)
        assert first <= n
        parent[:first] = known

    def roots_of(x):
        r = parent[x]
        while True:
            up = parent[r]
            if np.array_equal(up, r):
                break
            r = up
        parent[x] = r  # (the paths compressed)
        return r

    for j in range(first, n):  # (row j is still its own root: only a row that has had its turn, or a column of one, is ever hooked)
        with np.errstate(invalid="ignore"):
            hits = np.nonzero(D[j, :j] <= T)[0]
        if hits.size == 0:
            continue
        roots = np.unique(roots_of(hits))
        parent[roots] = roots[0]  # the smallest: every root among them is below j
        parent[j] = roots[0]
    labels = roots_of(np.arange(n, dtype=np.int64)) if n else parent
    return labels.astype(np.uint32), int(np.sum(labels == np.arange(n)))


def cluster_sizes(labels):
    """the clusters' sizes, largest first"""
    counts = np.bincount(np.asarray(labels, dtype=np.int64)) if len(labels) else np.zeros(0, dtype=np.int64)
    return sorted(counts[counts > 0].tolist(), reverse=True)
