"""numpy reference of the range query (kpop_neighbours_within, include/kpop_hip.h): from an r2 x r1 distance matrix and a threshold
to the CSR lists.  Row j's hits are the columns i with D[j, i] <= T (a NaN is never one), in ascending (distance, column) order with
-0 ordered as +0: the multimap of lib/Matrix.ml:641-650, cut at a distance instead of a count.  The distances keep their bits."""
import numpy as np


def within_ref(D, T):
    """-> (offsets u64 [r2 + 1], idx u32, dist f64)"""
    D = np.asarray(D, dtype=np.float64)
    T = float(T)
    if T != T:
        raise ValueError("the threshold is not a number")
    r2 = D.shape[0]
    offsets = np.zeros(r2 + 1, dtype=np.uint64)
    idx, dist = [], []
    for j in range(r2):
        row = D[j]
        with np.errstate(invalid="ignore"):
            hits = np.nonzero(row <= T)[0]
        order = np.lexsort((hits, row[hits] + 0.0))  # (x + 0.0: -0 becomes +0 in the key alone)
        hits = hits[order]
        idx.append(hits.astype(np.uint32))
        dist.append(row[hits])
        offsets[j + 1] = offsets[j] + np.uint64(len(hits))
    return (offsets, np.concatenate(idx) if idx else np.zeros(0, dtype=np.uint32),
            np.concatenate(dist) if dist else np.zeros(0, dtype=np.float64))


def rows_of(res):
    """(offsets, idx, dist) -> [(idx of row j, dist of row j)]"""
    offsets, idx, dist = res
    return [(idx[int(offsets[j]):int(offsets[j + 1])], dist[int(offsets[j]):int(offsets[j + 1])]) for j in range(len(offsets) - 1)]


def same_lists(got, want, what=""):
    """offsets, idx and dist bit for bit (the sign of a zero included)"""
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert a.dtype == b.dtype, (what, k, a.dtype, b.dtype)
        if a.dtype == np.float64:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, k, int(np.sum(a.view(np.uint64) != b.view(np.uint64))))
        else:
            assert np.array_equal(a, b), (what, k, int(np.sum(a != b)))
