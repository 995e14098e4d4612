"""numpy reference of DBSCAN on a resident set (kpop_dbscan, include/kpop_hip.h): from a square matrix of
distances, a radius and a count to every row's degree, label and core row.  Only the LOWER triangle is read (the pair of rows i < j
is D[j, i]), the diagonal never, and a NaN compares false: it is within nothing.

    degree[i]  = 1 + the rows j != i with d(i, j) <= eps        (the row counts itself)
    core       = degree >= min_pts
    clusters   = clusters_ref on the matrix with the entries of every row that is not core set to NaN: the connected components of
                 the core rows, a label the smallest core row index of the component
    border     = a row that is not core with a core row within eps: core_of the core row first under np.lexsort((index, d + 0.0)),
                 the label that row's
    noise      = every other row: label and core_of NOISE
No scipy."""
import numpy as np

from clusters_ref import clusters_ref

NOISE = 0xFFFFFFFF


def lower_symmetric(D):
    """the symmetric matrix whose both triangles are D's lower one, the diagonal NaN: what the reference reads, and nothing else"""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    L = np.tril(D, -1)
    S = L + L.T
    S[np.arange(n), np.arange(n)] = np.nan
    # (tril and the sum keep a NaN of the lower triangle; a NaN of the upper one or of the diagonal is gone)
    return S


def dbscan_ref(D, eps, min_pts):
    """-> (labels u32 [n], core_of u32 [n], degree u32 [n], counts u32 [3]: clusters, core rows, noise rows)"""
    eps, min_pts = float(eps), int(min_pts)
    if eps != eps:
        raise ValueError("eps is not a number")
    if min_pts < 1:
        raise ValueError("min_pts is zero")
    S = lower_symmetric(D)
    n = S.shape[0]
    with np.errstate(invalid="ignore"):
        within = S <= eps
    degree = 1 + within.sum(axis=1)
    core = degree >= min_pts
    cut = np.array(S)
    cut[~core, :] = np.nan
    cut[:, ~core] = np.nan
    comp = clusters_ref(cut, eps)[0].astype(np.int64)  # a row that is not core is alone there
    labels = np.full(n, NOISE, dtype=np.int64)
    core_of = np.full(n, NOISE, dtype=np.int64)
    labels[core] = comp[core]
    core_of[core] = np.nonzero(core)[0]
    for i in np.nonzero(~core)[0]:
        cand = np.nonzero(within[i] & core)[0]
        if cand.size == 0:
            continue
        best = cand[np.lexsort((cand, S[i, cand] + 0.0))[0]]  # (d with -0 taken as +0, index)
        core_of[i] = best
        labels[i] = comp[best]
    counts = [int(np.sum(core & (labels == np.arange(n)))), int(core.sum()), int(np.sum(labels == NOISE))]
    return labels.astype(np.uint32), core_of.astype(np.uint32), degree.astype(np.uint32), np.array(counts, dtype=np.uint32)


def check_invariants(labels, core_of, degree, counts, min_pts):
    """what INTEGRATION.md 6i says of every result, whatever the distances were"""
    labels, core_of, degree = (np.asarray(a).astype(np.int64) for a in (labels, core_of, degree))
    n = len(labels)
    idx = np.arange(n)
    core = degree >= min_pts
    noise = labels == NOISE
    assert np.all(degree >= 1)
    assert np.array_equal(core_of[core], idx[core]) and np.all(labels[core] <= idx[core])
    assert not np.any(noise & core) and np.array_equal(noise, core_of == NOISE)
    live = ~noise
    assert np.all(core[labels[live]]) and np.array_equal(labels[labels[live]], labels[live])
    assert np.all(core[core_of[live]]) and np.array_equal(labels[core_of[live]], labels[live])
    assert list(counts) == [int(np.sum(core & (labels == idx))), int(core.sum()), int(noise.sum())]
