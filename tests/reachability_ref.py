"""numpy reference of the mutual-reachability forest of a resident set (kpop_reachability_tree, include/kpop_hip.h; INTEGRATION.md
6j): from a square matrix of distances and a count to every row's core distance and to THE minimum spanning forest under the weight
max(d, core_i, core_j).  Only the LOWER triangle is read (the pair of rows i < j is D[j, i]), the diagonal never, and a NaN is no
distance: it takes no place in a row's order and is no edge.

    core[i]   = +0 for min_pts = 1; otherwise the (min_pts - 1)-th least of row i's distances to the OTHER rows that are numbers
                (+inf is one, -0 is +0), NaN when there are fewer
    mr[i, j]  = max(d, core[i], core[j]), NaN if any of the three is
    forest    = forest_ref of that matrix: the order (mr, i, j) is strict, so the forest is unique
    cut at T  = the edges within T united; a row with core <= T gets the smallest row index of its component, every other row NOISE
No scipy."""
import numpy as np

from dbscan_ref import NOISE, lower_symmetric
from forest_ref import cut_ref, forest_ref


def core_ref(D, min_pts):
    """-> core f64 [n]"""
    min_pts = int(min_pts)
    if min_pts < 1:
        raise ValueError("min_pts is zero")
    S = lower_symmetric(D) + 0.0
    n = S.shape[0]
    if min_pts == 1:
        return np.zeros(n)
    k = min_pts - 1
    if k > n - 1:
        return np.full(n, np.nan)
    ordered = np.sort(S, axis=1)  # NaN last: the numbers of a row ascending, then what is no number
    return np.where(np.isnan(ordered[:, k - 1]), np.nan, ordered[:, k - 1])


def reach_matrix(D, core):
    """-> the symmetric n x n matrix of mutual-reachability weights, the diagonal NaN (np.maximum hands a NaN on)"""
    S = lower_symmetric(D) + 0.0
    core = np.asarray(core, dtype=np.float64)
    return np.maximum(np.maximum(S, core[:, None]), core[None, :])


def reachability_forest_ref(D, min_pts, max_distance=np.inf):
    """-> (edge_i u32, edge_j u32, edge_dist f64, core f64 [n], labels u32 [n])"""
    core = core_ref(D, min_pts)
    ei, ej, ed, labels = forest_ref(reach_matrix(D, core), max_distance)
    return ei, ej, ed, core, labels


def reachability_cut_ref(n, edge_i, edge_j, edge_dist, core, T):
    """-> (labels u32 [n], counts u32 [3]: the components with a core row, the core rows, the noise rows).  Any list of edges"""
    labels, _ = cut_ref(n, edge_i, edge_j, edge_dist, T)
    core = np.asarray(core, dtype=np.float64)
    assert core.shape == (n,)
    with np.errstate(invalid="ignore"):
        is_core = core <= float(T)
    counts = [len(np.unique(labels[is_core])), int(is_core.sum()), int(n - is_core.sum())]
    out = np.where(is_core, labels, NOISE).astype(np.uint32)
    return out, np.array(counts, dtype=np.uint32)
