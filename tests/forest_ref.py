"""numpy reference of the single-linkage tree (kpop_spanning_forest, include/kpop_hip.h): from a square matrix of distances to THE
minimum spanning forest of the graph that joins rows i < j iff D[j, i] <= max_distance -- the LOWER triangle alone is read, the diagonal
never, and a NaN compares false: it is no edge.  Edges are ordered by (d with -0 taken as +0, i, j) ascending; the order is strict, so
the forest is unique and no algorithm has a say in it.  Here: Prim's, a tree grown vertex by vertex from the smallest row not yet
reached, every step a few numpy operations over the rows (tests/test_forest_ref.py holds it against Kruskal's and against exhaustive
enumeration).  No scipy."""
import numpy as np


def cut_ref(n, edge_i, edge_j, edge_dist, T):
    """-> (labels u32 [n], n_clusters): the ends of the edges with edge_dist <= T united (a NaN joins nothing), a row's label the
    smallest row index of its component.  Any list of edges i < j < n, a forest or not."""
    T = float(T)
    if T != T:
        raise ValueError("the threshold is not a number")
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j, d in zip(np.asarray(edge_i).tolist(), np.asarray(edge_j).tolist(), np.asarray(edge_dist, dtype=np.float64).tolist()):
        if not (0 <= i < j < n):
            raise ValueError("an edge is a pair i < j < n")
        if d <= T:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(x) for x in range(n)], dtype=np.uint32)
    return labels, int(np.sum(labels == np.arange(n)))


def forest_ref(D, max_distance=np.inf):
    """-> (edge_i u32, edge_j u32, edge_dist f64, labels u32 [n]): the forest's edges i < j ascending by (d, i, j), a zero distance as
    +0; labels[r] the smallest row index of row r's component at max_distance"""
    D = np.asarray(D, dtype=np.float64)
    max_distance = float(max_distance)
    if max_distance != max_distance:
        raise ValueError("the distance is not a number")
    n = D.shape[0]
    assert D.shape == (n, n)
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    W = np.where(low, D, D.T) + 0.0  # W[a, b] = D[max(a, b), min(a, b)]; -0 + 0 = +0
    with np.errstate(invalid="ignore"):
        allowed = W <= max_distance
    np.fill_diagonal(allowed, False)
    rows = np.arange(n)
    reached = np.zeros(n, dtype=bool)
    has = np.zeros(n, dtype=bool)  # a row outside the tree with an allowed edge into it
    best_d = np.zeros(n)  # ... the least such edge {row, best_u[row]}: for a fixed row the edges {row, u} order by (d, u)
    best_u = np.zeros(n, dtype=np.int64)
    ei, ej, ed = [], [], []

    def reach(v):
        reached[v] = True
        has[v] = False
        better = allowed[v] & ~reached & (~has | (W[v] < best_d) | ((W[v] == best_d) & (v < best_u)))
        best_d[better] = W[v][better]
        best_u[better] = v
        has[better] = True

    for start in range(n):
        if reached[start]:
            continue
        reach(start)
        while True:
            cand = rows[has]
            if cand.size == 0:
                break
            least = cand[best_d[cand] == best_d[cand].min()]
            lo, hi = np.minimum(least, best_u[least]), np.maximum(least, best_u[least])
            k = np.lexsort((hi, lo))[0]
            ei.append(int(lo[k]))
            ej.append(int(hi[k]))
            ed.append(float(best_d[least[k]]))
            reach(int(least[k]))
    ei, ej, ed = np.array(ei, dtype=np.uint32), np.array(ej, dtype=np.uint32), np.array(ed, dtype=np.float64)
    order = np.lexsort((ej, ei, ed))
    ei, ej, ed = ei[order], ej[order], ed[order]
    labels, _ = cut_ref(n, ei, ej, ed, np.inf)
    return ei, ej, ed, labels
