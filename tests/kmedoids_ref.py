"""Alternating k-medoids over a square distance matrix, in numpy with math.fsum: INTEGRATION.md section 6m written down and nothing else.
Test infrastructure: nothing of the product.

D[j, i] is the distance of row j to row i (the diagonal is never read).  ASSIGNMENT to a medoid list M: row M[c] has class c and dist +0;
every other row j gets the class least under (D[j, M[c]] with -0 as +0, c ascending) over the c whose distance is a number, and dist[j] is
that distance; a row with no such c is left out (NO_CLASS, +inf, own_mean NaN, in no sum).  own_mean[j]: the sum of D[j, i] over the other
rows of j's class -- math.fsum's: the exact sum, rounded once -- divided by n_c - 1, +0 when n_c == 1.  UPDATE: M'[c] is the member of class
c least under (own_mean with -0 as +0, row index) among those whose own_mean is a number; a class without one keeps M[c].  The loop:
    L = assign(init); cost[0]; n_iter = 0
    for t = 0, 1, ...: own_mean of L, M' = update; M' == M: converged, stop; t == max_iter: stop; M = M'; L = assign(M); n_iter += 1; cost[n_iter]
cost[t]: math.fsum of dist over the rows not left out."""
import collections
import math

import numpy as np

NO_CLASS = 0xFFFFFFFF
NAN = float("nan")

KMedoidsRef = collections.namedtuple("KMedoidsRef", "medoid class_of dist own_mean class_rows cost n_iter converged")


def assign_ref(D, medoids):
    """class_of u32 [r], dist f64 [r]"""
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    assert D.shape == (r, r)
    M = [int(m) for m in medoids]
    class_of = np.full(r, NO_CLASS, dtype=np.uint32)
    dist = np.full(r, np.inf)
    if M:
        d = D[:, M] + 0.0  # (-0 + 0 is +0)
        ok = ~np.isnan(d)
        least = np.where(ok, d, np.inf).min(axis=1)
        first = np.argmax(ok & (d == least[:, None]), axis=1)  # the first of the least: c ascending
        kept = ok.any(axis=1)
        class_of[kept] = first[kept].astype(np.uint32)
        dist[kept] = least[kept]
    pos = {}
    for c, m in enumerate(M):  # a medoid belongs to its own position, also when it is a duplicate of an earlier medoid
        pos.setdefault(m, c)
    for m, c in pos.items():
        class_of[m] = c
        dist[m] = 0.0
    return class_of, dist


def own_means_ref(D, class_of, k):
    """own_mean f64 [r], class_rows u32 [k]"""
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    own = np.full(r, NAN)
    rows = np.zeros(k, dtype=np.uint32)
    for c in range(k):
        idx = np.flatnonzero(class_of == c)
        rows[c] = len(idx)
        for j in idx:
            others = idx[idx != j]
            own[j] = math.fsum(D[j, others]) / len(others) if len(others) else 0.0
    return own, rows


def update_ref(own, class_of, medoids):
    out = []
    for c, m in enumerate(medoids):
        cand = [(own[i] + 0.0, int(i)) for i in np.flatnonzero(class_of == c) if own[i] == own[i]]
        out.append(min(cand)[1] if cand else int(m))
    return out


def cost_ref(class_of, dist):
    return math.fsum(dist[class_of != NO_CLASS])


def kmedoids_ref(D, init, max_iter):
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    assert D.shape == (r, r)
    if init is None:
        raise ValueError("init: null")
    M = [int(m) for m in init]
    k = len(M)
    if k == 0 or k > r or any(not 0 <= m < r for m in M) or len(set(M)) != k:
        raise ValueError("init: between 1 and r distinct rows of the set")
    if k > 65535:
        raise NotImplementedError("the 16-bit class key")
    max_iter = int(max_iter)
    class_of, dist = assign_ref(D, M)
    cost = [cost_ref(class_of, dist)]
    n_iter, t = 0, 0
    while True:
        own, rows = own_means_ref(D, class_of, k)
        new = update_ref(own, class_of, M)
        if new == M:
            converged = True
            break
        if t == max_iter:
            converged = False
            break
        M = new
        class_of, dist = assign_ref(D, M)
        n_iter += 1
        t += 1
        cost.append(cost_ref(class_of, dist))
    return KMedoidsRef(np.array(M, dtype=np.uint32), class_of, dist, own, rows, np.array(cost, dtype=np.float64), n_iter, converged)
