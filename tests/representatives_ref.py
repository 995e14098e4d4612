"""The numpy reference of the representatives at a distance: the greedy cover of the rows in row order,
from a square distance matrix of which the lower triangle alone is read (D[j, i], i < j)."""
import numpy as np


def representatives_ref(D, T, known=None):
    """-> (rep_of u32 [r], rep_dist f64 [r], n_reps).  Row i is a representative iff no representative r < i has D[i, r] <= T (a NaN
    compares false); any other row goes to the representative below it that is least under (D[i, r] with -0 taken as +0, r).  known: the
    rep_of of the first len(known) rows, taken as they are (their rep_dist is read off the matrix)."""
    T = float(T)
    if T != T:
        raise ValueError("the distance is not a number")
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    rep_of = np.zeros(r, dtype=np.uint32)
    rep_dist = np.zeros(r, dtype=np.float64)
    reps = []
    n_known = 0 if known is None else len(known)
    for i in range(n_known):
        rep_of[i] = known[i]
        if known[i] == i:
            reps.append(i)
        else:
            rep_dist[i] = D[i, known[i]] + 0.0  # (-0 + 0 is +0)
    for i in range(n_known, r):
        best = None
        if reps:
            d = D[i, reps] + 0.0
            with np.errstate(invalid="ignore"):
                hit = d <= T
            if hit.any():
                dd = np.where(hit, d, np.inf)
                k = int(np.argmin(dd))  # the first of the least: positions ascend with the representatives' indices
                if hit[k]:
                    best = k
                else:  # every hit lies at +inf (T is +inf): the first hit
                    best = int(np.argmax(hit))
        if best is None:
            rep_of[i] = i
            reps.append(i)
        else:
            rep_of[i] = reps[best]
            rep_dist[i] = D[i, reps[best]] + 0.0
    return rep_of, rep_dist, len(reps)


def check_invariants(D, T, rep_of):
    """whether rep_of satisfies the invariants of section 6h over the matrix D at T: those that determine the result"""
    r = len(rep_of)
    with np.errstate(invalid="ignore"):
        for i in range(r):
            ri = int(rep_of[i])
            if ri > i or rep_of[ri] != ri:
                return False
        reps = [i for i in range(r) if rep_of[i] == i]
        for a in reps:
            for b in reps:
                if b < a and D[a, b] <= T:
                    return False
        for i in range(r):
            ri = int(rep_of[i])
            if ri == i:
                continue
            if not D[i, ri] <= T:
                return False
            # the least under (d, r) among the representatives below the row
            for b in reps:
                if b < i and D[i, b] <= T and (D[i, b] + 0.0, b) < (D[i, ri] + 0.0, ri):
                    return False
    return True
