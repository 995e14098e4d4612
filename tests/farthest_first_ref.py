"""The farthest-first traversal over a square distance matrix, in numpy: INTEGRATION.md section 6l written down and nothing else.

D[x, c] is the distance of row x to row c (the diagonal is never read).  Every row has a cover distance, +inf at first, and a cover row,
NOISE at first.  Picking row c marks it; for every unpicked row x, D[x, c] replaces the cover distance iff it is a number and strictly
less (-0 taken as +0), and the cover row becomes c.  Pick t < len(seeds) is seeds[t]; every later pick is the unpicked row greatest
under (cover distance descending, row index ascending); before such a pick the traversal stops if that row's cover distance is
<= cover_radius, and it stops at max_picks picks (above the number of rows: that number)."""
import collections

import numpy as np

NOISE = 0xFFFFFFFF

FarthestFirstRef = collections.namedtuple("FarthestFirstRef", "pick pick_radius pick_parent rep_of rep_dist")


def farthest_first_ref(D, max_picks=None, cover_radius=-1.0, seeds=()):
    D = np.asarray(D, dtype=np.float64)
    r = D.shape[0]
    assert D.shape == (r, r)
    if cover_radius != cover_radius:
        raise ValueError("the radius is not a number")
    max_picks = r if max_picks is None else int(max_picks)
    seeds = [int(s) for s in seeds]
    if len(seeds) > max_picks or any(not 0 <= s < r for s in seeds) or len(set(seeds)) != len(seeds):
        raise ValueError("seeds: distinct rows of the set, no more than max_picks")
    max_picks = min(max_picks, r)
    cover = np.full(r, np.inf)
    cover_row = np.full(r, NOISE, dtype=np.uint32)
    picked = np.zeros(r, dtype=bool)
    pick, pick_radius, pick_parent = [], [], []
    while len(pick) < max_picks:
        if len(pick) < len(seeds):
            c = seeds[len(pick)]
        else:
            left = np.flatnonzero(~picked)
            c = int(left[np.argmax(cover[left])])  # the first of the greatest: the smallest row index
            if cover[c] <= cover_radius:
                break
        pick.append(c)
        pick_radius.append(cover[c])
        pick_parent.append(cover_row[c])
        picked[c] = True
        with np.errstate(invalid="ignore"):
            d = D[:, c] + 0.0  # (-0 + 0 is +0)
            nearer = ~picked & (d < cover)  # a NaN compares false
        cover[nearer] = d[nearer]
        cover_row[nearer] = c
    rows = np.arange(r, dtype=np.uint32)
    rep_of = np.where(picked, rows, cover_row).astype(np.uint32)
    rep_dist = np.where(picked, 0.0, cover)
    return FarthestFirstRef(np.array(pick, dtype=np.uint32), np.array(pick_radius, dtype=np.float64), np.array(pick_parent, dtype=np.uint32), rep_of, rep_dist)
