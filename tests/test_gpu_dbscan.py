"""DBSCAN on a resident set (kpop_dbscan, include/kpop_hip.h): degrees, core rows, the clusters of the core rows,
border rows and noise, without the distance matrix.

The contract: labels, core_of, degree and counts array-equal to tests/dbscan_ref.py on the oracle's matrix of the set against
itself, and the same on every run.  For the euclidean and cosine kinds the GPU's distances are the oracle's bit for bit; the Minkowski
kind goes through the GPU's pow, which agrees with the oracle's to rtol 1e-11 (tests/test_gpu_refset.py): there eps is put into a
gap of the oracle's distances of at least 1e-8 relative (asserted), so that no pair is ambiguous, and the result is compared against
dbscan_ref of the GPU's own vector-pipe matrix (tests/test_gpu_clusters.py does the same)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dbscan_ref import NOISE, check_invariants, dbscan_ref

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID = -1
SHAPES = [(130, 9), (1000, 16), (300, 200)]
MIN_PTS = (1, 2, 3, 5)
QUANTILE = 0.01
# eps is the 0.01 quantile of the oracle's matrix.  At 130 x 9 the diagonal's zeros are 0.8 % of the matrix and the normalised cosine
# kind has a single cluster there at min_pts = 3 (18 core, 2 border, 110 noise): that shape takes the 0.03 quantile, at which every
# kind, normalised or not, has 54 to 84 core rows, 3 to 19 border rows, 27 to 73 noise rows and 2 to 9 clusters
QUANTILE_OF = {(130, 9): 0.03}
INF = float("inf")

# the hand-made case of INTEGRATION.md 6i (tests/test_dbscan_ref.py holds the reference's side of it)
HAND_X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
HAND_EPS, HAND_MIN_PTS = 0.375, 4
HAND_DEGREE = [4, 4, 4, 5, 4, 4, 4, 3, 1, 5]
HAND_LABELS = [0, 0, 0, 3, 3, 3, 3, 3, NOISE, 0]
HAND_CORE_OF = [0, 1, 2, 3, 4, 5, 6, 3, NOISE, 9]
HAND_COUNTS = [2, 8, 1]


def clustered_rows(r1, d, seed=None):
    """tests/test_gpu_clusters.py's rows: r1 // 25 centres on a grid of tenths, every row a centre plus noise on a grid of hundredths;
    the last min(40, r1 // 3) rows a chain along dimension 0 in steps of 0.25 from a point at +5; row 7 a duplicate of row 3, row 9
    zero"""
    rng = np.random.RandomState(r1 + d if seed is None else seed)
    centres = np.round(rng.normal(size=(max(r1 // 25, 1), d)), 1)
    m = centres[rng.randint(len(centres), size=r1)] + np.round(0.02 * rng.normal(size=(r1, d)), 2)
    n_chain = min(40, r1 // 3)
    chain = np.full((n_chain, d), 5.0)
    chain[:, 0] += 0.25 * np.arange(n_chain)
    m[r1 - n_chain:] = chain
    if r1 > 12:
        m[7] = m[3]  # a duplicated row: distance zero
        m[9] = 0.0  # a zero row: its norm is replaced by 1 (lib/Matrix.ml:67)
    return m


_operands = {}


def operands(oracle, r1, d):
    """made once a shape, never changed"""
    if (r1, d) not in _operands:
        m = clustered_rows(r1, d)
        metric = oracle.metric_powers(oracle.synth_inertia(d))
        for a in (m, metric):
            a.setflags(write=False)
        _operands[(r1, d)] = (m, metric)
    return _operands[(r1, d)]


def self_matrix(oracle, m, metric, kind, p, normalize):
    """oracle.distance_rowwise(m, m, ...), its query rows in eight slabs on eight threads (a pair's distance depends on its two rows
    alone, and the call holds no state): the Minkowski kind's pow costs seconds on one"""
    r1 = m.shape[0]
    cuts = np.linspace(0, r1, 9).astype(int)
    with ThreadPoolExecutor(8) as pool:
        slabs = list(pool.map(lambda k: oracle.distance_rowwise(m, m[cuts[k]:cuts[k + 1]], metric, kind, p, normalize), range(8)))
    return np.vstack([s for s in slabs if s.shape[0]]) if r1 else np.zeros((0, 0))


_matrices = {}


def oracle_matrix(oracle, r1, d, kind, p, normalize):
    """the oracle's r1 x r1 matrix of a shape's rows against themselves: computed once, shared, read-only"""
    key = (r1, d, kind, normalize)
    if key not in _matrices:
        m, metric = operands(oracle, r1, d)
        D = self_matrix(oracle, m, metric, kind, p, normalize)
        D.setflags(write=False)
        _matrices[key] = D
    return _matrices[key]


def on_the_vector_pipe(rs, m2):
    from kpop_amd import api
    api.tune("distance_mfma", 0)
    try:
        return rs.distance_rowwise(m2)
    finally:
        api.tune("distance_mfma", 1)


def gap_threshold(D, q):
    """tests/test_gpu_clusters.py's rule: the midpoint of the first two consecutive distinct oracle distances at or above the q-quantile
    that lie >= 1e-8 (relative) apart"""
    u = np.unique(D[np.isfinite(D)])
    k = int(np.searchsorted(u, np.quantile(D, q)))
    while k + 1 < len(u) and not (u[k + 1] - u[k] >= 1e-8 * u[k + 1]):
        k += 1
    assert k + 1 < len(u)
    gap = (u[k + 1] - u[k]) / u[k + 1]
    print("    Minkowski eps at quantile %s: relative gap %.3g" % (q, gap))
    assert gap >= 1e-8
    return (u[k] + u[k + 1]) / 2


def eps_of(D, kind, q=QUANTILE):
    return float(np.quantile(D, q)) if kind != 2 else gap_threshold(D, q)


def kinds_of_rows(ref, min_pts):
    """(core, border, noise, clusters) of a reference result"""
    labels, _, degree, counts = ref
    core = degree >= min_pts
    noise = labels == NOISE
    return int(core.sum()), int(np.sum(~core & ~noise)), int(noise.sum()), int(counts[0])


def check_result(got, want, what):
    for name, g, w in zip(("labels", "core_of", "degree", "counts"), got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int(np.sum(g != w)))


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_dbscan_vs_oracle(kpop, oracle, r1, d, kind, p):
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize)
        D = oracle_matrix(oracle, r1, d, kind, p, normalize)
        eps = eps_of(D, kind, QUANTILE_OF.get((r1, d), QUANTILE))
        # the reference alone, before the GPU is asked: at min_pts = 3 there are core rows, border rows, noise and several clusters
        n_core, n_border, n_noise, n_clusters = kinds_of_rows(dbscan_ref(D, eps, 3), 3)
        print("  %s eps=%.17g min_pts=3: %d core, %d border, %d noise, %d clusters" % (what, eps, n_core, n_border, n_noise, n_clusters))
        assert n_core >= 1 and n_border >= 1 and n_noise >= 1 and n_clusters >= 2, what
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            of = on_the_vector_pipe(rs, m) if kind == 2 else D
            for min_pts in MIN_PTS:
                want = dbscan_ref(of, eps, min_pts)
                got = rs.dbscan(eps, min_pts)
                print("  %s min_pts=%d: %d core, %d border, %d noise, %d clusters" % ((what, min_pts) + kinds_of_rows(want, min_pts)))
                check_result(got, want, (what, min_pts))
                check_invariants(*got, min_pts)
        finally:
            rs.free()


def hand_rows():
    m = np.zeros((len(HAND_X), 3))
    m[:, 0] = HAND_X
    return m


def check_hand(got, what):
    labels, core_of, degree, counts = got
    assert degree.tolist() == HAND_DEGREE, what
    assert labels.tolist() == HAND_LABELS, what
    assert core_of.tolist() == HAND_CORE_OF, what
    assert counts.tolist() == HAND_COUNTS, what


def test_the_hand_made_case(kpop):
    import torch
    from kpop_amd import api
    m, metric = hand_rows(), np.ones(3)
    check_hand(kpop.distance_dbscan(m, metric, 0, 2.0, False, HAND_EPS, HAND_MIN_PTS), "distance_dbscan")
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        check_hand(rs.dbscan(HAND_EPS, HAND_MIN_PTS), "RefSet.dbscan")
        dev = torch.device("cuda:0")
        n = len(HAND_X)
        work = torch.empty(max(api.dev_dbscan_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
        labels, core_of, degree = (torch.full((n,), -3, dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.full((3,), -3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            api.dev_dbscan(rs, HAND_EPS, HAND_MIN_PTS, work.data_ptr(), labels.data_ptr(), core_of.data_ptr(), degree.data_ptr(), counts.data_ptr(),
                           stream=stream.cuda_stream)
        stream.synchronize()
        check_hand(tuple(t.cpu().numpy().view(np.uint32) for t in (labels, core_of, degree, counts)), "the device form")
    finally:
        rs.free()
    # the same rows in another order: the labels are the smallest core row index of each cluster
    other = np.zeros((n, 3))
    other[:, 0] = [1.125, 1.25, 1.375, 1.5, 0.75, 0.0, 0.125, 0.25, 0.375, 5.0]
    labels, core_of, degree, counts = kpop.distance_dbscan(other, metric, 0, 2.0, False, HAND_EPS, HAND_MIN_PTS)
    assert labels.tolist() == [0, 0, 0, 0, 0, 5, 5, 5, 5, NOISE] and core_of[4] == 0 and counts.tolist() == HAND_COUNTS


def test_relations_to_the_clusters_and_the_range_query(kpop, oracle):
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        D = oracle_matrix(oracle, r1, d, 0, 2.0, normalize)
        eps = float(np.quantile(D, QUANTILE))
        rs = kpop.RefSet(m, metric, 0, 2.0, normalize)
        try:
            single, n_single = rs.clusters(eps)
            sizes = np.bincount(single, minlength=r1)[single]
            assert np.any(sizes == 1) and np.any(sizes > 1)
            # min_pts = 1: the clusters at that distance, bit for bit, and no noise
            labels, core_of, degree, counts = rs.dbscan(eps, 1)
            assert np.array_equal(labels, single) and np.array_equal(core_of, np.arange(r1)) and counts.tolist() == [n_single, r1, 0]
            # min_pts = 2: a component of two or more rows keeps its label, a singleton is noise
            labels2, _, degree2, counts2 = rs.dbscan(eps, 2)
            assert np.array_equal(labels2, np.where(sizes == 1, NOISE, single).astype(np.uint32))
            assert counts2.tolist() == [int(np.sum((single == np.arange(r1)) & (sizes > 1))), int(np.sum(sizes > 1)), int(np.sum(sizes == 1))]
            # the degree is the length of the row's list in the range query, which holds the row itself at distance 0
            offsets, idx, dist = rs.within(m, eps)
            lengths = np.diff(offsets.astype(np.int64))
            assert np.all(np.isfinite(m)) and np.array_equal(degree.astype(np.int64), lengths) and np.array_equal(degree2, degree)
            assert np.all(idx[offsets[:-1].astype(np.int64)] <= np.arange(r1)) and np.all(dist[offsets[:-1].astype(np.int64)] == 0.0)
        finally:
            rs.free()


def test_invariants_and_three_runs(kpop, oracle):
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for kind, p in KINDS:
        D = oracle_matrix(oracle, r1, d, kind, p, True)
        rs = kpop.RefSet(m, metric, kind, p, True)
        try:
            for eps in (float(np.quantile(D, 0.01)), float(np.quantile(D, 0.05))):
                for min_pts in (3, 8):
                    first = rs.dbscan(eps, min_pts)
                    check_invariants(*first, min_pts)
                    for _ in range(2):
                        again = rs.dbscan(eps, min_pts)
                        for a, b in zip(first, again):
                            assert np.array_equal(a, b), (kind, eps, min_pts)
        finally:
            rs.free()


def test_a_nan_row_and_a_zero_row(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    bad = np.array(m)
    bad[20, 4] = np.nan
    assert not bad[9].any()
    for kind, p in KINDS[:2]:
        for normalize in (True, False):
            D = self_matrix(oracle, bad, metric, kind, p, normalize)
            assert np.all(np.isnan(np.delete(D[20], 20))) and np.all(np.isnan(np.delete(D[:, 20], 20)))
            rs = kpop.RefSet(bad, metric, kind, p, normalize)
            try:
                for eps in (float(np.nanquantile(D, 0.05)), INF):
                    for min_pts in (1, 2, 3):
                        want = dbscan_ref(D, eps, min_pts)
                        got = rs.dbscan(eps, min_pts)
                        check_result(got, want, (kind, normalize, eps, min_pts))
                        assert got[2][20] == 1 and got[0][20] == (20 if min_pts == 1 else NOISE)
                        if eps == INF:
                            # the zero row (its norm is replaced by 1, lib/Matrix.ml:67) is a row like any other: its degree is
                            # the number of its distances that are numbers, itself included
                            assert got[2][9] == 1 + int(np.sum(~np.isnan(np.delete(D[9], 9)))) and got[2][9] >= 2
            finally:
                rs.free()


def test_a_dense_set(kpop):
    """600 identical rows and 10 far ones: every pair of the 600 is a hit, 179,700 of them in a few tiles -- what the counters in LDS
    and the one add a node must not lose"""
    d, eps = 16, 0.5
    rng = np.random.RandomState(610)
    m = np.zeros((610, d))
    m[:5] = 100.0 * np.arange(1, 6)[:, None]
    m[5:605] = np.round(rng.normal(size=d), 2)
    m[605:] = -100.0 * np.arange(1, 6)[:, None]
    rs = kpop.RefSet(m, np.ones(d), 0, 2.0, False)
    try:
        labels, core_of, degree, counts = rs.dbscan(eps, 600)
        assert np.all(degree[5:605] == 600) and np.all(degree[:5] == 1) and np.all(degree[605:] == 1)
        assert np.all(labels[5:605] == 5) and np.all(labels[:5] == NOISE) and np.all(labels[605:] == NOISE)
        assert np.array_equal(core_of[5:605], np.arange(5, 605)) and counts.tolist() == [1, 600, 10]  # one cluster, no border row
        labels, core_of, degree, counts = rs.dbscan(eps, 601)
        assert np.all(labels == NOISE) and np.all(core_of == NOISE) and counts.tolist() == [0, 0, 610]
        assert np.all(degree[5:605] == 600)
    finally:
        rs.free()


def test_beyond_65535_rows(kpop):
    """70,000 rows take the tiles of a long set (32 columns x 256 rows) and fold grid.y.  No quadratic reference: groups of 1 .. 6 rows
    on centres of a lattice of step 4, every row its centre plus noise of at most 0.01 a coordinate, eps = 0.375 -- by the triangle
    inequality every pair of one group lies below eps and every pair of two groups above it, so that a row's degree is its group's
    size; the groups' rows are scattered over the set.  At min_pts = 4 a group of four or more is a cluster under its first row and
    every smaller one is noise.  The hand-made case sits on a far centre of its own, its ten rows in order and thousands of rows apart:
    the border row and its tie between two core rows cross the tiles.  256 sampled rows are recounted from their rows of the
    vector-pipe matrix"""
    r1, d, step, noise, eps, min_pts = 70000, 8, 4.0, 0.01, HAND_EPS, HAND_MIN_PTS
    rng = np.random.RandomState(70008)
    n_hand = len(HAND_X)
    sizes = np.tile(np.arange(1, 7), (r1 - n_hand) // 21 + 1)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), r1 - n_hand)) + 1].copy()
    sizes[-1] -= int(sizes.sum()) - (r1 - n_hand)
    assert sizes.sum() == r1 - n_hand and sizes.min() >= 1 and len(sizes) < 4 ** d
    group_of = np.repeat(np.arange(len(sizes)), sizes)
    centres = step * np.array([[(c // 4 ** k) % 4 for k in range(d)] for c in range(len(sizes))], dtype=np.float64)
    spread = 2.0 * noise * np.sqrt(d)  # two rows of one centre at most
    assert spread < eps / 1.5 and step - spread > 10 * eps
    hand_at = np.arange(n_hand) * 6997 + 33  # ascending: the hand-made rows keep their order
    others = np.setdiff1d(np.arange(r1), hand_at)
    where = others[rng.permutation(len(others))]  # where[k]: the row of the k-th member
    m = np.zeros((r1, d))
    m[where] = centres[group_of] + rng.uniform(-noise, noise, size=(len(where), d))
    m[hand_at] = -64.0  # far from the lattice, which lies in [0, 12]
    m[hand_at, 0] += HAND_X
    want_degree = np.zeros(r1, dtype=np.int64)
    want_degree[where] = sizes[group_of]
    want_degree[hand_at] = HAND_DEGREE
    first = np.full(len(sizes), r1, dtype=np.int64)
    np.minimum.at(first, group_of, where)
    want_labels = np.zeros(r1, dtype=np.int64)
    want_labels[where] = np.where(sizes[group_of] >= min_pts, first[group_of], NOISE)
    hand_map = np.append(hand_at, NOISE)  # (the last entry: NOISE stays NOISE)
    want_labels[hand_at] = hand_map[np.where(np.array(HAND_LABELS) == NOISE, n_hand, HAND_LABELS)]
    want_core_of = np.where(want_degree >= min_pts, np.arange(r1), NOISE)
    want_core_of[hand_at] = hand_map[np.where(np.array(HAND_CORE_OF) == NOISE, n_hand, HAND_CORE_OF)]
    rs = kpop.RefSet(m, np.ones(d), 0, 2.0, False)
    try:
        labels, core_of, degree, counts = rs.dbscan(eps, min_pts)
        assert np.array_equal(degree, want_degree)
        assert np.array_equal(labels, want_labels)
        assert np.array_equal(core_of, want_core_of)
        assert counts.tolist() == [int(np.sum(sizes >= min_pts)) + 2, int(np.sum(want_degree >= min_pts)), int(np.sum(want_labels == NOISE))]
        check_invariants(labels, core_of, degree, counts, min_pts)
        again = rs.dbscan(eps, min_pts)
        assert all(np.array_equal(a, b) for a, b in zip(again, (labels, core_of, degree, counts)))
        sample = np.concatenate([hand_at, rng.choice(others, 256 - n_hand, replace=False)])
        G = on_the_vector_pipe(rs, m[sample])
        assert G.shape == (256, r1)
        assert np.array_equal(np.sum(G <= eps, axis=1), degree[sample])  # (the row itself is in its list, at distance 0)
    finally:
        rs.free()


def raw_dbscan(rs_handle, eps, min_pts, labels, core_of, degree, counts):
    from kpop_amd import _lib
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    return _lib.load().kpop_dbscan(rs_handle, eps, min_pts, ptr(labels), ptr(core_of), ptr(degree), ptr(counts))


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    eps = float(np.quantile(D, 0.05))
    want = dbscan_ref(D, eps, 3)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        for bad_eps, bad_min_pts in ((float("nan"), 3), (eps, 0), (float("nan"), 0)):
            with pytest.raises(kpop.KPopError) as e:
                rs.dbscan(bad_eps, bad_min_pts)
            assert e.value.code == ERR_INVALID and "kpop_dbscan" in str(e.value)
            with pytest.raises(kpop.KPopError) as e:
                kpop.distance_dbscan(m, metric, 0, 2.0, True, bad_eps, bad_min_pts)
            assert e.value.code == ERR_INVALID
        check_result(kpop.distance_dbscan(m, metric, 0, 2.0, True, eps, 3), want, "distance_dbscan")
        # eps < 0: every degree is 1
        labels, core_of, degree, counts = rs.dbscan(-1.0, 1)
        assert np.array_equal(labels, np.arange(r1)) and np.array_equal(core_of, np.arange(r1)) and np.all(degree == 1)
        assert counts.tolist() == [r1, r1, 0]
        labels, core_of, degree, counts = rs.dbscan(-1.0, 2)
        assert np.all(labels == NOISE) and np.all(core_of == NOISE) and np.all(degree == 1) and counts.tolist() == [0, 0, r1]
        # min_pts > r1: all noise, even where every row lies within every other; at r1 itself one cluster of core rows
        labels, core_of, degree, counts = rs.dbscan(INF, r1 + 1)
        assert np.all(labels == NOISE) and np.all(degree == r1) and counts.tolist() == [0, 0, r1]
        assert rs.dbscan(INF, r1)[3].tolist() == [1, r1, 0]
        assert rs.dbscan(INF, 0xFFFFFFFF)[3].tolist() == [0, 0, r1]
        # core_of and degree may be NULL; labels and counts may not
        labels, counts = np.zeros(r1, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
        assert raw_dbscan(rs.handle, eps, 3, labels, None, None, counts) == 0
        assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[3])
        only_degree = np.zeros(r1, dtype=np.uint32)
        assert raw_dbscan(rs.handle, eps, 3, labels, None, only_degree, counts) == 0 and np.array_equal(only_degree, want[2])
        assert raw_dbscan(rs.handle, eps, 3, None, None, None, counts) == ERR_INVALID
        assert raw_dbscan(rs.handle, eps, 3, labels, None, None, None) == ERR_INVALID
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.dbscan(eps, 3)
    assert e.value.code == ERR_INVALID
    assert raw_dbscan(None, eps, 3, np.zeros(r1, dtype=np.uint32), None, None, np.zeros(3, dtype=np.uint32)) == ERR_INVALID
    # an empty set: KPOP_OK and the counts all zero -- the error of a bad argument still comes first
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        labels, core_of, degree, counts = empty.dbscan(eps, 3)
        assert labels.size == 0 and core_of.size == 0 and degree.size == 0 and counts.tolist() == [0, 0, 0]
        with pytest.raises(kpop.KPopError):
            empty.dbscan(eps, 0)
    finally:
        empty.free()
    assert kpop.distance_dbscan(np.zeros((0, d)), metric, 0, 2.0, True, eps, 3)[3].tolist() == [0, 0, 0]


def test_device_form_on_streams(kpop, oracle):
    """kpop_dev_dbscan with its own workspace on a stream of the caller's; two sets on two streams with different (eps, min_pts), back
    to back, give what the host form gives; core_of and degree may be NULL"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    cases = [(1000, 16, 0, 2.0, True, 0.01, 3), (300, 200, 1, 2.0, False, 0.05, 5)]
    sets, wants, bufs, streams = [], [], [], []
    try:
        for r1, d, kind, p, normalize, q, min_pts in cases:
            m, metric = operands(oracle, r1, d)
            eps = float(np.quantile(oracle_matrix(oracle, r1, d, kind, p, normalize), q))
            rs = kpop.RefSet(m, metric, kind, p, normalize)
            sets.append((rs, eps, min_pts, r1))
            wants.append(rs.dbscan(eps, min_pts))  # the host form (checked against the oracle above)
            work = torch.empty(max(api.dev_dbscan_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)  # reserved ahead
            out = tuple(torch.full((r1,), -3, dtype=torch.int32, device=dev) for _ in range(3))
            counts = torch.full((3,), -3, dtype=torch.int32, device=dev)
            bufs.append((work, out, counts))
            streams.append(torch.cuda.Stream(device=dev))
        torch.cuda.synchronize()

        def enqueue(k, with_optional=True):
            rs, eps, min_pts, _ = sets[k]
            work, (labels, core_of, degree), counts = bufs[k]
            api.dev_dbscan(rs, eps, min_pts, work.data_ptr(), labels.data_ptr(), core_of.data_ptr() if with_optional else None,
                           degree.data_ptr() if with_optional else None, counts.data_ptr(), stream=streams[k].cuda_stream)

        def result(k):
            _, out, counts = bufs[k]
            return tuple(t.cpu().numpy().view(np.uint32) for t in out + (counts,))

        # each alone on its stream, twice on the same buffers: nothing is left over from the first call
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                enqueue(k)
                enqueue(k)
            streams[k].synchronize()
            check_result(result(k), wants[k], "device form")
        for _, out, counts in bufs:
            for t in out + (counts,):
                t.fill_(-3)
        torch.cuda.synchronize()
        # both enqueued before either is waited for
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                enqueue(k)
        for stream in streams:
            stream.synchronize()
        for k in range(2):
            check_result(result(k), wants[k], "two streams")
        # without core_of and degree: they are not written, the rest is the same
        for t in bufs[0][1] + (bufs[0][2],):
            t.fill_(-3)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            enqueue(0, with_optional=False)
        streams[0].synchronize()
        labels, core_of, degree, counts = result(0)
        assert np.array_equal(labels, wants[0][0]) and np.array_equal(counts, wants[0][3])
        assert np.all(core_of.view(np.int32) == -3) and np.all(degree.view(np.int32) == -3)
        # the arguments of the device form
        rs, eps, min_pts, _ = sets[0]
        work, (labels_t, _, _), counts_t = bufs[0]
        for args in ((float("nan"), 3, work.data_ptr(), labels_t.data_ptr(), counts_t.data_ptr()), (eps, 0, work.data_ptr(), labels_t.data_ptr(), counts_t.data_ptr()),
                     (eps, 3, None, labels_t.data_ptr(), counts_t.data_ptr()), (eps, 3, work.data_ptr(), None, counts_t.data_ptr()),
                     (eps, 3, work.data_ptr(), labels_t.data_ptr(), None)):
            with pytest.raises(kpop.KPopError) as e:
                api.dev_dbscan(rs, args[0], args[1], args[2], args[3], None, None, args[4], stream=streams[0].cuda_stream)
            assert e.value.code == ERR_INVALID and "kpop_dev_dbscan" in str(e.value)
        torch.cuda.synchronize()
    finally:
        for rs, _, _, _ in sets:
            rs.free()
