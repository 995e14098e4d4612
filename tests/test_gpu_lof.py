"""The local outlier factor of a resident set and of query rows against it (kpop_lof, kpop_lof_score, include/kpop_hip.h;
INTEGRATION.md 6n), without the distance matrix.

The contract: over the oracle's matrix -- for the euclidean and cosine kinds the bits of the reference chain -- the four arrays of
tests/lof_ref.py, whose sums are math.fsum's.  For the Minkowski kind the matrix is the library's own on the vector pipe, for the
reason tests/test_gpu_silhouette.py gives (the GPU's pow agrees with the oracle's to rtol 1e-11 only), held to the oracle's at that rtol.

THE BOUNDS, derived and not measured.  kdist and n_neigh are exact on every case: the k-distance is an order statistic of bit-exact
distances and membership a comparison of them, so no case is left out and no cap is needed.  With n = n_neigh.max() of the case and
u = 2^-53: a sum of at most n non-negative terms in any order lies within n u relative of the exact one (every partial sum is at most
the total, every addition rounds once), and the reference's sum is the exact one rounded once more.  lrd is one division of such a
sum on each side: within (n + 2) u relative.  lof is a sum of n such values (each within (n + 2) u, the sum's own n u on top), a
division by the count and one by lrd (another (n + 2) u), with the reference's own roundings: within 4 (n + 2) u relative, first
order, with room.  Where every coordinate is dyadic and one-dimensional S1 is exact and one division is correctly rounded on both
sides: lrd holds bit for bit.  Infinities and NaNs are compared by class (and a declared NaN by its bits), never by tolerance.

THE SEGMENTS, under lof_segments of lof.hip (at most 16, at most one a column tile of 64 rows below 65,536 rows, as many as make 2,048
workgroups with the row strips): a set of 300 rows is swept in 5 segments, 129 rows in 3, 65 in 2, up to 64 rows in 1; 3 query rows
against 2,000 rows in 16 segments, against 60 rows in 1; 65,600 rows (tiles of 32 columns) in 8 segments, 3 query rows against them in 16."""
import ctypes as C

import numpy as np
import pytest

from lof_ref import QNAN_BITS, U, lof_ref, lof_rows_ref, lof_score_ref, neighbourhood_max, same_bits
from test_lof_ref import (HAND_K, HAND_KDIST, HAND_LOF, HAND_LRD, HAND_N, HAND_Q, HAND_Q_KDIST, HAND_Q_LOF, HAND_Q_LRD, HAND_Q_N, HAND_X)

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
NAMES = ("kdist", "n_neigh", "lrd", "lof")
INF = float("inf")


def line_rows(x, n_dims):
    m = np.zeros((len(x), n_dims))
    m[:, 0] = x
    return m


def dyadic(rng, n, below=8192):
    """multiples of 1/8 below 2^10"""
    return rng.randint(0, below, size=n) / 8.0


def on_the_vector_pipe(rs, m2):
    from kpop_amd import api
    api.tune("distance_mfma", 0)
    try:
        return rs.distance_rowwise(m2)
    finally:
        api.tune("distance_mfma", 1)


def all_same_bits(got, want):
    return all(np.array_equal(g, w) if w.dtype == np.uint32 else same_bits(g, w) for g, w in zip(got, want))


def within(g, w, bound, what):
    """infinities and NaNs by class, the rest within bound relative"""
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    assert np.array_equal(np.isinf(g), np.isinf(w)) and not np.any(np.signbit(g[~np.isnan(g)])), what
    assert np.all(g[np.isnan(g)].view(np.uint64) == QNAN_BITS), what  # every NaN written is the declared one
    ok = np.isfinite(w)
    err = float(np.max(np.abs(g[ok] - w[ok]) / np.where(w[ok] == 0, 1.0, w[ok]))) if ok.any() else 0.0
    print("    %s: relative error %.3g of %.3g" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def check(got, want, what, exact_sums=False):
    assert tuple(got._fields) == NAMES and all(g.shape == w.shape for g, w in zip(got, want)), what
    assert got.kdist.dtype == np.float64 and same_bits(got.kdist, want.kdist), (what, "kdist")
    assert got.n_neigh.dtype == np.uint32 and np.array_equal(got.n_neigh, want.n_neigh), (what, "n_neigh")
    n = neighbourhood_max(want.n_neigh)
    if exact_sums:
        assert same_bits(got.lrd, want.lrd), (what, "lrd")
    within(got.lrd, want.lrd, (n + 2) * U, (what, "lrd"))
    within(got.lof, want.lof, 4 * (n + 2) * U, (what, "lof"))


def exact_set(kpop, oracle, x, n_dims):
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False) if len(x) else np.zeros((0, 0))
    assert np.array_equal(D, np.abs(np.subtract.outer(np.asarray(x, dtype=np.float64), x)))  # every distance is exact
    return kpop.RefSet(m, metric, 0, 2.0, False), D


# (r1, n_dims); k: the strip heights of the k-NN lists (k <= 32, <= 64, more) and their edges, and one k >= r1 a size
SIZES = [(1, 1), (2, 3), (3, 16), (63, 17), (64, 33), (65, 1), (129, 3), (300, 16), (129, 16)]
KS = (1, 2, 32, 33, 64, 65, 128)


@pytest.mark.parametrize("r1,n_dims", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_exact_sizes(kpop, oracle, r1, n_dims):
    rng = np.random.RandomState(1000 * r1 + n_dims)
    rs, D = exact_set(kpop, oracle, dyadic(rng, r1), n_dims)
    try:
        for k in dict.fromkeys([k for k in KS if k < r1] + [min(r1, 128)]):  # (the last one: k >= r1 wherever 128 allows it)
            got = rs.lof(k)
            check(got, lof_ref(D, k), (r1, n_dims, k), exact_sums=True)
            assert same_bits(got.kdist, rs.core_distances(k + 1)), (r1, k)
            if k >= r1:
                assert np.all(got.kdist.view(np.uint64) == QNAN_BITS) and not got.n_neigh.any()
    finally:
        rs.free()


def test_exact_copies_and_ties(kpop, oracle):
    """sixteen values for 150 rows: clumps of more than k copies (lrd +inf, lof 1.0), rows beside them (+inf), tie groups taken whole"""
    rng = np.random.RandomState(5)
    rs, D = exact_set(kpop, oracle, dyadic(rng, 150, below=16), 17)
    try:
        for k in (1, 4, 20, 40):
            got = rs.lof(k)
            want = lof_ref(D, k)
            check(got, want, ("copies", k), exact_sums=True)
            assert same_bits(got.kdist, rs.core_distances(k + 1))
        assert np.any(np.isinf(rs.lof(4).lrd)) and np.any(rs.lof(4).n_neigh > 4)
    finally:
        rs.free()


def test_the_worked_case(kpop, oracle):
    rs, D = exact_set(kpop, oracle, HAND_X, 3)
    try:
        got = rs.lof(HAND_K)
        check(got, lof_ref(D, HAND_K), "INTEGRATION.md 6n", exact_sums=True)
        assert got.kdist.tolist() == HAND_KDIST and got.n_neigh.tolist() == HAND_N and got.lrd.tolist() == HAND_LRD and got.lof.tolist() == HAND_LOF
        q = line_rows(HAND_Q, 3)
        score = rs.lof_score(q, HAND_K, got.kdist, got.lrd)
        check(score, lof_score_ref(oracle.distance_rowwise(line_rows(HAND_X, 3), q, np.ones(3), 0, 2.0, False), HAND_K, got.kdist, got.lrd), "6n, queries",
              exact_sums=True)
        assert score.kdist.tolist() == HAND_Q_KDIST and score.n_neigh.tolist() == HAND_Q_N and score.lrd.tolist() == HAND_Q_LRD
        assert score.lof.tolist() == HAND_Q_LOF
        assert all_same_bits(kpop.distance_lof(line_rows(HAND_X, 3), np.ones(3), HAND_K, 0, 2.0, False), got)
    finally:
        rs.free()


RANDOM = [(300, 5, 0), (300, 5, 1), (300, 5, 2), (257, 40, 0), (257, 40, 1), (257, 40, 2)]


@pytest.mark.parametrize("r1,n_dims,kind", RANDOM, ids=["%dx%d-%s" % (r, d, ("euclidean", "cosine", "minkowski")[k]) for r, d, k in RANDOM])
def test_random_rows(kpop, oracle, r1, n_dims, kind):
    """both forms on rows whose sums are not exact; 300 and 257 rows are swept in 5 segments"""
    p = KINDS[kind][1]
    rng = np.random.RandomState(500 + 10 * n_dims + kind)
    m, m2 = rng.normal(size=(r1, n_dims)), rng.normal(size=(37, n_dims))
    m2[5] = m[11]  # a query equal to a set row
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    for normalize in (True, False):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            D = oracle.distance_rowwise(m, m, metric, kind, p, normalize)
            E = oracle.distance_rowwise(m, m2, metric, kind, p, normalize)
            if kind == 2:
                G, H = on_the_vector_pipe(rs, m), on_the_vector_pipe(rs, m2)
                off = ~np.eye(r1, dtype=bool)
                assert np.allclose(G[off], D[off], rtol=1e-11, atol=0) and np.allclose(H, E, rtol=1e-11, atol=1e-300)
                D, E = G, H
            for k in (5, 20):
                what = (r1, n_dims, kind, normalize, k)
                got = rs.lof(k)
                check(got, lof_ref(D, k), what)
                assert same_bits(got.kdist, rs.core_distances(k + 1)), what
                assert np.any(got.lrd != np.round(got.lrd * 8) / 8)  # (not the exact kind of case)
                score = rs.lof_score(m2, k, got.kdist, got.lrd)
                check(score, lof_score_ref(E, k, got.kdist, got.lrd), what + ("queries",))
                assert score.kdist[5] <= got.kdist[11]  # row 11 itself, at its own distance, is one of the k
        finally:
            rs.free()


def device_forms(kpop, rs, k, m2, guard=8):
    """kpop_dev_lof and kpop_dev_lof_score on a stream of the caller's, each with its own workspace -> (Lof, Lof, every guard untouched)"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, r2 = rs.info()["r1"], len(m2)
    types = [torch.float64, torch.int32, torch.float64, torch.float64]

    def outputs(n):
        return [torch.full((n + guard,), -3, dtype=t, device=dev) for t in types]

    def guarded(nbytes):
        return torch.full((max(nbytes, 1) + 64,), 0xA5, dtype=torch.uint8, device=dev)

    def result(outs, n, work, nbytes):
        host = [t.cpu().numpy() for t in outs]
        host = [a.view(np.uint32) if a.dtype == np.int32 else a for a in host]
        clean = all(np.all(a[n:] == (-3.0 if a.dtype == np.float64 else 0xFFFFFFFD)) for a in host)
        clean = clean and bool(torch.all(work[max(nbytes, 1):] == 0xA5).item())
        return kpop.Lof(*[a[:n] for a in host]), clean

    set_bytes, score_bytes = api.dev_lof_workspace_bytes(rs, k), api.dev_lof_score_workspace_bytes(rs, r2, k)
    work, work2 = guarded(set_bytes), guarded(score_bytes)
    outs, outs2 = outputs(r1), outputs(r2)
    d_m2 = torch.from_numpy(np.ascontiguousarray(m2)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        api.dev_lof(rs, k, work.data_ptr(), *[t.data_ptr() for t in outs], stream=stream.cuda_stream)
        api.dev_lof_score(rs, k, outs[0].data_ptr(), outs[2].data_ptr(), d_m2.data_ptr(), r2, work2.data_ptr(), *[t.data_ptr() for t in outs2],
                          stream=stream.cuda_stream)
    stream.synchronize()
    a, clean_a = result(outs, r1, work, set_bytes)
    b, clean_b = result(outs2, r2, work2, score_bytes)
    return a, b, clean_a and clean_b


SEGMENTS = [(300, 9, 40, "5 segments, 40 query rows in 5"), (2000, 16, 3, "16 segments"), (60, 16, 3, "1 segment")]


@pytest.mark.parametrize("r1,n_dims,r2,what", SEGMENTS, ids=["%dx%d-%d" % s[:3] for s in SEGMENTS])
def test_segments_runs_and_device_forms(kpop, oracle, r1, n_dims, r2, what):
    """more than one segment and one; identical on a second run; the device forms on a stream of the caller's equal the host forms and
    stay inside their workspace and their outputs.  The set of 2,000 rows is not held to the quadratic reference: its query rows are,
    over the oracle's 3 x 2,000 distances, with the set's arrays passed in"""
    rng = np.random.RandomState(r1 + r2)
    m, m2 = rng.normal(size=(r1, n_dims)), rng.normal(size=(r2, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    for kind, p, normalize, k in ((0, 2.0, True, 20), (1, 2.0, False, 7)):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            first = rs.lof(k)
            assert all_same_bits(rs.lof(k), first), "a second run"
            if r1 <= 300:
                check(first, lof_ref(oracle.distance_rowwise(m, m, metric, kind, p, normalize), k), (what, kind))
            assert same_bits(first.kdist, rs.core_distances(k + 1)) and np.all(first.n_neigh >= k)
            score = rs.lof_score(m2, k, first.kdist, first.lrd)
            assert all_same_bits(rs.lof_score(m2, k, first.kdist, first.lrd), score), "a second run, queries"
            check(score, lof_score_ref(oracle.distance_rowwise(m, m2, metric, kind, p, normalize), k, first.kdist, first.lrd), (what, kind, "queries"))
            dev_set, dev_score, clean = device_forms(kpop, rs, k, m2)
            assert all_same_bits(dev_set, first) and all_same_bits(dev_score, score) and clean, (what, kind)
            assert all_same_bits(kpop.distance_lof(m, metric, k, kind, p, normalize), first)
        finally:
            rs.free()


def test_the_long_set_tile_shape(kpop, oracle):
    """65,600 rows take the tiles of a long set (32 columns x 256 rows, a thread 4 x 8), the set form in 8 segments and 3 query rows in
    16.  No quadratic reference: 20 rows against their 20 rows of oracle distances (tests/lof_ref.py's lof_rows_ref), the neighbours'
    k-distances and densities taken from the call's own arrays -- kdist is held to core_distances on every row.  Dyadic coordinates
    in one dimension, nearly all distinct: every distance and every S1 is exact"""
    r1, n_dims, k = 65600, 3, 5
    rng = np.random.RandomState(65600)
    x = dyadic(rng, r1, below=1 << 22)
    x[[7, 70000 % r1, 300]] = x[9]  # a clump of 4 copies, short of k + 1
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.lof(k)
        assert same_bits(got.kdist, rs.core_distances(k + 1)) and np.all(got.n_neigh >= k)
        sample = np.concatenate([[0, 7, 9, 255, 256, r1 - 1], rng.choice(r1, 14, replace=False)]).astype(np.int64)
        E = oracle.distance_rowwise(m, m[sample], metric, 0, 2.0, False)
        assert E.shape == (len(sample), r1)
        check(kpop.Lof(*[a[sample] for a in got]), lof_rows_ref(E, sample, k, got.kdist, got.lrd), "the long set", exact_sums=True)
        q = line_rows([x[9], x[100] + 0.0625, 1e6], n_dims)
        score = rs.lof_score(q, k, got.kdist, got.lrd)
        check(score, lof_score_ref(oracle.distance_rowwise(m, q, metric, 0, 2.0, False), k, got.kdist, got.lrd), "the long set, queries", exact_sums=True)
        assert 0.0 < score.kdist[0] <= got.kdist[9] and score.n_neigh[0] >= 5  # the four copies at distance 0, and one more row
    finally:
        rs.free()


def test_conventions(kpop, oracle):
    # a clump of k + 1 copies has lrd +inf and lof 1.0; the row beside it lof +inf
    rs, D = exact_set(kpop, oracle, [5, 5, 5, 6, 9, 9.5, 10], 3)
    try:
        got = rs.lof(2)
        check(got, lof_ref(D, 2), "a clump", exact_sums=True)
        assert got.lrd[:3].tolist() == [INF] * 3 and got.lof[:3].tolist() == [1.0] * 3 and got.lof[3] == INF and got.n_neigh[3] == 3
        same = rs.lof_score(line_rows([5, 5.5], 3), 2, got.kdist, got.lrd)  # a query on the clump, and one beside it
        assert same.kdist.tolist() == [0.0, 0.5] and same.n_neigh.tolist() == [3, 4] and same.lrd[0] == INF and same.lof.tolist() == [1.0, INF]
    finally:
        rs.free()
    # a row with a NaN: the declared NaN, no neighbours, and in nobody's neighbourhood; a +inf coordinate: distances that are numbers
    rng = np.random.RandomState(21)
    r1, n_dims, bad, far = 130, 5, 77, 20
    m = np.round(rng.normal(size=(r1, n_dims)), 2)
    m[bad, 2] = np.nan
    m[far, 1] = INF
    metric = np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
    assert np.all(np.isnan(np.delete(D[bad], bad))) and np.all(np.delete(D[far], [far, bad]) == INF)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        for k in (3, 128):
            got = rs.lof(k)
            check(got, lof_ref(D, k), ("a NaN row, an infinite row", k))
            assert all(a.view(np.uint64)[bad] == QNAN_BITS for a in (got.kdist, got.lrd, got.lof)) and got.n_neigh[bad] == 0
            assert got.kdist[far] == INF and got.n_neigh[far] == r1 - 2 and got.lrd[far] == 0.0
            if k == 3:  # (at k = 128 every k-distance is the infinite one: every lrd 0, every lof 0 / 0)
                assert got.lof[far] == INF and np.all(np.isfinite(np.delete(got.lof, [bad, far])))
            keep = np.delete(np.arange(r1), bad)
            rest = kpop.distance_lof(m[keep], metric, k, 0, 2.0, False)
            assert all_same_bits([a[keep] for a in got][:2], rest[:2])  # the row is in nobody's neighbourhood
        got = rs.lof(3)
        score = rs.lof_score(m[[bad, far, 3]], 3, got.kdist, got.lrd)  # (a +inf query row against the +inf row: inf - inf, not a number)
        E = oracle.distance_rowwise(m, m[[bad, far, 3]], metric, 0, 2.0, False)
        check(score, lof_score_ref(E, 3, got.kdist, got.lrd), "NaN and infinite query rows")
        assert score.n_neigh[0] == 0 and score.lof.view(np.uint64)[0] == QNAN_BITS and score.kdist[2] <= got.kdist[3]
    finally:
        rs.free()


def test_a_set_after_growth(kpop, oracle):
    r1, n_dims, k = 300, 9, 6
    rng = np.random.RandomState(8)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    for normalize in (True, False):
        fresh = kpop.RefSet(m, metric, 0, 2.0, normalize)
        grown = kpop.RefSet(m[:170], metric, 0, 2.0, normalize, capacity=r1)
        try:
            before = grown.lof(k)
            grown.append(m[170:])
            assert all_same_bits(grown.lof(k), fresh.lof(k))
            assert not same_bits(before.kdist, fresh.lof(k).kdist[:170])  # a new row lowers old rows' k-distances: no known_rows
        finally:
            fresh.free()
            grown.free()


def raw(fn, lead, outs):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32))  # noqa: E731
    return fn(*lead, *[ptr(a) for a in outs])


def test_arguments(kpop, oracle):
    from kpop_amd import _lib, api
    lib = _lib.load()
    rng = np.random.RandomState(2)
    r1, n_dims, k = 70, 3, 4
    rs, D = exact_set(kpop, oracle, dyadic(rng, r1), n_dims)
    q = line_rows(dyadic(rng, 5), n_dims)
    f64p = C.POINTER(C.c_double)
    try:
        want = rs.lof(k)
        score = rs.lof_score(q, k, want.kdist, want.lrd)
        for bad_k, code in ((0, ERR_INVALID), (129, ERR_UNSUPPORTED)):
            for call in (lambda: rs.lof(bad_k), lambda: rs.lof_score(q, bad_k, want.kdist, want.lrd),
                         lambda: kpop.distance_lof(line_rows([1, 2, 3], 3), np.ones(3), bad_k, 0, 2.0, False),
                         lambda: api.dev_lof(rs, bad_k, None), lambda: api.dev_lof_score(rs, bad_k, None, None, None, 1, None)):
                with pytest.raises(kpop.KPopError) as e:
                    call()
                assert e.value.code == code and "kpop_" in str(e.value)
            assert api.dev_lof_workspace_bytes(rs, bad_k) == 0 and api.dev_lof_score_workspace_bytes(rs, 5, bad_k) == 0
        assert 0 < api.dev_lof_workspace_bytes(rs, 128) < api.dev_lof_workspace_bytes(rs, 1) < 1 << 22  # O(r1), and lists where k < r1
        with pytest.raises(kpop.KPopError):  # the device forms need their workspace
            api.dev_lof(rs, k, None)
        # every output pointer may be NULL; any one alone is what it is with the others
        set_lead = [rs.handle, k]
        sk, sl = np.ascontiguousarray(want.kdist), np.ascontiguousarray(want.lrd)
        score_lead = [rs.handle, k, sk.ctypes.data_as(f64p), sl.ctypes.data_as(f64p), q.ctypes.data_as(f64p), len(q)]
        for fn, lead, full in ((lib.kpop_lof, set_lead, want), (lib.kpop_lof_score, score_lead, score)):
            assert raw(fn, lead, [None] * 4) == 0
            for i in range(4):
                outs = [None] * 4
                outs[i] = np.zeros_like(full[i])
                assert raw(fn, lead, outs) == 0
                assert all_same_bits([outs[i]], [full[i]]), NAMES[i]
        assert raw(lib.kpop_lof_score, [rs.handle, k, None, sl.ctypes.data_as(f64p), q.ctypes.data_as(f64p), len(q)], [None] * 4) == ERR_INVALID
        # r2 = 0: KPOP_OK, nothing written
        none = rs.lof_score(np.zeros((0, n_dims)), k, want.kdist, want.lrd)
        assert all(len(a) == 0 for a in none)
        assert raw(lib.kpop_lof_score, [rs.handle, k, None, None, None, 0], [None] * 4) == 0
        with pytest.raises(ValueError):
            rs.lof_score(q, k, want.kdist[:5], want.lrd)
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.lof(k)
    assert e.value.code == ERR_INVALID
    # r1 < k in the query form: the NaN row; an empty set: KPOP_OK -- the error of a bad k still comes first
    small, _ = exact_set(kpop, oracle, [1.0, 2.0, 4.0], n_dims)
    empty = kpop.RefSet(np.zeros((0, n_dims)), np.ones(n_dims), 0, 2.0, False)
    try:
        for rs_, n in ((small, 3), (empty, 0)):
            got = rs_.lof_score(q, 4, np.zeros(n), np.zeros(n))
            assert all(np.all(a.view(np.uint64) == QNAN_BITS) for a in (got.kdist, got.lrd, got.lof)) and not got.n_neigh.any() and len(got.lof) == 5
        got = small.lof_score(q, 3, *small.lof(3)[::2])  # (r1 == k: every row of the set is a neighbour, and none of them has a k-distance)
        assert np.all(got.n_neigh == 3) and np.all(np.isnan(got.lrd))
        got = empty.lof(3)
        assert all(len(a) == 0 for a in got)
        assert raw(lib.kpop_lof, [empty.handle, 3], [None] * 4) == 0
        with pytest.raises(kpop.KPopError):
            empty.lof(0)
    finally:
        small.free()
        empty.free()
