"""Clusters at a distance (kpop_clusters_within, include/kpop_hip.h): the connected components of the graph that joins rows i < j of a
resident set iff d(j, i) <= T.

The contract: labels[i] is the smallest row index of row i's component and n_clusters the number of components, array-equal to
tests/clusters_ref.py on the oracle's matrix of the set against itself, and the same on every run.  For the euclidean and cosine kinds
the GPU's distances are the oracle's bit for bit; the Minkowski kind goes through the GPU's pow, which agrees with the oracle's to rtol
1e-11 (tests/test_gpu_refset.py): there a threshold is put into a gap of the oracle's distances of at least 1e-8 relative (asserted), so
that no pair is ambiguous, and the threshold of the inclusive tie is the GPU's own value of that distance, compared against
clusters_ref of the GPU's own matrix (tests/test_gpu_within.py does the same)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from clusters_ref import cluster_sizes, clusters_ref

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID = -1
SHAPES = [(130, 9), (1000, 16), (5000, 16), (300, 200)]
QUANTILES = (0.001, 0.01, 0.05)
INF = float("inf")


def clustered_rows(r1, d, seed=None):
    """r1 // 25 centres on a grid of tenths, every row a centre plus noise on a grid of hundredths; the last min(40, r1 // 3) rows a
    chain along dimension 0 in steps of 0.25 from a point at +5; row 7 a duplicate of row 3, row 9 zero"""
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
    """the oracle's r1 x r1 matrix of a shape's rows against themselves: computed once, shared, read-only (the large ones are
    forgotten by the test that is done with them)"""
    key = (r1, d, kind, normalize)
    if key not in _matrices:
        m, metric = operands(oracle, r1, d)
        D = self_matrix(oracle, m, metric, kind, p, normalize)
        D.setflags(write=False)
        _matrices[key] = D
    return _matrices[key]


def forget_matrices(r1, d):
    for key in [k for k in _matrices if k[:2] == (r1, d)]:
        del _matrices[key]


def on_the_vector_pipe(rs, m2):
    from kpop_amd import api
    api.tune("distance_mfma", 0)
    try:
        return rs.distance_rowwise(m2)
    finally:
        api.tune("distance_mfma", 1)


def distinct(D):
    return np.unique(D[np.isfinite(D)])


def gap_threshold(D, q, u):
    """tests/test_gpu_within.py: the midpoint of the first two consecutive distinct oracle distances (u = distinct(D)) at or above the
    q-quantile that lie >= 1e-8 (relative) apart"""
    k = int(np.searchsorted(u, np.quantile(D, q)))
    while k + 1 < len(u) and not (u[k + 1] - u[k] >= 1e-8 * u[k + 1]):
        k += 1
    assert k + 1 < len(u)
    gap = (u[k + 1] - u[k]) / u[k + 1]
    print("    Minkowski threshold at quantile %s: relative gap %.3g" % (q, gap))
    assert gap >= 1e-8
    return (u[k] + u[k + 1]) / 2


def transitive_pairs(D, labels, T):
    """pairs of one cluster that lie farther apart than T: joined through other rows alone"""
    same = labels[:, None] == labels[None, :]
    with np.errstate(invalid="ignore"):
        return int(np.sum(np.tril(same & (D > T), -1)))


def check_labels(got, want, what):
    labels, n = got
    assert labels.dtype == np.uint32 and labels.shape == want[0].shape, what
    assert np.array_equal(labels, want[0]), (what, int(np.sum(labels != want[0])))
    assert n == want[1], (what, n, want[1])
    assert np.all(labels <= np.arange(len(labels))) and np.array_equal(labels[labels], labels), what


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_clusters_vs_oracle(kpop, oracle, r1, d, kind, p):
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize)
        D = oracle_matrix(oracle, r1, d, kind, p, normalize)
        # the reference alone, before the GPU is asked: at the 0.01 quantile the graph is neither empty nor complete, and a cluster
        # holds rows that are joined through other rows only
        u = distinct(D) if kind == 2 else None
        T01 = float(np.quantile(D, 0.01)) if kind != 2 else gap_threshold(D, 0.01, u)
        ref01 = clusters_ref(D, T01)
        sizes = cluster_sizes(ref01[0])
        far = transitive_pairs(D, ref01[0], T01)
        print("  %s q0.01: %d clusters, largest %d, %d pairs of one cluster beyond T" % (what, ref01[1], sizes[0], far))
        assert 3 <= ref01[1] <= r1 - 3 and sizes[0] >= 5 and far >= 1, what
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m) if kind == 2 else D
            thresholds = [("zero", 0.0, D), ("tie", float(G[3, 0]), G), ("negative", -1.0, D)]
            thresholds += [("q%g" % q, float(np.quantile(D, q)) if kind != 2 else gap_threshold(D, q, u), D) for q in QUANTILES]
            if r1 == 130:
                thresholds.append(("inf", INF, D))
            for name, T, of in thresholds:
                want = ref01 if (name == "q0.01") else clusters_ref(of, T)
                got = rs.clusters(T)
                print("  %s %s T=%.17g: %d clusters, largest %d" % (what, name, T, want[1], cluster_sizes(want[0])[0]))
                check_labels(got, want, (what, name))
                again = rs.clusters(T)  # the same bits, whoever arrived first
                assert np.array_equal(again[0], got[0]) and again[1] == got[1], (what, name, "a second run")
                if name == "zero":
                    assert got[0][7] == 3, what
                if name == "tie":
                    assert got[0][3] == got[0][0], what  # the inclusive boundary
                if name == "negative":
                    assert np.array_equal(got[0], np.arange(r1)) and got[1] == r1, what
                if name == "inf":
                    assert not got[0].any() and got[1] == 1, what
        finally:
            rs.free()
    if r1 >= 5000:
        forget_matrices(r1, d)


def test_a_nan_row_is_a_cluster_of_its_own(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    bad = np.array(m)
    bad[20, 4] = np.nan
    for kind, p in KINDS[:2]:
        for normalize in (True, False):
            D = self_matrix(oracle, bad, metric, kind, p, normalize)
            assert np.all(np.isnan(np.delete(D[20], 20))) and np.all(np.isnan(np.delete(D[:, 20], 20)))
            rs = kpop.RefSet(bad, metric, kind, p, normalize)
            try:
                for T in (float(np.nanquantile(D, 0.05)), INF):
                    want = clusters_ref(D, T)
                    assert want[0][20] == 20 and want[1] < r1
                    check_labels(rs.clusters(T), want, (kind, normalize, T))
                assert rs.clusters(INF)[1] == 2
            finally:
                rs.free()


def test_a_dense_cluster(kpop, oracle):
    """4,000 rows of one lineage: 8 million hits onto one root, the case a compare-and-swap per hit would crawl on"""
    r1, d, T = 6000, 16, 0.05
    rng = np.random.RandomState(6016)
    m = np.round(rng.normal(size=(r1, d)), 1)
    m[1000:5000] = rng.normal(size=d) + 1e-3 * rng.normal(size=(4000, d))
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    D = self_matrix(oracle, m, metric, 0, 2.0, False)
    with np.errstate(invalid="ignore"):
        hits = int(np.sum(np.tril(D <= T, -1)))
    assert hits >= 7_900_000
    want = clusters_ref(D, T)
    assert np.all(want[0][1000:5000] == 1000) and cluster_sizes(want[0])[0] == 4000
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.clusters(T)
        check_labels(got, want, "dense")
        assert np.array_equal(rs.clusters(T)[0], got[0])
    finally:
        rs.free()


def test_beyond_65535_rows(kpop):
    """70,000 rows take the tiles of a long set (32 columns x 256 rows).  No quadratic reference: 700 centres on a lattice of step 4, row
    i at centre i % 700 plus noise of at most 0.01 a coordinate, T = 0.1 -- by the triangle inequality every pair of one centre lies
    below T and every pair of two centres above it, so that row i's label is i % 700"""
    r1, d, n_centres, step, noise, T = 70000, 8, 700, 4.0, 0.01, 0.1
    rng = np.random.RandomState(70008)
    digits = np.array([[(c // 3 ** k) % 3 for k in range(d)] for c in range(n_centres)], dtype=np.float64)
    assert len({tuple(r) for r in digits.tolist()}) == n_centres
    centres = step * digits
    eps = rng.uniform(-noise, noise, size=(r1, d))
    assert np.abs(eps).max() <= noise
    m = centres[np.arange(r1) % n_centres] + eps
    spread = 2.0 * noise * np.sqrt(d)  # two rows of one centre at most: both off by `noise` in every coordinate, in opposite directions
    assert spread < T / 1.5
    assert step - spread > 10 * T  # two centres differ by a step in one coordinate at least
    rs = kpop.RefSet(m, np.ones(d), 0, 2.0, False)
    try:
        labels, n = rs.clusters(T)
        assert np.array_equal(labels, (np.arange(r1) % n_centres).astype(np.uint32))
        assert n == n_centres
        assert np.array_equal(rs.clusters(T)[0], labels)
        # grown from the first 66,000 rows: row tiles wholly below the known rows are skipped, the one they end in is not
        first = labels[:66000]
        grown, n_grown = rs.clusters(T, known=first)
        assert np.array_equal(grown, labels) and n_grown == n
    finally:
        rs.free()


def raw_clusters(rs, T, known_rows, labels):
    from kpop_amd import _lib
    n = C.c_uint32(12345)
    rc = _lib.load().kpop_clusters_within(rs.handle, T, known_rows, labels.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n))
    return rc, n.value


def test_growing(kpop, oracle):
    """a set of 3,000 rows with room for 4,000 is clustered, 1,000 rows are appended -- bridges between clusters among them -- and it is
    clustered again from the earlier labels: the from-scratch result, bit for bit"""
    r0, r1, d, kind, p, normalize = 3000, 4000, 16, 0, 2.0, False
    m0 = clustered_rows(r0, d)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    D0 = self_matrix(oracle, m0, metric, kind, p, normalize)
    T = float(np.quantile(D0, 0.01))
    ref0 = clusters_ref(D0, T)
    # three bridges: points along the segment between a row of the largest cluster and a row of another, less than T apart (without
    # normalisation the distance along a segment is proportional to the step); the rest are copies of rows there are, which join the
    # cluster of their original
    rng = np.random.RandomState(4016)
    big = np.bincount(ref0[0]).argsort()[::-1][:4]
    assert np.bincount(ref0[0])[big[3]] >= 5
    more = []
    for other in big[1:]:
        a, b = m0[big[0]], m0[other]
        steps = int(np.ceil(2.0 * D0[other, big[0]] / T))
        more.extend(a + (b - a) * (k / (steps + 1.0)) for k in range(1, steps + 1))
    assert len(more) < 800
    more.extend(m0[rng.randint(r0, size=r1 - r0 - len(more))])
    more = np.array(more)[rng.permutation(r1 - r0)]
    m1 = np.vstack([m0, more])
    D1 = self_matrix(oracle, m1, metric, kind, p, normalize)
    ref1 = clusters_ref(D1, T)
    assert ref1[1] <= ref0[1] - 3  # the bridges joined clusters that were apart
    assert np.array_equal(clusters_ref(D1, T, known=ref0[0])[0], ref1[0])
    rs = kpop.RefSet(m0, metric, kind, p, normalize, capacity=r1)
    try:
        first = rs.clusters(T)
        check_labels(first, ref0, "before the append")
        rs.append(more)
        grown = rs.clusters(T, known=first[0])
        check_labels(grown, ref1, "grown")
        check_labels(rs.clusters(T), ref1, "from scratch")
        check_labels(rs.clusters(T, known=first[0][:1234]), ref1, "grown from a part of the earlier labels")
        # known_rows = r1: nothing is examined, the labels come back as they were given
        given = grown[0].copy()
        rc, n = raw_clusters(rs, T, r1, given)
        assert rc == 0 and n == ref1[1] and np.array_equal(given, grown[0])
        same, n_same = rs.clusters(T, known=grown[0])
        assert np.array_equal(same, grown[0]) and n_same == ref1[1]
        # labels that no call returns
        bad = grown[0].copy()
        bad[5] = 6  # above its own row
        rc, _ = raw_clusters(rs, T, r1, bad)
        assert rc == ERR_INVALID
        bad = np.arange(r1, dtype=np.uint32)
        bad[10] = 4
        bad[4] = 2  # the label of row 10 is not its own label
        with pytest.raises(kpop.KPopError) as e:
            rs.clusters(T, known=bad[:2000])
        assert e.value.code == ERR_INVALID
        rc, _ = raw_clusters(rs, T, r1 + 1, grown[0].copy())  # more known rows than rows
        assert rc == ERR_INVALID
    finally:
        rs.free()


def test_consistent_with_the_range_query(kpop, oracle):
    """the components of the graph whose edges are RefSet.within's lists of the set against itself are RefSet.clusters' labels"""
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        D = oracle_matrix(oracle, r1, d, 0, 2.0, normalize)
        rs = kpop.RefSet(m, metric, 0, 2.0, normalize)
        try:
            for q in (0.01, 0.05):
                T = float(np.quantile(D, q))
                offsets, idx, _ = rs.within(m, T)
                apart = np.ones((r1, r1))
                apart[np.repeat(np.arange(r1), np.diff(offsets.astype(np.int64))), idx] = 0.0
                assert np.array_equal(apart, apart.T)  # the chain is symmetric
                check_labels(rs.clusters(T), clusters_ref(apart, 0.5), (normalize, q))
        finally:
            rs.free()


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    T = float(np.quantile(D, 0.05))
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        with pytest.raises(kpop.KPopError) as e:
            rs.clusters(float("nan"))
        assert e.value.code == ERR_INVALID
        want = clusters_ref(D, T)
        check_labels(kpop.distance_clusters(m, metric, 0, 2.0, True, T), want, "distance_clusters")
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.clusters(T)
    assert e.value.code == ERR_INVALID
    # a set of another slot (two slots on the one GPU, as tests/test_gpu_refset.py makes them)
    kpop.init_devices([0, 0])
    try:
        rs = kpop.RefSet(m, metric, 0, 2.0, True)
        try:
            kpop.use_device(1)
            with pytest.raises(kpop.KPopError) as e:
                rs.clusters(T)
            assert e.value.code == ERR_INVALID and "slot" in str(e.value)
            kpop.use_device(0)
            check_labels(rs.clusters(T), want, "back on its slot")
        finally:
            kpop.use_device(0)
            rs.free()
    finally:
        kpop.init(0)
    # a null handle (what a freed RefSet holds is None: the library is never handed a dangling pointer)
    from kpop_amd import _lib
    labels = np.zeros(r1, dtype=np.uint32)
    n = C.c_uint32()
    assert _lib.load().kpop_clusters_within(None, T, 0, labels.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)) == ERR_INVALID
    # an empty set
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        labels, n = empty.clusters(T)
        assert labels.size == 0 and n == 0
    finally:
        empty.free()
    labels, n = kpop.distance_clusters(np.zeros((0, d)), metric, 0, 2.0, True, T)
    assert labels.size == 0 and n == 0


def test_device_form_on_streams(kpop, oracle):
    """kpop_dev_clusters_within with its own workspace on a stream of the caller's; two sets on two streams back to back give what each
    gives alone"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    cases = [(1000, 16, 0, 2.0, True), (5000, 16, 1, 2.0, False)]
    sets, wants, bufs, streams = [], [], [], []
    try:
        for r1, d, kind, p, normalize in cases:
            m, metric = operands(oracle, r1, d)
            D = oracle_matrix(oracle, r1, d, kind, p, normalize)
            T = float(np.quantile(D, 0.01))
            rs = kpop.RefSet(m, metric, kind, p, normalize)
            sets.append((rs, T, r1))
            wants.append(clusters_ref(D, T))
            check_labels(rs.clusters(T), wants[-1], "host form")
            work = torch.empty(max(api.dev_clusters_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
            labels = torch.full((r1,), -3, dtype=torch.int32, device=dev)
            count = torch.full((1,), -3, dtype=torch.int32, device=dev)
            bufs.append((work, labels, count))
            streams.append(torch.cuda.Stream(device=dev))
        torch.cuda.synchronize()
        # each alone on its stream, twice on the same buffers: nothing is left over from the first call
        for (rs, T, r1), (work, labels, count), stream, want in zip(sets, bufs, streams, wants):
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_clusters_within(rs, T, work.data_ptr(), labels.data_ptr(), count.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            check_labels((labels.cpu().numpy().view(np.uint32), int(count.item())), want, "device form")
            labels.fill_(-3)
            count.fill_(-3)
        torch.cuda.synchronize()
        # both enqueued before either is waited for
        for (rs, T, r1), (work, labels, count), stream in zip(sets, bufs, streams):
            with torch.cuda.stream(stream):
                api.dev_clusters_within(rs, T, work.data_ptr(), labels.data_ptr(), count.data_ptr(), stream=stream.cuda_stream)
        for stream in streams:
            stream.synchronize()
        for (work, labels, count), want in zip(bufs, wants):
            check_labels((labels.cpu().numpy().view(np.uint32), int(count.item())), want, "two streams")
        # grown on the device: the first half's labels in place, trusted
        rs, T, r1 = sets[0]
        work, labels, count = bufs[0]
        half = clusters_ref(oracle_matrix(oracle, *cases[0][:2], cases[0][2], cases[0][3], cases[0][4])[:r1 // 2, :r1 // 2], T)[0]
        labels.fill_(-3)
        labels[:r1 // 2] = torch.from_numpy(half.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            api.dev_clusters_within(rs, T, work.data_ptr(), labels.data_ptr(), count.data_ptr(), known_rows=r1 // 2, stream=streams[0].cuda_stream)
        streams[0].synchronize()
        check_labels((labels.cpu().numpy().view(np.uint32), int(count.item())), wants[0], "device form, grown")
    finally:
        for rs, _, _ in sets:
            rs.free()
