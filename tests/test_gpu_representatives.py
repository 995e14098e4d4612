"""Representatives at a distance (kpop_representatives_within, include/kpop_hip.h): the greedy cover of a
resident set in row order.

The contract: rep_of, rep_dist and n_reps array-equal to tests/representatives_ref.py on the oracle's matrix of the set against itself,
and the same on every run.  For the euclidean and cosine kinds the GPU's distances are the oracle's bit for bit; the Minkowski kind goes
through the GPU's pow, which agrees with the oracle's to rtol 1e-11 (tests/test_gpu_refset.py): there a threshold is put into a gap of
the oracle's distances of at least 1e-8 relative (asserted), so that no pair is ambiguous, and the result is compared against
representatives_ref of the GPU's own vector-pipe matrix (tests/test_gpu_clusters.py and tests/test_gpu_within.py do the same).  The
helpers are those of tests/test_gpu_clusters.py."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from representatives_ref import representatives_ref

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
    """the oracle's r1 x r1 matrix of a shape's rows against themselves: computed once, shared, read-only (the Minkowski ones of the
    largest shape are forgotten by the test that is done with them)"""
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


def not_their_first_hit(D, T, rep_of):
    """the rows whose representative is not the first representative below them within T"""
    reps = np.flatnonzero(rep_of == np.arange(len(rep_of)))
    n = 0
    with np.errstate(invalid="ignore"):
        for i in np.flatnonzero(rep_of != np.arange(len(rep_of))):
            below = reps[:np.searchsorted(reps, i)]
            n += int(below[np.argmax(D[i, below] <= T)] != rep_of[i])
    return n


def check_result(got, want, D, what):
    rep_of, rep_dist, n = got
    r1 = len(want[0])
    assert rep_of.dtype == np.uint32 and rep_of.shape == (r1,) and rep_dist.dtype == np.float64 and rep_dist.shape == (r1,), what
    assert np.array_equal(rep_of, want[0]), (what, int(np.sum(rep_of != want[0])))
    assert np.array_equal(rep_dist, want[1]), (what, int(np.sum(rep_dist != want[1])))
    assert n == want[2], (what, n, want[2])
    rows = np.arange(r1)
    assert np.all(rep_of <= rows) and np.array_equal(rep_of[rep_of], rep_of) and n == int(np.sum(rep_of == rows)), what
    assert not np.signbit(rep_dist).any(), what
    if D is not None:
        other = rep_of != rows
        assert np.array_equal(rep_dist[other], D[rows[other], rep_of[other]] + 0.0), what  # (-0 + 0 is +0)
        assert not rep_dist[~other].any(), what


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_representatives_vs_oracle(kpop, oracle, r1, d, kind, p):
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize)
        D = oracle_matrix(oracle, r1, d, kind, p, normalize)
        u = distinct(D) if kind == 2 else None
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            # the matrix the result is held to: the oracle's, or -- the Minkowski kind -- the GPU's own on the vector pipe, the thresholds
            # in gaps of the oracle's
            G = on_the_vector_pipe(rs, m) if kind == 2 else D
            if kind == 2:
                assert np.allclose(G, D, rtol=1e-9, atol=0.0, equal_nan=True), what
            thresholds = [("q%g" % q, float(np.quantile(D, q)) if kind != 2 else gap_threshold(D, q, u)) for q in QUANTILES]
            ref01 = representatives_ref(G, thresholds[1][1])
            # the inclusive tie: the largest distance at which the 0.01 quantile assigns a row.  At that threshold the result is the
            # same (every assigned row still lies within it of its representative, the representatives are still apart), and the row
            # assigned at exactly that distance is decided by the equality
            T_tie = float(ref01[1].max())
            assert T_tie > 0.0, what
            thresholds += [("tie", T_tie), ("zero", 0.0), ("negative", -1.0), ("inf", INF)]
            for name, T in thresholds:
                want = ref01 if name == "q0.01" else representatives_ref(G, T)
                far = not_their_first_hit(G, T, want[0]) if name.startswith("q") else -1
                print("  %s %s T=%.17g: %d representatives, %d rows not with their first hit" % (what, name, T, want[2], far))
                if name.startswith("q"):  # the case is not trivial
                    assert 1 < want[2] < r1, (what, name)
                # (the reference alone says so, before the GPU is asked; on the 130 rows the 0.01 quantile lies inside the noise of a
                # centre, where a row has one representative within reach)
                if name == "q0.05" or (name == "q0.01" and r1 >= 300):
                    assert far >= 1, (what, name)
                if name == "tie":
                    assert np.array_equal(want[0], ref01[0]) and int(np.sum(want[1] == T)) >= 1, what
                got = rs.representatives(T)
                check_result(got, want, G, (what, name))
                again = rs.representatives(T)  # the same bits on every run
                assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and again[2] == got[2], (what, name, "a second run")
                if name == "zero":
                    assert got[0][7] == got[0][3] and got[1][7] == 0.0, what  # the duplicated row, at +0
                if name == "negative":
                    assert np.array_equal(got[0], np.arange(r1)) and got[2] == r1 and not got[1].any(), what
                if name == "inf":
                    assert not got[0].any() and got[2] == 1, what
        finally:
            rs.free()
    if kind == 2 and r1 >= 5000:
        for key in [k for k in _matrices if k[:3] == (r1, d, 2)]:
            del _matrices[key]


def test_the_sequential_dependence(kpop, oracle):
    """a chain of 200 rows across the step boundary at row 2048, stepping 0.25 along dimension 0 from a far-away point, T = 2.4 steps:
    exactly every third chain row is a representative, and that is decided row after row"""
    r1, d = 5000, 16
    m0, metric = operands(oracle, r1, d)
    m = np.array(m0)
    first, n_chain = 1950, 200
    m[first:first + n_chain] = 50.0
    m[first:first + n_chain, 0] += 0.25 * np.arange(n_chain)
    D = self_matrix(oracle, m, metric, 0, 2.0, False)
    T = 2.4 * float(D[first + 1, first])
    want = representatives_ref(D, T)
    chain = np.arange(first, first + n_chain)
    assert np.array_equal(np.flatnonzero(want[0][chain] == chain), np.arange(0, n_chain, 3))
    assert np.array_equal(want[0][chain], first + 3 * (np.arange(n_chain) // 3))
    assert want[0][1952] == 1950 and D[1952, 1953] < D[1952, 1950]  # not the nearer but later 1953
    assert want[0][2048] == 2046 and want[0][2049] == 2049  # across the step boundary
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        check_result(rs.representatives(T), want, D, "chain")
    finally:
        rs.free()


def raw_representatives(rs, T, known_rows, rep_of, rep_dist):
    from kpop_amd import _lib
    n = C.c_uint32(12345)
    rc = _lib.load().kpop_representatives_within(rs.handle, T, known_rows, rep_of.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 None if rep_dist is None else rep_dist.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n))
    return rc, n.value


def test_growing(kpop, oracle):
    """the first n rows are thinned, the others appended, and the set thinned again from the earlier result: the from-scratch one, bit
    for bit -- for prefixes that end nowhere, at one row, just before and behind a step's end, and inside a step and a tile"""
    r1, d, kind, p, normalize = 5000, 16, 0, 2.0, False
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, kind, p, normalize)
    T = float(np.quantile(D, 0.01))
    want = representatives_ref(D, T)
    assert 100 < want[2] < r1 - 100
    for n in (0, 1, 2047, 2049, 3000):
        rs = kpop.RefSet(m[:n], metric, kind, p, normalize, capacity=r1)
        try:
            first = rs.representatives(T)
            check_result(first, tuple(w[:n] for w in want[:2]) + (int(np.sum(want[0][:n] == np.arange(n))),), D, ("the first", n))  # the prefix property
            rs.append(m[n:])
            check_result(rs.representatives(T, known=first[:2]), want, D, ("grown from", n))
            grown = rs.representatives(T, known=first[0])
            assert np.array_equal(grown[0], want[0]) and grown[2] == want[2]
            assert np.array_equal(grown[1][n:], want[1][n:]) and np.all(np.isnan(grown[1][:n]))  # rep_dist of the known rows: not written
            if n == 3000:
                check_result(rs.representatives(T), want, D, "from scratch")
                # known_rows = r1: nothing is examined, both arrays come back as they were given
                given, dist = want[0].copy(), np.full(r1, -5.0)
                rc, count = raw_representatives(rs, T, r1, given, dist)
                assert rc == 0 and count == want[2] and np.array_equal(given, want[0]) and np.all(dist == -5.0)
                # a partly known call leaves rep_dist of the known rows alone
                given, dist = want[0].copy(), np.full(r1, -5.0)
                given[n:] = 77
                rc, count = raw_representatives(rs, T, n, given, dist)
                assert rc == 0 and count == want[2] and np.array_equal(given, want[0])
                assert np.all(dist[:n] == -5.0) and np.array_equal(dist[n:], want[1][n:])
                # entries that no call returns
                bad = want[0].copy()
                bad[5] = 6  # above its own row
                assert raw_representatives(rs, T, r1, bad, None)[0] == ERR_INVALID
                bad = np.arange(r1, dtype=np.uint32)
                bad[10] = 4
                bad[4] = 2  # row 10 points to a row that does not stand for itself
                with pytest.raises(kpop.KPopError) as e:
                    rs.representatives(T, known=bad[:2000])
                assert e.value.code == ERR_INVALID
                assert raw_representatives(rs, T, r1 + 1, want[0].copy(), None)[0] == ERR_INVALID  # more known rows than rows
        finally:
            rs.free()


def test_special_rows(kpop, oracle):
    """a row with a NaN stands for itself alone; a row with an Inf lies at an infinite or NaN distance of every other"""
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    bad = np.array(m)
    bad[20, 4] = np.nan
    bad[30, 2] = np.inf
    for kind, p in KINDS[:2]:
        for normalize in (True, False):
            D = self_matrix(oracle, bad, metric, kind, p, normalize)
            assert np.all(np.isnan(np.delete(D[20], 20)))
            rs = kpop.RefSet(bad, metric, kind, p, normalize)
            try:
                for T in (float(np.nanquantile(D[np.isfinite(D)], 0.05)), 0.0, INF):
                    want = representatives_ref(D, T)
                    assert want[0][20] == 20 and int(np.sum(want[0] == 20)) == 1 and want[2] < r1
                    check_result(rs.representatives(T), want, None, (kind, normalize, T))
                got = rs.representatives(0.0)
                assert got[0][7] == 3 and got[1][7] == 0.0 and not np.signbit(got[1][7])  # the duplicated row
                if normalize:  # the zero row, its norm taken as 1: no other row is at distance zero of it
                    assert got[0][9] == 9 and int(np.sum(got[0] == 9)) == 1
            finally:
                rs.free()


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    T = float(np.quantile(D, 0.05))
    want = representatives_ref(D, T)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        with pytest.raises(kpop.KPopError) as e:
            rs.representatives(float("nan"))
        assert e.value.code == ERR_INVALID
        check_result(kpop.distance_representatives(m, metric, 0, 2.0, True, T), want, D, "distance_representatives")
        # rep_dist = NULL
        rep_of = np.full(r1, 99999, dtype=np.uint32)
        rc, n = raw_representatives(rs, T, 0, rep_of, None)
        assert rc == 0 and n == want[2] and np.array_equal(rep_of, want[0])
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.representatives(T)
    assert e.value.code == ERR_INVALID
    # an empty set, and a set of one row
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        rep_of, rep_dist, n = empty.representatives(T)
        assert rep_of.size == 0 and rep_dist.size == 0 and n == 0
    finally:
        empty.free()
    rep_of, rep_dist, n = kpop.distance_representatives(np.zeros((0, d)), metric, 0, 2.0, True, T)
    assert rep_of.size == 0 and n == 0
    for T1 in (T, -1.0, INF):
        rep_of, rep_dist, n = kpop.distance_representatives(m[:1], metric, 0, 2.0, True, T1)
        assert rep_of.tolist() == [0] and rep_dist.tolist() == [0.0] and n == 1


def test_beyond_65535_rows(kpop):
    """70,000 rows take the tiles of a long set (32 columns x 256 rows) and 35 steps.  No quadratic reference: 700 centres on a lattice of
    step 4, every row at a centre plus noise of at most 0.01 a coordinate, T = 0.1.  The result is held to the invariants that determine
    it (section 6h), through the range query: the representatives list each other never, and every other row's representative is the
    first entry of its list among the representatives -- ascending by (distance, index) -- that lies below the row"""
    r1, d, n_centres, step, noise, T = 70000, 8, 700, 4.0, 0.01, 0.1
    rng = np.random.RandomState(70008)
    digits = np.array([[(c // 3 ** k) % 3 for k in range(d)] for c in range(n_centres)], dtype=np.float64)
    assert len({tuple(r) for r in digits.tolist()}) == n_centres
    centre_of = rng.randint(n_centres, size=r1)
    m = step * digits[centre_of] + rng.uniform(-noise, noise, size=(r1, d))
    metric = np.ones(d)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        rep_of, rep_dist, n = rs.representatives(T)
        again = rs.representatives(T)
        assert np.array_equal(again[0], rep_of) and np.array_equal(again[1], rep_dist) and again[2] == n  # the same bits
    finally:
        rs.free()
    rows = np.arange(r1)
    assert np.all(rep_of <= rows) and np.array_equal(rep_of[rep_of], rep_of)
    reps = np.flatnonzero(rep_of == rows)
    assert n == len(reps) and 1 < n < r1
    assert n == len(np.unique(centre_of))  # (what the generator implies; the invariants below do not rest on it)
    assert not rep_dist[reps].any() and not np.signbit(rep_dist).any()
    # two representatives are farther apart than T: each lists itself alone
    offsets, idx, _ = kpop.distance_within(m[reps], m[reps], metric, T, 0, 2.0, False)
    assert np.array_equal(offsets, np.arange(n + 1, dtype=np.uint64)) and np.array_equal(idx, np.arange(n))
    # every other row: the first entry of its list whose original index is below the row
    others = np.flatnonzero(rep_of != rows)
    offsets, idx, dist = kpop.distance_within(m[reps], m[others], metric, T, 0, 2.0, False)
    owner = np.repeat(np.arange(len(others)), np.diff(offsets.astype(np.int64)))
    eligible = np.flatnonzero(reps[idx] < others[owner])
    has, first = np.unique(owner[eligible], return_index=True)
    assert np.array_equal(has, np.arange(len(others)))  # every one of them is covered from below
    pick = eligible[first]
    assert np.array_equal(reps[idx[pick]], rep_of[others])
    assert np.array_equal(dist[pick] + 0.0, rep_dist[others])


def test_device_form_on_streams(kpop, oracle):
    """kpop_dev_representatives_within with its own workspace on a stream of the caller's; two sets on two streams back to back give
    what the host form gives, and the words behind d_rep_of and d_rep_dist stay as they were"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    cases = [(1000, 16, 0, 2.0, True), (5000, 16, 1, 2.0, False)]
    GUARD = 8
    sets, wants, bufs, streams = [], [], [], []

    def check_device(buf, want, r1, what):
        work, rep_of, rep_dist, count = buf
        got_of, got_dist = rep_of.cpu().numpy().view(np.uint32), rep_dist.cpu().numpy()
        check_result((got_of[:r1], got_dist[:r1], int(count.item())), want, None, what)
        assert np.all(got_of[r1:] == np.uint32(0xFFFFFFFD)) and np.all(got_dist[r1:] == -3.0), what  # the guard words

    def reset(buf):
        buf[1].fill_(-3)
        buf[2].fill_(-3.0)
        buf[3].fill_(-3)

    try:
        for r1, d, kind, p, normalize in cases:
            m, metric = operands(oracle, r1, d)
            D = oracle_matrix(oracle, r1, d, kind, p, normalize)
            T = float(np.quantile(D, 0.01))
            rs = kpop.RefSet(m, metric, kind, p, normalize)
            sets.append((rs, T, r1))
            wants.append(rs.representatives(T))  # the host form
            check_result(wants[-1], representatives_ref(D, T), D, "host form")
            work = torch.empty(max(api.dev_representatives_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
            bufs.append((work, torch.empty(r1 + GUARD, dtype=torch.int32, device=dev), torch.empty(r1 + GUARD, dtype=torch.float64, device=dev),
                         torch.empty(1, dtype=torch.int32, device=dev)))
            reset(bufs[-1])
            streams.append(torch.cuda.Stream(device=dev))
        torch.cuda.synchronize()
        # each alone on its stream, twice on the same buffers: nothing is left over from the first call
        for (rs, T, r1), buf, stream, want in zip(sets, bufs, streams, wants):
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_representatives_within(rs, T, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            check_device(buf, want, r1, "device form")
            reset(buf)
        torch.cuda.synchronize()
        # both enqueued before either is waited for
        for (rs, T, r1), buf, stream in zip(sets, bufs, streams):
            with torch.cuda.stream(stream):
                api.dev_representatives_within(rs, T, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), stream=stream.cuda_stream)
        for stream in streams:
            stream.synchronize()
        for (rs, T, r1), buf, want in zip(sets, bufs, wants):
            check_device(buf, want, r1, "two streams")
        # grown on the device: the first 2,500 rows' entries in place, trusted; without rep_dist
        rs, T, r1 = sets[1]
        buf, want = bufs[1], wants[1]
        reset(buf)
        half = 2500
        buf[1][:half] = torch.from_numpy(want[0][:half].view(np.int32).copy()).to(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[1]):
            api.dev_representatives_within(rs, T, buf[0].data_ptr(), buf[1].data_ptr(), None, buf[3].data_ptr(), known_rows=half, stream=streams[1].cuda_stream)
        streams[1].synchronize()
        assert np.array_equal(buf[1].cpu().numpy().view(np.uint32)[:r1], want[0]) and int(buf[3].item()) == want[2]
        assert np.all(buf[1].cpu().numpy()[r1:] == -3) and np.all(buf[2].cpu().numpy() == -3.0)
    finally:
        for rs, _, _ in sets:
            rs.free()


def test_consistent_with_the_clusters(kpop, oracle):
    """a cover refines the components: every row carries the label of its representative, and there are no fewer representatives than
    clusters"""
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        D = oracle_matrix(oracle, r1, d, 0, 2.0, normalize)
        rs = kpop.RefSet(m, metric, 0, 2.0, normalize)
        try:
            for q in (0.01, 0.05):
                T = float(np.quantile(D, q))
                rep_of, _, n = rs.representatives(T)
                labels, n_clusters = rs.clusters(T)
                assert np.array_equal(labels[rep_of], labels) and n >= n_clusters
        finally:
            rs.free()
