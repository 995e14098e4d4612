"""Range queries on a resident set (kpop_neighbours_within, include/kpop_hip.h): every row of the set within a distance of a query row.

The contract: row j's list is { i : d(j, i) <= T } in ascending (distance, index) order, where d(j, i) is the value
RefSet.distance_rowwise writes on the vector pipe (kpop_tune("distance_mfma", 0)), bit for bit and under any tune setting; for the
euclidean and cosine kinds that value is the oracle's, bit for bit.  The Minkowski kind goes through the GPU's pow, which agrees with the
oracle's to rtol 1e-11 (tests/test_gpu_refset.py): there a threshold is put into a gap of the oracle's distances that is far wider than
that (1e-8 relative, asserted), so that no pair is ambiguous, and the index sets are compared; the threshold of the tie at the inclusive
boundary is the GPU's own value of that distance, which the oracle cannot name to the last bit."""
import ctypes as C

import numpy as np
import pytest

from within_ref import rows_of, same_lists, within_ref

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_CAPACITY = -1, -2
SHAPES = [(130, 9, 37), (1000, 16, 40), (5000, 16, 12), (20000, 64, 9), (300, 200, 33)]
QUANTILES = (0.001, 0.01, 0.2)
INF = float("inf")


def rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=True):
    """tests/test_gpu_refset.py"""
    m1 = np.round(rng.normal(size=(r1, d)), 1) if grid else rng.normal(size=(r1, d))
    if r1 > 12:
        m1[7] = m1[3]  # a duplicated row: a tie in every query row's distances
        m1[9] = 0.0  # a zero row: its norm is replaced by 1 (lib/Matrix.ml:67)
    return m1


_operands = {}


def operands(oracle, r1, d, r2):
    """made once a shape, never changed"""
    if (r1, d, r2) not in _operands:
        rng = np.random.RandomState(r1 + d)
        grid = d <= 16
        m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid)
        m2 = np.round(rng.normal(size=(r2, d)), 1) if grid else rng.normal(size=(r2, d))
        m2[min(5, r2 - 1)] = m1[11]  # a zero distance
        m2[1] = m1[3]  # ... and two more: rows 3 and 7 are the same
        metric = oracle.metric_powers(oracle.synth_inertia(d))
        for a in (m1, m2, metric):
            a.setflags(write=False)
        _operands[(r1, d, r2)] = (m1, m2, metric)
    return _operands[(r1, d, r2)]


def on_the_vector_pipe(rs, m2):
    """the r2 x r1 matrix of the reference chain's distances"""
    from kpop_amd import api
    api.tune("distance_mfma", 0)
    try:
        return rs.distance_rowwise(m2)
    finally:
        api.tune("distance_mfma", 1)


def gap_threshold(D, q):
    """the midpoint of the first two consecutive distinct oracle distances at or above the q-quantile that lie >= 1e-8 (relative) apart"""
    u = np.unique(D[np.isfinite(D)])
    k = int(np.searchsorted(u, np.quantile(D, q)))
    while k + 1 < len(u) and not (u[k + 1] - u[k] >= 1e-8 * u[k + 1]):
        k += 1
    assert k + 1 < len(u)
    gap = (u[k + 1] - u[k]) / u[k + 1]
    print("    Minkowski threshold at quantile %s: relative gap %.3g" % (q, gap))
    assert gap >= 1e-8
    return (u[k] + u[k + 1]) / 2


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d,r2", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_within_vs_oracle_and_rowwise(kpop, oracle, r1, d, r2, kind, p):
    m1, m2, metric = operands(oracle, r1, d, r2)
    for normalize in (True, False):
        what = (r1, d, r2, kind, normalize)
        D = oracle.distance_rowwise(m1, m2, metric, kind, p, normalize)
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            if kind != 2:
                assert np.array_equal(G.view(np.uint64), D.view(np.uint64)), what
            else:
                np.testing.assert_allclose(G, D, rtol=1e-11, atol=0)
            assert G[0, 3] == G[0, 7] and D[0, 3] == D[0, 7]
            thresholds = [("zero", 0.0), ("tie", D[0, 3] if kind != 2 else G[0, 3]), ("negative", -1.0)]
            thresholds += [("q%g" % q, float(np.quantile(D, q)) if kind != 2 else gap_threshold(D, q)) for q in QUANTILES]
            if r1 == 130:
                thresholds.append(("inf", INF))
            for name, T in thresholds:
                got = rs.within(m2, T)
                offsets, idx, dist = got
                assert offsets.dtype == np.uint64 and idx.dtype == np.uint32 and dist.dtype == np.float64
                print("  %s %s T=%.17g: %d pairs, longest list %d" % (what, name, T, int(offsets[-1]), int(np.diff(offsets.astype(np.int64)).max())))
                # the lists are those of the rowwise matrix: same columns, same order, the distances bit for bit
                same_lists(got, within_ref(G, T), (what, name, "rowwise"))
                for j, (ji, jd) in enumerate(rows_of(got)):
                    assert np.array_equal(jd.view(np.uint64), G[j, ji].view(np.uint64)), (what, name, j)
                    assert np.array_equal(np.lexsort((ji, jd)), np.arange(len(ji))), (what, name, j)  # sorted by its own (dist, idx)
                want = within_ref(D, T)
                if kind != 2:
                    same_lists(got, want, (what, name, "oracle"))
                elif name != "tie":  # (the tie's threshold is the GPU's value of that distance: the oracle's may lie a rounding above it)
                    assert np.array_equal(offsets, want[0]), (what, name)
                    for j, ((gi, gd), (wi, wd)) in enumerate(zip(rows_of(got), rows_of(want))):
                        assert np.array_equal(np.sort(gi), np.sort(wi)), (what, name, j)
                        np.testing.assert_allclose(gd, D[j, gi], rtol=1e-11, atol=0)
                if name == "zero":
                    pairs = [(j, int(i)) for j, (ji, _) in enumerate(rows_of(got)) for i in ji]
                    assert pairs == [(1, 3), (1, 7), (min(5, r2 - 1), 11)], (what, pairs)
                if name == "tie":
                    row0 = rows_of(got)[0][0].tolist()
                    assert 3 in row0 and row0.index(7) == row0.index(3) + 1, (what, row0)
                if name == "negative":
                    assert not offsets.any() and idx.size == 0 and dist.size == 0
                if name == "inf":
                    assert offsets.tolist() == [j * r1 for j in range(r2 + 1)]
                if (r1, name) == (20000, "q0.2"):  # rows beyond one block's sort
                    assert int(np.diff(offsets.astype(np.int64)).max()) > 4096
                    same_lists(rs.within(m2, T), got, (what, "a second run"))  # the same bits, whoever arrived first
        finally:
            rs.free()


@pytest.mark.parametrize("kind", [0, 1], ids=["euclidean", "cosine"])
def test_route_independence(kpop, oracle, kind):
    """60,000 x 256 against 300 rows: 2^32 products and more, where the plain rowwise call takes the matrix cores.  The range query does
    not: the same lists with distance_mfma at its default and at 0, those of the vector pipe's matrix"""
    from kpop_amd import api
    r1, d, r2 = 60000, 256, 300
    assert r1 * r2 * d >= 2 ** 32
    rng = np.random.RandomState(r1 + d)
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=False)
    m2 = rng.normal(size=(r2, d))
    m2[5] = m1[11]
    m2[1] = m1[3]
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    for normalize in (True, False):
        rs = kpop.RefSet(m1, metric, kind, 2.0, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            T = float(np.quantile(G[::7, ::11], 0.001))
            want = within_ref(G, T)
            assert want[0][-1] > r2
            by_default = rs.within(m2, T)
            try:
                api.tune("distance_mfma", 0)
                at_zero = rs.within(m2, T)
            finally:
                api.tune("distance_mfma", 1)
            same_lists(by_default, at_zero, (kind, normalize, "default against 0"))
            same_lists(by_default, want, (kind, normalize, "against the vector pipe's matrix"))
            zero = rows_of(rs.within(m2, 0.0))
            assert zero[1][0].tolist() == [3, 7] and zero[5][0].tolist() == [11]
        finally:
            rs.free()


def raw_call(rs, m2, T, capacity, idx, dist):
    """kpop_neighbours_within on the caller's arrays (None: count only) -> (status, offsets)"""
    from kpop_amd import _lib
    m2 = np.ascontiguousarray(m2, dtype=np.float64)
    offsets = np.full(m2.shape[0] + 1, 12345, dtype=np.uint64)
    rc = _lib.load().kpop_neighbours_within(rs.handle, m2.ctypes.data_as(C.POINTER(C.c_double)), m2.shape[0], T, capacity,
                                            offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            None if dist is None else dist.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, offsets


def test_contract_edges(kpop, oracle):
    r1, d, r2 = 1000, 16, 40
    m1, m2, metric = operands(oracle, r1, d, r2)
    D = oracle.distance_rowwise(m1, m2, metric, 0, 2.0, True)
    T = float(np.quantile(D, 0.01))
    want = within_ref(D, T)
    total = int(want[0][-1])
    assert total > r2
    rs = kpop.RefSet(m1, metric, 0, 2.0, True, capacity=r1 + 8)
    try:
        # one entry short: the status says so, the offsets are complete, the lists are not touched
        idx = np.full(total, 0xDEADBEEF, dtype=np.uint32)
        dist = np.full(total, -7.5, dtype=np.float64)
        rc, offsets = raw_call(rs, m2, T, total - 1, idx, dist)
        assert rc == ERR_CAPACITY
        assert np.array_equal(offsets, want[0])
        assert np.all(idx == 0xDEADBEEF) and np.all(dist == -7.5)
        with pytest.raises(kpop.KPopError) as e:
            rs.within(m2, T, capacity=total - 1)
        assert e.value.code == ERR_CAPACITY
        # exactly enough, and more than enough
        rc, offsets = raw_call(rs, m2, T, total, idx, dist)
        assert rc == 0
        same_lists((offsets, idx, dist), want, "exact capacity")
        same_lists(rs.within(m2, T, capacity=total + 1000), want, "spare capacity")
        # count only
        rc, offsets = raw_call(rs, m2, T, 0, None, None)
        assert rc == 0 and np.array_equal(offsets, want[0])
        rc, offsets = raw_call(rs, m2, T, 10 ** 9, None, None)  # (no lists: the capacity says nothing)
        assert rc == 0 and np.array_equal(offsets, want[0])
        # no query rows; a threshold that is not a number
        o, i, x = rs.within(np.zeros((0, d)), T)
        assert o.tolist() == [0] and i.size == 0 and x.size == 0
        with pytest.raises(kpop.KPopError) as e:
            rs.within(m2, float("nan"))
        assert e.value.code == ERR_INVALID
        # a query row with a NaN in it: every distance of the row is one, its list is empty, the other rows' are what they were
        bad = np.array(m2)
        bad[2, 4] = np.nan
        got = rows_of(rs.within(bad, T))
        for j, ((gi, gd), (wi, wd)) in enumerate(zip(got, rows_of(want))):
            if j == 2:
                assert gi.size == 0 and len(wi) > 0
            else:
                assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
        assert rows_of(rs.within(bad, INF))[2][0].size == 0
        # the unprepared call
        same_lists(kpop.distance_within(m1, m2, metric, T), want, "distance_within")
        same_lists(kpop.distance_within(m1, m2, metric, T, capacity=total), want, "distance_within with a capacity")
        with pytest.raises(kpop.KPopError) as e:
            kpop.distance_within(m1, m2, metric, T, capacity=total - 1)
        assert e.value.code == ERR_CAPACITY
        # rows appended to the set are found: a copy of query row 0 at distance 0
        more = np.array(m1[20:24])
        more[2] = m2[0]
        rs.append(more)
        zero = rows_of(rs.within(m2, 0.0))
        assert zero[0][0].tolist() == [r1 + 2] and zero[0][1].tolist() == [0.0]
        assert zero[1][0].tolist() == [3, 7] and zero[5][0].tolist() == [11]
        same_lists(rs.within(m2, T), within_ref(oracle.distance_rowwise(np.vstack([m1, more]), m2, metric, 0, 2.0, True), T), "after append")
    finally:
        rs.free()
    # an empty set
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        o, i, x = empty.within(m2, INF)
        assert o.tolist() == [0] * (r2 + 1) and i.size == 0 and x.size == 0
    finally:
        empty.free()


def test_device_form_on_a_stream(kpop, oracle):
    """kpop_dev_neighbours_within on a stream of the caller's, the workspace sized by kpop_dev_neighbours_within_workspace_bytes: the host
    form's lists; with too little room the offsets alone, the lists untouched; without lists the count"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, d, r2 = 20000, 64, 9
    m1, m2, metric = operands(oracle, r1, d, r2)
    for kind, p, normalize in ((0, 2.0, True), (2, P_MINK, False)):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            T = float(np.quantile(G, 0.2))  # (lists of more than one block's sort among them)
            want = rs.within(m2, T)
            same_lists(want, within_ref(G, T), "host form")
            total = int(want[0][-1])
            t_m2 = torch.from_numpy(np.array(m2)).to(dev)
            stream = torch.cuda.Stream(device=dev)
            for capacity, lists in ((total + 5, True), (total - 1, True), (0, False)):
                work = torch.empty(api.dev_neighbours_within_workspace_bytes(rs, r2, capacity), dtype=torch.uint8, device=dev)
                offs = torch.full((r2 + 1,), 77, dtype=torch.int64, device=dev)
                idx = torch.full((max(capacity, 1),), -3, dtype=torch.int32, device=dev)
                dist = torch.full((max(capacity, 1),), -7.5, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    for _ in range(2):  # (a second call on the same buffers: nothing is left over from the first)
                        api.dev_neighbours_within(rs, t_m2.data_ptr(), r2, T, capacity, work.data_ptr(), offs.data_ptr(), idx.data_ptr() if lists else None,
                                                  dist.data_ptr() if lists else None, stream=stream.cuda_stream)
                stream.synchronize()
                assert np.array_equal(offs.cpu().numpy().view(np.uint64), want[0]), (kind, capacity)
                if capacity >= total:
                    same_lists((want[0], idx.cpu().numpy().view(np.uint32)[:total], dist.cpu().numpy()[:total]), want, ("device form", kind))
                    assert torch.all(idx[total:] == -3) and torch.all(dist[total:] == -7.5)
                else:
                    assert torch.all(idx == -3) and torch.all(dist == -7.5)
        finally:
            rs.free()


LONG_SETS = [(70000, 8, 5), (70000, 24, 300)]


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d,r2", LONG_SETS, ids=["%dx%dx%d" % s for s in LONG_SETS])
def test_sets_of_65536_rows_and_more(kpop, oracle, r1, d, r2, kind, p):
    """from 65,536 rows on (and up to 4,096 query rows) the tiles are 32 columns x 256 rows, a thread 4 columns x 8 rows: the shape every
    large database takes.  One ragged tile of query rows (5) and two (300), d no multiple of 16; against within_ref of the vector pipe's
    matrix, bit for bit, at T = 0, at the tie of the inclusive boundary, at a quantile whose rows hold more than 4,096 hits (the chunk
    merge), with the capacity exact and one short"""
    m1, m2, metric = operands(oracle, r1, d, r2)
    assert r1 >= 65536 and r2 <= 4096
    for normalize in (True, False):
        what = (r1, d, r2, kind, normalize)
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            assert G[0, 3] == G[0, 7]
            for name, T in (("zero", 0.0), ("tie", G[0, 3]), ("q0.1", float(np.quantile(G[:, ::3], 0.1))), ("negative", -1.0)):
                want = within_ref(G, T)
                total = int(want[0][-1])
                got = rs.within(m2, T)
                print("  %s %s T=%.17g: %d pairs, longest list %d" % (what, name, T, total, int(np.diff(want[0].astype(np.int64)).max())))
                same_lists(got, want, (what, name))
                if name == "zero":
                    rows = rows_of(got)
                    assert {3, 7} <= set(rows[1][0].tolist()) and 11 in rows[min(5, r2 - 1)][0].tolist(), what
                if name == "tie":
                    row0 = rows_of(got)[0][0].tolist()
                    assert row0.index(7) == row0.index(3) + 1, what
                if name == "q0.1":
                    assert int(np.diff(want[0].astype(np.int64)).max()) > 4096, what
                    idx = np.full(total, 0xDEADBEEF, dtype=np.uint32)
                    dist = np.full(total, -7.5, dtype=np.float64)
                    rc, offsets = raw_call(rs, m2, T, total - 1, idx, dist)
                    assert rc == ERR_CAPACITY and np.array_equal(offsets, want[0]), what
                    assert np.all(idx == 0xDEADBEEF) and np.all(dist == -7.5), what
                    rc, offsets = raw_call(rs, m2, T, total, idx, dist)
                    assert rc == 0, what
                    same_lists((offsets, idx, dist), want, (what, "exact capacity"))
        finally:
            rs.free()
