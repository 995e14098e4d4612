"""The single-linkage tree of a resident set (kpop_spanning_forest, include/kpop_hip.h): the minimum spanning forest of the graph that
joins rows i < j iff d(j, i) <= max_distance, under the strict order (d, i, j).

The contract: the forest is unique, so edges, distances and labels are array-equal to tests/forest_ref.py on the oracle's matrix of the
set against itself, on every run; and cutting the forest at any T <= max_distance gives RefSet.clusters(T) exactly.  For the euclidean
and cosine kinds the GPU's distances are the oracle's bit for bit; the Minkowski kind goes through the GPU's pow, which agrees with the
oracle's to rtol 1e-11 only (tests/test_gpu_refset.py) -- where distances tie or nearly tie, the order of the edges is that of the GPU's
own bits, so the reference there is forest_ref of the GPU's own vector-pipe matrix (RefSet.distance_rowwise under distance_mfma 0), as
tests/test_gpu_clusters.py does for its inclusive tie.  The rows are that file's: clustered on grids, a duplicated row, a zero row, an
equal-step chain -- full of exact ties, which is the point."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from clusters_ref import clusters_ref
from forest_ref import cut_ref, forest_ref

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID = -1
SHAPES = [(130, 9), (1000, 16), (300, 200)]
INF = float("inf")


def clustered_rows(r1, d, seed=None):
    """tests/test_gpu_clusters.py's rows: r1 // 25 centres on a grid of tenths, every row a centre plus noise on a grid of hundredths;
    the last min(40, r1 // 3) rows a chain along dimension 0 in steps of 0.25 from a point at +5; row 7 a duplicate of row 3, row 9 zero"""
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
    """oracle.distance_rowwise(m, m, ...), its query rows in eight slabs on eight threads"""
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


def lower(D):
    return D[np.tril_indices(D.shape[0], -1)]


def check_forest(got, want, what):
    ei, ej, ed, labels = got
    assert ei.dtype == np.uint32 and ej.dtype == np.uint32 and ed.dtype == np.float64 and labels.dtype == np.uint32, what
    assert len(ei) == len(want[0]), (what, len(ei), len(want[0]))
    assert np.array_equal(ei, want[0]) and np.array_equal(ej, want[1]), (what, int(np.sum((ei != want[0]) | (ej != want[1]))))
    assert np.array_equal(ed, want[2]), what
    assert np.array_equal(labels, want[3]), what
    assert len(ei) == len(labels) - int(np.sum(labels == np.arange(len(labels)))), what


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_forest_vs_reference(kpop, oracle, r1, d, kind, p):
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            D = on_the_vector_pipe(rs, m) if kind == 2 else oracle_matrix(oracle, r1, d, kind, p, normalize)
            caps = [("inf", INF), ("q0.01", float(np.quantile(lower(D), 0.01))), ("tie", float(D[3, 0]))]
            for name, cap in caps:
                want = forest_ref(D, cap)
                n_clusters = r1 - len(want[0])
                print("  %s %s max_distance=%.17g: %d edges, %d components, %d distinct distances among them"
                      % (what, name, cap, len(want[0]), n_clusters, len(np.unique(want[2]))))
                if name == "inf":
                    assert len(want[0]) == r1 - 1, what  # one tree
                    assert normalize or len(np.unique(want[2])) < r1 - 30, what  # ... with ties in it: the chain's equal steps
                    assert want[2][0] == 0.0 and (want[0][0], want[1][0]) == (3, 7), what  # the duplicated row: the first edge
                if name == "q0.01":
                    assert 3 <= n_clusters <= r1 - 3, what  # neither empty nor complete
                if name == "tie":
                    assert want[3][3] == want[3][0], what  # the inclusive boundary: rows 0 and 3 lie exactly max_distance apart
                got = rs.spanning_forest(cap)
                check_forest(got, want, (what, name))
                again = rs.spanning_forest(cap)  # the same bits, whoever arrived first
                assert all(np.array_equal(x, y) for x, y in zip(again, got)), (what, name, "a second run")
        finally:
            rs.free()


def test_the_cut_equals_the_clusters(kpop, oracle):
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        D = oracle_matrix(oracle, r1, d, 0, 2.0, normalize)
        rs = kpop.RefSet(m, metric, 0, 2.0, normalize)
        try:
            ei, ej, ed, labels = rs.spanning_forest()
            assert len(ei) == r1 - 1 and not labels.any()
            thresholds = [float(np.quantile(lower(D), q)) for q in (0.001, 0.01, 0.05, 0.5)] + [float(D[3, 0])]
            counts = []
            for T in thresholds:
                want = rs.clusters(T)
                got = kpop.forest_cut(r1, ei, ej, ed, T)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (normalize, T)
                assert got[1] == r1 - int(np.sum(ed <= T))  # (a forest: every edge within T joins two components)
                counts.append(got[1])
                # the forest with T as its cap: the clusters' labels, and as many edges as the count says
                ci, cj, cd, clabels = rs.spanning_forest(T)
                assert np.array_equal(clabels, want[0]) and len(ci) == r1 - want[1], (normalize, T)
                keep = ed <= T
                assert np.array_equal(ci, ei[keep]) and np.array_equal(cj, ej[keep]) and np.array_equal(cd, ed[keep]), (normalize, T)
            print("  normalize=%s: clusters at the five cuts %s" % (normalize, counts))
            assert len(set(counts)) >= 4  # the cuts are different clusterings
        finally:
            rs.free()


def ruler_rows(r1):
    """rows on a line, the gap before row k = 1 + (the exponent of 2 in k): 1 2 1 3 1 2 1 4 ..."""
    k = np.arange(1, r1)
    gaps = 1 + np.log2(k & -k).astype(np.int64)
    x = np.concatenate([[0], np.cumsum(gaps)]).astype(np.float64)
    return np.stack([x, np.zeros(r1)], axis=1), gaps


def boruvka_rounds_on_a_line(gaps):
    """rounds until the intervals of a line are one, every interval joining across the lesser of its two boundary gaps under the
    order (gap, left row): the nearest foreign row of an interval of a line lies across one of its boundaries"""
    n = len(gaps) + 1
    cut = np.ones(n - 1, dtype=bool)  # cut[k]: rows k and k + 1 lie in different intervals
    rounds = 0
    while cut.any():
        bounds = np.nonzero(cut)[0]
        starts = np.concatenate([[0], bounds + 1])
        chosen = set()
        for s in range(len(starts)):
            sides = []
            if s > 0:
                sides.append((gaps[bounds[s - 1]], bounds[s - 1]))
            if s < len(bounds):
                sides.append((gaps[bounds[s]], bounds[s]))
            chosen.add(min(sides)[1])
        cut[list(chosen)] = False
        rounds += 1
    return rounds


def device_forest(kpop, rs, r1, cap, stream=None, bufs=None):
    """kpop_dev_spanning_forest with a workspace of its own of the size the sizing call returns -> (buffers, a function that reads them)"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    if bufs is None:
        room = max(r1 - 1, 1)
        bufs = dict(work=torch.empty(max(api.dev_spanning_forest_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev),
                    n=torch.full((1,), -3, dtype=torch.int32, device=dev), ei=torch.full((room,), -3, dtype=torch.int32, device=dev),
                    ej=torch.full((room,), -3, dtype=torch.int32, device=dev), ed=torch.full((room,), -3.0, dtype=torch.float64, device=dev),
                    labels=torch.full((max(r1, 1),), -3, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
    api.dev_spanning_forest(rs, cap, bufs["work"].data_ptr(), bufs["n"].data_ptr(), bufs["ei"].data_ptr(), bufs["ej"].data_ptr(), bufs["ed"].data_ptr(),
                            bufs["labels"].data_ptr(), stream=stream.cuda_stream if stream is not None else 0)

    def read():
        n = int(bufs["n"].item())
        return (bufs["ei"].cpu().numpy().view(np.uint32)[:n], bufs["ej"].cpu().numpy().view(np.uint32)[:n], bufs["ed"].cpu().numpy()[:n],
                bufs["labels"].cpu().numpy().view(np.uint32)[:r1])
    return bufs, read


@pytest.mark.parametrize("r1", [1024, 1025])
def test_as_many_rounds_as_a_set_can_need(kpop, r1):
    """components pair up exactly once a round: 1,024 rows need log2 = 10 rounds, the most 1,024 rows can need, in the host form (which
    stops when a round adds nothing) and in the device form (which enqueues ceil(log2 r1)).  The 1,025th row joins in the first round, by
    its only gap: 10 rounds again, of the 11 that the device form enqueues -- the last returns at once"""
    import torch
    m, gaps = ruler_rows(r1)
    rounds = boruvka_rounds_on_a_line(gaps)
    assert rounds == 10, rounds
    D = np.abs(m[:, None, 0] - m[None, :, 0])  # whole numbers: the chain's bits
    want = forest_ref(D, INF)
    order = np.lexsort((np.arange(r1 - 1), gaps))  # the path 0-1-2-..., its edges by (gap, left row)
    assert np.array_equal(want[0], order) and np.array_equal(want[1], order + 1) and np.array_equal(want[2], gaps[order].astype(np.float64))
    rs = kpop.RefSet(m, np.ones(2), 0, 2.0, False)
    try:
        check_forest(rs.spanning_forest(), want, ("ruler", r1, "host form"))
        _, read = device_forest(kpop, rs, r1, INF)
        torch.cuda.synchronize()
        check_forest(read(), want, ("ruler", r1, "device form"))
    finally:
        rs.free()


def test_nan_and_inf(kpop, oracle):
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
                for cap in (INF, float(np.nanquantile(lower(D), 0.05))):
                    want = forest_ref(D, cap)
                    got = rs.spanning_forest(cap)
                    check_forest(got, want, (kind, normalize, cap))
                    ei, ej, _, labels = got
                    assert labels[20] == 20 and int(np.sum(labels == 20)) == 1 and not np.any(ei == 20) and not np.any(ej == 20)
                assert len(rs.spanning_forest(INF)[0]) == r1 - 2  # two components: the rest, and the NaN row
            finally:
                rs.free()
    # a row so large that its distances overflow: it joins under +inf alone, and last
    huge = np.array(m)
    huge[30] = 1e200
    D = self_matrix(oracle, huge, metric, 0, 2.0, False)
    assert np.all(np.isinf(np.delete(D[30], 30)))
    rs = kpop.RefSet(huge, metric, 0, 2.0, False)
    try:
        want = forest_ref(D, INF)
        got = rs.spanning_forest(INF)
        check_forest(got, want, "overflow, +inf")
        ei, ej, ed, labels = got
        assert len(ei) == r1 - 1 and np.isinf(ed[-1]) and np.all(np.isfinite(ed[:-1])) and (ei[-1], ej[-1]) == (0, 30) and not labels.any()
        got = rs.spanning_forest(1e300)
        check_forest(got, forest_ref(D, 1e300), "overflow, a finite cap")
        assert len(got[0]) == r1 - 2 and got[3][30] == 30 and not np.any(got[0] == 30) and not np.any(got[1] == 30)
    finally:
        rs.free()


def test_beyond_65535_rows(kpop, oracle):
    """The locator takes the tiles of a long set (32 columns x 256 rows, a thread 4 x 8) from 65,536 rows on, as clusters_tiles does:
    70,000 rows on tests/test_gpu_clusters.py's lattice -- 700 centres of step 4, row i at centre i % 700 plus noise of at most 0.01 a
    coordinate, max_distance = 0.1.  No quadratic reference: every pair of one centre lies below 0.1 and every pair of two centres
    above, so the forest is the union of 700 independent trees of 100 rows, each checked exactly against forest_ref on the oracle's
    100 x 100 block, and row i's label is i % 700"""
    r1, d, n_centres, step, noise, T = 70000, 8, 700, 4.0, 0.01, 0.1
    rng = np.random.RandomState(70008)
    digits = np.array([[(c // 3 ** k) % 3 for k in range(d)] for c in range(n_centres)], dtype=np.float64)
    assert len({tuple(r) for r in digits.tolist()}) == n_centres
    eps = rng.uniform(-noise, noise, size=(r1, d))
    m = step * digits[np.arange(r1) % n_centres] + eps
    spread = 2.0 * noise * np.sqrt(d)
    assert spread < T / 1.5 and step - spread > 10 * T
    metric = np.ones(d)
    wi, wj, wd = [], [], []
    for c in range(n_centres):
        rows = np.arange(c, r1, n_centres)
        block = oracle.distance_rowwise(m[rows], m[rows], metric, 0, 2.0, False)
        assert block.max() <= T
        bi, bj, bd, _ = forest_ref(block, T)
        assert len(bi) == len(rows) - 1
        wi.append(rows[bi])  # (the rows ascend: i < j and the order inside the block are kept)
        wj.append(rows[bj])
        wd.append(bd)
    wi, wj, wd = np.concatenate(wi), np.concatenate(wj), np.concatenate(wd)
    order = np.lexsort((wj, wi, wd))
    want = (wi[order].astype(np.uint32), wj[order].astype(np.uint32), wd[order], (np.arange(r1) % n_centres).astype(np.uint32))
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.spanning_forest(T)
        check_forest(got, want, "70,000 rows")
        assert len(got[0]) == r1 - n_centres
    finally:
        rs.free()


def raw_forest(rs_handle, cap, r1, labels=True):
    from kpop_amd import _lib
    room = max(r1 - 1, 1)
    ei, ej, ed = np.full(room, 12345, dtype=np.uint32), np.full(room, 12345, dtype=np.uint32), np.zeros(room)
    lab = np.full(max(r1, 1), 12345, dtype=np.uint32)
    n = C.c_uint32(12345)
    u32p = C.POINTER(C.c_uint32)
    rc = _lib.load().kpop_spanning_forest(rs_handle, cap, C.byref(n), ei.ctypes.data_as(u32p), ej.ctypes.data_as(u32p),
                                          ed.ctypes.data_as(C.POINTER(C.c_double)), lab.ctypes.data_as(u32p) if labels else None)
    return rc, n.value, ei, ej, ed, lab


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    cap = float(np.quantile(lower(D), 0.05))
    want = forest_ref(D, cap)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        with pytest.raises(kpop.KPopError) as e:
            rs.spanning_forest(float("nan"))
        assert e.value.code == ERR_INVALID
        ei, ej, ed, labels = rs.spanning_forest(-1.0)  # below zero: no edge
        assert len(ei) == len(ej) == len(ed) == 0 and np.array_equal(labels, np.arange(r1))
        rc, n, ei, ej, ed, _ = raw_forest(rs.handle, cap, r1, labels=False)  # labels may be NULL
        assert rc == 0 and n == len(want[0])
        assert np.array_equal(ei[:n], want[0]) and np.array_equal(ej[:n], want[1]) and np.array_equal(ed[:n], want[2])
        check_forest(kpop.distance_spanning_forest(m, metric, 0, 2.0, True, cap), want, "distance_spanning_forest")
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.spanning_forest(cap)
    assert e.value.code == ERR_INVALID
    assert raw_forest(None, cap, r1)[0] == ERR_INVALID  # a null handle
    # a set of another slot (two slots on the one GPU, as tests/test_gpu_refset.py makes them)
    kpop.init_devices([0, 0])
    try:
        rs = kpop.RefSet(m, metric, 0, 2.0, True)
        try:
            kpop.use_device(1)
            with pytest.raises(kpop.KPopError) as e:
                rs.spanning_forest(cap)
            assert e.value.code == ERR_INVALID and "slot" in str(e.value)
            kpop.use_device(0)
            check_forest(rs.spanning_forest(cap), want, "back on its slot")
        finally:
            kpop.use_device(0)
            rs.free()
    finally:
        kpop.init(0)
    # no rows; one row
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        ei, ej, ed, labels = empty.spanning_forest()
        assert len(ei) == len(ej) == len(ed) == 0 and labels.size == 0
        rc, n = raw_forest(empty.handle, INF, 0)[:2]
        assert rc == 0 and n == 0
    finally:
        empty.free()
    one = kpop.RefSet(m[:1], metric, 0, 2.0, True)
    try:
        ei, ej, ed, labels = one.spanning_forest()
        assert len(ei) == len(ej) == len(ed) == 0 and labels.tolist() == [0]
    finally:
        one.free()
    ei, ej, ed, labels = kpop.distance_spanning_forest(np.zeros((0, d)), metric, 0, 2.0, True)
    assert len(ei) == 0 and labels.size == 0
    two = kpop.distance_spanning_forest(m[[3, 7]], metric, 0, 2.0, True)
    assert two[0].tolist() == [0] and two[1].tolist() == [1] and two[2].tolist() == [0.0] and two[3].tolist() == [0, 0]


def test_device_form_on_streams(kpop, oracle):
    """kpop_dev_spanning_forest with its own workspace on a stream of the caller's; two sets on two streams back to back give what each
    gives alone, and a second run on the same buffers the same bits"""
    import torch
    dev = torch.device("cuda:0")
    cases = [(1000, 16, 0, 2.0, True, 0.01), (300, 200, 1, 2.0, False, None)]
    sets, wants, bufs, streams = [], [], [], []
    try:
        for r1, d, kind, p, normalize, q in cases:
            m, metric = operands(oracle, r1, d)
            D = oracle_matrix(oracle, r1, d, kind, p, normalize)
            cap = INF if q is None else float(np.quantile(lower(D), q))
            rs = kpop.RefSet(m, metric, kind, p, normalize)
            sets.append((rs, cap, r1))
            wants.append(forest_ref(D, cap))
            check_forest(rs.spanning_forest(cap), wants[-1], "host form")
            bufs.append(None)
            streams.append(torch.cuda.Stream(device=dev))
        # each alone on its stream, twice on the same buffers: nothing is left over from the first call
        for k, ((rs, cap, r1), stream, want) in enumerate(zip(sets, streams, wants)):
            with torch.cuda.stream(stream):
                bufs[k], read = device_forest(kpop, rs, r1, cap, stream=stream)
                device_forest(kpop, rs, r1, cap, stream=stream, bufs=bufs[k])
            stream.synchronize()
            check_forest(read(), want, "device form")
            for name in ("n", "ei", "ej", "labels"):
                bufs[k][name].fill_(-3)
            bufs[k]["ed"].fill_(-3.0)
        torch.cuda.synchronize()
        # both enqueued before either is waited for
        reads = []
        for (rs, cap, r1), b, stream in zip(sets, bufs, streams):
            with torch.cuda.stream(stream):
                reads.append(device_forest(kpop, rs, r1, cap, stream=stream, bufs=b)[1])
        for stream in streams:
            stream.synchronize()
        for read, want in zip(reads, wants):
            check_forest(read(), want, "two streams")
        # without labels: they then live in the workspace
        from kpop_amd import api
        (rs, cap, r1), b = sets[0], bufs[0]
        for name in ("n", "ei", "ej"):
            b[name].fill_(-3)
        b["ed"].fill_(-3.0)
        torch.cuda.synchronize()
        api.dev_spanning_forest(rs, cap, b["work"].data_ptr(), b["n"].data_ptr(), b["ei"].data_ptr(), b["ej"].data_ptr(), b["ed"].data_ptr(), None,
                                stream=streams[0].cuda_stream)
        streams[0].synchronize()
        check_forest(reads[0](), wants[0], "no labels")  # (the labels of the call before: untouched)
    finally:
        for rs, _, _ in sets:
            rs.free()
