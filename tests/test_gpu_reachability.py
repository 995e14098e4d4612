"""The mutual-reachability forest of a resident set (kpop_reachability_tree, include/kpop_hip.h): every row's core
distance -- the distance to its (min_pts - 1)-th nearest other row -- and the minimum spanning forest of the graph whose edge i < j
weighs max(d(j, i), core_i, core_j), under the strict order (weight, i, j).

The contract: the core distances and the forest are unique, so they are array-equal to tests/reachability_ref.py on the oracle's matrix
of the set against itself, on every run; with min_pts = 1 the result is RefSet.spanning_forest's; cutting the forest at any
T <= max_distance gives RefSet.dbscan(T, min_pts)'s labels on the core rows and leaves every other row alone (DBSCAN*).  The reference
matrix is tests/test_gpu_forest.py's: the oracle's for the euclidean and cosine kinds, the GPU's own vector-pipe matrix for the Minkowski
kind (its pow agrees with the oracle's to rtol 1e-11 only, and the order of ties is that of the GPU's own bits).  The rows are that
file's too: clustered on grids, a duplicated row, a zero row, an equal-step chain -- mutual-reachability weights tie far more often than
distances (every edge out of a row within its core distance weighs at least that), which is the point."""
import ctypes as C

import numpy as np
import pytest

from dbscan_ref import NOISE
from forest_ref import cut_ref
from reachability_ref import core_ref, reachability_cut_ref, reachability_forest_ref
from test_gpu_forest import (INF, KINDS, SHAPES, boruvka_rounds_on_a_line, check_forest, lower, on_the_vector_pipe, operands, oracle_matrix, ruler_rows,
                             self_matrix)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
# 33 | 34 and 65 | 66: either side of the limits k = 32 and k = 64 of the lists' strip shapes (k = min_pts - 1); 129: k = 128, the cap
MIN_PTS = [1, 2, 5, 33, 34, 65, 66, 129]
NAN_BITS = 0x7FF8000000000000


def same_core(got, want):
    return got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True) and not np.any(np.signbit(got[got == 0.0]))


def check_reach(got, want, what):
    """(edge_i, edge_j, edge_dist, core_dist, labels) against the reference's, array for array"""
    assert same_core(got[3], want[3]), (what, "core distances")
    check_forest((got[0], got[1], got[2], got[4]), (want[0], want[1], want[2], want[4]), what)
    nans = got[3][np.isnan(got[3])]
    assert np.all(nans.view(np.uint64) == NAN_BITS), what


_own = {}


def matrix(kpop, oracle, rs, r1, d, kind, p, normalize):
    """the reference matrix of a shape: the oracle's, or for the Minkowski kind the GPU's own on the vector pipe -- made once, read-only"""
    if kind != 2:
        return oracle_matrix(oracle, r1, d, kind, p, normalize)
    key = (r1, d, normalize)
    if key not in _own:
        D = on_the_vector_pipe(rs, operands(oracle, r1, d)[0])
        D.setflags(write=False)
        _own[key] = D
    return _own[key]


@pytest.mark.parametrize("min_pts", MIN_PTS)
@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_forest_vs_reference(kpop, oracle, r1, d, kind, p, min_pts):
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize, min_pts)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            D = matrix(kpop, oracle, rs, r1, d, kind, p, normalize)
            core = core_ref(D, min_pts)
            assert same_core(rs.core_distances(min_pts), core), what  # (relation 4: the call of its own gives the forest's)
            assert np.isfinite(core).all(), what  # (129 others at the most are asked for, and the smallest set has 129)
            for name, cap in [("inf", INF), ("q0.03", float(np.quantile(lower(D), 0.03))), ("tie", float(D[3, 0]))]:
                want = reachability_forest_ref(D, min_pts, cap)
                print("  %s %s max_distance=%.17g: %d edges, %d distinct weights among them" % (what, name, cap, len(want[0]), len(np.unique(want[2]))))
                if name == "inf":
                    assert len(want[0]) == r1 - 1, what  # one tree
                    # the ties: fewer distinct weights than edges -- a property of these rows, asserted of the reference alone.  As
                    # they are, the chain's equal steps tie whatever min_pts is; normalised, the duplicated rows 3 and 7 share one
                    # core distance, which from min_pts = 3 on is the weight of their edge and of the edge that joins the pair to
                    # the rest (at min_pts 1 and 2 it is zero and ties with nothing: the cosine kind has no tie at all there)
                    assert (normalize and min_pts <= 2) or len(np.unique(want[2])) < len(want[2]), what
                got = rs.reachability_forest(min_pts, cap)
                check_reach(got, want, (what, name))
                again = rs.reachability_forest(min_pts, cap)  # the same bits, whoever arrived first
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(again, got)), (what, name, "a second run")
        finally:
            rs.free()


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as it is"])
def test_the_four_relations(kpop, oracle, normalize):
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, normalize)
    quantiles = [float(np.quantile(lower(D), q)) for q in (0.001, 0.01, 0.05, 0.5)]
    rs = kpop.RefSet(m, metric, 0, 2.0, normalize)
    try:
        # 1. min_pts = 1: the single-linkage tree, array for array
        for cap in (INF, quantiles[1], float(D[3, 0]), -1.0):
            ei, ej, ed, core, labels = rs.reachability_forest(1, cap)
            assert all(np.array_equal(a, b) for a, b in zip((ei, ej, ed, labels), rs.spanning_forest(cap))), cap
            assert np.array_equal(core.view(np.uint64), np.zeros(r1, dtype=np.uint64))
        for min_pts in (2, 5, 33):
            ei, ej, ed, core, labels = rs.reachability_forest(min_pts)
            assert len(ei) == r1 - 1 and not labels.any()
            clusters = []
            for T in quantiles:
                # 2. the cut is DBSCAN*: dbscan's labels on the core rows, every other row a component of its own
                want, _, degree, counts = rs.dbscan(T, min_pts)
                is_core = degree >= min_pts
                assert np.array_equal(core <= T, is_core), (min_pts, T)  # core_dist <= eps iff degree >= min_pts
                cut = kpop.forest_cut(r1, ei, ej, ed, T)[0]
                assert np.array_equal(cut[is_core], want[is_core]), (min_pts, T)
                assert np.array_equal(cut[~is_core], np.arange(r1)[~is_core]) and np.all(np.bincount(cut, minlength=r1)[cut[~is_core]] == 1), (min_pts, T)
                got, got_counts = kpop.reachability_cut(r1, ei, ej, ed, core, T)
                assert np.array_equal(got[is_core], want[is_core]) and np.all(got[~is_core] == NOISE), (min_pts, T)
                assert got_counts.tolist() == [int(counts[0]), int(counts[1]), r1 - int(counts[1])], (min_pts, T)
                assert all(np.array_equal(a, b) for a, b in zip((got, got_counts), reachability_cut_ref(r1, ei, ej, ed, core, T)))
                clusters.append(int(counts[0]))
                # 3. a forest capped at T: the prefix of the uncapped one, the same core distances, the cut's labels
                ci, cj, cd, ccore, clabels = rs.reachability_forest(min_pts, T)
                keep = ed <= T
                assert np.array_equal(ci, ei[keep]) and np.array_equal(cj, ej[keep]) and np.array_equal(cd, ed[keep]), (min_pts, T)
                assert np.array_equal(ccore, core) and np.array_equal(clabels, cut), (min_pts, T)
            print("  normalize=%s min_pts=%d: clusters at the four cuts %s" % (normalize, min_pts, clusters))
            assert len(set(clusters)) >= (3 if min_pts <= 5 else 2)  # the cuts are different clusterings
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
                for min_pts in (1, 2, 5, 129):
                    for cap in (INF, float(np.nanquantile(lower(D), 0.05))):
                        want = reachability_forest_ref(D, min_pts, cap)
                        got = rs.reachability_forest(min_pts, cap)
                        check_reach(got, want, (kind, normalize, min_pts, cap))
                        ei, ej, _, core, labels = got
                        assert labels[20] == 20 and int(np.sum(labels == 20)) == 1 and not np.any(ei == 20) and not np.any(ej == 20)
                        # the NaN row has no core distance from min_pts = 2 on; every other row's list simply lacks it: 128 others,
                        # exactly what min_pts = 129 asks for
                        assert (core[20] == 0.0) if min_pts == 1 else np.isnan(core[20])
                        assert np.isfinite(np.delete(core, 20)).all()
                    assert len(rs.reachability_forest(min_pts)[0]) == r1 - 2  # two components: the rest, and the NaN row
            finally:
                rs.free()
    # a row so large that its distances overflow: +inf is a number, so it is in every list's order -- behind all the others -- and the
    # others' core distances stay finite up to min_pts = r1 - 1; it joins under +inf alone, and last
    huge = np.array(m)
    huge[30] = 1e200
    D = self_matrix(oracle, huge, metric, 0, 2.0, False)
    assert np.all(np.isinf(np.delete(D[30], 30)))
    rs = kpop.RefSet(huge, metric, 0, 2.0, False)
    try:
        for min_pts in (2, 5, 129):
            want = reachability_forest_ref(D, min_pts)
            got = rs.reachability_forest(min_pts)
            check_reach(got, want, ("overflow, +inf", min_pts))
            ei, ej, ed, core, labels = got
            assert np.isinf(core[30]) and np.isfinite(np.delete(core, 30)).all()
            assert len(ei) == r1 - 1 and np.isinf(ed[-1]) and np.all(np.isfinite(ed[:-1])) and (ei[-1], ej[-1]) == (0, 30) and not labels.any()
            got = rs.reachability_forest(min_pts, 1e300)
            check_reach(got, reachability_forest_ref(D, min_pts, 1e300), ("overflow, a finite cap", min_pts))
            assert len(got[0]) == r1 - 2 and got[4][30] == 30 and not np.any(got[0] == 30) and not np.any(got[1] == 30)
    finally:
        rs.free()


def raw_reach(rs_handle, min_pts, cap, r1, core=True, labels=True, edges=True, count=True):
    from kpop_amd import _lib
    room = max(r1 - 1, 1)
    ei, ej, ed = np.full(room, 12345, dtype=np.uint32), np.full(room, 12345, dtype=np.uint32), np.full(room, -7.0)
    co = np.full(max(r1, 1), -7.0)
    lab = np.full(max(r1, 1), 12345, dtype=np.uint32)
    n = C.c_uint32(12345)
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    rc = _lib.load().kpop_reachability_tree(rs_handle, min_pts, cap, C.byref(n) if count else None, ei.ctypes.data_as(u32p) if edges else None,
                                            ej.ctypes.data_as(u32p) if edges else None, ed.ctypes.data_as(f64p) if edges else None,
                                            co.ctypes.data_as(f64p) if core else None, lab.ctypes.data_as(u32p) if labels else None)
    return rc, n.value, ei, ej, ed, co, lab


def test_arguments(kpop, oracle):
    from kpop_amd import _lib
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    cap = float(np.quantile(lower(D), 0.05))
    want = reachability_forest_ref(D, 5, cap)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        for call in (lambda mp: rs.reachability_forest(mp, cap), rs.core_distances, lambda mp: kpop.distance_reachability_forest(m, metric, 0, 2.0, True, mp)):
            with pytest.raises(kpop.KPopError) as e:
                call(0)
            assert e.value.code == ERR_INVALID
            with pytest.raises(kpop.KPopError) as e:
                call(130)
            assert e.value.code == ERR_UNSUPPORTED and "129" in str(e.value)
        for sizing in (kpop.dev_reachability_forest_workspace_bytes, kpop.dev_core_distances_workspace_bytes):
            assert sizing(rs, 0) == 0 and sizing(rs, 130) == 0 and sizing(rs, 129) > 0
        with pytest.raises(kpop.KPopError) as e:
            rs.reachability_forest(5, float("nan"))
        assert e.value.code == ERR_INVALID
        ei, ej, ed, core, labels = rs.reachability_forest(5, -1.0)  # below zero: no edge, the core distances all the same
        assert len(ei) == len(ej) == len(ed) == 0 and np.array_equal(labels, np.arange(r1)) and same_core(core, want[3])
        # poisoned buffers: what is written is the result, what lies behind the edges is left alone; core_dist and labels may be NULL
        rc, n, ei, ej, ed, co, lab = raw_reach(rs.handle, 5, cap, r1)
        assert rc == 0 and n == len(want[0]) and n < r1 - 1
        check_reach((ei[:n], ej[:n], ed[:n], co, lab), want, "poisoned buffers")
        assert np.all(ei[n:] == 12345) and np.all(ej[n:] == 12345) and np.all(ed[n:] == -7.0)
        rc, n, ei, ej, ed, co, lab = raw_reach(rs.handle, 5, cap, r1, core=False, labels=False)
        assert rc == 0 and n == len(want[0]) and np.all(co == -7.0) and np.all(lab == 12345)
        assert np.array_equal(ei[:n], want[0]) and np.array_equal(ej[:n], want[1]) and np.array_equal(ed[:n], want[2])
        assert raw_reach(rs.handle, 5, cap, r1, edges=False)[0] == ERR_INVALID
        assert raw_reach(rs.handle, 5, cap, r1, count=False)[0] == ERR_INVALID
        assert _lib.load().kpop_core_distances(rs.handle, 5, None) == ERR_INVALID
        check_reach(kpop.distance_reachability_forest(m, metric, 0, 2.0, True, 5, cap), want, "distance_reachability_forest")
        # min_pts > r1 (within the cap of 129 on a shorter set): nobody has that many others
        few = kpop.RefSet(m[:40], metric, 0, 2.0, True)
        try:
            for min_pts in (41, 129):
                ei, ej, ed, core, labels = few.reachability_forest(min_pts)
                assert len(ei) == 0 and np.array_equal(labels, np.arange(40)) and np.all(core.view(np.uint64) == NAN_BITS)
                assert np.all(few.core_distances(min_pts).view(np.uint64) == NAN_BITS)
            check_reach(few.reachability_forest(40), reachability_forest_ref(D[:40, :40], 40), "min_pts = r1")
        finally:
            few.free()
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.reachability_forest(5, cap)
    assert e.value.code == ERR_INVALID
    assert raw_reach(None, 5, cap, r1)[0] == ERR_INVALID  # a null handle
    # no rows; one row; two rows
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        assert [a.size for a in empty.reachability_forest(3)] == [0] * 5 and empty.core_distances(3).size == 0
        rc, n = raw_reach(empty.handle, 3, INF, 0)[:2]
        assert rc == 0 and n == 0
    finally:
        empty.free()
    one = kpop.RefSet(m[:1], metric, 0, 2.0, True)
    try:
        for min_pts, bits in ((1, 0), (2, NAN_BITS)):
            ei, ej, ed, core, labels = one.reachability_forest(min_pts)
            assert len(ei) == len(ej) == len(ed) == 0 and labels.tolist() == [0] and core.view(np.uint64).tolist() == [bits]
    finally:
        one.free()
    assert [a.size for a in kpop.distance_reachability_forest(np.zeros((0, d)), metric, 0, 2.0, True, 2)] == [0] * 5
    for min_pts, edges in ((1, [0.0]), (2, [0.0]), (3, [])):  # rows 3 and 7 are duplicates: each is the other's only neighbour, at 0
        two = kpop.distance_reachability_forest(m[[3, 7]], metric, 0, 2.0, True, min_pts)
        assert two[0].tolist() == [0] * len(edges) and two[1].tolist() == [1] * len(edges) and two[2].tolist() == edges
        assert two[4].tolist() == ([0, 0] if edges else [0, 1])
        assert two[3].view(np.uint64).tolist() == ([0, 0] if edges else [NAN_BITS] * 2)


def device_reach(kpop, rs, r1, min_pts, cap, stream=None, bufs=None, core=True, labels=True):
    """kpop_dev_reachability_tree with a workspace of its own of the size the sizing call returns -> (buffers, a function that reads them)"""
    import torch
    dev = torch.device("cuda:0")
    if bufs is None:
        room = max(r1 - 1, 1)
        bufs = dict(work=torch.empty(max(kpop.dev_reachability_forest_workspace_bytes(rs, min_pts), 1), dtype=torch.uint8, device=dev),
                    n=torch.full((1,), -3, dtype=torch.int32, device=dev), ei=torch.full((room,), -3, dtype=torch.int32, device=dev),
                    ej=torch.full((room,), -3, dtype=torch.int32, device=dev), ed=torch.full((room,), -3.0, dtype=torch.float64, device=dev),
                    core=torch.full((max(r1, 1),), -3.0, dtype=torch.float64, device=dev), labels=torch.full((max(r1, 1),), -3, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
    kpop.dev_reachability_forest(rs, min_pts, cap, bufs["work"].data_ptr(), bufs["n"].data_ptr(), bufs["ei"].data_ptr(), bufs["ej"].data_ptr(),
                                 bufs["ed"].data_ptr(), bufs["core"].data_ptr() if core else None, bufs["labels"].data_ptr() if labels else None,
                                 stream=stream.cuda_stream if stream is not None else 0)

    def read():
        n = int(bufs["n"].item())
        return (bufs["ei"].cpu().numpy().view(np.uint32)[:n], bufs["ej"].cpu().numpy().view(np.uint32)[:n], bufs["ed"].cpu().numpy()[:n],
                bufs["core"].cpu().numpy()[:r1], bufs["labels"].cpu().numpy().view(np.uint32)[:r1])
    return bufs, read


@pytest.mark.parametrize("r1", [1024, 1025])
def test_as_many_rounds_as_a_set_can_need(kpop, r1):
    """tests/test_gpu_forest.py's ruler: gaps 1 2 1 3 1 2 1 4 ... on a line.  At min_pts = 2 a row's core distance is the lesser of its two
    gaps, which exceeds neither, so the path's edges weigh their gaps again and components pair up exactly once a round: 10 rounds, the
    most 1,024 rows can need, in the host form (which stops when a round adds nothing) and in the device form (which enqueues
    ceil(log2 r1), 11 for 1,025 rows: the last returns at once)"""
    import torch
    m, gaps = ruler_rows(r1)
    D = np.abs(m[:, None, 0] - m[None, :, 0])  # whole numbers: the chain's bits
    want = reachability_forest_ref(D, 2)
    side = np.concatenate([[gaps[0]], np.minimum(gaps[1:], gaps[:-1]), [gaps[-1]]]).astype(np.float64)
    assert np.array_equal(want[3], side)
    weights = np.maximum(gaps, np.maximum(side[:-1], side[1:]))  # the path 0-1-2-..., its edges by (weight, left row)
    order = np.lexsort((np.arange(r1 - 1), weights))
    assert np.array_equal(want[0], order) and np.array_equal(want[1], order + 1) and np.array_equal(want[2], weights[order])
    assert boruvka_rounds_on_a_line(weights) == 10
    rs = kpop.RefSet(m, np.ones(2), 0, 2.0, False)
    try:
        check_reach(rs.reachability_forest(2), want, ("ruler", r1, "host form"))
        _, read = device_reach(kpop, rs, r1, 2, INF)
        torch.cuda.synchronize()
        check_reach(read(), want, ("ruler", r1, "device form"))
    finally:
        rs.free()


def test_device_form_on_streams(kpop, oracle):
    """kpop_dev_reachability_tree and kpop_dev_core_distances with their own workspaces on a stream of the caller's; two sets on two streams
    back to back give what each gives alone, and a second run on the same buffers the same bits"""
    import torch
    dev = torch.device("cuda:0")
    cases = [(1000, 16, 0, 2.0, True, 0.03, 5), (300, 200, 1, 2.0, False, None, 66)]
    sets, wants, bufs, streams = [], [], [], []
    try:
        for r1, d, kind, p, normalize, q, min_pts in cases:
            m, metric = operands(oracle, r1, d)
            D = oracle_matrix(oracle, r1, d, kind, p, normalize)
            cap = INF if q is None else float(np.quantile(lower(D), q))
            rs = kpop.RefSet(m, metric, kind, p, normalize)
            sets.append((rs, min_pts, cap, r1))
            wants.append(reachability_forest_ref(D, min_pts, cap))
            check_reach(rs.reachability_forest(min_pts, cap), wants[-1], "host form")
            bufs.append(None)
            streams.append(torch.cuda.Stream(device=dev))
        # each alone on its stream, twice on the same buffers: nothing is left over from the first call
        for k, ((rs, min_pts, cap, r1), stream, want) in enumerate(zip(sets, streams, wants)):
            with torch.cuda.stream(stream):
                bufs[k], read = device_reach(kpop, rs, r1, min_pts, cap, stream=stream)
                device_reach(kpop, rs, r1, min_pts, cap, stream=stream, bufs=bufs[k])
            stream.synchronize()
            check_reach(read(), want, "device form")
            for name in ("n", "ei", "ej", "labels"):
                bufs[k][name].fill_(-3)
            bufs[k]["ed"].fill_(-3.0)
            bufs[k]["core"].fill_(-3.0)
        torch.cuda.synchronize()
        # both enqueued before either is waited for
        reads = []
        for (rs, min_pts, cap, r1), b, stream in zip(sets, bufs, streams):
            with torch.cuda.stream(stream):
                reads.append(device_reach(kpop, rs, r1, min_pts, cap, stream=stream, bufs=b)[1])
        for stream in streams:
            stream.synchronize()
        for read, want in zip(reads, wants):
            check_reach(read(), want, "two streams")
        # without core distances and labels: they then live in the workspace
        (rs, min_pts, cap, r1), b = sets[0], bufs[0]
        for name in ("n", "ei", "ej"):
            b[name].fill_(-3)
        b["ed"].fill_(-3.0)
        torch.cuda.synchronize()
        device_reach(kpop, rs, r1, min_pts, cap, stream=streams[0], bufs=b, core=False, labels=False)
        streams[0].synchronize()
        check_reach(reads[0](), wants[0], "neither core distances nor labels")  # (those of the call before: untouched)
        # the core distances alone
        for (rs, min_pts, cap, r1), stream, want in zip(sets, streams, wants):
            work = torch.empty(max(kpop.dev_core_distances_workspace_bytes(rs, min_pts), 1), dtype=torch.uint8, device=dev)
            core = torch.full((r1,), -3.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            kpop.dev_core_distances(rs, min_pts, work.data_ptr(), core.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert same_core(core.cpu().numpy(), want[3])
    finally:
        for rs, _, _, _ in sets:
            rs.free()


def test_growth(kpop, oracle):
    """there is no known_rows: after an append the call is made again in full, and gives what a fresh set of all the rows gives"""
    r1, d, r0 = 1000, 16, 700
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    rs = kpop.RefSet(m[:r0], metric, 0, 2.0, True, capacity=r1)
    fresh = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        for min_pts in (5, 66):
            check_reach(rs.reachability_forest(min_pts), reachability_forest_ref(D[:r0, :r0], min_pts), ("before the append", min_pts))
        rs.append(m[r0:])
        for min_pts in (5, 66):
            want = reachability_forest_ref(D, min_pts)
            grown = rs.reachability_forest(min_pts)
            check_reach(grown, want, ("grown", min_pts))
            assert all(np.array_equal(a, b) for a, b in zip(grown, fresh.reachability_forest(min_pts))), min_pts
            assert same_core(rs.core_distances(min_pts), want[3])
    finally:
        rs.free()
        fresh.free()


def test_beyond_65535_rows(kpop, oracle):
    """The tiles of a long set (32 columns x 256 rows, a thread 4 x 8) from 65,536 rows on, and five slabs of the core distances' lists:
    tests/test_gpu_forest.py's 70,000-row lattice -- 700 centres of step 4, row i at centre i % 700 plus noise of at most 0.01 a
    coordinate -- at min_pts = 5, max_distance = 0.1.  No quadratic reference: every pair of one centre lies below 0.1 and every pair of
    two centres above, so each row's four nearest are block mates, its core distance is its block's, and the forest is the union of 700
    independent trees of 100 rows, each checked exactly against the reference on the oracle's 100 x 100 block"""
    r1, d, n_centres, step, noise, T, min_pts = 70000, 8, 700, 4.0, 0.01, 0.1, 5
    rng = np.random.RandomState(70008)
    digits = np.array([[(c // 3 ** k) % 3 for k in range(d)] for c in range(n_centres)], dtype=np.float64)
    assert len({tuple(r) for r in digits.tolist()}) == n_centres
    eps = rng.uniform(-noise, noise, size=(r1, d))
    m = step * digits[np.arange(r1) % n_centres] + eps
    spread = 2.0 * noise * np.sqrt(d)
    assert spread < T / 1.5 and step - spread > 10 * T
    metric = np.ones(d)
    wi, wj, wd, wcore = [], [], [], np.zeros(r1)
    for c in range(n_centres):
        rows = np.arange(c, r1, n_centres)
        block = oracle.distance_rowwise(m[rows], m[rows], metric, 0, 2.0, False)
        assert block.max() <= T
        bi, bj, bd, bcore, _ = reachability_forest_ref(block, min_pts, T)
        assert len(bi) == len(rows) - 1
        wi.append(rows[bi])  # (the rows ascend: i < j and the order inside the block are kept)
        wj.append(rows[bj])
        wd.append(bd)
        wcore[rows] = bcore
    wi, wj, wd = np.concatenate(wi), np.concatenate(wj), np.concatenate(wd)
    order = np.lexsort((wj, wi, wd))
    want = (wi[order].astype(np.uint32), wj[order].astype(np.uint32), wd[order], wcore, (np.arange(r1) % n_centres).astype(np.uint32))
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.reachability_forest(min_pts, T)
        check_reach(got, want, "70,000 rows")
        assert len(got[0]) == r1 - n_centres
    finally:
        rs.free()
