"""The k-NN vote on a labelled resident set (kpop_knn_vote, include/kpop_hip.h).

The contract: the four outputs are knn_vote_ref (tests/knn_vote_ref.py) of the matrix RefSet.distance_rowwise writes on the vector pipe
(kpop_tune("distance_mfma", 0)), bit for bit and under any tune setting; for the euclidean and cosine kinds that matrix is the oracle's,
bit for bit.  The Minkowski kind goes through the GPU's pow, which agrees with the oracle's to rtol 1e-11 (tests/test_gpu_refset.py):
there the comparison with the oracle is made on the continuous shapes and on the rows whose k + 1 smallest oracle distances lie either
on each other or >= 1e-8 (relative) apart, so that no order is ambiguous; the classes, votes and lengths are then the oracle's and the
distance agrees to 1e-11.  (A gap of exactly 0 in these operands comes from the duplicated row, whose two chains are the same operations
on the same numbers on any machine: a tie there is a tie here.)"""
import ctypes as C

import numpy as np
import pytest

from knn_vote_ref import NO_CLASS, knn_lists, knn_vote_ref, same_votes, vote
from test_gpu_within import P_MINK, on_the_vector_pipe, operands

pytestmark = pytest.mark.gpu

KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
SHAPES = [(130, 9, 37), (1000, 16, 40), (5000, 16, 12), (20000, 64, 9), (300, 200, 33), (100, 16, 257)]
KS = (1, 2, 5, 32, 128)


def labellings(r1):
    return [("mod7", (np.arange(r1) % 7).astype(np.uint32)), ("own", np.arange(r1, dtype=np.uint32))]


def unambiguous_rows(D, k):
    """the rows whose k + 1 smallest distances have every consecutive gap either 0 or >= 1e-8 relative"""
    ok = np.zeros(D.shape[0], dtype=bool)
    for j, row in enumerate(D):
        s = np.sort(row[~np.isnan(row)])[:k + 1]
        gaps = np.diff(s)
        ok[j] = bool(np.all((gaps == 0) | (gaps >= 1e-8 * s[1:])))
    return ok


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d,r2", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_vote_vs_oracle_and_rowwise(kpop, oracle, r1, d, r2, kind, p):
    m1, m2, metric = operands(oracle, r1, d, r2)
    for normalize in (True, False):
        D = oracle.distance_rowwise(m1, m2, metric, kind, p, normalize)
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            if kind != 2:
                assert np.array_equal(G.view(np.uint64), D.view(np.uint64))
            for k in KS:
                for name, class_of in labellings(r1):
                    what = (r1, d, r2, kind, normalize, k, name)
                    got = rs.knn_vote(m2, class_of, k=k)
                    assert [a.dtype for a in got] == [np.uint32, np.uint32, np.uint32, np.float64] and all(a.shape == (r2,) for a in got)
                    same_votes(got, knn_vote_ref(G, class_of, k), (what, "rowwise"))
                    if kind != 2:
                        same_votes(got, knn_vote_ref(D, class_of, k), (what, "oracle"))
                    elif d > 16:
                        ok = unambiguous_rows(D, k)
                        print("  %s: %d of %d rows left out as ambiguous" % (what, int((~ok).sum()), r2))
                        assert (~ok).sum() * 20 <= r2, what
                        want = knn_vote_ref(D, class_of, k)
                        for q in range(3):
                            assert np.array_equal(got[q][ok], want[q][ok]), (what, q)
                        np.testing.assert_allclose(got[3][ok], want[3][ok], rtol=1e-11, atol=0)
            # rows 3 and 7 of the set are the same row and query row 1 is that row: the tie group is listed whole
            if r1 > 12:
                cls, votes, n, first = rs.knn_vote(m2, np.arange(r1), k=1)
                assert (int(cls[1]), int(votes[1]), int(n[1]), float(first[1])) == (3, 1, 2, 0.0), (r1, d, r2, kind, normalize)
        finally:
            rs.free()


@pytest.mark.parametrize("r1,d,r2", SHAPES[:2], ids=["%dx%dx%d" % s for s in SHAPES[:2]])
def test_the_summary_is_a_second_witness(kpop, oracle, r1, d, r2):
    """on operands without a NaN the list is the summary line's: the same n, and a vote over its idx gives the same class and count"""
    m1, m2, metric = operands(oracle, r1, d, r2)
    rs = kpop.RefSet(m1, metric, 0, 2.0, True)
    try:
        for k in (1, 2, 5, 32):
            for name, class_of in labellings(r1):
                cls, votes, n, first = rs.knn_vote(m2, class_of, k=k)
                stats, sn, idx, dist, z = rs.distance_summary(m2, keep_at_most=k, max_neighbours=int(n.max()))
                assert np.array_equal(sn, n), (k, name)
                for j in range(r2):
                    c, v, _, _ = vote(idx[j, :sn[j]], dist[j, :sn[j]], class_of)
                    assert (c, v) == (int(cls[j]), int(votes[j])), (k, name, j)
    finally:
        rs.free()


@pytest.mark.parametrize("n_copies", [3000, 600])
def test_a_tie_group_far_longer_than_k(kpop, oracle, n_copies):
    """3,000 copies of one row among 5,000, over every column tile and segment, classes alternating 1, 0, 1, ... from the first copy on:
    the query that is that row lists all of them (k = 5), 1,500 votes each way, and class 1 holds the first of them.  The row beside it
    has no such group and is what it is without.  With k = 128 the lists of the segments hold every copy, and the group is longer than
    the vote takes from lists (1,024) at 3,000 copies, shorter at 600: both ways to the same answer"""
    r1, d = 5000, 16
    rng = np.random.RandomState(77)
    m1 = rng.normal(size=(r1, d))
    copies = np.nonzero((np.arange(r1) * 3) % 25 < n_copies // 200)[0]
    assert len(copies) == n_copies and copies[0] == 0
    m1[copies] = m1[0]
    class_of = (2 + np.arange(r1) % 5).astype(np.uint32)
    class_of[copies] = 1 - np.arange(n_copies) % 2
    m2 = np.vstack([m1[0], rng.normal(size=d)])
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    for kind, p in KINDS:
        for normalize in (True, False):
            rs = kpop.RefSet(m1, metric, kind, p, normalize)
            try:
                G = on_the_vector_pipe(rs, m2)
                assert np.all(G[0, copies] == 0.0) and np.count_nonzero(G[0] == 0.0) == n_copies
                for k in (5, 128):
                    got = rs.knn_vote(m2, class_of, k=k)
                    assert (int(got[0][0]), int(got[1][0]), int(got[2][0]), float(got[3][0])) == (1, n_copies // 2, n_copies, 0.0), (kind, normalize, k)
                    same_votes(got, knn_vote_ref(G, class_of, k), (kind, normalize, k))
                    if G[1, 0] > np.sort(G[1])[k - 1]:  # the copies, all at one distance from the row beside it, lie beyond its k nearest: no tie there
                        assert int(got[2][1]) == k
            finally:
                rs.free()


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
def test_sets_of_65536_rows_and_more(kpop, oracle, kind, p):
    """a long set: 1,094 column tiles in 103 segments a strip, five strips of query rows, the last ragged (300 rows), d no multiple of 16;
    against knn_vote_ref of the vector pipe's matrix on rows of the first and the last two strips (the reference sorts a whole row at a time:
    28 rows of 70,000)"""
    r1, d, r2 = 70000, 24, 300
    m1, m2, metric = operands(oracle, r1, d, r2)
    rows = np.r_[0:8, 250:262, 292:300]
    for normalize in (True, False):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)[rows]
            assert G[1, 3] == G[1, 7] == 0.0
            for k in (5, 6, 7):
                lists = knn_lists(G, k)
                for name, class_of in (("mod7", np.arange(r1) % 7), ("mod60000", np.arange(r1) % 60000)):  # (at most 65,535 classes)
                    got = rs.knn_vote(m2, class_of, k=k)
                    same_votes(tuple(a[rows] for a in got), knn_vote_ref(G, class_of, k, lists=lists), (kind, normalize, k, name))
            cls, votes, n, first = rs.knn_vote(m2, np.arange(r1) % 60000, k=1)
            assert (int(cls[1]), int(votes[1]), int(n[1]), float(first[1])) == (3, 1, 2, 0.0), (kind, normalize)
        finally:
            rs.free()


def test_nan_and_infinity(kpop, oracle):
    m1, m2, metric = operands(oracle, 130, 9, 37)
    r1 = 100
    m1 = np.array(m1[:r1])
    m1[20, 2] = np.nan  # never listed
    m1[40] = 1e200  # +inf under normalize = False: listed, last
    m2 = np.array(m2)
    m2[6] = np.nan  # no list at all
    for normalize in (True, False):
        rs = kpop.RefSet(m1, metric, 0, 2.0, normalize)
        try:
            G = on_the_vector_pipe(rs, m2)
            assert np.isnan(G[:, 20]).all() and np.isnan(G[6]).all()
            for k in (1, 5, 128):
                for name, class_of in labellings(r1):
                    got = rs.knn_vote(m2, class_of, k=k)
                    same_votes(got, knn_vote_ref(G, class_of, k), (normalize, k, name))
                    assert (int(got[0][6]), int(got[1][6]), int(got[2][6])) == (NO_CLASS, 0, 0) and np.isnan(got[3][6])
            n = rs.knn_vote(m2, np.arange(r1), k=128)[2]
            assert np.array_equal(n, (~np.isnan(G)).sum(axis=1)) and n[6] == 0 and n.max() <= r1 - 1  # everything that is a number
            if not normalize:
                assert np.isposinf(np.delete(G[:, 40], 6)).all()
                assert all(l[-1] == 40 for j, l in enumerate(knn_lists(G, 128)) if j != 6)
                # the row at +inf is the only one of its class: it is in the list, so the class has its vote
                class_of = np.zeros(r1, dtype=np.uint32)
                class_of[40] = 1
                cls, votes, n, first = rs.knn_vote(m2, class_of, k=128, n_classes=2)
                assert np.array_equal(np.delete(votes, 6), np.full(36, r1 - 2)) and np.array_equal(np.delete(n, 6), np.full(36, r1 - 1))
        finally:
            rs.free()


def raw_call(rs, class_of, n_classes, m2, k, with_first=True):
    """kpop_knn_vote on the caller's arrays -> (status, cls, votes, n, first)"""
    from kpop_amd import _lib
    m2 = np.ascontiguousarray(m2, dtype=np.float64)
    class_of = np.ascontiguousarray(class_of, dtype=np.uint32)
    r2 = m2.shape[0]
    cls, votes, n = (np.full(r2 + 1, 12345, dtype=np.uint32) for _ in range(3))
    first = np.full(r2 + 1, -7.5)
    u32 = C.POINTER(C.c_uint32)
    rc = _lib.load().kpop_knn_vote(rs.handle, class_of.ctypes.data_as(u32), n_classes, m2.ctypes.data_as(C.POINTER(C.c_double)), r2, k,
                                   cls.ctypes.data_as(u32), votes.ctypes.data_as(u32), n.ctypes.data_as(u32),
                                   first.ctypes.data_as(C.POINTER(C.c_double)) if with_first else None)
    return rc, cls, votes, n, first


def test_contract_edges(kpop, oracle):
    r1, d, r2 = 1000, 16, 40
    m1, m2, metric = operands(oracle, r1, d, r2)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    rs = kpop.RefSet(m1, metric, 0, 2.0, True, capacity=r1 + 8)
    try:
        G = on_the_vector_pipe(rs, m2)
        want = knn_vote_ref(G, class_of, 5)
        rc, cls, votes, n, first = raw_call(rs, class_of, 7, m2, 5)
        assert rc == 0
        same_votes((cls[:r2], votes[:r2], n[:r2], first[:r2]), want, "raw")
        assert (cls[r2], votes[r2], n[r2], first[r2]) == (12345, 12345, 12345, -7.5)  # nothing behind the last row
        # without the distances
        rc, cls, votes, n, first = raw_call(rs, class_of, 7, m2, 5, with_first=False)
        assert rc == 0 and np.all(first == -7.5)
        same_votes((cls[:r2], votes[:r2], n[:r2]), want[:3], "no first_dist")
        # the limits: k, n_classes, the labels
        assert raw_call(rs, class_of, 7, m2, 0)[0] == ERR_INVALID
        assert raw_call(rs, class_of, 7, m2, 129)[0] == ERR_UNSUPPORTED
        assert raw_call(rs, class_of, 6, m2, 5)[0] == ERR_INVALID  # a label of 6
        assert raw_call(rs, class_of, 65536, m2, 5)[0] == ERR_UNSUPPORTED
        rc, cls, votes, n, first = raw_call(rs, class_of, 65535, m2, 5)
        assert rc == 0
        same_votes((cls[:r2], votes[:r2], n[:r2], first[:r2]), want, "65,535 classes")
        for k, code in ((0, ERR_INVALID), (129, ERR_UNSUPPORTED)):
            with pytest.raises(kpop.KPopError) as e:
                rs.knn_vote(m2, class_of, k=k)
            assert e.value.code == code
        # no query rows
        assert all(a.size == 0 for a in rs.knn_vote(np.zeros((0, d)), class_of))
        # three runs, the same bits
        for _ in range(2):
            same_votes(rs.knn_vote(m2, class_of, k=5), want, "again")
        # the unprepared call
        same_votes(kpop.distance_knn_vote(m1, class_of, m2, metric, k=5), want, "distance_knn_vote")
        # after append, with longer labels: what a fresh set over all rows gives
        more = np.array(m1[20:24])
        more[2] = m2[0]
        rs.append(more)
        longer = np.concatenate([class_of, np.array([3, 3, 6, 3], dtype=np.uint32)])
        got = rs.knn_vote(m2, longer, k=5)
        nearest = rs.knn_vote(m2, longer, k=1)
        assert (int(nearest[0][0]), int(nearest[2][0]), float(nearest[3][0])) == (6, 1, 0.0)  # the copy of query row 0 is its nearest row
        both = np.vstack([m1, more])
        same_votes(got, knn_vote_ref(oracle.distance_rowwise(both, m2, metric, 0, 2.0, True), longer, 5), "after append")
        fresh = kpop.RefSet(both, metric, 0, 2.0, True)
        try:
            same_votes(got, fresh.knn_vote(m2, longer, k=5), "a fresh set")
        finally:
            fresh.free()
    finally:
        rs.free()
    # an empty set
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        cls, votes, n, first = empty.knn_vote(m2, np.zeros(0, dtype=np.uint32), k=5)
        assert np.all(cls == NO_CLASS) and not votes.any() and not n.any() and np.isnan(first).all()
    finally:
        empty.free()


def test_no_tune_setting_changes_the_result(kpop, oracle):
    from kpop_amd import api
    r1, d, r2 = 5000, 16, 12
    m1, m2, metric = operands(oracle, r1, d, r2)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            want = knn_vote_ref(on_the_vector_pipe(rs, m2), class_of, 5)
            for key, values, default in (("distance_mfma", (0, 1), 1), ("class_set", (0, 2), 1)):
                for v in values:
                    try:
                        api.tune(key, v)
                        same_votes(rs.knn_vote(m2, class_of, k=5), want, (kind, key, v))
                    finally:
                        api.tune(key, default)
        finally:
            rs.free()


def test_device_form_on_a_stream(kpop, oracle):
    """kpop_dev_knn_vote on a stream of the caller's, twice back to back without a synchronisation between: the host form's bits, and a
    guard word behind every output and behind the workspace is what it was"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, d, r2 = 20000, 64, 9
    m1, m2, metric = operands(oracle, r1, d, r2)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    for kind, p, normalize, k in ((0, 2.0, True, 5), (2, P_MINK, False, 128), (1, 2.0, True, 1)):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            want = rs.knn_vote(m2, class_of, k=k)
            same_votes(want, knn_vote_ref(on_the_vector_pipe(rs, m2), class_of, k), ("host form", kind))
            t_m2 = torch.from_numpy(np.array(m2)).to(dev)
            t_cl = torch.from_numpy(class_of.astype(np.int32)).to(dev)
            nbytes = api.dev_knn_vote_workspace_bytes(rs, r2, k, 7)
            assert nbytes == api.dev_knn_vote_workspace_bytes(rs, r2, k, 7) and nbytes < (64 << 20)
            work = torch.full((nbytes + 8,), 0x5A, dtype=torch.uint8, device=dev)
            outs = [torch.full((r2 + 1,), -3, dtype=torch.int32, device=dev) for _ in range(3)]
            first = torch.full((r2 + 1,), -7.5, dtype=torch.float64, device=dev)
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for _ in range(2):  # (a second call on the same buffers: nothing is left over from the first)
                    api.dev_knn_vote(rs, t_cl.data_ptr(), 7, t_m2.data_ptr(), r2, k, work.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), first.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            got = tuple(o.cpu().numpy().view(np.uint32)[:r2] for o in outs) + (first.cpu().numpy()[:r2],)
            same_votes(got, want, ("device form", kind))
            assert all(int(o[r2]) == -3 for o in outs) and float(first[r2]) == -7.5
            assert torch.all(work[nbytes:] == 0x5A)
            if kind == 0:  # labels beyond n_classes: the device form trusts the array and guards its tables -- such a row counts, and votes for nobody
                with torch.cuda.stream(stream):
                    api.dev_knn_vote(rs, t_cl.data_ptr(), 5, t_m2.data_ptr(), r2, k, work.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), first.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                got = tuple(o.cpu().numpy().view(np.uint32)[:r2] for o in outs) + (first.cpu().numpy()[:r2],)
                same_votes(got, knn_vote_ref(on_the_vector_pipe(rs, m2), class_of, k, n_classes=5), "labels beyond n_classes")
                assert torch.all(work[nbytes:] == 0x5A)
        finally:
            rs.free()
