"""k-NN validation on a labelled resident set (kpop_knn_validate, kpop_knn_ks_vote, include/kpop_hip.h).

The contract: the outputs are knn_validate_ref (tests/knn_validate_ref.py) -- knn_vote_ref over the matrix RefSet.distance_rowwise writes
on the vector pipe (kpop_tune("distance_mfma", 0)) with the set's rows as the query, the entries that are left out set to NaN -- bit for
bit and under any tune setting; for the euclidean and cosine kinds that matrix is the oracle's, bit for bit, so the expected arrays are
the oracle's too.  No row is left out of a comparison.  Every slice of the many-k vote is the k-NN vote at that k, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from knn_validate_ref import knn_validate_ref, leave_out, same_validation
from knn_vote_ref import NO_CLASS, knn_lists, knn_vote_ref, same_votes
from test_gpu_knn_vote import SHAPES as VOTE_SHAPES
from test_gpu_within import P_MINK, on_the_vector_pipe, operands

pytestmark = pytest.mark.gpu

KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
# r1 x dims: three column tiles, ragged; 1,000; several segments a strip; dims no multiple of 16
SHAPES = [(130, 9), (1000, 16), (3000, 16), (300, 200)]
# (the last four change the strip's height: 64, 32 and 16 rows)
LADDERS = [(1,), (1, 2, 5), (3, 32), (5, 33, 64), (1, 128)]
GROUPS = ["none", "folds", "triples"]


def labellings(r1):
    return [("mod7", (np.arange(r1) % 7).astype(np.uint32)), ("own", np.arange(r1, dtype=np.uint32))]


def groups(name, r1):
    return {"none": None, "folds": (np.arange(r1) % 10).astype(np.uint32), "triples": (np.arange(r1) // 3).astype(np.uint32)}[name]


def lists_of(E, ks):
    """knn_lists(E, k) for every k of ks from one sort of the rows -> {k: lists}: the order does not depend on k (a stable sort by the
    distance with -0 as +0 keeps the columns ascending among equals and puts the NaNs last)"""
    key = E + 0.0
    order = np.argsort(key, axis=1, kind="stable")
    srt = np.take_along_axis(key, order, axis=1)
    cnt = (~np.isnan(E)).sum(axis=1)
    out = {}
    for k in ks:
        lists = []
        for j in range(E.shape[0]):
            c = int(cnt[j])
            n = min(int(k), c)
            if 0 < n < c:
                n = int(np.searchsorted(srt[j, :c], srt[j, n - 1], side="right"))
            lists.append(order[j, :n])
        out[k] = lists
    return out


def expected(G, rows, class_of, ks, group_of=None, n_classes=None, lists=None):
    """knn_validate_ref for the rows `rows` of the set, of whose distances G holds the lines -> (cls, votes, n, first, correct), correct
    counted over these rows"""
    rows = np.asarray(rows)
    E = np.array(G)
    if group_of is None:
        E[np.arange(len(rows)), rows] = np.nan
    else:
        E[group_of[rows][:, None] == group_of[None, :]] = np.nan
    if lists is None:
        lists = lists_of(E, ks)
    outs = [knn_vote_ref(E, class_of, k, n_classes, lists=lists[k]) for k in ks]
    cls, votes, n, first = (np.stack([o[q] for o in outs]) for q in range(4))
    correct = np.array([np.count_nonzero((c != NO_CLASS) & (c == class_of[rows])) for c in cls], dtype=np.uint64)
    return cls, votes, n, first, correct


def test_the_fast_lists_are_the_reference_lists(oracle):
    """lists_of against knn_lists of tests/knn_vote_ref.py, and expected() against knn_validate_ref, on a matrix with ties, -0 and NaNs"""
    m1, _, metric = operands(oracle, 130, 9, 37)
    D = np.array(oracle.distance_rowwise(m1, m1, metric, 0, 2.0, True))
    D[5, 9] = -0.0
    D[17] = np.nan
    D[:, 17] = np.nan
    for name in GROUPS:
        g = groups(name, 130)
        E = leave_out(D, g)
        ks = (1, 2, 5, 33, 128)
        fast = lists_of(E, ks)
        for k in ks:
            assert all(np.array_equal(a, b) for a, b in zip(fast[k], knn_lists(E, k))), (name, k)
        for _, class_of in labellings(130):
            same_validation(expected(D, np.arange(130), class_of, ks, g), knn_validate_ref(D, class_of, ks, g), name)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_validate_vs_rowwise_and_oracle(kpop, oracle, r1, d, kind, p, normalize, group):
    m1, _, metric = operands(oracle, r1, d, 40)
    g = groups(group, r1)
    rs = kpop.RefSet(m1, metric, kind, p, normalize)
    try:
        G = on_the_vector_pipe(rs, m1)
        if kind != 2:  # the oracle's matrix is this one, bit for bit: what follows is the oracle's answer too
            assert np.array_equal(G.view(np.uint64), oracle.distance_rowwise(m1, m1, metric, kind, p, normalize).view(np.uint64))
        E = leave_out(G, g)
        lists = lists_of(E, sorted({k for ks in LADDERS for k in ks}))
        for ks in LADDERS:
            for name, class_of in labellings(r1):
                what = (r1, d, kind, normalize, group, ks, name)
                got = rs.knn_validate(class_of, ks=ks, group_of=g)
                assert [a.dtype for a in got] == [np.uint32, np.uint32, np.uint32, np.float64, np.uint64]
                assert all(a.shape == (len(ks), r1) for a in got[:4]) and got[4].shape == (len(ks),)
                want = expected(G, np.arange(r1), class_of, ks, g, lists=lists)
                same_validation(got, want, what)
                n_classes = int(class_of.max()) + 1
                for t in range(len(ks)):  # the accuracy's bookkeeping
                    assert int(kpop.confusion_matrix(class_of, got[0][t], n_classes).trace()) == int(got[4][t]), what
        # rows 3 and 7 of the set are the same row: each lists the other at distance 0, and not itself -- the duplicate stays, the row
        # itself does not
        cls, votes, n, first, _ = rs.knn_validate(np.arange(r1), ks=(1,))
        assert (int(cls[0][3]), int(votes[0][3]), int(n[0][3]), float(first[0][3])) == (7, 1, 1, 0.0), (r1, d, kind, normalize)
        assert (int(cls[0][7]), int(votes[0][7]), int(n[0][7]), float(first[0][7])) == (3, 1, 1, 0.0), (r1, d, kind, normalize)
    finally:
        rs.free()


@pytest.mark.parametrize("kind,p", KINDS, ids=["euclidean", "cosine", "minkowski"])
@pytest.mark.parametrize("r1,d,r2", VOTE_SHAPES[:4], ids=["%dx%dx%d" % s for s in VOTE_SHAPES[:4]])
def test_every_slice_of_the_many_k_vote_is_the_vote(kpop, oracle, r1, d, r2, kind, p):
    """the second witness of the many-k kernel: knn_vote_ks slice by slice against knn_vote called once a k, bit for bit"""
    m1, m2, metric = operands(oracle, r1, d, r2)
    for normalize in (True, False):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            for name, class_of in labellings(r1):
                one = {k: rs.knn_vote(m2, class_of, k=k) for k in sorted({k for ks in LADDERS for k in ks})}
                for ks in LADDERS:
                    got = rs.knn_vote_ks(m2, class_of, ks)
                    assert all(a.shape == (len(ks), r2) for a in got)
                    for t, k in enumerate(ks):
                        same_votes(tuple(a[t] for a in got), one[k], (r1, d, r2, kind, normalize, name, ks, k))
        finally:
            rs.free()


def test_tie_groups_inside_the_merged_list(kpop, oracle):
    """a set built of groups of 1, 2, .. 6 identical rows, scattered over the column tiles, and ks = (1, 2, 3, 5, 8): a row's cuts fall
    inside, at the end of and behind tie groups at distance 0 and further out, the cut keys lie below the K-th key and the group inside the
    merged list"""
    rng = np.random.RandomState(5)
    sizes = np.tile(np.arange(1, 7), 12)
    of_group = np.repeat(np.arange(len(sizes)), sizes)
    r1, d = len(of_group), 9
    base = np.round(rng.normal(size=(len(sizes), d)), 1)
    where = rng.permutation(r1)
    m1 = np.zeros((r1, d))
    m1[where] = base[of_group]
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    ks = (1, 2, 3, 5, 8)
    copy_of = np.zeros(r1, dtype=np.int64)
    copy_of[where] = of_group  # the rows of a tie group share a class: a group votes as one
    by_copies = ("copies", (copy_of % 5).astype(np.uint32))
    for kind, p in KINDS:
        for normalize in (True, False):
            rs = kpop.RefSet(m1, metric, kind, p, normalize)
            try:
                G = on_the_vector_pipe(rs, m1)
                assert np.count_nonzero(G == 0.0) >= int((sizes * sizes).sum())
                for gname in GROUPS:
                    g = groups(gname, r1)
                    for name, class_of in labellings(r1) + [by_copies]:
                        same_validation(rs.knn_validate(class_of, ks=ks, group_of=g), knn_validate_ref(G, class_of, ks, g), (kind, normalize, gname, name))
                # the many-k vote over the same set, its rows as queries (the row itself counts there)
                class_of = (np.arange(r1) % 7).astype(np.uint32)
                got = rs.knn_vote_ks(m1[:50], class_of, ks)
                for t, k in enumerate(ks):
                    same_votes(tuple(a[t] for a in got), knn_vote_ref(G[:50], class_of, k), (kind, normalize, "vote_ks", k))
            finally:
                rs.free()


@pytest.mark.parametrize("n_copies", [3000, 600])
def test_a_tie_group_far_longer_than_k(kpop, oracle, n_copies):
    """the 3,000 (600) copies of one row among 5,000 of tests/test_gpu_knn_vote.py, ks = (5, 128): a copy row lists the other n_copies - 1
    copies at every k, and nothing else.  Over all 5,000 rows the columns are cut into two segments, whose 2 x 128 slots drop ties either
    way: the tables.  Over the first 30 rows alone (the device form) they are cut into 79, no segment drops a tie, and the group comes from
    the segments' lists at 600 (fewer than the 1,024 the vote takes from lists) and from the tables at 3,000: both ways to the same
    answer.  Every copy row's numbers are checked; 60 rows, copies and others, against the reference bit for bit"""
    import torch
    from kpop_amd import api
    r1, d = 5000, 16
    rng = np.random.RandomState(77)
    m1 = rng.normal(size=(r1, d))
    copies = np.nonzero((np.arange(r1) * 3) % 25 < n_copies // 200)[0]
    assert len(copies) == n_copies and copies[0] == 0
    m1[copies] = m1[0]
    class_of = (2 + np.arange(r1) % 5).astype(np.uint32)
    class_of[copies] = 1 - np.arange(n_copies) % 2
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    rows = np.r_[0:30, 2485:2500, 4985:5000]
    ks = (5, 128)
    for kind, p, normalize in ((0, 2.0, True), (2, P_MINK, False), (1, 2.0, True)):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m1[rows])
            assert np.all(G[0, copies] == 0.0) and np.count_nonzero(G[0] == 0.0) == n_copies
            for g in (None, (np.arange(r1) % 10).astype(np.uint32)):
                cls, votes, n, first, correct = got = rs.knn_validate(class_of, ks=ks, group_of=g)
                want = expected(G, rows, class_of, ks, g)
                for t in range(len(ks)):
                    same_votes(tuple(a[t][rows] for a in got[:4]), tuple(a[t] for a in want[:4]), (kind, normalize, g is None, ks[t]))
                    assert int(correct[t]) == np.count_nonzero(cls[t] == class_of)
                dev = torch.device("cuda:0")
                few = dev_validate(api, torch, rs, torch.from_numpy(class_of.astype(np.int32)).to(dev), 7,
                                   None if g is None else torch.from_numpy(g.astype(np.int32)).to(dev), 0, 30, ks, torch.cuda.Stream(device=dev))
                same_validation(few, tuple(a[:, :30] for a in got[:4]) + (np.array([np.count_nonzero(c[:30] == class_of[:30]) for c in cls], dtype=np.uint64),),
                                (kind, normalize, g is None, "the first 30 rows"))
                if g is None:
                    # a copy: the other copies, half of them of each class; class 1 holds copy 0 -- or, for copy 0 itself, one member fewer
                    assert np.all(n[:, copies] == n_copies - 1) and np.all(first[:, copies] == 0.0)
                    assert np.all(votes[:, copies[1:]] == n_copies // 2) and np.all(cls[:, copies[1::2]] == 1)
                    assert np.all(votes[:, 0] == n_copies // 2) and np.all(cls[:, 0] == 0)
        finally:
            rs.free()


def test_nan_and_infinity(kpop, oracle):
    """a row holding a NaN has no list and is in nobody's; a row at +inf (normalize = False) is listed, last"""
    m1, _, metric = operands(oracle, 130, 9, 37)
    r1 = 100
    m1 = np.array(m1[:r1])
    m1[20, 2] = np.nan
    m1[40] = 1e200
    for normalize in (True, False):
        rs = kpop.RefSet(m1, metric, 0, 2.0, normalize)
        try:
            G = on_the_vector_pipe(rs, m1)
            assert np.isnan(G[:, 20]).all() and np.isnan(G[20]).all()
            if not normalize:
                assert np.isposinf(np.delete(G[:, 40], [20, 40])).all()
            for gname in ("none", "folds"):
                g = groups(gname, r1)
                for name, class_of in labellings(r1):
                    ks = (1, 5, 128)
                    got = rs.knn_validate(class_of, ks=ks, group_of=g)
                    same_validation(got, knn_validate_ref(G, class_of, ks, g), (normalize, gname, name))
                    assert np.all(got[0][:, 20] == NO_CLASS) and not got[1][:, 20].any() and not got[2][:, 20].any() and np.isnan(got[3][:, 20]).all()
            n = rs.knn_validate(np.arange(r1), ks=(128,))[2][0]
            assert n[20] == 0 and np.all(np.delete(n, 20) == r1 - 2)  # everybody but the row itself and the NaN row
        finally:
            rs.free()


def raw_validate(rs, class_of, n_classes, group_of, ks, r1, n_ks=None):
    """kpop_knn_validate on the caller's arrays, a guard word behind each -> (status, cls, votes, n, first, correct)"""
    from kpop_amd import _lib
    u32 = C.POINTER(C.c_uint32)
    class_of = np.ascontiguousarray(class_of, dtype=np.uint32)
    ks = np.ascontiguousarray(ks, dtype=np.uint32)
    n_ks = len(ks) if n_ks is None else n_ks
    room = max(n_ks, 1) * r1 + 1
    cls, votes, n = (np.full(room, 12345, dtype=np.uint32) for _ in range(3))
    first = np.full(room, -7.5)
    correct = np.full(max(n_ks, 1) + 1, 99, dtype=np.uint64)
    g = None if group_of is None else np.ascontiguousarray(group_of, dtype=np.uint32)
    rc = _lib.load().kpop_knn_validate(rs.handle, class_of.ctypes.data_as(u32) if class_of.size else None, n_classes, None if g is None else g.ctypes.data_as(u32),
                                       ks.ctypes.data_as(u32) if ks.size else None, n_ks, cls.ctypes.data_as(u32), votes.ctypes.data_as(u32), n.ctypes.data_as(u32),
                                       first.ctypes.data_as(C.POINTER(C.c_double)), correct.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, cls, votes, n, first, correct


def test_contract_edges(kpop, oracle):
    r1, d = 130, 9
    m1, m2, metric = operands(oracle, r1, d, 37)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    rs = kpop.RefSet(m1, metric, 0, 2.0, True)
    try:
        G = on_the_vector_pipe(rs, m1)
        ks = (1, 2, 5)
        want = knn_validate_ref(G, class_of, ks)
        rc, cls, votes, n, first, correct = raw_validate(rs, class_of, 7, None, ks, r1)
        assert rc == 0
        same_validation((cls[:-1].reshape(3, r1), votes[:-1].reshape(3, r1), n[:-1].reshape(3, r1), first[:-1].reshape(3, r1), correct[:3]), want, "raw")
        assert (cls[-1], votes[-1], n[-1], first[-1], correct[3]) == (12345, 12345, 12345, -7.5, 99)  # nothing behind the last slice
        # the ladder: empty, a zero, not strictly ascending; beyond 128, more than 32 of them
        for bad, code in (((), ERR_INVALID), ((0,), ERR_INVALID), ((0, 3), ERR_INVALID), ((2, 2), ERR_INVALID), ((3, 1), ERR_INVALID), ((1, 5, 4), ERR_INVALID),
                          ((129,), ERR_UNSUPPORTED), ((5, 129), ERR_UNSUPPORTED), (tuple(range(1, 34)), ERR_UNSUPPORTED)):
            assert raw_validate(rs, class_of, 7, None, bad, r1)[0] == code, bad
            with pytest.raises(kpop.KPopError) as e:
                rs.knn_validate(class_of, ks=bad)
            assert e.value.code == code, bad
            with pytest.raises(kpop.KPopError) as e:
                rs.knn_vote_ks(m2, class_of, bad)
            assert e.value.code == code, bad
        assert raw_validate(rs, class_of, 7, None, (1, 2), r1, n_ks=0)[0] == ERR_INVALID
        # the classes
        assert raw_validate(rs, class_of, 0, None, ks, r1)[0] == ERR_INVALID
        assert raw_validate(rs, class_of, 6, None, ks, r1)[0] == ERR_INVALID  # a label of 6
        assert raw_validate(rs, class_of, 65536, None, ks, r1)[0] == ERR_UNSUPPORTED
        with pytest.raises(kpop.KPopError) as e:
            rs.knn_vote_ks(m2, class_of, ks, n_classes=6)
        assert e.value.code == ERR_INVALID
        rc, cls, votes, n, first, correct = raw_validate(rs, class_of, 65535, None, ks, r1)
        assert rc == 0
        same_validation((cls[:-1].reshape(3, r1), votes[:-1].reshape(3, r1), n[:-1].reshape(3, r1), first[:-1].reshape(3, r1), correct[:3]), want, "65,535 classes")
        # 32 values of k
        ks32 = tuple(range(1, 33))
        same_validation(rs.knn_validate(class_of, ks=ks32), knn_validate_ref(G, class_of, ks32), "32 values")
        got = rs.knn_vote_ks(m2, class_of, ks32)
        for t, k in enumerate(ks32):
            same_votes(tuple(a[t] for a in got), rs.knn_vote(m2, class_of, k=k), ("32 values", k))
        # no query rows
        assert all(a.shape == (3, 0) for a in rs.knn_vote_ks(np.zeros((0, d)), class_of, ks))
        # the unprepared call
        same_validation(kpop.distance_knn_validate(m1, class_of, metric, ks=ks), want, "distance_knn_validate")
        folds = groups("folds", r1)
        same_validation(kpop.distance_knn_validate(m1, class_of, metric, ks=ks, group_of=folds), knn_validate_ref(G, class_of, ks, folds), "... with groups")
        # the whole set in one group: nobody has a list
        cls, votes, n, first, correct = rs.knn_validate(class_of, ks=ks, group_of=np.zeros(r1))
        assert np.all(cls == NO_CLASS) and not votes.any() and not n.any() and np.isnan(first).all() and not correct.any()
    finally:
        rs.free()
    # a set of one row, and an empty set
    one = kpop.RefSet(m1[:1], metric, 0, 2.0, True)
    try:
        cls, votes, n, first, correct = one.knn_validate([0], ks=(1, 4))
        assert np.all(cls == NO_CLASS) and not votes.any() and not n.any() and np.isnan(first).all() and correct.tolist() == [0, 0]
    finally:
        one.free()
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        got = empty.knn_validate(np.zeros(0, dtype=np.uint32), ks=(1, 4))
        assert all(a.shape == (2, 0) for a in got[:4]) and got[4].tolist() == [0, 0]
        cls, votes, n, first = empty.knn_vote_ks(m2, np.zeros(0, dtype=np.uint32), (1, 4))
        assert np.all(cls == NO_CLASS) and not votes.any() and not n.any() and np.isnan(first).all()
    finally:
        empty.free()


def test_the_same_bits_on_every_run_and_under_every_tune_setting(kpop, oracle):
    from kpop_amd import api
    r1, d = 3000, 16
    m1, m2, metric = operands(oracle, r1, d, 40)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    folds = groups("folds", r1)
    ks = (1, 5, 33)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            want = rs.knn_validate(class_of, ks=ks, group_of=folds)
            same_validation(want, expected(on_the_vector_pipe(rs, m1), np.arange(r1), class_of, ks, folds), (kind, "reference"))
            want_v = rs.knn_vote_ks(m2, class_of, ks)
            same_validation(rs.knn_validate(class_of, ks=ks, group_of=folds), want, (kind, "again"))
            for key, values, default in (("distance_mfma", (0, 1), 1), ("class_set", (0, 2), 1)):
                for v in values:
                    try:
                        api.tune(key, v)
                        same_validation(rs.knn_validate(class_of, ks=ks, group_of=folds), want, (kind, key, v))
                        for t in range(len(ks)):
                            same_votes(tuple(a[t] for a in rs.knn_vote_ks(m2, class_of, ks)), tuple(a[t] for a in want_v), (kind, key, v, "vote_ks"))
                    finally:
                        api.tune(key, default)
        finally:
            rs.free()


def dev_validate(api, torch, rs, t_cl, n_classes, t_g, first_row, n_rows, ks, stream, calls=1):
    """kpop_dev_knn_validate on a stream with guard words behind every output and the workspace -> (cls, votes, n, first, correct)"""
    dev = t_cl.device
    n_ks = len(ks)
    nbytes = api.dev_knn_validate_workspace_bytes(rs, n_rows, max(ks), n_classes)
    work = torch.full((nbytes + 8,), 0x5A, dtype=torch.uint8, device=dev)
    outs = [torch.full((n_ks * n_rows + 1,), -3, dtype=torch.int32, device=dev) for _ in range(3)]
    first = torch.full((n_ks * n_rows + 1,), -7.5, dtype=torch.float64, device=dev)
    correct = torch.full((n_ks + 1,), 77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(calls):  # (a second call on the same buffers: nothing is left over, the counts are written, not added to)
            api.dev_knn_validate(rs, t_cl.data_ptr(), n_classes, None if t_g is None else t_g.data_ptr(), first_row, n_rows, ks, work.data_ptr(),
                                 outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), first.data_ptr(), correct.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert all(int(o[-1]) == -3 for o in outs) and float(first[-1]) == -7.5 and int(correct[-1]) == 77
    assert torch.all(work[nbytes:] == 0x5A)
    got = tuple(o.cpu().numpy().view(np.uint32)[:-1].reshape(n_ks, n_rows) for o in outs)
    return got + (first.cpu().numpy()[:-1].reshape(n_ks, n_rows), correct.cpu().numpy().view(np.uint64)[:n_ks])


def test_device_form_on_a_stream(kpop, oracle):
    """kpop_dev_knn_validate over row ranges, on a stream of the caller's, twice back to back: each range is the slice of the whole, its
    counts are the range's own, and a guard word behind every output and behind the workspace is what it was"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, d = 1000, 16
    m1, _, metric = operands(oracle, r1, d, 40)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    t_cl = torch.from_numpy(class_of.astype(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    for kind, p, normalize, ks, gname in ((0, 2.0, True, (1, 2, 5), "none"), (2, P_MINK, False, (5, 33, 64), "folds"), (1, 2.0, True, (1, 128), "triples")):
        g = groups(gname, r1)
        t_g = None if g is None else torch.from_numpy(g.astype(np.int32)).to(dev)
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            whole = rs.knn_validate(class_of, ks=ks, group_of=g)
            same_validation(whole, expected(on_the_vector_pipe(rs, m1), np.arange(r1), class_of, ks, g), ("host form", kind))
            assert api.dev_knn_validate_workspace_bytes(rs, r1, max(ks), 7) < (64 << 20)
            for first_row, n_rows in ((0, r1), (37, 130), (r1 - 1, 1)):
                got = dev_validate(api, torch, rs, t_cl, 7, t_g, first_row, n_rows, ks, stream, calls=2)
                sl = slice(first_row, first_row + n_rows)
                want = tuple(a[:, sl] for a in whole[:4]) + (np.array([np.count_nonzero(c[sl] == class_of[sl]) for c in whole[0]], dtype=np.uint64),)
                same_validation(got, want, ("device form", kind, first_row, n_rows))
            if kind == 0:
                # labels beyond n_classes: the device form trusts the array and guards its tables -- such a row counts, and votes for nobody
                got = dev_validate(api, torch, rs, t_cl, 5, t_g, 0, r1, ks, stream)
                same_validation(got, expected(on_the_vector_pipe(rs, m1), np.arange(r1), class_of, ks, g, n_classes=5), "labels beyond n_classes")
                # a range beyond the set, and no rows at all
                with pytest.raises(kpop.KPopError) as e:
                    dev_validate(api, torch, rs, t_cl, 7, t_g, r1 - 3, 4, ks, stream)
                assert e.value.code == ERR_INVALID
                correct = torch.full((4,), 77, dtype=torch.int64, device=dev)
                api.dev_knn_validate(rs, t_cl.data_ptr(), 7, None, 5, 0, ks, None, None, None, None, None, correct.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                assert correct.cpu().tolist() == [0, 0, 0, 77]
        finally:
            rs.free()


def test_the_many_k_vote_on_a_stream(kpop, oracle):
    """kpop_dev_knn_ks_vote: the host form's bits, guard words behind the outputs and the workspace"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, d, r2 = 5000, 16, 12
    m1, m2, metric = operands(oracle, r1, d, r2)
    class_of = (np.arange(r1) % 7).astype(np.uint32)
    t_cl = torch.from_numpy(class_of.astype(np.int32)).to(dev)
    t_m2 = torch.from_numpy(np.array(m2)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    for kind, p, normalize, ks in ((0, 2.0, True, (1, 2, 5)), (2, P_MINK, False, (3, 128))):
        rs = kpop.RefSet(m1, metric, kind, p, normalize)
        try:
            want = rs.knn_vote_ks(m2, class_of, ks)
            n_ks = len(ks)
            nbytes = api.dev_knn_vote_ks_workspace_bytes(rs, r2, max(ks), 7)
            assert nbytes == api.dev_knn_vote_workspace_bytes(rs, r2, max(ks), 7)
            work = torch.full((nbytes + 8,), 0x5A, dtype=torch.uint8, device=dev)
            outs = [torch.full((n_ks * r2 + 1,), -3, dtype=torch.int32, device=dev) for _ in range(3)]
            first = torch.full((n_ks * r2 + 1,), -7.5, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_knn_vote_ks(rs, t_cl.data_ptr(), 7, t_m2.data_ptr(), r2, ks, work.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                        outs[2].data_ptr(), first.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            got = tuple(o.cpu().numpy().view(np.uint32)[:-1].reshape(n_ks, r2) for o in outs) + (first.cpu().numpy()[:-1].reshape(n_ks, r2),)
            for t in range(n_ks):
                same_votes(tuple(a[t] for a in got), tuple(a[t] for a in want), (kind, ks[t]))
            assert all(int(o[-1]) == -3 for o in outs) and float(first[-1]) == -7.5 and torch.all(work[nbytes:] == 0x5A)
        finally:
            rs.free()


def test_host_form_over_more_than_one_range(kpop, oracle):
    """1,500 rows and 60,000 classes: the tie tables, 8 x 60,000 bytes a row, bound the range.  By the rule in knn_validate.hip
    (knn_rows_a_call: a quarter of a GiB over the bytes a row takes -- 482,256 of workspace at K = 5 with the 32 segments of 1,024 rows,
    60 of outputs for three k and 32 more) a range is 556 rows: the host form walks three ranges, 556 + 556 + 388, and sums their counts.
    It equals the device form over all 1,500 rows at once, and the reference"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1, d, n_classes = 1500, 16, 60000
    assert (256 << 20) // (482256 + 60 + 32) == 556
    rng = np.random.RandomState(r1)
    m1 = np.round(rng.normal(size=(r1, d)), 1)
    m1[700:720] = m1[3]  # a tie group across the first two ranges
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    class_of = ((np.arange(r1) * 7) % 11 + 59000).astype(np.uint32)
    ks = (1, 2, 5)
    t_cl = torch.from_numpy(class_of.astype(np.int32)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    rs = kpop.RefSet(m1, metric, 0, 2.0, True)
    try:
        G = on_the_vector_pipe(rs, m1)
        for gname in ("none", "folds"):
            g = groups(gname, r1)
            t_g = None if g is None else torch.from_numpy(g.astype(np.int32)).to(dev)
            got = rs.knn_validate(class_of, ks=ks, group_of=g, n_classes=n_classes)
            same_validation(got, dev_validate(api, torch, rs, t_cl, n_classes, t_g, 0, r1, ks, stream), ("one range", gname))
            same_validation(got, knn_validate_ref(G, class_of, ks, g), ("reference", gname))
    finally:
        rs.free()
