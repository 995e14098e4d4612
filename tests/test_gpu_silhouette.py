"""The silhouette and the medoids of a labelled resident set (kpop_silhouette, include/kpop_hip.h), without the
distance matrix.

The contract: over the oracle's matrix of the set against itself -- for the euclidean and cosine kinds the bits of the reference
chain -- the seven arrays of tests/silhouette_ref.py, whose sums are math.fsum's.  Where every distance and every sum is exact
(dyadic coordinates in one dimension) the comparison is bit for bit.  On random rows a sum of n = r1 terms in any order lies within
n 2^-53 relative of the exact one, a mean has one more rounding and the reference two of its own: own_mean and other_mean within
(n + 2) 2^-53 relative, the silhouette within 4 (n + 2) 2^-53 absolute; other_class and medoid are compared where the reference's two
least values lie further apart than that margin, which the inputs are drawn to give for every row (asserted).  The Minkowski kind
goes through the GPU's pow, which agrees with the oracle's to rtol 1e-11 only (tests/test_gpu_refset.py), so there the matrix is the
one the declaration names: what kpop_refset_distance_rowwise writes on the vector pipe with the set's rows as the query
(tests/test_gpu_dbscan.py and tests/test_gpu_clusters.py do the same), held to the oracle's at that rtol."""
import ctypes as C

import numpy as np
import pytest

from silhouette_ref import NO_CLASS, medoids_ref, rows_ref, same_bits, second_least_other, silhouette_ref

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
QNAN_BITS = 0x7FF8000000000000
NAMES = ("own_mean", "other_mean", "other_class", "silhouette", "class_rows", "medoid", "medoid_mean")


def line_rows(x, n_dims):
    m = np.zeros((len(x), n_dims))
    m[:, 0] = x
    return m


def dyadic(rng, n, below=8192):
    """multiples of 1/8 below 2^10"""
    return rng.randint(0, below, size=n) / 8.0


def labelling(rng, sizes, left_out=0, interleave=True):
    class_of = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.full(left_out, NO_CLASS)]).astype(np.uint32)
    return class_of[rng.permutation(len(class_of))] if interleave else class_of


def on_the_vector_pipe(rs, m2):
    from kpop_amd import api
    api.tune("distance_mfma", 0)
    try:
        return rs.distance_rowwise(m2)
    finally:
        api.tune("distance_mfma", 1)


def check_exact(got, want, what):
    assert tuple(got._fields) == NAMES
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if w.dtype == np.float64:
            assert g.dtype == np.float64 and same_bits(g, w), (what, name, g[:8], w[:8])
        else:
            assert g.dtype == np.uint32 and np.array_equal(g, w), (what, name, g[:8], w[:8])


def exact_case(kpop, oracle, x, n_dims, class_of, n_classes, what):
    m = line_rows(x, n_dims)
    metric = np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False) if len(x) else np.zeros((0, 0))
    assert np.array_equal(D, np.abs(np.subtract.outer(np.asarray(x, dtype=np.float64), x)))  # every distance is exact
    want = silhouette_ref(D, class_of, n_classes)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.silhouette(class_of, n_classes)
    finally:
        rs.free()
    check_exact(got, want, what)
    return got


# (r1, n_dims): every r1 of the list, every n_dims of the list
SIZES = [(1, 1), (2, 3), (3, 16), (63, 17), (64, 33), (65, 1), (129, 3), (300, 16), (65, 17), (65, 33), (129, 16)]


@pytest.mark.parametrize("r1,n_dims", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_exact_sizes(kpop, oracle, r1, n_dims):
    rng = np.random.RandomState(1000 * r1 + n_dims)
    x = dyadic(rng, r1)
    n_cls = min(r1, 3)
    cuts = np.sort(rng.choice(np.arange(1, r1), n_cls - 1, replace=False)) if n_cls > 1 else np.zeros(0, dtype=int)
    sizes = np.diff(np.concatenate([[0], cuts, [r1]])).astype(int)
    for interleave in (True, False):
        exact_case(kpop, oracle, x, n_dims, labelling(rng, sizes, 0, interleave), n_cls, (r1, n_dims, interleave))


@pytest.mark.parametrize("interleave", [True, False], ids=["interleaved", "sorted"])
def test_exact_class_sizes_round_a_column_tile(kpop, oracle, interleave):
    """classes of 1, 63, 64, 65 and 130 rows: a column tile of 64 positions, its edges and its cut; two empty classes between them and
    rows left out"""
    rng = np.random.RandomState(77)
    sizes = [1, 63, 0, 64, 65, 0, 130]
    class_of = labelling(rng, sizes, 9, interleave)
    got = exact_case(kpop, oracle, dyadic(rng, len(class_of)), 3, class_of, len(sizes), "tile sizes")
    assert got.class_rows.tolist() == sizes
    left = class_of == NO_CLASS
    for a in (got.own_mean, got.other_mean, got.silhouette):
        assert np.all(a[left].view(np.uint64) == QNAN_BITS)  # the declared NaN, not any NaN
    assert np.all(got.other_class[left] == NO_CLASS) and np.all(got.medoid_mean[[2, 5]].view(np.uint64) == QNAN_BITS)


def test_exact_edge_labellings(kpop, oracle):
    rng = np.random.RandomState(5)
    r1 = 70
    x = dyadic(rng, r1)
    # more classes than rows, most of them empty
    got = exact_case(kpop, oracle, x, 3, (rng.randint(0, 40, size=r1) * 5).astype(np.uint32), 200, "n_classes > r1")
    assert np.sum(got.class_rows == 0) >= 160
    # one class that has rows: no other class
    got = exact_case(kpop, oracle, x, 3, np.full(r1, 4, dtype=np.uint32), 6, "a single class")
    assert np.all(np.isnan(got.other_mean)) and np.all(got.other_class == NO_CLASS) and np.all(np.isnan(got.silhouette))
    assert got.medoid[4] < r1 and np.all(np.delete(got.medoid, 4) == NO_CLASS)
    # every row left out
    got = exact_case(kpop, oracle, x, 3, np.full(r1, NO_CLASS, dtype=np.uint32), 2, "every row left out")
    assert np.all(np.isnan(got.own_mean)) and got.class_rows.tolist() == [0, 0] and got.medoid.tolist() == [NO_CLASS] * 2
    # every row a class of its own
    got = exact_case(kpop, oracle, x, 3, rng.permutation(r1).astype(np.uint32), r1, "singletons")
    assert np.all(got.silhouette == 0.0) and not np.any(np.signbit(got.silhouette)) and np.all(got.class_rows == 1)
    # duplicates at distance 0: sixteen values for 150 rows, so that whole classes coincide (0 / 0) and means tie
    x = dyadic(rng, 150, below=16)
    got = exact_case(kpop, oracle, x, 17, labelling(rng, [40, 30, 50, 20], 10), 4, "duplicates")
    exact_case(kpop, oracle, np.full(9, 2.5), 1, np.array([0, 1, 0, 1, 2, 2, 0, 1, NO_CLASS], dtype=np.uint32), 3, "one point")


def test_designed_ties(kpop, oracle):
    # the other class: classes 1 and 2 at the same mean distance of row 0 -- class 1, although its row comes later
    got = exact_case(kpop, oracle, [5.0, 3.0, 7.0, 5.5], 3, np.array([0, 2, 1, 0], dtype=np.uint32), 3, "other-class tie")
    assert got.other_class[0] == 1 and got.other_mean[0] == 2.0
    assert got.other_class[3] == 1 and got.other_mean[3] == 1.5  # no tie: class 1 at 1.5, class 2 at 2.5
    # the medoid: rows 1 and 2 of class 0 both at (1 + 1 + 2) / 3 -- row 1; rows 5 and 6 of class 1 are one point -- row 5
    got = exact_case(kpop, oracle, [4.0, 5.0, 6.0, 7.0, 64.0, 32.0, 32.0], 1, np.array([0, 0, 0, 0, 1, 1, 1], dtype=np.uint32), 2, "medoid tie")
    assert got.medoid.tolist() == [1, 5] and got.medoid_mean.tolist() == [4 / 3, 16.0]
    assert got.own_mean[1] == got.own_mean[2] and got.own_mean[5] == got.own_mean[6]


def test_the_worked_case(kpop, oracle):
    from test_silhouette_ref import HAND_CLASS, HAND_OTHER, HAND_OWN, HAND_X
    got = exact_case(kpop, oracle, HAND_X, 3, np.array(HAND_CLASS, dtype=np.uint32), 2, "INTEGRATION.md 6k")
    for j in range(10):
        if HAND_OWN[j] is not None:
            assert got.own_mean[j] == HAND_OWN[j] and got.other_mean[j] == HAND_OTHER[j]
    assert got.silhouette[7] == 0.0 and not np.signbit(got.silhouette[7]) and got.silhouette[3] == 0.7 and got.silhouette[0] == 19 / 24
    assert got.medoid.tolist() == [1, 4] and got.class_rows.tolist() == [4, 5]
    # from kpop_dbscan's own labels
    rs = kpop.RefSet(line_rows(HAND_X, 3), np.ones(3), 0, 2.0, False)
    try:
        class_of, n_classes, label_of_class = kpop.dense_labels(rs.dbscan(0.375, 4)[0])
        assert class_of.tolist() == HAND_CLASS and label_of_class.tolist() == [0, 3]
        check_exact(rs.silhouette(class_of), got, "dense labels")
        mean, overall = kpop.silhouette_summary(class_of, got.silhouette)
        assert mean[0] == sum(got.silhouette[[0, 1, 2, 9]].tolist()) / 4 and overall == sum(np.delete(got.silhouette, 8).tolist()) / 9
    finally:
        rs.free()


RANDOM = [(7, 0), (7, 1), (7, 2), (40, 0), (40, 1), (40, 2)]


@pytest.mark.parametrize("n_dims,kind", RANDOM, ids=["%d-%s" % (d, ("euclidean", "cosine", "minkowski")[k]) for d, k in RANDOM])
def test_random_rows(kpop, oracle, n_dims, kind):
    r1 = n = 500
    p = KINDS[kind][1]
    margin = (n + 2) * 2.0 ** -53
    rng = np.random.RandomState(500 + 10 * n_dims + kind)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    for normalize in (True, False):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            D = oracle.distance_rowwise(m, m, metric, kind, p, normalize)
            if kind == 2:
                G = on_the_vector_pipe(rs, m)
                off = ~np.eye(r1, dtype=bool)
                assert np.allclose(G[off], D[off], rtol=1e-11, atol=0)
                D = G
            for n_classes in (1, 2, 37):
                class_of = rng.randint(0, n_classes, size=r1).astype(np.uint32)
                what = (n_dims, kind, normalize, n_classes)
                want = silhouette_ref(D, class_of, n_classes)
                got = rs.silhouette(class_of, n_classes)
                for name in ("own_mean", "other_mean"):
                    g, w = getattr(got, name), want[NAMES.index(name)]
                    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name)
                    ok = ~np.isnan(w)
                    err = float(np.max(np.abs(g[ok] - w[ok]) / w[ok])) if ok.any() else 0.0
                    print("    %s %s: relative error %.3g of %.3g" % (what, name, err, margin))
                    assert err <= margin, (what, name, err)
                assert np.array_equal(np.isnan(got.silhouette), np.isnan(want[3])), what
                ok = ~np.isnan(want[3])
                err = float(np.max(np.abs(got.silhouette[ok] - want[3][ok]))) if ok.any() else 0.0
                print("    %s silhouette: absolute error %.3g of %.3g" % (what, err, 4 * margin))
                assert err <= 4 * margin, (what, err)
                # the inputs give every row a clear other class, and every class a clear medoid
                if n_classes > 2:
                    two = second_least_other(D, range(r1), class_of, n_classes)
                    assert np.all(two[:, 1] - two[:, 0] > 2 * margin * two[:, 1]), what
                assert np.array_equal(got.other_class, want[2]), what
                for c in range(n_classes):
                    o = np.sort(want[0][class_of == c])
                    assert len(o) < 2 or o[1] - o[0] > 2 * margin * o[1], (what, c)
                assert np.array_equal(got.medoid, want[5]) and np.array_equal(got.class_rows, want[4]), what
                assert same_bits(got.medoid_mean, got.own_mean[got.medoid]), what  # bits kept
        finally:
            rs.free()


def device_form(kpop, rs, class_of, n_classes, guard=8):
    """kpop_dev_silhouette on a stream of the caller's with its own workspace -> (Silhouette, the guard words behind every output)"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1 = len(class_of)
    work = torch.empty(max(api.dev_silhouette_workspace_bytes(rs, n_classes), 1), dtype=torch.uint8, device=dev)
    d_cls = torch.from_numpy(class_of.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev)
    sizes = [r1, r1, r1, r1, n_classes, n_classes, n_classes]
    types = [torch.float64, torch.float64, torch.int32, torch.float64, torch.int32, torch.int32, torch.float64]
    outs = [torch.full((n + guard,), -3, dtype=t, device=dev) for n, t in zip(sizes, types)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        api.dev_silhouette(rs, d_cls.data_ptr(), n_classes, work.data_ptr(), *[t.data_ptr() for t in outs], stream=stream.cuda_stream)
    stream.synchronize()
    host = [t.cpu().numpy() for t in outs]
    host = [a.view(np.uint32) if a.dtype == np.int32 else a for a in host]
    return kpop.Silhouette(*[a[:n] for a, n in zip(host, sizes)]), [a[n:] for a, n in zip(host, sizes)]


def guards_untouched(guards):
    return all(np.all(g == (-3.0 if g.dtype == np.float64 else 0xFFFFFFFD)) for g in guards)


def test_the_three_contract_properties(kpop, oracle):
    """the same bits on every run; class numbers do not matter; the host, device and unprepared forms agree -- on rows whose sums are
    NOT exact, so that an order of additions that moved would show"""
    r1, n_dims, n_classes = 300, 17, 7
    rng = np.random.RandomState(3)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    class_of = labelling(rng, [1, 64, 65, 0, 100, 40, 20], 10)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            first = rs.silhouette(class_of, n_classes)
            check_exact(rs.silhouette(class_of, n_classes), first, "a second run")
            sums = np.array(first.own_mean[~np.isnan(first.own_mean)])
            assert np.any(sums != np.round(sums * 8) / 8)  # (not the exact kind of case)
            # renumbered by a random permutation: new class of old class c is perm[c]
            perm = rng.permutation(n_classes).astype(np.uint32)
            inv = np.argsort(perm)
            moved = rs.silhouette(np.where(class_of == NO_CLASS, NO_CLASS, perm[np.minimum(class_of, n_classes - 1)]).astype(np.uint32), n_classes)
            for name in ("own_mean", "other_mean", "silhouette"):
                assert same_bits(getattr(moved, name), getattr(first, name)), (kind, name)
            assert same_bits(moved.medoid_mean[perm], first.medoid_mean) and np.array_equal(moved.medoid[perm], first.medoid)
            assert np.array_equal(moved.class_rows[perm], first.class_rows)
            back = np.where(moved.other_class == NO_CLASS, NO_CLASS, inv[np.minimum(moved.other_class, n_classes - 1)]).astype(np.uint32)
            assert np.array_equal(back, first.other_class)
            # the three forms
            got, guards = device_form(kpop, rs, class_of, n_classes)
            check_exact(got, first, "the device form")
            assert guards_untouched(guards)
            check_exact(kpop.distance_silhouette(m, metric, class_of, kind, p, normalize, n_classes), first, "the unprepared form")
        finally:
            rs.free()


def test_a_set_after_growth(kpop, oracle):
    r1, n_dims = 300, 9
    rng = np.random.RandomState(8)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    class_of = labelling(rng, [100, 90, 80], 30)
    for normalize in (True, False):
        fresh = kpop.RefSet(m, metric, 0, 2.0, normalize)
        grown = kpop.RefSet(m[:170], metric, 0, 2.0, normalize, capacity=r1)
        try:
            want = fresh.silhouette(class_of, 3)
            kept = np.flatnonzero(class_of[:170] != NO_CLASS)
            before = grown.silhouette(class_of[:170], 3)
            grown.append(m[170:])
            got = grown.silhouette(class_of, 3)
            check_exact(got, want, "after append")
            assert not same_bits(before.own_mean[kept], got.own_mean[kept])  # a new row changes every mean
        finally:
            fresh.free()
            grown.free()


def test_a_row_holding_a_nan(kpop, oracle):
    r1, n_dims = 130, 5
    rng = np.random.RandomState(21)
    m = np.round(rng.normal(size=(r1, n_dims)), 2)
    bad = 77
    m[bad, 2] = np.nan
    metric = np.ones(n_dims)
    class_of = labelling(rng, [50, 45, 35])
    a = int(class_of[bad])
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
    assert np.all(np.isnan(np.delete(D[bad], bad))) and np.all(np.isnan(np.delete(D[:, bad], bad)))
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.silhouette(class_of, 3)
        want = silhouette_ref(D, class_of, 3)
        in_a = class_of == a
        # exactly the declared rows: the own_mean and the silhouette of the class of the row; the row's own other_mean
        assert np.array_equal(np.isnan(got.own_mean), in_a) and np.array_equal(np.isnan(got.silhouette), in_a)
        assert np.array_equal(np.isnan(got.other_mean), np.arange(r1) == bad) and got.other_class[bad] == NO_CLASS
        assert not np.any(got.other_class[~in_a] == a)  # a NaN mean is never the least
        assert got.medoid[a] == NO_CLASS and np.isnan(got.medoid_mean[a]) and np.all(np.delete(got.medoid, a) < r1)
        assert np.array_equal(got.other_class, want[2]) and np.array_equal(got.medoid, want[5])
        for name in ("own_mean", "other_mean"):
            g, w = getattr(got, name), want[NAMES.index(name)]
            ok = ~np.isnan(w)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.all(np.abs(g[ok] - w[ok]) <= (r1 + 2) * 2.0 ** -53 * w[ok])
        # the same row left out: nothing but its own outputs is a NaN
        left = np.array(class_of)
        left[bad] = NO_CLASS
        got = rs.silhouette(left, 3)
        others = np.arange(r1) != bad
        for a_ in (got.own_mean, got.other_mean, got.silhouette):
            assert not np.any(np.isnan(a_[others])) and np.isnan(a_[bad])
        assert not np.any(np.isnan(got.medoid_mean)) and got.other_class[bad] == NO_CLASS
    finally:
        rs.free()


def test_the_long_set_tile_shape(kpop, oracle):
    """65,600 rows take the tiles of a long set (32 columns x 256 rows).  No quadratic reference: 64 rows -- 59 drawn, and the five
    medoids the call names -- against their 64 rows of oracle distances; dyadic coordinates, so that sums of 65,600 terms are exact"""
    r1, n_dims, n_classes = 65600, 3, 5
    rng = np.random.RandomState(65600)
    x = dyadic(rng, r1)
    class_of = rng.choice(np.array([0, 1, 2, 3, 4, NO_CLASS], dtype=np.uint32), size=r1, p=[0.4, 0.25, 0.15, 0.1, 0.05, 0.05]).astype(np.uint32)
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.silhouette(class_of, n_classes)
    finally:
        rs.free()
    assert np.array_equal(got.class_rows, np.bincount(class_of[class_of != NO_CLASS], minlength=n_classes))
    assert np.all(got.medoid < r1) and np.array_equal(class_of[got.medoid], np.arange(n_classes))
    left = np.flatnonzero(class_of == NO_CLASS)
    sample = np.concatenate([got.medoid, left[:3], rng.choice(r1, 56, replace=False)]).astype(np.int64)
    assert len(sample) == 64
    D = oracle.distance_rowwise(m, m[sample], metric, 0, 2.0, False)
    assert D.shape == (64, r1)
    own, other, ocls, sil = rows_ref(D, sample, class_of, n_classes)
    assert same_bits(got.own_mean[sample], own) and same_bits(got.other_mean[sample], other) and same_bits(got.silhouette[sample], sil)
    assert np.array_equal(got.other_class[sample], ocls)
    assert np.all(got.own_mean[left].view(np.uint64) == QNAN_BITS) and np.all(got.other_class[left] == NO_CLASS)
    # the medoids: their means bit for bit, and no sampled member of their class lies below them
    assert same_bits(got.medoid_mean, own[:n_classes])
    for k, j in enumerate(sample):
        c = class_of[j]
        if c != NO_CLASS:
            assert (own[k], j) >= (got.medoid_mean[c], got.medoid[c]), (k, j)
    keyed = np.lexsort((np.arange(r1), np.where(np.isnan(got.own_mean), np.inf, got.own_mean)))
    for c in range(n_classes):  # (over the call's own means: the least of each class under (mean, row))
        assert keyed[class_of[keyed] == c][0] == got.medoid[c]


def raw_silhouette(rs_handle, class_of, n_classes, outs):
    from kpop_amd import _lib
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32))  # noqa: E731
    return _lib.load().kpop_silhouette(rs_handle, ptr(class_of), n_classes, *[ptr(a) for a in outs])


def test_arguments(kpop, oracle):
    from kpop_amd import api
    r1, n_dims = 70, 3
    rng = np.random.RandomState(2)
    x = dyadic(rng, r1)
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    class_of = labelling(rng, [30, 25, 10], 5)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        want = rs.silhouette(class_of, 3)
        for n_classes, code in ((0, ERR_INVALID), (65536, ERR_UNSUPPORTED)):
            with pytest.raises(kpop.KPopError) as e:
                rs.silhouette(class_of, n_classes)
            assert e.value.code == code and "kpop_silhouette" in str(e.value)
            with pytest.raises(kpop.KPopError) as e:
                kpop.distance_silhouette(m, metric, class_of, 0, 2.0, False, n_classes)
            assert e.value.code == code
            assert api.dev_silhouette_workspace_bytes(rs, n_classes) == 0
            with pytest.raises(kpop.KPopError) as e:
                api.dev_silhouette(rs, None, n_classes, None)
            assert e.value.code == code and "kpop_dev_silhouette" in str(e.value)
        assert 0 < api.dev_silhouette_workspace_bytes(rs, 3) < api.dev_silhouette_workspace_bytes(rs, 65535) < 1 << 23  # O(r1 + n_classes)
        check_exact(rs.silhouette(class_of, 65535), kpop.Silhouette(*want[:4], *[np.concatenate([a, np.full(65532, f, dtype=a.dtype)])
                                                                                 for a, f in zip(want[4:], (0, NO_CLASS, np.nan))]), "65,535 classes")
        # a class out of range that is not NO_CLASS
        with pytest.raises(kpop.KPopError) as e:
            rs.silhouette(class_of, 2)
        assert e.value.code == ERR_INVALID and "class 2 of 2" in str(e.value)
        wrong = np.array(class_of)
        wrong[11] = NO_CLASS - 1
        with pytest.raises(kpop.KPopError) as e:
            rs.silhouette(wrong, 3)
        assert e.value.code == ERR_INVALID
        with pytest.raises(kpop.KPopError):  # the device form needs its workspace
            api.dev_silhouette(rs, None, 3, None)
        # in the device form the table is trusted and guarded: such a row counts as left out
        got, guards = device_form(kpop, rs, wrong, 3)
        left = np.array(class_of)
        left[11] = NO_CLASS
        check_exact(got, rs.silhouette(left, 3), "a class beyond n_classes on the device")
        assert guards_untouched(guards)
        # every output pointer may be NULL; any one alone is what it is with the others
        assert raw_silhouette(rs.handle, class_of, 3, [None] * 7) == 0
        for k in range(7):
            outs = [None] * 7
            outs[k] = np.zeros_like(want[k])
            assert raw_silhouette(rs.handle, class_of, 3, outs) == 0
            check = same_bits if want[k].dtype == np.float64 else np.array_equal
            assert check(outs[k], want[k]), NAMES[k]
        assert raw_silhouette(rs.handle, None, 3, [None] * 7) == ERR_INVALID
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.silhouette(class_of, 3)
    assert e.value.code == ERR_INVALID
    # an empty set: KPOP_OK, the classes all empty -- the error of a bad argument still comes first
    empty = kpop.RefSet(np.zeros((0, n_dims)), metric, 0, 2.0, False)
    try:
        got = empty.silhouette(np.zeros(0, dtype=np.uint32), 4)
        assert all(len(a) == 0 for a in got[:4]) and got.class_rows.tolist() == [0] * 4 and got.medoid.tolist() == [NO_CLASS] * 4
        assert np.all(np.isnan(got.medoid_mean))
        with pytest.raises(kpop.KPopError):
            empty.silhouette(np.zeros(0, dtype=np.uint32), 0)
        assert raw_silhouette(empty.handle, None, 4, [None] * 7) == 0
    finally:
        empty.free()
