"""The distances between every two classes of a labelled resident set (kpop_class_linkage, include/kpop_hip.h),
without the distance matrix, and the classes' tree on top of them.

The contract: over the oracle's matrix of the set against itself -- for the euclidean and cosine kinds the bits of the reference chain
-- the six arrays of tests/class_linkage_ref.py, whose sums are math.fsum's.  Where every distance and every sum is exact (dyadic
coordinates in one dimension: multiples of 1/8 below 2^10, exact up to 2^40 terms) the comparison is bit for bit, the declared NaN by
its bits.  On random rows min_dist, max_dist, min_i and min_j are exact all the same -- they are distances of the matrix, not sums --
and a mean over N = n_a n_b pairs (n_a^2 on the diagonal, where every pair is added twice) lies within (N + 2) 2^-53 relative of
fsum's: a sum of N non-negative terms in any order is within N 2^-53 relative of the exact one (tests/test_gpu_silhouette.py), the
mean has one more rounding and the reference two of its own.  The Minkowski kind goes through the GPU's pow, which agrees with the
oracle's to rtol 1e-11 only, so there the matrix is the one the declaration names: what kpop_refset_distance_rowwise writes on the
vector pipe with the set's rows as the query, held to the oracle's at that rtol (as tests/test_gpu_silhouette.py does)."""
import ctypes as C
import math

import numpy as np
import pytest

from class_linkage_ref import LINK_AVERAGE, NAMES, NO_CLASS, QNAN_BITS, class_linkage_ref, line_linkage_ref, same_bits
from test_gpu_silhouette import KINDS, SIZES, dyadic, labelling, line_rows, on_the_vector_pipe

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
F64_TABLES = ("mean_dist", "min_dist", "max_dist")


def check_exact(got, want, what, declared_nan=True):
    """all six arrays, bit for bit; declared_nan: every NaN of the reference is the declared one (no distance is a NaN)"""
    assert tuple(got._fields) == NAMES
    for name, g, w in zip(NAMES, got, want):
        w = np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if w.dtype == np.float64:
            assert g.dtype == np.float64 and same_bits(g, w), (what, name, g.ravel()[:8], w.ravel()[:8])
            if declared_nan:
                assert np.all(g[np.isnan(w)].view(np.uint64) == QNAN_BITS), (what, name)
        else:
            assert g.dtype == np.uint32 and np.array_equal(g, w), (what, name, g.ravel()[:8], w.ravel()[:8])


def check_symmetric(got, what):
    for name in NAMES[1:]:
        t = getattr(got, name)
        assert np.array_equal(t.view(np.uint64 if t.dtype == np.float64 else np.uint32), t.T.copy().view(np.uint64 if t.dtype == np.float64 else np.uint32)), (what, name)


def exact_case(kpop, oracle, x, n_dims, class_of, n_classes, what):
    m = line_rows(x, n_dims)
    metric = np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False) if len(x) else np.zeros((0, 0))
    assert np.array_equal(D, np.abs(np.subtract.outer(np.asarray(x, dtype=np.float64), x)))  # every distance is exact
    want = class_linkage_ref(D, class_of, n_classes)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.class_linkage(class_of, n_classes)
    finally:
        rs.free()
    check_exact(got, want, what)
    check_symmetric(got, what)
    return got


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
    """classes of 1, 63, 64, 65 and 130 rows: a column tile of 64 positions, its edges and its cut, and strips of 64 positions that span
    several classes; two empty classes between them and rows left out"""
    rng = np.random.RandomState(77)
    sizes = [1, 63, 0, 64, 65, 0, 130]
    class_of = labelling(rng, sizes, 9, interleave)
    got = exact_case(kpop, oracle, dyadic(rng, len(class_of)), 3, class_of, len(sizes), "tile sizes")
    assert got.class_rows.tolist() == sizes
    for name in F64_TABLES:
        t = getattr(got, name)
        assert np.all(t[[2, 5]].view(np.uint64) == QNAN_BITS) and np.all(t[:, [2, 5]].view(np.uint64) == QNAN_BITS) and t.view(np.uint64)[0, 0] == QNAN_BITS
    assert np.all(got.min_i[[2, 5]] == NO_CLASS) and np.all(got.min_j[:, [2, 5]] == NO_CLASS) and got.min_i[0, 0] == got.min_j[0, 0] == NO_CLASS
    assert not np.any(np.isin(np.flatnonzero(class_of == NO_CLASS), np.concatenate([got.min_i.ravel(), got.min_j.ravel()])))  # no row left out is named


def test_exact_edge_labellings(kpop, oracle):
    rng = np.random.RandomState(5)
    r1 = 70
    x = dyadic(rng, r1)
    # more classes than rows, most of them empty
    got = exact_case(kpop, oracle, x, 3, (rng.randint(0, 40, size=r1) * 5).astype(np.uint32), 200, "n_classes > r1")
    assert np.sum(got.class_rows == 0) >= 160
    # one class that has rows: its diagonal entry alone
    got = exact_case(kpop, oracle, x, 3, np.full(r1, 4, dtype=np.uint32), 6, "a single class")
    assert np.sum(~np.isnan(got.mean_dist)) == 1 and got.max_dist[4, 4] == x.max() - x.min()  # the diameter
    # every row left out
    got = exact_case(kpop, oracle, x, 3, np.full(r1, NO_CLASS, dtype=np.uint32), 2, "every row left out")
    assert got.class_rows.tolist() == [0, 0] and np.all(got.min_i == NO_CLASS)
    # every row a class of its own: the table IS the matrix, its diagonal empty
    order = rng.permutation(r1).astype(np.uint32)
    got = exact_case(kpop, oracle, x, 3, order, r1, "singletons")
    D = np.abs(np.subtract.outer(x, x))[np.ix_(np.argsort(order), np.argsort(order))]
    off = ~np.eye(r1, dtype=bool)
    assert np.array_equal(got.mean_dist[off], D[off]) and np.array_equal(got.min_dist[off], D[off]) and np.array_equal(got.max_dist[off], D[off])
    assert np.all(np.isnan(np.diag(got.mean_dist))) and np.all(got.class_rows == 1)
    # duplicates at distance 0: sixteen values for 150 rows, so that whole classes coincide and least pairs tie: (d, i, j) decides
    x = dyadic(rng, 150, below=16)
    got = exact_case(kpop, oracle, x, 17, labelling(rng, [40, 30, 50, 20], 10), 4, "duplicates")
    assert np.all(got.min_dist == 0.0) and not np.any(np.signbit(got.min_dist)) and np.all(got.min_i < got.min_j)
    got = exact_case(kpop, oracle, np.full(9, 2.5), 1, np.array([0, 1, 0, 1, 2, 2, 0, 1, NO_CLASS], dtype=np.uint32), 3, "one point")
    assert got.min_i.tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 4]] and got.min_j.tolist() == [[2, 1, 4], [1, 3, 4], [4, 4, 5]]


def test_the_worked_case(kpop, oracle):
    from test_class_linkage_ref import HAND_CLASS, HAND_MAX, HAND_MEAN, HAND_MIN, HAND_MIN_I, HAND_MIN_J, HAND_N, HAND_ROWS, HAND_TREES, HAND_X
    got = exact_case(kpop, oracle, HAND_X, 3, np.array(HAND_CLASS, dtype=np.uint32), HAND_N, "INTEGRATION.md 6o")
    hand = (np.array(HAND_ROWS, dtype=np.uint32), np.array(HAND_MEAN), np.array(HAND_MIN), np.array(HAND_MAX), np.array(HAND_MIN_I, dtype=np.uint32),
            np.array(HAND_MIN_J, dtype=np.uint32))
    check_exact(got, hand, "the section's table")
    for linkage, table in ((0, got.min_dist), (1, got.max_dist), (2, got.mean_dist)):
        tree = kpop.class_tree(got.class_rows, table, linkage)
        want = HAND_TREES[linkage]
        assert tree.left.tolist() == want[0] and tree.right.tolist() == want[1] and tree.height.tolist() == want[2] and tree.size.tolist() == want[3]


def test_the_long_set_tile_shape(kpop, oracle):
    """65,600 rows take the tiles of a long set (32 columns x 256 rows).  No quadratic reference: the line reference, exact by integer
    prefix sums; dyadic coordinates, so that sums of 10^9 terms are exact"""
    r1, n_dims, n_classes = 65600, 3, 5
    rng = np.random.RandomState(65600)
    x = dyadic(rng, r1)
    class_of = rng.choice(np.array([0, 1, 2, 3, 4, NO_CLASS], dtype=np.uint32), size=r1, p=[0.4, 0.25, 0.15, 0.1, 0.05, 0.05]).astype(np.uint32)
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        got = rs.class_linkage(class_of, n_classes)
    finally:
        rs.free()
    want = line_linkage_ref(x, class_of, n_classes)
    check_exact(got, want, "65,600 rows")
    check_symmetric(got, "65,600 rows")
    assert np.array_equal(np.abs(x[got.min_i] - x[got.min_j]), got.min_dist) and np.all(got.min_i < got.min_j)
    for a in range(n_classes):
        for b in range(n_classes):
            assert {int(class_of[got.min_i[a, b]]), int(class_of[got.min_j[a, b]])} == {a, b}


RANDOM = [(7, 0), (7, 1), (7, 2), (40, 0), (40, 1), (40, 2)]


def mean_errors(got, want, rows):
    """the largest of |mean - fsum's| / fsum's over the table, in units of its entry's bound (N + 2) 2^-53, and as a relative error"""
    n = rows.astype(np.float64)
    N = np.outer(n, n)
    worst, worst_rel = 0.0, 0.0
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / want, np.where(got == want, 0.0, np.inf))
    if ok.any():
        worst = float(np.max(rel[ok] / ((N[ok] + 2) * 2.0 ** -53)))
        worst_rel = float(np.max(rel[ok]))
    return worst, worst_rel


@pytest.mark.parametrize("n_dims,kind", RANDOM, ids=["%d-%s" % (d, ("euclidean", "cosine", "minkowski")[k]) for d, k in RANDOM])
def test_random_rows(kpop, oracle, n_dims, kind):
    r1 = 500
    p = KINDS[kind][1]
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
                want = class_linkage_ref(D, class_of, n_classes)
                got = rs.class_linkage(class_of, n_classes)
                assert np.array_equal(got.class_rows, want[0]), what
                for name in ("min_dist", "max_dist"):
                    assert same_bits(getattr(got, name), want[NAMES.index(name)]), (what, name)
                assert np.array_equal(got.min_i, want[4]) and np.array_equal(got.min_j, want[5]), what
                units, rel = mean_errors(got.mean_dist, want[1], want[0])
                print("    %s mean_dist: relative error %.3g, %.3g of its bound (N + 2) 2^-53" % (what, rel, units))
                assert units <= 1.0, (what, units)
                check_symmetric(got, what)
        finally:
            rs.free()


def device_form(kpop, rs, class_of, n_classes, guard=8):
    """kpop_dev_class_linkage on a stream of the caller's with its own workspace -> (ClassLinkage, the guard words behind every output)"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    nn = n_classes * n_classes
    work = torch.empty(max(api.dev_class_linkage_workspace_bytes(rs, n_classes), 1), dtype=torch.uint8, device=dev)
    d_cls = torch.from_numpy(class_of.astype(np.int64).astype(np.uint32).view(np.int32)).to(dev)
    sizes = [n_classes, nn, nn, nn, nn, nn]
    types = [torch.int32, torch.float64, torch.float64, torch.float64, torch.int32, torch.int32]
    outs = [torch.full((n + guard,), -3, dtype=t, device=dev) for n, t in zip(sizes, types)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        api.dev_class_linkage(rs, d_cls.data_ptr(), n_classes, work.data_ptr(), *[t.data_ptr() for t in outs], stream=stream.cuda_stream)
    stream.synchronize()
    host = [t.cpu().numpy() for t in outs]
    host = [a.view(np.uint32) if a.dtype == np.int32 else a for a in host]
    shaped = [host[0][:n_classes]] + [a[:nn].reshape(n_classes, n_classes) for a in host[1:]]
    return kpop.ClassLinkage(*shaped), [a[n:] for a, n in zip(host, sizes)]


def guards_untouched(guards):
    return all(np.all(g == (-3.0 if g.dtype == np.float64 else 0xFFFFFFFD)) for g in guards)


def test_the_contract_properties(kpop, oracle):
    """the same bits on every run; symmetric tables; what a renumbering of the classes may move; the host, device and unprepared forms
    agree -- on rows whose sums are NOT exact, so that an order of additions that moved would show"""
    r1, n_dims, n_classes = 300, 17, 7
    rng = np.random.RandomState(3)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    class_of = labelling(rng, [1, 64, 65, 0, 100, 40, 20], 10)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            first = rs.class_linkage(class_of, n_classes)
            check_exact(rs.class_linkage(class_of, n_classes), first, "a second run", declared_nan=False)
            check_symmetric(first, kind)
            sums = first.mean_dist[~np.isnan(first.mean_dist)]
            assert np.any(sums != np.round(sums * 8) / 8)  # (not the exact kind of case)
            # renumbered by a random permutation: new class of old class c is perm[c]
            perm = rng.permutation(n_classes).astype(np.uint32)
            moved = rs.class_linkage(np.where(class_of == NO_CLASS, NO_CLASS, perm[np.minimum(class_of, n_classes - 1)]).astype(np.uint32), n_classes)
            at = np.ix_(perm, perm)
            assert np.array_equal(moved.class_rows[perm], first.class_rows)
            assert same_bits(moved.min_dist[at], first.min_dist) and same_bits(moved.max_dist[at], first.max_dist)
            assert np.array_equal(moved.min_i[at], first.min_i) and np.array_equal(moved.min_j[at], first.min_j)
            D = oracle.distance_rowwise(m, m, metric, kind, p, normalize)
            want = class_linkage_ref(D, class_of, n_classes)
            for name, t in (("as given", first.mean_dist), ("renumbered", moved.mean_dist[at])):
                units, rel = mean_errors(t, want[1], want[0])
                print("    kind %d, %s: mean_dist relative error %.3g, %.3g of its bound" % (kind, name, rel, units))
                assert units <= 1.0, (kind, name, units)
            # the three forms
            got, guards = device_form(kpop, rs, class_of, n_classes)
            check_exact(got, first, "the device form", declared_nan=False)
            assert guards_untouched(guards)
            check_exact(kpop.distance_class_linkage(m, metric, class_of, kind, p, normalize, n_classes), first, "the unprepared form", declared_nan=False)
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
            want = fresh.class_linkage(class_of, 3)
            before = grown.class_linkage(class_of[:170], 3)
            grown.append(m[170:])
            got = grown.class_linkage(class_of, 3)
            check_exact(got, want, "after append", declared_nan=False)
            assert not same_bits(before.mean_dist, got.mean_dist)  # a new row changes every mean
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
        got = rs.class_linkage(class_of, 3)
        want = class_linkage_ref(D, class_of, 3)
        # exactly the means of the class's row and column
        expect = np.zeros((3, 3), dtype=bool)
        expect[a, :] = expect[:, a] = True
        assert np.array_equal(np.isnan(got.mean_dist), expect)
        # every least and greatest distance is still a number, and never comes from that row
        assert not np.any(np.isnan(got.min_dist)) and not np.any(np.isnan(got.max_dist))
        assert not np.any(got.min_i == bad) and not np.any(got.min_j == bad)
        assert same_bits(got.min_dist, want[2]) and same_bits(got.max_dist, want[3])
        assert np.array_equal(got.min_i, want[4]) and np.array_equal(got.min_j, want[5])
        units, _ = mean_errors(got.mean_dist, want[1], want[0])
        assert units <= 1.0
        # the same row left out: no NaN at all (no pair set here is empty)
        left = np.array(class_of)
        left[bad] = NO_CLASS
        got = rs.class_linkage(left, 3)
        for name in F64_TABLES:
            assert not np.any(np.isnan(getattr(got, name))), name
        assert got.class_rows[a] == np.sum(class_of == a) - 1
    finally:
        rs.free()


def raw_class_linkage(rs_handle, class_of, n_classes, outs):
    from kpop_amd import _lib
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32))  # noqa: E731
    return _lib.load().kpop_class_linkage(rs_handle, ptr(class_of), n_classes, *[ptr(a) for a in outs])


def test_arguments(kpop, oracle):
    from kpop_amd import api
    r1, n_dims = 70, 3
    rng = np.random.RandomState(2)
    x = dyadic(rng, r1)
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    class_of = labelling(rng, [30, 25, 10], 5)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        want = rs.class_linkage(class_of, 3)
        for n_classes, code in ((0, ERR_INVALID), (4097, ERR_UNSUPPORTED)):
            with pytest.raises(kpop.KPopError) as e:
                rs.class_linkage(class_of, n_classes)
            assert e.value.code == code and "kpop_class_linkage" in str(e.value)
            with pytest.raises(kpop.KPopError) as e:
                kpop.distance_class_linkage(m, metric, class_of, 0, 2.0, False, n_classes)
            assert e.value.code == code
            assert api.dev_class_linkage_workspace_bytes(rs, n_classes) == 0
            with pytest.raises(kpop.KPopError) as e:
                api.dev_class_linkage(rs, None, n_classes, None)
            assert e.value.code == code and "kpop_dev_class_linkage" in str(e.value)
        # O((r1 / TJ + n_classes) n_classes) partials of 32 bytes, and the grouping
        assert 0 < api.dev_class_linkage_workspace_bytes(rs, 3) < 1 << 23
        assert 4096 * 4096 * 32 < api.dev_class_linkage_workspace_bytes(rs, 4096) < (4096 + 3) * 4096 * 32 + (1 << 23)
        # a class out of range that is not NO_CLASS
        with pytest.raises(kpop.KPopError) as e:
            rs.class_linkage(class_of, 2)
        assert e.value.code == ERR_INVALID and "class 2 of 2" in str(e.value)
        wrong = np.array(class_of)
        wrong[11] = NO_CLASS - 1
        with pytest.raises(kpop.KPopError) as e:
            rs.class_linkage(wrong, 3)
        assert e.value.code == ERR_INVALID
        with pytest.raises(kpop.KPopError):  # the device form needs its workspace
            api.dev_class_linkage(rs, None, 3, None)
        # in the device form the table is trusted and guarded: such a row counts as left out
        got, guards = device_form(kpop, rs, wrong, 3)
        left = np.array(class_of)
        left[11] = NO_CLASS
        check_exact(got, rs.class_linkage(left, 3), "a class beyond n_classes on the device")
        assert guards_untouched(guards)
        # every output pointer may be NULL; any one alone is what it is with the others
        assert raw_class_linkage(rs.handle, class_of, 3, [None] * 6) == 0
        for k in range(6):
            outs = [None] * 6
            outs[k] = np.zeros_like(want[k])
            assert raw_class_linkage(rs.handle, class_of, 3, outs) == 0
            check = same_bits if want[k].dtype == np.float64 else np.array_equal
            assert check(outs[k], want[k]), NAMES[k]
        assert raw_class_linkage(rs.handle, None, 3, [None] * 6) == ERR_INVALID
        # 4,096 classes on 70 rows: the classes that have rows as with 40 classes, everything else empty
        spread = (rng.randint(0, 40, size=r1)).astype(np.uint32)
        small, big = rs.class_linkage(spread, 40), rs.class_linkage(spread, 4096)
        assert big.mean_dist.shape == (4096, 4096) and big.class_rows.shape == (4096,)
        check_exact(kpop.ClassLinkage(big.class_rows[:40], *[t[:40, :40] for t in big[1:]]), small, "4,096 classes, the first 40")
        for name in F64_TABLES:
            t = getattr(big, name).view(np.uint64)
            assert np.all(t[40:] == QNAN_BITS) and np.all(t[:, 40:] == QNAN_BITS), name
        assert np.all(big.min_i[40:] == NO_CLASS) and np.all(big.min_j[:, 40:] == NO_CLASS) and not np.any(big.class_rows[40:])
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.class_linkage(class_of, 3)
    assert e.value.code == ERR_INVALID
    # an empty set: KPOP_OK, the classes all empty -- the error of a bad argument still comes first
    empty = kpop.RefSet(np.zeros((0, n_dims)), metric, 0, 2.0, False)
    try:
        got = empty.class_linkage(np.zeros(0, dtype=np.uint32), 4)
        assert got.class_rows.tolist() == [0] * 4 and np.all(got.min_i == NO_CLASS) and np.all(got.min_j == NO_CLASS)
        for name in F64_TABLES:
            assert getattr(got, name).shape == (4, 4) and np.all(getattr(got, name).view(np.uint64) == QNAN_BITS)
        with pytest.raises(kpop.KPopError):
            empty.class_linkage(np.zeros(0, dtype=np.uint32), 0)
        assert raw_class_linkage(empty.handle, None, 4, [None] * 6) == 0
    finally:
        empty.free()


def test_from_dbscan_to_a_tree(kpop, oracle):
    """RefSet.dbscan's labels through dense_labels and class_linkage into class_tree(..., LINK_AVERAGE): three well-separated blobs, the
    two nearer ones merge first, and the root's height is the mean over the cross pairs of rows"""
    rng = np.random.RandomState(31)
    n_dims = 6
    centres = np.zeros((3, n_dims))
    centres[1, 0], centres[2, 1] = 10.0, 40.0
    sizes = [40, 30, 50]
    m = np.concatenate([c + 0.3 * rng.normal(size=(n, n_dims)) for c, n in zip(centres, sizes)])
    m = m[rng.permutation(len(m))]
    metric = np.ones(n_dims)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        labels = rs.dbscan(2.5, 4)[0]
        class_of, n_classes, _ = kpop.dense_labels(labels)
        assert n_classes == 3 and not np.any(class_of == NO_CLASS)
        got = rs.class_linkage(class_of)
    finally:
        rs.free()
    assert sorted(got.class_rows.tolist()) == sorted(sizes)
    tree = kpop.class_tree(got.class_rows, got.mean_dist, LINK_AVERAGE)
    assert len(tree.left) == 2 and tree.size.tolist()[1] == 120 and tree.height[0] < tree.height[1]
    near = {int(tree.left[0]), int(tree.right[0])}
    far = ({0, 1, 2} - near).pop()
    # the nearer two are the blobs at the origin and at 10: their rows lie below 20 in the second coordinate
    assert all(np.all(m[class_of == c, 1] < 20) for c in near) and np.all(m[class_of == far, 1] > 20)
    assert (int(tree.left[1]), int(tree.right[1])) == (far, 3)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
    cross = D[np.ix_(np.flatnonzero(class_of != far), np.flatnonzero(class_of == far))].ravel()
    want = math.fsum(cross) / len(cross)
    err, bound = abs(tree.height[1] - want) / want, (len(cross) + 2) * 2.0 ** -53
    print("    the root's height: relative error %.3g of %.3g" % (err, bound))
    assert err <= bound
    assert kpop.class_tree_newick(tree, 3)[0].count(":") == 4
