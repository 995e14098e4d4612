"""The density peaks of a resident set (kpop_density_peaks, include/kpop_hip.h), without the distance matrix.

The contract: over the oracle's matrix -- for the euclidean and cosine kinds the bits of the reference chain -- the arrays of
tests/density_peaks_ref.py, EXACTLY: delta is one of the bit-exact distances, parent, labels and counts are integers, so there is no
tolerance and no case is left out.  For the Minkowski kind the matrix is the library's own on the vector pipe, for the reason
tests/test_gpu_silhouette.py gives (the GPU's pow agrees with the oracle's to rtol 1e-11 only), held to the oracle's at that rtol.

THE SEGMENTS, under density_peaks_segments of density_peaks.hip (at most 16, at most one a column tile of 64 positions below 65,536
rows; the cuts at the same tile numbers for every strip, a strip of 64 positions walking the tiles with a position below its last):
a set of 1 row launches a strip that walks nothing; up to 65 rows every strip walks ONE tile in one segment (row 64, alone in the
second strip, needs tile 0 only); 129 rows: the last strip in TWO segments; 300 rows: the last strip in FIVE, the strips before it in
1 .. 4, the segments behind a strip's walk returning at once; 65,600 rows (tiles of 32 positions, strips of 256): 16 segments of 129
tiles, the last strip walking all 2,050."""
import ctypes as C

import numpy as np
import pytest

from density_peaks_ref import INF, NOISE, QNAN_BITS, chain_case, components_within, density_peaks_ref, same_bits
from test_density_peaks_ref import HAND_CUTS, HAND_DELTA, HAND_DENSITY, HAND_EPS, HAND_PARENT, HAND_X

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID = -1


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


def check(got, want, what):
    assert tuple(got._fields) == ("density", "delta", "parent", "labels", "counts"), what
    assert got.density.dtype == np.float64 and same_bits(got.density, want.density), (what, "density")
    assert got.delta.dtype == np.float64 and same_bits(got.delta, want.delta), (what, "delta")
    assert got.parent.dtype == np.uint32 and np.array_equal(got.parent, want.parent), (what, "parent")
    if want.labels is None:
        assert got.labels is None and got.counts is None, what
        return
    assert got.labels.dtype == np.uint32 and np.array_equal(got.labels, want.labels), (what, "labels")
    assert got.counts.dtype == np.uint32 and np.array_equal(got.counts, want.counts), (what, "counts")
    keep = got.labels != NOISE
    assert np.array_equal(got.labels[got.labels[keep]], got.labels[keep]), what


def equal(a, b):
    return (same_bits(a.density, b.density) and same_bits(a.delta, b.delta) and np.array_equal(a.parent, b.parent)
            and (a.labels is None) == (b.labels is None) and (a.labels is None or (np.array_equal(a.labels, b.labels) and np.array_equal(a.counts, b.counts))))


def exact_set(kpop, oracle, x, n_dims):
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False) if len(x) else np.zeros((0, 0))
    assert np.array_equal(D, np.abs(np.subtract.outer(np.asarray(x, dtype=np.float64), x)))  # every distance is exact
    return kpop.RefSet(m, metric, 0, 2.0, False), D


SIZES = [(1, 1), (2, 3), (3, 16), (63, 17), (64, 33), (65, 1), (129, 3), (300, 16)]


@pytest.mark.parametrize("r1,n_dims", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_exact_sizes(kpop, oracle, r1, n_dims):
    """dyadic rows on a line, every distance exact: the degree density at two radii and a random given density (with ties, and without),
    each with and without a cut"""
    rng = np.random.RandomState(1000 * r1 + n_dims)
    rs, D = exact_set(kpop, oracle, dyadic(rng, r1), n_dims)
    try:
        for eps in (8.0, 60.0):
            check(rs.density_peaks(eps=eps), density_peaks_ref(D, eps=eps), (r1, n_dims, eps))
            check(rs.density_peaks(eps=eps, min_delta=eps), density_peaks_ref(D, eps=eps, min_delta=eps), (r1, n_dims, eps, "cut"))
        for density in (rng.randint(0, 5, size=r1).astype(np.float64), rng.standard_normal(r1)):
            check(rs.density_peaks(density=density), density_peaks_ref(D, density=density), (r1, n_dims, "given"))
            check(rs.density_peaks(density=density, min_density=0.5, min_delta=20.0), density_peaks_ref(D, density=density, min_density=0.5, min_delta=20.0),
                  (r1, n_dims, "given", "cut"))
    finally:
        rs.free()


def test_the_worked_case(kpop, oracle):
    rs, D = exact_set(kpop, oracle, HAND_X, 3)
    try:
        got = rs.density_peaks(eps=HAND_EPS)
        check(got, density_peaks_ref(D, eps=HAND_EPS), "INTEGRATION.md 6p")
        assert got.density.tolist() == HAND_DENSITY and got.delta.tolist() == HAND_DELTA and got.parent.tolist() == HAND_PARENT
        for (min_density, min_delta), labels, counts in HAND_CUTS:
            cut = rs.density_peaks(eps=HAND_EPS, min_density=min_density, min_delta=min_delta)
            assert cut.labels.tolist() == labels and cut.counts.tolist() == counts and equal(cut._replace(labels=None, counts=None), got)
            again = kpop.distance_density_peaks(line_rows(HAND_X, 3), np.ones(3), 0, 2.0, False, eps=HAND_EPS, min_density=min_density, min_delta=min_delta)
            assert equal(again, cut)  # the one-shot form
    finally:
        rs.free()


RANDOM = [(200, 20, 0), (200, 20, 1), (200, 20, 2)]


@pytest.mark.parametrize("r1,n_dims,kind", RANDOM, ids=["%dx%d-%s" % (r, d, ("euclidean", "cosine", "minkowski")[k]) for r, d, k in RANDOM])
def test_random_rows(kpop, oracle, r1, n_dims, kind):
    p = KINDS[kind][1]
    rng = np.random.RandomState(700 + kind)
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
            eps = float(np.percentile(D[~np.eye(r1, dtype=bool)], 10))
            what = (r1, n_dims, kind, normalize)
            check(rs.density_peaks(eps=eps, min_delta=eps), density_peaks_ref(D, eps=eps, min_delta=eps), what)
            density = rng.randint(0, 7, size=r1).astype(np.float64)
            check(rs.density_peaks(density=density, min_density=3.0, min_delta=eps), density_peaks_ref(D, density=density, min_density=3.0, min_delta=eps),
                  what + ("given",))
            assert equal(kpop.distance_density_peaks(m, metric, kind, p, normalize, eps=eps, min_delta=eps), rs.density_peaks(eps=eps, min_delta=eps))
        finally:
            rs.free()


def test_ties(kpop, oracle):
    rng = np.random.RandomState(9)
    # all densities equal: the parent is the nearest row of smaller index
    x = dyadic(rng, 150, below=64)  # copies, and ties of distance
    rs, D = exact_set(kpop, oracle, x, 5)
    try:
        got = rs.density_peaks(density=np.full(150, 2.5), min_delta=0.0)
        check(got, density_peaks_ref(D, density=np.full(150, 2.5), min_delta=0.0), "equal densities")
        for j in range(1, 150):
            d = D[j, :j]
            assert got.delta[j] == d.min() and got.parent[j] == int(np.flatnonzero(d == d.min())[0])
        assert got.parent[0] == 0 and got.delta[0] == INF
        check(rs.density_peaks(eps=-1.0, min_delta=0.0), got._replace(density=np.ones(150)), "a negative eps: the row order")
        # copies of a row: delta = +0, the parent the smallest index among the copies ranking above
        got = rs.density_peaks(eps=0.0, min_delta=0.0)
        check(got, density_peaks_ref(D, eps=0.0, min_delta=0.0), "copies")
        copies = [j for j in range(150) if got.delta[j] == 0]
        assert len(copies) > 20 and not np.any(np.signbit(got.delta))
        for j in copies:
            same = np.flatnonzero(x == x[j])
            assert got.parent[j] == same[0] and got.density[j] == len(same) and j != same[0]
    finally:
        rs.free()
    # -0.0 coordinates, and -0.0 densities beside +0.0
    m = np.zeros((40, 3))
    m[:, 0] = dyadic(rng, 40, below=32)
    m[::3] *= -1.0  # (-0.0 in the columns that are zero)
    assert np.any(np.signbit(m[:, 1]))
    D = oracle.distance_rowwise(m, m, np.ones(3), 0, 2.0, False)
    density = np.where(np.arange(40) % 2 == 0, -0.0, 0.0)
    rs = kpop.RefSet(m, np.ones(3), 0, 2.0, False)
    try:
        got = rs.density_peaks(density=density, min_delta=1.0)
        check(got, density_peaks_ref(D, density=density, min_delta=1.0), "-0.0")
        assert not np.any(np.signbit(got.delta)) and got.counts[1] == 1  # -0 equals +0: one order, one root
        check(rs.density_peaks(eps=0.0), density_peaks_ref(D, eps=0.0), "-0.0, degrees")
    finally:
        rs.free()


def test_the_long_set_tile_shape_and_the_deep_chain(kpop, oracle):
    """65,600 rows take the tiles of a long set (32 positions x 256, a thread 4 x 8) in 16 segments.  Row i sits at pos[i] of a seeded
    permutation, in the first coordinate; the density is -(pos - c)^2: delta is 1 everywhere, the parent one step toward c, the row at c
    the one root (tests/density_peaks_ref.py's chain_case, held to brute force at 1,000 rows by tests/test_density_peaks_ref.py).  The
    chain is over 43,000 rows deep: min_delta = +inf holds the pointer doubling.  The reference is O(n)"""
    r1 = 65600
    pos, density, delta, parent = chain_case(r1, 65600)
    m = line_rows(pos.astype(np.float64), 3)
    sample = np.arange(0, r1, 4100)
    E = oracle.distance_rowwise(m, m[sample], np.ones(3), 0, 2.0, False)
    assert np.array_equal(E, np.abs(np.subtract.outer(pos[sample], pos)).astype(np.float64))  # every distance is exact
    root = int(np.flatnonzero(pos == r1 // 3)[0])
    rs = kpop.RefSet(m, np.ones(3), 0, 2.0, False)
    try:
        got = rs.density_peaks(density=density, min_delta=INF)
        assert same_bits(got.density, density) and same_bits(got.delta, delta) and np.array_equal(got.parent, parent)
        assert np.all(got.labels == root) and got.counts.tolist() == [1, 1, 0]
        got = rs.density_peaks(density=density, min_delta=0.5)
        assert same_bits(got.delta, delta) and np.array_equal(got.parent, parent)
        assert np.array_equal(got.labels, np.arange(r1)) and got.counts.tolist() == [r1, 1, 0]
    finally:
        rs.free()


def test_cross_call_facts(kpop, oracle):
    rng = np.random.RandomState(31)
    r1, n_dims = 260, 6
    m = np.concatenate([rng.normal(size=(160, n_dims)) * 0.3, rng.normal(size=(100, n_dims)) * 1.2 + 3.0])
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
        for eps in (float(np.percentile(D, 5)), float(np.percentile(D, 20))):
            got = rs.density_peaks(eps=eps, min_delta=eps)
            check(got, density_peaks_ref(D, eps=eps, min_delta=eps), ("facts", eps))
            assert same_bits(got.density, rs.dbscan(eps, 1)[2].astype(np.float64))  # density_out is dbscan's degree
            comp = rs.clusters(eps)[0]
            assert np.array_equal(comp, components_within(D, eps))
            assert np.array_equal(comp[got.labels], comp)  # the refinement: rows j and labels[j] in one component at eps
            assert np.all(got.delta >= rs.core_distances(2))  # no nearer than the nearest row
            for min_density, min_delta in ((-INF, eps), (3.0, 0.5 * eps), (-INF, INF)):
                call = rs.density_peaks(eps=eps, min_density=min_density, min_delta=min_delta)
                labels, counts = kpop.density_peaks_cut(got.density, got.delta, got.parent, min_density, min_delta)
                assert np.array_equal(labels, call.labels) and np.array_equal(counts, call.counts)
            class_of, n_classes, _ = kpop.dense_labels(got.labels)  # the labels go into the silhouette like the other calls'
            assert n_classes == got.counts[0] and len(rs.silhouette(class_of, n_classes).silhouette) == r1
    finally:
        rs.free()


def test_conventions(kpop, oracle):
    rng = np.random.RandomState(21)
    r1, n_dims, bad = 130, 5, 77
    m = np.round(rng.normal(size=(r1, n_dims)), 2)
    m[bad, 2] = np.nan
    metric = np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
    assert np.all(np.isnan(np.delete(D[bad], bad)))
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        # a row with a NaN coordinate: a root, a cluster of its own, nobody's parent -- also at the top of the order
        for density in (None, np.where(np.arange(r1) == bad, 99.0, rng.randint(0, 4, size=r1))):
            got = rs.density_peaks(eps=1.0, density=density, min_delta=INF)
            check(got, density_peaks_ref(D, eps=1.0, density=density, min_delta=INF), "a NaN row")
            assert got.parent[bad] == bad and got.delta[bad] == INF and got.labels[bad] == bad and np.sum(got.parent == bad) == 1
            assert got.counts.tolist() == [2, 2, 0] and np.sum(got.labels == bad) == 1
        # NaN densities: left out; +-inf densities: numbers
        density = rng.randint(0, 4, size=r1).astype(np.float64)
        density[[3, 64, 129]] = np.nan
        density[[5, 100]] = INF
        density[7] = -INF
        got = rs.density_peaks(density=density, min_density=1.0, min_delta=0.5)
        check(got, density_peaks_ref(D, density=density, min_density=1.0, min_delta=0.5), "NaN and infinite densities")
        for j in (3, 64, 129):
            assert got.delta.view(np.uint64)[j] == QNAN_BITS and got.parent[j] == NOISE and got.labels[j] == NOISE and not np.any(got.parent == j)
        assert got.counts[2] == 3 and got.parent[5] == 5 and got.parent[100] == 5 and got.parent[7] != 7
        assert np.array_equal(np.isnan(got.density), np.isnan(density))
        # every density a NaN: everybody left out
        got = rs.density_peaks(density=np.full(r1, np.nan), min_delta=1.0)
        assert np.all(got.parent == NOISE) and np.all(got.labels == NOISE) and got.counts.tolist() == [0, 0, r1]
        assert np.all(got.delta.view(np.uint64) == QNAN_BITS)
    finally:
        rs.free()


def test_a_set_after_growth(kpop, oracle):
    r1, n_dims = 300, 9
    rng = np.random.RandomState(8)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, True)
    eps = float(np.percentile(D, 10))
    for normalize in (True, False):
        fresh = kpop.RefSet(m, metric, 0, 2.0, normalize)
        grown = kpop.RefSet(m[:170], metric, 0, 2.0, normalize, capacity=r1)
        try:
            before = grown.density_peaks(eps=eps, min_delta=eps)
            grown.append(m[170:])
            assert equal(grown.density_peaks(eps=eps, min_delta=eps), fresh.density_peaks(eps=eps, min_delta=eps))
            if normalize:
                check(fresh.density_peaks(eps=eps, min_delta=eps), density_peaks_ref(D, eps=eps, min_delta=eps), "fresh")
                assert not same_bits(before.density, fresh.density_peaks(eps=eps).density[:170])  # a new row changes degrees: no known_rows
        finally:
            fresh.free()
            grown.free()


def device_form(kpop, rs, eps, density, min_density, min_delta, guard=8):
    """kpop_dev_density_peaks on a stream of the caller's with exactly workspace_bytes of workspace -> (DensityPeaks, every guard untouched)"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    r1 = rs.info()["r1"]
    types = [torch.float64, torch.float64, torch.int32, torch.int32]
    outs = [torch.full((r1 + guard,), -3, dtype=t, device=dev) for t in types] + [torch.full((3 + guard,), -3, dtype=torch.int32, device=dev)]
    nbytes = api.dev_density_peaks_workspace_bytes(rs)
    work = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d_density = None if density is None else torch.from_numpy(np.ascontiguousarray(density, dtype=np.float64)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        api.dev_density_peaks(rs, eps, work.data_ptr(), None if d_density is None else d_density.data_ptr(), min_density, min_delta,
                              *[t.data_ptr() for t in outs], stream=stream.cuda_stream)
    stream.synchronize()
    host = [t.cpu().numpy() for t in outs]
    host = [a.view(np.uint32) if a.dtype == np.int32 else a for a in host]
    sizes = [r1] * 4 + [3]
    clean = all(np.all(a[n:] == (-3.0 if a.dtype == np.float64 else 0xFFFFFFFD)) for a, n in zip(host, sizes))
    clean = clean and bool(torch.all(work[nbytes:] == 0xA5).item())
    return kpop.DensityPeaks(*[a[:n] for a, n in zip(host, sizes)]), clean


SEGMENTS = [(300, 9, "the last strip in 5 segments"), (60, 16, "1 segment"), (2000, 4, "16 segments of 2 tiles")]


@pytest.mark.parametrize("r1,n_dims,what", SEGMENTS, ids=["%dx%d" % s[:2] for s in SEGMENTS])
def test_runs_and_the_device_form(kpop, oracle, r1, n_dims, what):
    """identical on a second run; the device form on a stream of the caller's, behind guard words, with exactly workspace_bytes of
    workspace, equals the host form; the one-shot form equals the set form.  The set of 2,000 rows is held to the reference too"""
    rng = np.random.RandomState(r1)
    m = rng.normal(size=(r1, n_dims))
    metric = oracle.metric_powers(oracle.synth_inertia(n_dims))
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            D = oracle.distance_rowwise(m, m, metric, kind, p, normalize)
            eps = float(np.percentile(D, 8))
            given = rng.randint(0, 9, size=r1).astype(np.float64)
            for density in (None, given):
                first = rs.density_peaks(eps=eps, density=density, min_density=2.0, min_delta=eps)
                check(first, density_peaks_ref(D, eps=eps, density=density, min_density=2.0, min_delta=eps), (what, kind))
                assert equal(rs.density_peaks(eps=eps, density=density, min_density=2.0, min_delta=eps), first), "a second run"
                dev, clean = device_form(kpop, rs, eps, density, 2.0, eps)
                assert equal(dev, first) and clean, (what, kind)
                assert equal(kpop.distance_density_peaks(m, metric, kind, p, normalize, eps=eps, density=density, min_density=2.0, min_delta=eps), first)
        finally:
            rs.free()


def raw(fn, lead, outs):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32))  # noqa: E731
    return fn(*lead, *[ptr(a) for a in outs])


def test_arguments(kpop, oracle):
    from kpop_amd import _lib, api
    lib = _lib.load()
    rng = np.random.RandomState(2)
    r1, n_dims = 70, 3
    rs, D = exact_set(kpop, oracle, dyadic(rng, r1), n_dims)
    nan = float("nan")
    try:
        want = rs.density_peaks(eps=16.0, min_density=2.0, min_delta=16.0)
        check(want, density_peaks_ref(D, eps=16.0, min_density=2.0, min_delta=16.0), "arguments")
        given = np.ascontiguousarray(want.density)
        # a NaN eps without a density, NaN thresholds: KPOP_ERR_INVALID, in every form
        for call in (lambda: rs.density_peaks(), lambda: rs.density_peaks(eps=nan, min_delta=1.0), lambda: rs.density_peaks(eps=1.0, min_delta=nan),
                     lambda: rs.density_peaks(eps=1.0, min_density=nan, min_delta=1.0), lambda: rs.density_peaks(density=given, min_delta=nan),
                     lambda: kpop.distance_density_peaks(line_rows([1, 2, 3], 3), np.ones(3), 0, 2.0, False),
                     lambda: api.dev_density_peaks(rs, nan, None), lambda: api.dev_density_peaks(rs, 1.0, None, min_delta=nan)):
            with pytest.raises(kpop.KPopError) as e:
                call()
            assert e.value.code == ERR_INVALID and "kpop_" in str(e.value)
        # with a density given eps is not read
        assert equal(rs.density_peaks(eps=nan, density=given, min_density=2.0, min_delta=16.0), want)
        assert equal(rs.density_peaks(density=given, min_density=2.0, min_delta=16.0), want)
        with pytest.raises(kpop.KPopError):  # the device form needs its workspace
            api.dev_density_peaks(rs, 1.0, None)
        assert 0 < api.dev_density_peaks_workspace_bytes(rs) < 1 << 20  # O(r1)
        with pytest.raises(ValueError):
            rs.density_peaks(density=given[:5])
        # every output pointer may be NULL; any one alone is what it is with the others
        lead = [rs.handle, 16.0, None, 2.0, 16.0]
        full = list(want)
        assert raw(lib.kpop_density_peaks, lead, [None] * 5) == 0
        for i in range(5):
            outs = [None] * 5
            outs[i] = np.zeros_like(full[i])
            assert raw(lib.kpop_density_peaks, lead, outs) == 0
            assert same_bits(outs[i], full[i]) if outs[i].dtype == np.float64 else np.array_equal(outs[i], full[i]), i
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.density_peaks(eps=1.0)
    assert e.value.code == ERR_INVALID
    # r1 = 0: KPOP_OK, the counts zero -- the error of a NaN threshold still comes first; r1 = 1: a root
    empty = kpop.RefSet(np.zeros((0, n_dims)), np.ones(n_dims), 0, 2.0, False)
    one, _ = exact_set(kpop, oracle, [3.0], n_dims)
    try:
        got = empty.density_peaks(eps=1.0, min_delta=1.0)
        assert all(len(a) == 0 for a in got[:4]) and got.counts.tolist() == [0, 0, 0]
        counts = np.full(3, 7, dtype=np.uint32)
        assert raw(lib.kpop_density_peaks, [empty.handle, 1.0, None, 0.0, 1.0], [None, None, None, None, counts]) == 0 and not counts.any()
        with pytest.raises(kpop.KPopError):
            empty.density_peaks(eps=1.0, min_delta=nan)
        assert api.dev_density_peaks_workspace_bytes(empty) > 0
        got = one.density_peaks(eps=1.0, min_delta=1.0)
        assert got.density.tolist() == [1] and got.delta.tolist() == [INF] and got.parent.tolist() == [0] and got.labels.tolist() == [0]
        assert got.counts.tolist() == [1, 1, 0]
        got = one.density_peaks(density=[nan], min_delta=1.0)
        assert got.parent.tolist() == [NOISE] and got.counts.tolist() == [0, 0, 1]
    finally:
        empty.free()
        one.free()
