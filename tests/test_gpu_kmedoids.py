"""k-medoids on a resident set (kpop_kmedoids, include/kpop_hip.h).

EXACT CASES: a dyadic first coordinate, the other coordinates 0, euclidean, unit metric, raw -- every distance and every sum is exact
(asserted on the matrix first), so every output, the whole cost trajectory included, equals tests/kmedoids_ref.py bit for bit.
GENERAL CASES: the three kinds, normalised or not, on the operands tests/test_gpu_representatives.py shares; the matrix G is the oracle's
or, for the Minkowski kind, the GPU's own on the vector pipe (as tests/test_gpu_farthest_first.py does).  There the GPU's sums are not
math.fsum's: class_of / dist are held to assign_ref(G, medoid) bit for bit, own_mean to kpop_silhouette's bits (property 5), runs to their
continuations (property 3), cost to r1 2^-53 relative, and the update to contract (c) of section 6k: no member's fsum mean lies below its
class's medoid's by more than n_c 2^-52 relative.  Every case converges within max_iter = 100 under the reference: asserted before the
GPU is called."""
import ctypes as C
import math

import numpy as np
import pytest

from kmedoids_ref import NO_CLASS, assign_ref, kmedoids_ref, own_means_ref
from test_gpu_representatives import on_the_vector_pipe, operands, oracle_matrix, self_matrix

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
KIND_IDS = ["euclidean", "cosine", "minkowski"]
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
QNAN_BITS = 0x7FF8000000000000
FIELDS = ("medoid", "class_of", "dist", "own_mean", "class_rows", "cost")
CAP = 100


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_floats(g, w):
    """bit for bit where the values are numbers, a NaN where the other holds a NaN"""
    return g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(bits(g[~np.isnan(g)]), bits(w[~np.isnan(w)]))


def check(got, want, what, fields=FIELDS + ("n_iter", "converged")):
    for name in fields:
        g, w = getattr(got, name), getattr(want, name)
        if not isinstance(w, np.ndarray):
            assert g == w, (what, name, g, w)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        ok = same_floats(g, w) if w.dtype == np.float64 else np.array_equal(g, w)
        assert ok, (what, name, int(np.sum(bits(g) != bits(w))), g[:8], w[:8])


def run(rs, what, init, max_iter=CAP):
    """the call, twice: the same bits on every run (property 1)"""
    got, again = rs.kmedoids(init, max_iter), rs.kmedoids(init, max_iter)
    check(again, got, (what, "a second run"))
    return got


def line_rows(x, n_dims):
    m = np.zeros((len(x), n_dims))
    m[:, 0] = x
    return m


def exact_case(kpop, oracle, x, n_dims, init, what, max_iters=(CAP,)):
    x = np.asarray(x, dtype=np.float64)
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    D = oracle.distance_rowwise(m, m, metric, 0, 2.0, False)
    assert np.array_equal(D, np.abs(np.subtract.outer(x, x)))  # every distance is exact
    full = kmedoids_ref(D, init, CAP)
    assert full.converged, (what, "the reference does not converge in %d rounds" % CAP)
    # ... and so is every sum: of the distances of a row (a class's are some of them) and of a labelling's dist
    grid = 1024.0
    assert np.array_equal(D * grid, np.round(D * grid)) and D.sum(axis=1).max() * grid < 2.0 ** 52
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        out = {}
        for max_iter in max_iters:
            want = full if max_iter == CAP else kmedoids_ref(D, init, max_iter)
            out[max_iter] = run(rs, what, init, max_iter)
            check(out[max_iter], want, (what, max_iter))
        return out[max_iters[0]], full
    finally:
        rs.free()


def dyadic(rng, n, below=8192):
    """multiples of 1/8 below 2^10"""
    return rng.randint(0, below, size=n) / 8.0


def clumps(rng, sizes):
    """a clump a class, 4,096 apart, its rows within 16 of its centre on a grid of 1/8; shuffled"""
    x = np.concatenate([4096.0 * c + rng.randint(0, 256, size=n) / 8.0 for c, n in enumerate(sizes)])
    return x[rng.permutation(len(x))]


SHAPES = [(1, 4), (2, 4), (63, 9), (64, 9), (65, 9), (130, 9), (300, 200), (1000, 16)]
KS = (1, 2, 31, 32, 33, 65)


@pytest.mark.parametrize("r1,n_dims", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_exact_sizes(kpop, oracle, r1, n_dims):
    """k around a group of 32 medoids and around two groups, k = r1: all singletons; max_iter = 0, 1 and to convergence"""
    rng = np.random.RandomState(100 * r1 + n_dims)
    x = dyadic(rng, r1, 1024) + 128.0 * rng.randint(0, 6, size=r1)
    worst = 0
    for k in sorted(set(k for k in KS + (r1,) if k <= r1)):
        init = rng.permutation(r1)[:k]
        got, full = exact_case(kpop, oracle, x, n_dims, init, (r1, n_dims, k), (CAP, 0, 1))
        worst = max(worst, full.n_iter)
        assert got.converged and np.all(got.cost[1:] <= got.cost[:-1])  # property 4, bit for bit
        if k == r1:
            assert got.n_iter == 0 and not got.dist.any() and not got.own_mean.any() and np.all(got.class_rows == 1)
    print("  %d x %d: at most %d rounds" % (r1, n_dims, worst))


def test_exact_class_sizes_round_a_column_tile(kpop, oracle):
    """classes of w - 1, w, w + 1 and 2 w + 1 rows (w = 64: the column tile of a short set) and one row alone, from clumps far apart"""
    rng = np.random.RandomState(7)
    sizes = [63, 64, 65, 129, 1]
    x = clumps(rng, sizes)
    init = [int(np.flatnonzero((x >= 4096.0 * c) & (x < 4096.0 * c + 64))[0]) for c in range(len(sizes))]
    got, _ = exact_case(kpop, oracle, x, 3, init, "tile sizes", (CAP, 0))
    assert got.class_rows.tolist() == sizes and got.converged
    # a row tile of the grouped order spans several of these classes: 16 classes of 9 rows, and k = 16 of 144 rows
    sizes = [9] * 16
    x = clumps(rng, sizes)
    init = [int(np.flatnonzero((x >= 4096.0 * c) & (x < 4096.0 * c + 64))[0]) for c in range(len(sizes))]
    got, _ = exact_case(kpop, oracle, x, 3, init, "small classes")
    assert got.class_rows.tolist() == sizes


def test_exact_edge_cases(kpop, oracle):
    # the worked case of section 6m
    x = [0, .125, .25, 1.125, 1.25, 1.375, 1.5, .75, 5, .375]
    got, _ = exact_case(kpop, oracle, x, 3, [0, 8, 6], "worked", (CAP, 0, 1, 2))
    assert got.medoid.tolist() == [2, 8, 4] and got.cost.tolist() == [2.25, 1.5] and got.n_iter == 1 and got.converged
    assert got.dist.tolist() == [.25, .125, 0, .125, 0, .125, .25, .5, 0, .125] and got.class_of.tolist() == [0, 0, 0, 2, 2, 2, 2, 0, 1, 0]
    # a duplicate of a medoid that is itself an initial medoid keeps its own position: rows 1 and 2 are one point
    got, _ = exact_case(kpop, oracle, [0, 1, 1, 3, 7, 0, 1], 2, [1, 2], "duplicate medoids", (0, CAP))
    assert got.class_of.tolist() == [0, 0, 1, 0, 0, 0, 0] and got.class_rows.tolist() == [6, 1]
    # a medoid tie on the mean: rows 1 and 2 of 0, 1, 2, 3 both have mean 4/3 -- the smaller row
    got, _ = exact_case(kpop, oracle, [0, 2, 4, 6, 100], 1, [0, 4], "medoid tie")
    assert got.medoid.tolist() == [1, 4]
    # an assignment tie between two medoids: row 1 lies midway -- the earlier position, whichever row that is
    for init, c in (([0, 2], 0), ([2, 0], 0)):
        got, _ = exact_case(kpop, oracle, [0, 4, 8], 5, init, "assignment tie", (0,))
        assert got.class_of[1] == c and got.dist[1] == 4.0
    # -0 and +0 coordinates: a zero distance is +0
    got, _ = exact_case(kpop, oracle, [-0.0, 0.0, 0.0, 1.0], 1, [3, 1], "zeros", (0, CAP))
    assert not np.signbit(got.dist).any() and not np.signbit(got.own_mean).any()


def test_the_long_set_tile_shape(kpop, oracle):
    """65,600 rows take the tiles of a long set (32 columns x 256 rows), k = 64: two groups of medoids.  No quadratic matrix: the
    reference's steps over the 1-D coordinates in integer arithmetic (units of 1/8; a row's sum of distances from the sorted class's
    prefix sums) -- every sum is exact, so no order of additions can differ --, and a sample of rows is held to math.fsum"""
    r1, n_dims, k = 65600, 3, 64
    rng = np.random.RandomState(65600)
    x = dyadic(rng, r1, 512) + 256.0 * rng.randint(0, 80, size=r1)  # multiples of 1/8 below 2^15: sums of 65,600 distances stay below 2^31
    init = rng.permutation(r1)[:k].astype(np.uint32)

    def assign(M):
        d = np.abs(x[:, None] - x[M][None, :])
        c = np.argmin(d, axis=1).astype(np.uint32)  # the first of the least
        dist = d[np.arange(r1), c]
        c[M] = np.arange(k)
        dist[M] = 0.0
        return c, dist

    def means(c):
        own, rows = np.zeros(r1), np.zeros(k, dtype=np.uint32)
        for cc in range(k):
            idx = np.flatnonzero(c == cc)
            rows[cc] = len(idx)
            X = np.round(x[idx] * 8).astype(np.int64)
            order = np.argsort(X, kind="stable")
            Xs = X[order]
            before = np.concatenate([[0], np.cumsum(Xs)[:-1]])
            pos, n = np.arange(len(idx), dtype=np.int64), len(idx)
            s = np.empty(n, dtype=np.int64)
            s[order] = Xs * pos - before + (Xs.sum() - before - Xs) - Xs * (n - 1 - pos)
            assert s.max() < 2 ** 52
            own[idx] = (s / 8.0) / (n - 1) if n > 1 else 0.0
        return own, rows

    def update(own, c, M):
        return np.array([np.flatnonzero(c == cc)[np.argmin(own[c == cc])] for cc in range(k)], dtype=np.uint32)

    traj, M = [], init
    c, dist = assign(M)
    cost = [dist.sum()]
    for t in range(CAP + 1):
        own, rows = means(c)
        new = update(own, c, M)
        traj.append((M, c, dist, own, rows, list(cost)))
        if np.array_equal(new, M):
            break
        M = new
        c, dist = assign(M)
        cost.append(dist.sum())
    else:
        raise AssertionError("the reference does not converge in %d rounds" % CAP)
    print("  65,600 rows, k = 64: %d rounds" % (len(traj) - 1))
    assert len(traj) - 1 >= 2
    m, metric = line_rows(x, n_dims), np.ones(n_dims)
    rs = kpop.RefSet(m, metric, 0, 2.0, False)
    try:
        for max_iter in (0, 2, CAP):
            t = min(max_iter, len(traj) - 1)
            M, c, dist, own, rows, cost = traj[t]
            got = rs.kmedoids(init, max_iter)
            assert got.n_iter == t and got.converged == (t == len(traj) - 1), (max_iter, got.n_iter, got.converged)
            assert np.array_equal(got.medoid, M) and np.array_equal(got.class_of, c) and np.array_equal(got.class_rows, rows), max_iter
            assert np.array_equal(bits(got.dist), bits(dist)) and np.array_equal(bits(got.own_mean), bits(own)), max_iter
            assert np.array_equal(bits(got.cost), bits(np.array(cost))), (max_iter, got.cost, cost)
        # the sample: math.fsum over the row's class
        for j in rng.randint(0, r1, size=40):
            idx = np.flatnonzero(got.class_of == got.class_of[j])
            idx = idx[idx != j]
            assert got.own_mean[j] == math.fsum(np.abs(x[idx] - x[j])) / len(idx)
        assert got.cost[-1] == math.fsum(got.dist)
        # property 5 on the long set's tiles
        sil = rs.silhouette(got.class_of, k)
        assert np.array_equal(bits(sil.own_mean), bits(got.own_mean)) and np.array_equal(sil.medoid, got.medoid)
        with pytest.raises(kpop.KPopError) as e:  # the 16-bit class key
            rs.kmedoids(np.arange(65536, dtype=np.uint32), 1)
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        rs.free()


def general_case(kpop, rs, G, init, what):
    """max_iter = 0, 1, 2, ... until converged"""
    r1, k = G.shape[0], len(init)
    full = kmedoids_ref(G, init, CAP)
    assert full.converged, (what, "the reference does not converge in %d rounds" % CAP)
    runs = []
    for max_iter in range(CAP + 1):
        got = run(rs, what, init, max_iter)
        runs.append(got)
        assert got.n_iter == max_iter or got.converged, (what, max_iter)
        assert len(got.cost) == got.n_iter + 1 and got.class_rows.sum() == np.sum(got.class_of != NO_CLASS)
        # consistency: the assignment to medoid[], bit for bit
        c, dist = assign_ref(G, got.medoid)
        assert np.array_equal(got.class_of, c) and np.array_equal(bits(got.dist), bits(dist)), (what, max_iter)
        kept = got.class_of != NO_CLASS
        assert abs(got.cost[-1] - math.fsum(got.dist[kept])) <= r1 * 2.0 ** -53 * got.cost[-1], (what, max_iter)
        assert np.all(got.cost[1:] <= got.cost[:-1] * (1 + r1 * 2.0 ** -53)), (what, got.cost)  # property 4
        if got.converged:
            break
    print("  %s: %d rounds, cost %.6g -> %.6g" % (what, got.n_iter, got.cost[0], got.cost[-1]))
    assert got.converged and len(runs) >= 2
    for t, got in enumerate(runs):
        # property 5: the silhouette of the labelling
        sil = rs.silhouette(got.class_of, k)
        assert np.array_equal(np.isnan(sil.own_mean), got.class_of == NO_CLASS)
        assert same_floats(got.own_mean, sil.own_mean) and np.array_equal(sil.class_rows, got.class_rows), (what, t)
        assert np.all(bits(got.own_mean[got.class_of == NO_CLASS]) == QNAN_BITS)
        nxt = got if got.converged else runs[t + 1]
        assert np.array_equal(sil.medoid, nxt.medoid), (what, t)
        # contract (c): in math.fsum's means no member lies below its class's next medoid by more than n_c 2^-52 relative
        fs, _ = own_means_ref(G, got.class_of, k)
        for c in range(k):
            idx = np.flatnonzero(got.class_of == c)
            idx = idx[~np.isnan(fs[idx])]
            if len(idx):
                assert fs[idx].min() >= fs[nxt.medoid[c]] * (1 - len(idx) * 2.0 ** -52), (what, t, c)
        # property 3: one more round from this run's medoids is the next run
        if not got.converged:
            more = rs.kmedoids(got.medoid, 1)
            check(more, runs[t + 1], (what, t, "continued"), ("medoid", "class_of", "dist", "own_mean", "class_rows", "converged"))
            assert np.array_equal(bits(np.concatenate([got.cost, more.cost[1:]])), bits(runs[t + 1].cost)), (what, t)
    # from the last medoids: a fixed point at once
    again = rs.kmedoids(runs[-1].medoid, 0)
    check(again, runs[-1], (what, "fixed point"), ("medoid", "class_of", "dist", "own_mean", "class_rows", "converged"))
    assert again.n_iter == 0 and bits(again.cost)[0] == bits(runs[-1].cost)[-1]
    return runs[-1]


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("kind,p", KINDS, ids=KIND_IDS)
def test_general_cases(kpop, oracle, kind, p, normalize):
    for r1, d, k in ((130, 9, 5), (1000, 16, 40)):
        m, metric = operands(oracle, r1, d)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            G = on_the_vector_pipe(rs, m) if kind == 2 else oracle_matrix(oracle, r1, d, kind, p, normalize)
            seeds = rs.farthest_first(max_picks=k)
            last = general_case(kpop, rs, G, seeds.pick, (r1, d, k, kind, normalize))
            # an int is the k-centre seeding, a FarthestFirst its picks
            check(rs.kmedoids(k), last, "k"), check(rs.kmedoids(seeds), last, "a FarthestFirst")
            # property 6: the initial medoids in another order
            perm = np.random.RandomState(k).permutation(k)
            other = rs.kmedoids(seeds.pick[perm], 0)
            first = rs.kmedoids(seeds.pick, 0)
            assert np.array_equal(other.medoid, first.medoid[perm]) and np.array_equal(bits(other.dist), bits(first.dist))
            d2 = np.sort(G[:, first.medoid] + 0.0, axis=1)
            rest = np.setdiff1d(np.arange(r1), first.medoid)
            if not np.any(d2[rest, 0] == d2[rest, 1]):  # no row equidistant from two medoids
                inv = np.empty(k, dtype=np.int64)
                inv[perm] = np.arange(k)
                assert np.array_equal(inv[first.class_of], other.class_of) and np.array_equal(first.class_rows[perm], other.class_rows)
                assert same_floats(other.own_mean, first.own_mean)
        finally:
            rs.free()


@pytest.mark.parametrize("kind,p", KINDS[:2], ids=KIND_IDS[:2])
def test_rows_holding_a_nan(kpop, oracle, kind, p):
    """two NaN rows, one of them an initial medoid: it is a class of one, the other row is left out"""
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    m = np.array(m)
    m[0, 1] = np.nan
    m[r1 // 2, 3] = np.nan
    G = self_matrix(oracle, m, metric, kind, p, True)
    rs = kpop.RefSet(m, metric, kind, p, True)
    try:
        init = np.array([20, 0, 100, 50], dtype=np.uint32)
        last = general_case(kpop, rs, G, init, ("nan", kind))
        for got in (last, rs.kmedoids(init, 0)):
            assert got.medoid[1] == 0 and got.class_of[0] == 1 and got.class_rows[1] == 1 and got.dist[0] == 0.0 and got.own_mean[0] == 0.0
            assert got.class_of[r1 // 2] == NO_CLASS and got.dist[r1 // 2] == np.inf and bits(got.own_mean)[r1 // 2] == QNAN_BITS
            assert got.class_rows.sum() == r1 - 1 and np.isfinite(got.cost).all()
    finally:
        rs.free()


def test_device_form_unprepared_form_and_growth(kpop, oracle):
    """kpop_dev_kmedoids on a stream of the caller's -- max_iter + 1 rounds enqueued, nothing read back --, its workspace of exactly the
    stated size and its outputs with guard words behind them; kpop_distance_kmedoids; and after append the old medoids as init"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    GUARD = 8
    for r1, d, kind, p, normalize, k, max_iter in ((1000, 16, 0, 2.0, True, 40, 30), (1000, 16, 1, 2.0, False, 33, 2), (130, 9, 2, P_MINK, True, 5, 0)):
        m, metric = operands(oracle, r1, d)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            init = rs.farthest_first(max_picks=k).pick
            want = rs.kmedoids(init, max_iter)  # the host form
            check(kpop.distance_kmedoids(m, metric, init, kind, p, normalize, max_iter), want, "the unprepared form")
            need = api.dev_kmedoids_workspace_bytes(rs, k, max_iter)
            assert 0 < need <= 64 * 1024 + 400 * r1 + 64 * k + 8 * max_iter  # O(r1 + k + max_iter): no copy of the rows
            work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
            medoid, class_rows, class_of = (torch.full((n + GUARD,), -3, dtype=torch.int32, device=dev) for n in (k, k, r1))
            dist, own, cost = (torch.full((n + GUARD,), -3.0, dtype=torch.float64, device=dev) for n in (r1, r1, max_iter + 1))
            counts = torch.full((2 + GUARD,), -3, dtype=torch.int32, device=dev)
            d_init = torch.from_numpy(init.view(np.int32).copy()).to(dev)
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_kmedoids(rs, k, d_init.data_ptr(), max_iter, work.data_ptr(), counts.data_ptr(), medoid.data_ptr(), class_of.data_ptr(), dist.data_ptr(),
                                     own.data_ptr(), class_rows.data_ptr(), cost.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            n_iter, converged = (int(v) for v in counts.cpu().numpy()[:2])
            assert (n_iter, bool(converged)) == (want.n_iter, want.converged)
            got = [a.cpu().numpy() for a in (medoid, class_of, dist, own, class_rows, cost)]
            got = [a.view(np.uint32) if a.dtype == np.int32 else a for a in got]
            sizes = (k, r1, r1, r1, k, max_iter + 1)
            full_cost = np.concatenate([want.cost, np.full(max_iter - want.n_iter, np.nan)])
            for name, a, size, w in zip(FIELDS, got, sizes, list(want[:5]) + [full_cost]):
                ok = same_floats(a[:size], w) if w.dtype == np.float64 else np.array_equal(a[:size], w)
                assert ok, (r1, kind, name)
                assert np.all(a[size:] == (-3.0 if a.dtype == np.float64 else np.uint32(0xFFFFFFFD))), (r1, kind, name, "guard")
            assert np.all(bits(got[5][want.n_iter + 1:max_iter + 1]) == QNAN_BITS)  # past n_iter: the quiet NaN
            assert np.all(counts.cpu().numpy()[2:] == -3) and np.all(work.cpu().numpy()[need:] == 0xA5), (r1, kind)
            # without any output but the counts
            api.dev_kmedoids(rs, k, d_init.data_ptr(), max_iter, work.data_ptr(), counts.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            assert counts.cpu().numpy()[:2].tolist() == [n_iter, converged]
        finally:
            rs.free()
    # a run, 100 rows appended, the old medoids as init: a fresh run from them on the grown set
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        D = oracle_matrix(oracle, r1, d, kind, p, normalize)
        rs = kpop.RefSet(m[:900], metric, kind, p, normalize, capacity=r1)
        fresh = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            old = rs.kmedoids(12)
            assert old.converged
            rs.append(m[900:])
            grown = run(rs, "grown", old.medoid)
            check(grown, fresh.kmedoids(old.medoid), "grown against a fresh set")
            c, dist = assign_ref(D, grown.medoid)
            assert np.array_equal(grown.class_of, c) and np.array_equal(bits(grown.dist), bits(dist)) and grown.converged
        finally:
            rs.free()
            fresh.free()


def raw(rs, k, init, max_iter, outputs, n_iter=True, converged=True):
    """kpop_kmedoids through ctypes; outputs: six arrays or None each (medoid, class_of, dist, own_mean, class_rows, cost)"""
    from kpop_amd import _lib
    n, conv = C.c_uint32(12345), C.c_int(12345)
    ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32)) for a in outputs]
    init = None if init is None else np.asarray(init, dtype=np.uint32)
    rc = _lib.load().kpop_kmedoids(rs.handle, k, None if init is None else init.ctypes.data_as(C.POINTER(C.c_uint32)), max_iter, *ptr,
                                   C.byref(n) if n_iter else None, C.byref(conv) if converged else None)
    return rc, n.value, conv.value


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        init = [3, 50, 100]
        want = rs.kmedoids(init, 4)
        for bad in ([], list(range(r1)) + [0], [r1], [3, 5, 3]):
            with pytest.raises(kpop.KPopError) as e:
                rs.kmedoids(bad, 4)
            assert e.value.code == ERR_INVALID, bad
            with pytest.raises(kpop.KPopError) as e:
                kpop.distance_kmedoids(m, metric, bad, 0, 2.0, True, 4)
            assert e.value.code == ERR_INVALID, bad
        assert raw(rs, 3, None, 4, [None] * 6)[0] == ERR_INVALID  # a null init
        assert raw(rs, 3, init, 4, [None] * 6, n_iter=False)[0] == ERR_INVALID  # the counts must be there
        assert raw(rs, 3, init, 4, [None] * 6, converged=False)[0] == ERR_INVALID
        # every other output may be NULL: all of them, and each alone
        assert raw(rs, 3, init, 4, [None] * 6) == (0, want.n_iter, int(want.converged))
        for j in range(6):
            out = [np.full(3, 77, dtype=np.uint32), np.full(r1, 77, dtype=np.uint32), np.full(r1, 77.0), np.full(r1, 77.0), np.full(3, 77, dtype=np.uint32), np.full(5, 77.0)]
            assert raw(rs, 3, init, 4, [a if i == j else None for i, a in enumerate(out)]) == (0, want.n_iter, int(want.converged))
            w = want[j] if j < 5 else np.concatenate([want.cost, np.full(4 - want.n_iter, np.nan)])
            assert same_floats(out[j], w) if w.dtype == np.float64 else np.array_equal(out[j], w), j
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.kmedoids([0])
    assert e.value.code == ERR_INVALID
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        with pytest.raises(kpop.KPopError) as e:  # k > r1 = 0
            empty.kmedoids([0])
        assert e.value.code == ERR_INVALID
    finally:
        empty.free()
