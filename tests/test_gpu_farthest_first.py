"""The farthest-first traversal of a resident set (kpop_farthest_first, include/kpop_hip.h).

The contract: pick, pick_radius, pick_parent, rep_of, rep_dist and the number of picks array-equal (the floats bit-equal) to
tests/farthest_first_ref.py on the matrix of the set against itself, and the same on every run.  For the euclidean and cosine kinds
that matrix is the oracle's, whose bits the GPU's chain reproduces; the Minkowski kind goes through the GPU's pow, so there the
reference runs on the GPU's own vector-pipe matrix (as tests/test_gpu_representatives.py does) -- no gap condition is needed, the
contract being equality with those bits.  The rows and the helpers are those of tests/test_gpu_representatives.py: a shape's operands
and its oracle matrix are made once and shared with that file."""
import ctypes as C

import numpy as np
import pytest

from farthest_first_ref import NOISE, farthest_first_ref
from test_gpu_representatives import on_the_vector_pipe, operands, oracle_matrix, self_matrix

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
KIND_IDS = ["euclidean", "cosine", "minkowski"]
ERR_INVALID = -1
INF = float("inf")
# one row, two rows, around the wavefront and the buckets of a workgroup, a strip and more than a strip, more dimensions than a
# step of the tile stages, several workgroups; "nan": 130 x 9 with a NaN row at index 0 and another in the middle
SHAPES = [(1, 4, False), (2, 4, False), (63, 9, False), (64, 9, False), (65, 9, False), (130, 9, False), (130, 9, True), (300, 200, False), (1000, 16, False)]
SHAPE_IDS = ["%dx%d%s" % (r, d, "nan" if bad else "") for r, d, bad in SHAPES]
FIELDS = ("pick", "pick_radius", "pick_parent", "rep_of", "rep_dist")


def rows_of(oracle, r1, d, bad):
    m, metric = operands(oracle, r1, d)
    if bad:
        m = np.array(m)
        m[0, 1] = np.nan
        m[r1 // 2, 3] = np.nan
    return m, metric


def reference_matrix(oracle, rs, m, metric, r1, d, bad, kind, p, normalize):
    """the matrix the result is held to: the oracle's, or -- the Minkowski kind -- the GPU's own on the vector pipe"""
    if kind == 2:
        return on_the_vector_pipe(rs, m)
    if bad:
        return self_matrix(oracle, m, metric, kind, p, normalize)
    return oracle_matrix(oracle, r1, d, kind, p, normalize)


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                                           y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(a[:5], b[:5]))


def run(rs, what, **kw):
    """the call, twice: the same bits on every run"""
    got, again = rs.farthest_first(**kw), rs.farthest_first(**kw)
    assert same_bits(got, again), (what, kw, "a second run")
    return got


def check(got, want, what):
    for name, g, w in zip(FIELDS, got[:5], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        bits = (g.view(np.uint64), w.view(np.uint64)) if g.dtype == np.float64 else (g, w)
        assert np.array_equal(*bits), (what, name, int(np.sum(bits[0] != bits[1])), g[:8], w[:8])
    n = len(got.pick)
    assert (n == 0 and got.n_passes == 0) or 1 <= got.n_passes <= n, (what, got.n_passes, n)


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("kind,p", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("r1,d,bad", SHAPES, ids=SHAPE_IDS)
def test_farthest_first_vs_reference(kpop, oracle, r1, d, bad, kind, p, normalize):
    m, metric = rows_of(oracle, r1, d, bad)
    what = (r1, d, bad, kind, normalize)
    rs = kpop.RefSet(m, metric, kind, p, normalize)
    try:
        G = reference_matrix(oracle, rs, m, metric, r1, d, bad, kind, p, normalize)
        # the full order
        want_full = farthest_first_ref(G)
        full = run(rs, what)
        check(full, want_full, (what, "full"))
        assert len(full.pick) == r1 and sorted(full.pick.tolist()) == list(range(r1))
        print("  %s: %d picks in %d passes" % (what, len(full.pick), full.n_passes))
        if bad:  # a NaN row is picked when its index comes up among the +inf rows: row 0 covers nothing, so row 1 is next at +inf, and
            # then the other NaN row, the one row that row 1 does not cover
            assert full.pick[:3].tolist() == [0, 1, r1 // 2] and np.all(full.pick_radius[:3] == INF) and np.all(full.pick_parent[:3] == NOISE)
            assert np.isfinite(full.pick_radius[3:]).all()
        if r1 > 12 and not bad:  # the duplicated row: the later of the two is picked at +0
            assert full.pick_radius[full.pick.tolist().index(7)] == 0.0 or full.pick_radius[full.pick.tolist().index(3)] == 0.0
        # max_picks, and the prefix property between two of them
        by_k = {}
        for k in (1, 2, 33, 257):
            by_k[k] = run(rs, what, max_picks=k)
            check(by_k[k], farthest_first_ref(G, max_picks=k), (what, "max_picks", k))
        assert same_bits([x[:min(33, r1)] for x in by_k[257][:3]], by_k[33][:3]), (what, "prefix")
        assert same_bits([x[:min(257, r1)] for x in full[:3]], by_k[257][:3]), (what, "prefix of the full order")
        # cover_radius: three quantiles of the distances that are finite, zero, +inf
        finite = G[np.isfinite(G) & ~np.eye(r1, dtype=bool)]
        radii = [float(np.quantile(finite, q)) for q in (0.01, 0.05, 0.25)] if finite.size else []
        for R in radii + [0.0, INF]:
            want = farthest_first_ref(G, cover_radius=R)
            got = run(rs, what, cover_radius=R)
            check(got, want, (what, "cover_radius", R))
            if R < INF:  # property 4
                assert np.all((got.rep_dist <= R) | (got.rep_dist == INF)) and np.all(got.pick_radius > R), (what, R)
            if R in radii[1:] and r1 >= 130:  # the case is not trivial
                assert 1 < len(got.pick) < r1, (what, R, len(got.pick))
        # seeds: the last row; the first 40 picks of the full run (property 3)
        for R in [-1.0] + radii[1:2]:
            got = run(rs, what, seeds=[r1 - 1], cover_radius=R)
            check(got, farthest_first_ref(G, seeds=[r1 - 1], cover_radius=R), (what, "seed", R))
        k = min(40, r1)
        again = run(rs, what, seeds=full.pick[:k])
        check(again, want_full, (what, "continued"))
        assert same_bits(again, full)
        check(run(rs, what, seeds=full, max_picks=r1), want_full, (what, "every pick a seed"))
        check(run(rs, what, seeds=full.pick[:k], max_picks=k), farthest_first_ref(G, max_picks=k), (what, "seeds alone"))
    finally:
        rs.free()


@pytest.mark.parametrize("kind,p", KINDS, ids=KIND_IDS)
def test_5000_rows(kpop, oracle, kind, p):
    """300 picks of 5,000 rows and a cover at a radius, held to property 5 through the rows' distances to the picks on the vector pipe:
    the r1 x r1 matrix is not formed"""
    r1, d = 5000, 16
    m, metric = operands(oracle, r1, d)
    for normalize in (True, False):
        what = (r1, d, kind, normalize)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            got = run(rs, what, max_picks=300)
            n = len(got.pick)
            assert n == 300 and len(set(got.pick.tolist())) == n and got.pick[0] == 0
            print("  %s: %d picks in %d passes, %.3f passes a pick" % (what, n, got.n_passes, got.n_passes / n))
            assert 1 <= got.n_passes <= n
            assert got.pick_radius[0] == INF and np.all(got.pick_radius[2:] <= got.pick_radius[1:-1])  # property 1
            Dp = on_the_vector_pipe(rs, m[got.pick]) + 0.0  # [pick t][row i]
            picked = np.zeros(r1, dtype=bool)
            picked[got.pick] = True
            least = Dp.min(axis=0)
            first = got.pick[np.argmax(Dp == least[None, :], axis=0)]
            assert np.array_equal(got.rep_dist[~picked], least[~picked]) and np.array_equal(got.rep_of[~picked], first[~picked]), what  # property 5
            assert np.array_equal(got.rep_of[picked], np.flatnonzero(picked)) and not got.rep_dist[picked].any(), what
            # a pick's radius and parent: the same, over the picks before it
            for t in (1, 2, 57, 299):
                col = Dp[:t, got.pick[t]]
                assert got.pick_radius[t] == col.min() and got.pick_parent[t] == got.pick[int(np.argmax(col == col.min()))], (what, t)
            # the next pick's radius bounds every row: the prefix is a cover at that radius
            assert got.rep_dist.max() <= got.pick_radius[-1], what
            # a cover at the radius of pick 150: the picks before the radius fell to it (properties 2 and 4)
            R = float(got.pick_radius[150])
            cut = run(rs, what, cover_radius=R)
            k = len(cut.pick)
            assert 1 < k <= 150 and np.all(got.pick_radius[:k] > R) and got.pick_radius[k] <= R, (what, k)
            assert same_bits([x[:k] for x in got[:3]], cut[:3]), what
            assert np.all(cut.rep_dist <= R), what
            assert 1 <= cut.n_passes <= k
        finally:
            rs.free()


def test_grown_set(kpop, oracle):
    """a run, 100 rows appended, and the traversal continued from the old picks as seeds: the reference's on the grown matrix"""
    r1, d = 1000, 16
    m, metric = operands(oracle, r1, d)
    for kind, p, normalize in ((0, 2.0, True), (1, 2.0, False)):
        D = oracle_matrix(oracle, r1, d, kind, p, normalize)
        rs = kpop.RefSet(m[:900], metric, kind, p, normalize, capacity=r1)
        try:
            old = run(rs, "before", max_picks=50)
            check(old, farthest_first_ref(D[:900, :900], max_picks=50), ("before", kind))
            rs.append(m[900:])
            grown = run(rs, "grown", max_picks=120, seeds=old)
            check(grown, farthest_first_ref(D, max_picks=120, seeds=old.pick), ("grown", kind))
            assert np.array_equal(grown.pick[:50], old.pick) and np.any(grown.pick[50:] >= 900)
        finally:
            rs.free()


def raw(rs, max_picks, cover_radius, seeds, outputs, n_picks=True):
    """kpop_farthest_first through ctypes; outputs: six arrays or None each (pick, pick_radius, pick_parent, rep_of, rep_dist, n_passes)"""
    from kpop_amd import _lib
    n = C.c_uint32(12345)
    seeds = np.asarray(seeds, dtype=np.uint32)
    ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_uint32)) for a in outputs]
    rc = _lib.load().kpop_farthest_first(rs.handle, max_picks, cover_radius, seeds.ctypes.data_as(C.POINTER(C.c_uint32)) if len(seeds) else None, len(seeds),
                                         C.byref(n) if n_picks else None, *ptr)
    return rc, n.value


def test_arguments(kpop, oracle):
    r1, d = 130, 9
    m, metric = operands(oracle, r1, d)
    D = oracle_matrix(oracle, r1, d, 0, 2.0, True)
    want = farthest_first_ref(D, max_picks=20)
    rs = kpop.RefSet(m, metric, 0, 2.0, True)
    try:
        for kw in (dict(cover_radius=float("nan")), dict(seeds=[r1]), dict(seeds=[3, 5, 3]), dict(seeds=[1, 2, 3], max_picks=2)):
            with pytest.raises(kpop.KPopError) as e:
                rs.farthest_first(**kw)
            assert e.value.code == ERR_INVALID, kw
        assert raw(rs, 20, -1.0, [], [None] * 6, n_picks=False)[0] == ERR_INVALID  # n_picks is the one pointer that must be there
        # every other output may be NULL: all of them, and each alone
        assert raw(rs, 20, -1.0, [], [None] * 6) == (0, 20)
        for k in range(6):
            out = [np.full(20, 77, dtype=np.uint32), np.full(20, 77.0), np.full(20, 77, dtype=np.uint32), np.full(r1, 77, dtype=np.uint32), np.full(r1, 77.0),
                   np.full(1, 77, dtype=np.uint32)]
            given = [a if j == k else None for j, a in enumerate(out)]
            assert raw(rs, 20, -1.0, [], given) == (0, 20)
            if k < 5:
                assert np.array_equal(out[k], want[k]), k
            else:
                assert 1 <= out[5][0] <= 20
        # max_picks = 0: nothing is picked and nothing covers
        none = rs.farthest_first(max_picks=0)
        assert len(none.pick) == 0 and np.all(none.rep_of == NOISE) and np.all(none.rep_dist == INF) and none.n_passes == 0
        check(kpop.distance_farthest_first(m, metric, 0, 2.0, True, max_picks=20), want, "distance_farthest_first")
        check(kpop.distance_farthest_first(m, metric, 0, 2.0, True, max_picks=20, seeds=want.pick[:3]), want, "distance_farthest_first, seeds")
    finally:
        rs.free()
    with pytest.raises(kpop.KPopError) as e:  # a freed set holds no handle any more
        rs.farthest_first()
    assert e.value.code == ERR_INVALID
    # an empty set
    empty = kpop.RefSet(np.zeros((0, d)), metric, 0, 2.0, True)
    try:
        got = empty.farthest_first()
        assert len(got.pick) == 0 and len(got.rep_of) == 0 and got.n_passes == 0
        with pytest.raises(kpop.KPopError):
            empty.farthest_first(seeds=[0], max_picks=4)
    finally:
        empty.free()
    got = kpop.distance_farthest_first(np.zeros((0, d)), metric, 0, 2.0, True)
    assert len(got.pick) == 0 and len(got.rep_dist) == 0


def test_device_form_on_a_stream(kpop, oracle):
    """kpop_dev_farthest_first on a stream of the caller's, its workspace of exactly the stated size with guard words behind it, its
    outputs with guard words behind them: what the host form gives, the guards untouched; twice on the same buffers"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    GUARD = 8
    for r1, d, kind, p, normalize, kw in ((1000, 16, 0, 2.0, True, dict(max_picks=257, cover_radius=-1.0)), (1000, 16, 1, 2.0, False, dict(max_picks=1000, cover_radius=None)),
                                          (130, 9, 2, P_MINK, True, dict(max_picks=33, cover_radius=-1.0))):
        m, metric = operands(oracle, r1, d)
        rs = kpop.RefSet(m, metric, kind, p, normalize)
        try:
            if kw["cover_radius"] is None:
                kw["cover_radius"] = float(rs.farthest_first(max_picks=60).pick_radius[-1])
            seeds = np.array([r1 - 1, 5], dtype=np.uint32)
            want = rs.farthest_first(seeds=seeds, **kw)  # the host form
            k = min(kw["max_picks"], r1)
            assert 2 < len(want.pick) <= k
            need = api.dev_farthest_first_workspace_bytes(rs, kw["max_picks"])
            assert 0 < need <= 64 * 1024 + 12 * r1 + 16 * k + 7 * 256  # O(r1 + max_picks): no copy of the rows
            work = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
            pick, parent, rep_of = (torch.full((n + GUARD,), -3, dtype=torch.int32, device=dev) for n in (k, k, r1))
            radius, rep_dist = (torch.full((n + GUARD,), -3.0, dtype=torch.float64, device=dev) for n in (k, r1))
            counts = torch.full((2 + GUARD,), -3, dtype=torch.int32, device=dev)
            d_seeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_farthest_first(rs, kw["max_picks"], kw["cover_radius"], work.data_ptr(), counts.data_ptr(), pick.data_ptr(), radius.data_ptr(),
                                           parent.data_ptr(), rep_of.data_ptr(), rep_dist.data_ptr(), d_seeds.data_ptr(), len(seeds), stream=stream.cuda_stream)
            stream.synchronize()
            n, n_passes = (int(x) for x in counts.cpu().numpy()[:2])
            assert n == len(want.pick) and n_passes == want.n_passes
            got = (pick.cpu().numpy().view(np.uint32), radius.cpu().numpy(), parent.cpu().numpy().view(np.uint32), rep_of.cpu().numpy().view(np.uint32),
                   rep_dist.cpu().numpy())
            assert same_bits([got[0][:n], got[1][:n], got[2][:n], got[3][:r1], got[4][:r1]], want), (r1, kind)
            # the entries behind the picks made, and the guard words behind every array
            for a, size in zip(got, (k, k, k, r1, r1)):
                assert np.all(a[size:] == (-3.0 if a.dtype == np.float64 else np.uint32(0xFFFFFFFD))), (r1, kind)
            for a in got[:3]:
                assert np.all(a[n:k] == (-3.0 if a.dtype == np.float64 else np.uint32(0xFFFFFFFD))), (r1, kind)
            assert np.all(counts.cpu().numpy()[2:] == -3) and np.all(work.cpu().numpy()[need:] == 0xA5), (r1, kind)
            # without any output but the counts
            api.dev_farthest_first(rs, kw["max_picks"], kw["cover_radius"], work.data_ptr(), counts.data_ptr(), d_seeds=d_seeds.data_ptr(), n_seeds=len(seeds),
                                   stream=stream.cuda_stream)
            stream.synchronize()
            assert counts.cpu().numpy()[:2].tolist() == [n, n_passes]
        finally:
            rs.free()
