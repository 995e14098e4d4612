"""The resident reference set (kpop_refset, include/kpop_hip.h): a first operand prepared once and queried many times.

The contract: on every route the unprepared call can take, and under every kpop_tune setting, a call on a set returns the arrays
of kpop_distance_rowwise / kpop_distance_summary on the same rows BIT FOR BIT (np.array_equal on every returned array), and
those agree with the oracle within the tolerances tests/test_gpu_distance.py holds the unprepared calls to."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_MINK = 1.5
KINDS = [(0, 2.0), (1, 2.0), (2, P_MINK)]
ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -2, -3


def same(got, want, what=""):
    """every returned array, bit for bit"""
    if isinstance(got, np.ndarray):
        got, want = (got,), (want,)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        assert np.array_equal(a, b, equal_nan=True), (what, i, int(np.sum(a != b)))


def same_summary(got, want, what=""):
    """(stats, n, idx, dist, z) bit for bit.  A row's neighbour slots beyond min(n, max_neighbours) are not part of the answer -- no
    call writes them, the host calls hand back whatever their scratch held -- so they are cleared in both before every array is compared"""
    def cleared(res):
        st, n, idx, dist, z = (np.array(a) for a in res)
        beyond = np.arange(idx.shape[1])[None, :] >= np.minimum(n, idx.shape[1])[:, None]
        idx[beyond], dist[beyond], z[beyond] = 0, 0.0, 0.0
        return st, n, idx, dist, z
    same(cleared(got), cleared(want), what)


def rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=True):
    m1 = np.round(rng.normal(size=(r1, d)), 1) if grid else rng.normal(size=(r1, d))
    if r1 > 12:
        m1[7] = m1[3]  # a duplicated row: a tie in every query row's distances
        m1[9] = 0.0  # a zero row: its norm is replaced by 1 (lib/Matrix.ml:67)
    return m1


def summary_vs_oracle(oracle, res, m1, m2, metric, kind, p, normalize, keep, cap, order_stats_exact):
    """tests/test_gpu_distance.py: test_distance_summary_vs_oracle / _large_reference_set / _on_the_matrix_cores"""
    st_o, offs, idx_o, dist_o, z_o = oracle.distance_summary(m1, m2, metric, kind, p, normalize, keep)
    st, n, idx, dist, z = res
    if order_stats_exact:
        np.testing.assert_allclose(st[:, :2], st_o[:, :2], rtol=1e-10, atol=1e-13)
        assert np.array_equal(st[:, 2:], st_o[:, 2:])  # median and MAD: order statistics
    else:
        np.testing.assert_allclose(st, st_o, rtol=1e-10, atol=1e-13)
    for j in range(m2.shape[0]):
        a, b = int(offs[j]), int(offs[j + 1])
        assert n[j] == b - a
        m = min(int(n[j]), cap)
        if kind != 2:
            assert idx[j, :m].tolist() == idx_o[a:a + m].tolist()
            assert np.array_equal(dist[j, :m], dist_o[a:a + m])
        else:
            np.testing.assert_allclose(dist[j, :m], dist_o[a:a + m], rtol=1e-11)
        np.testing.assert_allclose(z[j, :m], z_o[a:a + m], rtol=1e-8, atol=1e-9)


# route, r1, d, r2, [(keep, max_neighbours)], kinds, tune, order statistics exact against the oracle
SUMMARY_ROUTES = [
    ("wave", 65, 64, 40, [(2, 65)], KINDS, None, False),
    ("block", 1000, 16, 40, [(5, 1000)], KINDS, None, False),
    ("large", 5000, 16, 12, [(2, 2048)], KINDS, None, False),
    ("large300", 20000, 16, 12, [(300, 2048)], KINDS, None, False),
    ("mfma64", 70001, 64, 9, [(1, 512), (300, 512)], KINDS, None, True),
    ("mfma200", 70001, 200, 9, [(1, 512), (300, 512)], KINDS, None, True),
    ("fused", 140000, 16, 6, [(2, 8)], KINDS[2:], ("summary2", 2), False),
    ("sampled", 270000, 16, 6, [(2, 8)], KINDS[2:], None, False),
]


@pytest.mark.parametrize("route,r1,d,r2,keeps,kinds,tune,exact", SUMMARY_ROUTES, ids=[r[0] for r in SUMMARY_ROUTES])
def test_summary_on_every_route(kpop, oracle, route, r1, d, r2, keeps, kinds, tune, exact):
    from kpop_amd import api
    rng = np.random.RandomState(r1 + d)
    grid = d <= 16
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid)
    m2 = np.round(rng.normal(size=(r2, d)), 1) if grid else rng.normal(size=(r2, d))
    m2[min(5, r2 - 1)] = m1[11]  # a zero distance
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    if tune:
        api.tune(*tune)
    try:
        for kind, p in kinds:
            for normalize in (True, False):
                rs = kpop.RefSet(m1, metric, kind, p, normalize)
                try:
                    for keep, cap in keeps:
                        want = kpop.distance_summary(m1, m2, metric, kind, p, normalize, keep, max_neighbours=cap)
                        got = rs.distance_summary(m2, keep, max_neighbours=cap)
                        same_summary(got, want, (route, kind, normalize, keep))
                        summary_vs_oracle(oracle, got, m1, m2, metric, kind, p, normalize, keep, cap, exact and kind != 2)
                finally:
                    rs.free()
    finally:
        if tune:
            api.tune(tune[0], 1)


ROWWISE_ROUTES = [("staging", 65, 3000, 64, KINDS), ("mfma256", 300, 60000, 256, KINDS[:2]), ("mfma1635", 1636, 2000, 1635, KINDS[:2]),
                  ("copies", 130, 129, 100, KINDS[2:])]


@pytest.mark.parametrize("route,r1,r2,d,kinds", ROWWISE_ROUTES, ids=[r[0] for r in ROWWISE_ROUTES])
def test_rowwise_on_every_route(kpop, oracle, route, r1, r2, d, kinds):
    rng = np.random.RandomState(r1 * 7 + r2 + d)
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=False)
    m2 = rng.normal(size=(r2, d))
    m2[1] = 0.0
    m2[2] = m1[0]
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    sub = np.unique(np.concatenate([np.arange(min(r2, 64)), rng.randint(0, r2, size=100)]))  # (the oracle on a sample of a long second operand)
    for kind, p in kinds:
        for normalize in (True, False):
            rs = kpop.RefSet(m1, metric, kind, p, normalize)
            try:
                got = rs.distance_rowwise(m2)
            finally:
                rs.free()
            want = kpop.distance_rowwise(m1, m2, metric, kind, p, normalize)
            same(got, want, (route, kind, normalize))
            ref = oracle.distance_rowwise(m1, m2[sub], metric, kind, p, normalize)
            g = got[sub]
            err = np.abs(g - ref) / np.maximum(np.abs(ref), 1e-300)
            err[ref == g] = 0.0
            if route.startswith("mfma"):  # test_distance_rowwise_on_the_matrix_cores
                assert err.max() <= 1e-12, (route, kind, normalize, err.max())
            elif kind == 2:  # test_distance_rowwise_vs_oracle
                assert np.max(np.abs(g - ref)) <= 1e-11 * max(np.max(np.abs(ref)), 1e-300)
            else:
                assert np.array_equal(g, ref)


def test_one_set_many_batches(kpop, oracle):
    """batches of 1, 9 and 640 rows, rowwise and summary interleaved, twice round: nothing is sized by the call before"""
    rng = np.random.RandomState(11)
    r1, d = 70001, 64
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=False)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    batches = {r2: rng.normal(size=(r2, d)) for r2 in (1, 9, 640)}
    for kind, normalize in ((0, True), (1, False)):
        want_s = {r2: kpop.distance_summary(m1, b, metric, kind, 2.0, normalize, 300, max_neighbours=512) for r2, b in batches.items()}
        want_r = {r2: kpop.distance_rowwise(m1, b, metric, kind, 2.0, normalize) for r2, b in batches.items()}
        rs = kpop.RefSet(m1, metric, kind, 2.0, normalize)
        try:
            for turn in range(2):
                for r2 in (1, 640, 9):
                    same(rs.distance_rowwise(batches[r2]), want_r[r2], ("rowwise", kind, turn, r2))
                    same_summary(rs.distance_summary(batches[r2], 300, max_neighbours=512), want_s[r2], ("summary", kind, turn, r2))
        finally:
            rs.free()
    summary_vs_oracle(oracle, want_s[9], m1, batches[9], metric, 1, 2.0, False, 300, 512, True)


def test_tune_settings_between_calls_on_one_set(kpop, oracle):
    """every form of the matrix-core summary on ONE set, one after the other: the set hands each route the pieces that route would
    have computed (the two arithmetics of the scaled sums of squares among them)"""
    from kpop_amd import api
    rng = np.random.RandomState(12)
    r1, d = 70001, 64
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=False)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    m9, m640 = rng.normal(size=(9, d)), rng.normal(size=(640, d))
    m9[1] = m1[5]
    defaults = {"summary_mfma": 1, "summary_sample": 1, "summary_rawref": 1, "summary_lanes": 1}
    settings = [("summary_mfma", 1, m9), ("summary_mfma", 2, m9), ("summary_mfma", 0, m9), ("summary_sample", 0, m9), ("summary_sample", 1, m9),
                ("summary_rawref", 0, m9), ("summary_rawref", 1, m9), ("summary_lanes", 2, m640), ("summary_mfma", 2, m9), ("summary_mfma", 1, m9)]
    try:
        for kind, normalize in ((0, True), (0, False), (1, True)):
            rs = kpop.RefSet(m1, metric, kind, 2.0, normalize)
            try:
                for key, value, m2 in settings:
                    api.tune(key, value)
                    want = kpop.distance_summary(m1, m2, metric, kind, 2.0, normalize, 300, max_neighbours=512)
                    got = rs.distance_summary(m2, 300, max_neighbours=512)
                    api.tune(key, defaults[key])
                    same_summary(got, want, (kind, normalize, key, value))
                    if key == "summary_mfma" and value == 1 and m2 is m9:
                        summary_vs_oracle(oracle, got, m1, m2, metric, kind, 2.0, normalize, 300, 512, True)
            finally:
                rs.free()
    finally:
        for key, value in defaults.items():
            api.tune(key, value)


def test_append(kpop, oracle):
    """3,000 rows, then 5,000, then 70,001 (across 4,096 and 65,536), then 75,000 (the matrix-core route's scalars, copy and sample
    extended, not made afresh): each size answers as a fresh set over the same rows and as the unprepared call; a set created empty
    and filled likewise; one append too many leaves the set as it was"""
    rng = np.random.RandomState(13)
    d, r2 = 16, 9
    full = rows_with_a_zero_and_a_duplicate(rng, 75000, d)
    m2 = np.round(rng.normal(size=(r2, d)), 1)
    m2[5] = full[11]
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    for kind, p, normalize in ((0, 2.0, True), (2, P_MINK, True), (1, 2.0, False)):
        rs = kpop.RefSet(full[:3000], metric, kind, p, normalize, capacity=80000)
        empty = kpop.RefSet(np.zeros((0, d)), metric, kind, p, normalize, capacity=75000)
        try:
            assert empty.info()["r1"] == 0 and empty.info()["capacity"] == 75000
            st, n, _, _, _ = empty.distance_summary(m2, 2, max_neighbours=8)
            same((st, n), kpop.distance_summary(np.zeros((0, d)), m2, metric, kind, p, normalize, 2, max_neighbours=8)[:2], "empty")
            at = 0
            for size in (3000, 5000, 70001, 75000):
                if size > 3000:
                    rs.append(full[rs.info()["r1"]:size])
                empty.append(full[at:size])
                at = size
                assert rs.info()["r1"] == size == empty.info()["r1"]
                cap = min(size, 512)
                want = kpop.distance_summary(full[:size], m2, metric, kind, p, normalize, 300, max_neighbours=cap)
                fresh = kpop.RefSet(full[:size], metric, kind, p, normalize)
                try:
                    same_summary(fresh.distance_summary(m2, 300, max_neighbours=cap), want, ("fresh", kind, size))
                finally:
                    fresh.free()
                same_summary(rs.distance_summary(m2, 300, max_neighbours=cap), want, ("appended", kind, size))
                same_summary(empty.distance_summary(m2, 300, max_neighbours=cap), want, ("filled", kind, size))
                if size == 5000:
                    same(rs.distance_rowwise(m2), kpop.distance_rowwise(full[:size], m2, metric, kind, p, normalize), ("rowwise", kind, size))
                    summary_vs_oracle(oracle, want, full[:size], m2, metric, kind, p, normalize, 300, cap, False)
            with pytest.raises(kpop.KPopError) as e:
                rs.append(full[:10000])  # 85,000 rows
            assert e.value.code == ERR_CAPACITY
            assert rs.info()["r1"] == 75000
            same_summary(rs.distance_summary(m2, 300, max_neighbours=min(size, 512)), want, ("after the refused append", kind))
        finally:
            rs.free()
            empty.free()


def test_long_lists(kpop, oracle):
    """keep_at_most = 0 against 5,000 rows: every neighbour of every row, the lists beyond 2,048 completed on the host as
    kpop_distance_summary's are"""
    rng = np.random.RandomState(14)
    r1, d, r2 = 5000, 16, 3
    m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d)
    m2 = np.round(rng.normal(size=(r2, d)), 1)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    rs = kpop.RefSet(m1, metric, 0, 2.0, True)
    try:
        got = rs.distance_summary(m2, 0)
    finally:
        rs.free()
    want = kpop.distance_summary(m1, m2, metric, 0, 2.0, True, 0)
    assert got[1].tolist() == [r1] * r2 and got[2].shape == (r2, r1)
    same_summary(got, want, "long lists")
    summary_vs_oracle(oracle, got, m1, m2, metric, 0, 2.0, True, 0, r1, False)


def test_device_entry_points(kpop, oracle):
    """a set wrapped over the caller's tensor, calls on a stream of the caller's; the workspace holds the query side alone"""
    import torch
    from kpop_amd import api
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(15)
    d, r2, keep, cap = 200, 9, 300, 512
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    t_metric = torch.from_numpy(metric).to(dev)
    m2 = rng.normal(size=(r2, d))
    t_m2 = torch.from_numpy(m2).to(dev)
    stream = torch.cuda.Stream(device=dev)
    ws = {}
    for r1 in (5000, 70001):
        m1 = rows_with_a_zero_and_a_duplicate(rng, r1, d, grid=False)
        t_m1 = torch.from_numpy(m1).to(dev)
        before = t_m1.clone()
        torch.cuda.synchronize()
        rs = kpop.RefSet.wrap(t_m1.data_ptr(), r1, d, t_metric.data_ptr(), 0, 2.0, True, stream=stream.cuda_stream, keep=(t_m1, t_metric))
        try:
            assert rs.info() == dict(rs.info(), r1=r1, n_dims=d, capacity=r1)
            with pytest.raises(kpop.KPopError) as e:
                rs.append(m1[:1])  # borrowed rows do not grow
            assert e.value.code == ERR_INVALID
            ws[r1] = api.dev_refset_workspace_bytes(rs, r2)
            work = torch.empty(ws[r1], dtype=torch.uint8, device=dev)
            st = torch.zeros((r2, 4), dtype=torch.float64, device=dev)
            n = torch.zeros(r2, dtype=torch.int32, device=dev)
            idx = torch.zeros((r2, cap), dtype=torch.int32, device=dev)
            dist = torch.zeros((r2, cap), dtype=torch.float64, device=dev)
            z = torch.zeros((r2, cap), dtype=torch.float64, device=dev)
            out = torch.zeros((r2, r1), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for _ in range(2):
                    api.dev_refset_distance_summary(rs, t_m2.data_ptr(), r2, work.data_ptr(), st.data_ptr(), n.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                                                    z.data_ptr(), keep, cap, stream=stream.cuda_stream)
                    api.dev_refset_distance_rowwise(rs, t_m2.data_ptr(), r2, work.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            got = (st.cpu().numpy(), n.cpu().numpy().view(np.uint32), idx.cpu().numpy().view(np.uint32), dist.cpu().numpy(), z.cpu().numpy())
            want = kpop.distance_summary(m1, m2, metric, 0, 2.0, True, keep, max_neighbours=cap)
            same_summary(got, want, ("device summary", r1))
            same(out.cpu().numpy(), kpop.distance_rowwise(m1, m2, metric, 0, 2.0, True), ("device rowwise", r1))
            summary_vs_oracle(oracle, got, m1, m2, metric, 0, 2.0, True, keep, cap, r1 > 65536)
            # the per-row scalars, a sample, and the divided copy the rowwise call of 9 rows made: all of it reported, no second copy of the rows
            assert r1 * d * 8 <= rs.info()["device_bytes"] < r1 * d * 8 + 80 * r1 + (64 << 20)
        finally:
            rs.free()
        assert torch.equal(t_m1, before)  # the caller's rows: borrowed, intact, still the caller's
    assert ws[5000] == ws[70001]
    assert 100 * ws[70001] < api.dev_distance_workspace_bytes(70001, r2, d)


def test_pipeline_against_a_database(kpop, oracle):
    """OUT_SUMMARY of a streaming pipeline whose classes are 70,001 rows, the batch cut into chunks: what distance_summary gives
    for the twisted rows against those rows"""
    k, d, n_reads, read_len = 6, 16, 700, 120
    col_hash = oracle.enumerate_kmers(k)
    T = oracle.synth_twister(5, d, col_hash)
    tw = kpop.Twister.load(T, col_hash, k)
    rng = np.random.RandomState(16)
    classes = rows_with_a_zero_and_a_duplicate(rng, 70001, d, grid=False) * 0.05
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    bases, offsets = oracle.synth_reads(9, n_reads, read_len)
    pipe = kpop.Pipeline(tw, classes, metric, outputs=kpop.OUT_TWISTED | kpop.OUT_SUMMARY, keep_at_most=2, max_neighbours=8, chunk_reads=200)
    try:
        out = pipe.run(bases, offsets)
        assert pipe.stats()["chunks"] >= 3
    finally:
        pipe.close()
        tw.free()
    twisted = np.array(out["twisted"])
    want = kpop.distance_summary(classes, twisted, metric, 0, 2.0, True, 2, max_neighbours=8)
    same_summary((np.array(out["stats"]), np.array(out["n_neighbours"]), np.array(out["nb_index"]), np.array(out["nb_distance"]), np.array(out["nb_z"])), want,
                 "pipeline")
    pick = np.arange(0, n_reads, 100)
    summary_vs_oracle(oracle, tuple(a[pick] for a in want), classes, twisted[pick], metric, 0, 2.0, True, 2, 8, True)


def test_errors(kpop, oracle):
    from kpop_amd import _lib
    lib = _lib.load()
    f64p = C.POINTER(C.c_double)
    m1 = np.ones((4, 3))
    metric = np.ones(3)
    h = C.c_void_p()

    def create(rows=m1, r1=4, n_dims=3, met=metric, kind=0, p=2.0, cap=0, out=h):
        return lib.kpop_refset_create(rows.ctypes.data_as(f64p) if rows is not None else None, r1, n_dims,
                                      met.ctypes.data_as(f64p) if met is not None else None, kind, p, 1, cap, C.byref(out) if out is not None else None)

    def refused(rc, code):
        assert rc == code, rc
        assert lib.kpop_last_error()  # (says what was wrong)

    refused(create(n_dims=0), ERR_INVALID)
    refused(create(kind=7), ERR_INVALID)
    refused(create(kind=2, p=-1.0), ERR_INVALID)
    refused(create(rows=None), ERR_INVALID)
    refused(create(met=None), ERR_INVALID)
    refused(create(out=None), ERR_INVALID)
    refused(create(cap=2), ERR_INVALID)  # room for fewer rows than it is given
    refused(create(rows=np.ones((1, 32768)), r1=1, n_dims=32768, met=np.ones(32768)), ERR_UNSUPPORTED)
    refused(lib.kpop_dev_refset_wrap(None, 4, 3, None, 0, 2.0, 1, None, C.byref(h)), ERR_INVALID)
    refused(lib.kpop_refset_append(None, m1.ctypes.data_as(f64p), 1), ERR_INVALID)
    refused(lib.kpop_refset_info(None, None, None, None, None), ERR_INVALID)
    assert create() == 0 and h.value
    try:
        out = np.zeros((2, 4))
        refused(lib.kpop_refset_distance_rowwise(h, None, 2, out.ctypes.data_as(f64p)), ERR_INVALID)
        refused(lib.kpop_refset_distance_summary(h, m1.ctypes.data_as(f64p), 2, 2, 8, None, None, None, None, None), ERR_INVALID)
        refused(lib.kpop_refset_append(h, None, 1), ERR_INVALID)
        refused(lib.kpop_refset_append(h, m1.ctypes.data_as(f64p), 1), ERR_CAPACITY)
        refused(lib.kpop_dev_refset_distance_rowwise(h, None, 2, None, None, None), ERR_INVALID)
        assert lib.kpop_refset_distance_rowwise(h, m1.ctypes.data_as(f64p), 2, out.ctypes.data_as(f64p)) == 0
        assert np.array_equal(out, np.zeros((2, 4)))
    finally:
        assert lib.kpop_refset_free(h) == 0


def test_a_set_belongs_to_its_device_slot(kpop, oracle):
    """two slots on the one GPU (as tests/test_gpu_multi.py makes them): a set made on slot 0 is refused from slot 1"""
    m1, m2, metric = np.ones((4, 3)), np.zeros((2, 3)), np.ones(3)
    kpop.init_devices([0, 0])
    try:
        rs = kpop.RefSet(m1, metric)
        try:
            kpop.use_device(1)
            for call in (lambda: rs.distance_rowwise(m2), lambda: rs.distance_summary(m2), lambda: rs.append(m1)):
                with pytest.raises(kpop.KPopError) as e:
                    call()
                assert e.value.code == ERR_INVALID and "slot" in str(e.value)
            kpop.use_device(0)
            same(rs.distance_rowwise(m2), kpop.distance_rowwise(m1, m2, metric), "back on its slot")
        finally:
            kpop.use_device(0)
            rs.free()
    finally:
        kpop.init(0)
