"""Rowwise distances against a class set through class_set.hip's kernel (a row of the second operand in a lane's registers, the
class values as scalar operands) must be, bit for bit, what the tiled kernel gives (kpop_tune("class_set", 0)) and, for the
euclidean and the cosine distance, what the oracle gives: the same IEEE operations in the same order (lib/Space.ml:150-205,
lib/Matrix.ml:191-266).  "new" is class_set = 2 (every eligible shape), "old" is class_set = 0; the default (1) takes the new
path from THRESHOLD rows of the second operand on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EUCLIDEAN, COSINE, MINKOWSKI = 0, 1, 2
# mirrors kClassSetMinRows, kpop_amd/csrc/class_set.hip ("constexpr uint32_t kClassSetMinRows")
THRESHOLD = 128


class class_set:
    """with class_set(v): the knob at v, back at its default afterwards"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from kpop_amd import api
        api.tune("class_set", self.value)

    def __exit__(self, *exc):
        from kpop_amd import api
        api.tune("class_set", 1)
        return False


def operands(r1, r2, d, seed, decimals=None):
    """random rows with, where the shape has room for them: an all-zero row in each operand (norm 0 -> 1), a row of the second
    operand equal to a class (distance exactly 0), and two identical classes"""
    rng = np.random.RandomState(seed)
    m1, m2 = rng.normal(size=(r1, d)), rng.normal(size=(r2, d))
    if decimals is not None:
        m1, m2 = np.round(m1, decimals), np.round(m2, decimals)
    if r1 >= 3:
        m1[1] = m1[0]
    if r1 >= 2:
        m1[r1 - 1] = 0.0
    m2[0] = 0.0
    if r2 >= 2:
        m2[r2 - 1] = m1[0]
    return m1, m2


SHAPES = [(1, 1, 1), (1, 64, 8), (5, 63, 9), (3, 65, 1), (17, 65, 33), (65, 129, 63), (65, 300, 64), (66, 200, 64), (127, 130, 64),
          (4, 1000, 16)]


@pytest.mark.parametrize("kind", [EUCLIDEAN, COSINE])
@pytest.mark.parametrize("r1,r2,d", SHAPES)
def test_bits_small_shapes(kpop, oracle, kind, r1, r2, d):
    """class counts that are no multiple of the four wavefronts or of the classes a wavefront carries at once, last blocks of 1, 2
    and 63 rows, dimensions off the group of 8, both ends of the eligible ranges"""
    m1, m2 = operands(r1, r2, d, r1 * 7 + r2 + d)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    for normalize in (True, False):
        want = oracle.distance_rowwise(m1, m2, metric, kind, 2.0, normalize)
        with class_set(0):
            old = kpop.distance_rowwise(m1, m2, metric, kind, 2.0, normalize)
        with class_set(2):
            new = kpop.distance_rowwise(m1, m2, metric, kind, 2.0, normalize)
        assert new.shape == (r2, r1)
        assert np.array_equal(new, old), (kind, normalize)
        assert np.array_equal(new, want), (kind, normalize)
        if r2 >= 2:
            assert new[r2 - 1, 0] == 0.0  # the row that is a class


@pytest.mark.parametrize("kind", [EUCLIDEAN, COSINE])
def test_non_finite_and_extreme_rows(kpop, oracle, kind):
    r1, r2, d = 65, 130, 64
    m1, m2 = operands(r1, r2, d, 77 + kind)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    assert np.all(metric > 0) and np.all(np.isfinite(metric))  # (Inf * 0 would make NaNs of its own)
    j_nan, j_inf, i_nan, j_big, j_small = 5, 70, 33, 100, 129
    m2[j_nan, 17] = np.nan
    m2[j_inf, 40] = np.inf
    m1[i_nan, 63] = np.nan
    m2[j_big] *= 1e300
    m2[j_small] = np.random.RandomState(3).normal(size=d) * 1e-300
    for normalize in (True, False):
        with class_set(0):
            old = kpop.distance_rowwise(m1, m2, metric, kind, 2.0, normalize)
        with class_set(2):
            new = kpop.distance_rowwise(m1, m2, metric, kind, 2.0, normalize)
        assert np.array_equal(new, old, equal_nan=True), (kind, normalize)
        # NaN exactly where an operand held one: the row of the NaN element, the column of the NaN class -- and, when the rows are
        # normalised, the row of the Inf element (its norm is Inf, and Inf /. Inf is NaN; without normalisation its distances are Inf)
        expect = np.zeros((r2, r1), dtype=bool)
        expect[j_nan, :] = True
        expect[:, i_nan] = True
        if normalize:
            expect[j_inf, :] = True
        for name, got in (("old", old), ("new", new)):
            assert np.array_equal(np.isnan(got), expect), (name, kind, normalize, np.argwhere(np.isnan(got) != expect)[:8])
        if not normalize:
            keep = np.arange(r1) != i_nan
            assert np.all(np.isinf(new[j_inf, keep]))


def dev_buffers(m1, m2, metric):
    import torch
    dev = torch.device("cuda", 0)
    return dev, torch.from_numpy(m1).to(dev), torch.from_numpy(m2).to(dev), torch.from_numpy(metric).to(dev)


@pytest.mark.parametrize("kind", [EUCLIDEAN, COSINE])
def test_every_entry_point(kpop, oracle, kind):
    """kpop_dev_distance_rowwise, kpop_dev_distance_rowwise_norms with the norms kpop_dev_row_norms made, and a resident set: each
    through the new path gives the bits of kpop_dev_distance_rowwise through the old one"""
    import torch
    from kpop_amd import _lib, api
    lib = _lib.load()
    r1, r2, d = 65, 3000, 64
    m1, m2 = operands(r1, r2, d, 11 + kind)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    dev, t1, t2, tm = dev_buffers(m1, m2, metric)
    work = torch.empty(api.dev_distance_workspace_bytes(r1, r2, d), dtype=torch.uint8, device=dev)
    outs = [torch.zeros(r2, r1, dtype=torch.float64, device=dev) for _ in range(4)]
    norms = torch.zeros(r1, dtype=torch.float64, device=dev)
    with class_set(0):
        api.dev_distance_rowwise(t1.data_ptr(), r1, t2.data_ptr(), r2, d, tm.data_ptr(), work.data_ptr(), outs[0].data_ptr(), kind=kind)
        torch.cuda.synchronize()
    old = outs[0].cpu().numpy()
    with class_set(2):
        api.dev_distance_rowwise(t1.data_ptr(), r1, t2.data_ptr(), r2, d, tm.data_ptr(), work.data_ptr(), outs[1].data_ptr(), kind=kind)
        api.check(lib.kpop_dev_row_norms(t1.data_ptr(), r1, d, tm.data_ptr(), kind, 2.0, norms.data_ptr(), None))
        api.check(lib.kpop_dev_distance_rowwise_norms(t1.data_ptr(), r1, norms.data_ptr(), t2.data_ptr(), r2, d, tm.data_ptr(), kind, 2.0, 1,
                                                      work.data_ptr(), outs[2].data_ptr(), None))
        torch.cuda.synchronize()
        rs = kpop.RefSet.wrap(t1.data_ptr(), r1, d, tm.data_ptr(), kind, 2.0, True, keep=(t1, tm))
        try:
            work_rs = torch.empty(api.dev_refset_workspace_bytes(rs, r2), dtype=torch.uint8, device=dev)
            api.dev_refset_distance_rowwise(rs, t2.data_ptr(), r2, work_rs.data_ptr(), outs[3].data_ptr())
            torch.cuda.synchronize()
            host = rs.distance_rowwise(m2)
        finally:
            rs.free()
    for name, t in (("rowwise", outs[1]), ("rowwise_norms", outs[2]), ("refset", outs[3])):
        assert np.array_equal(t.cpu().numpy(), old), (name, kind)
    assert np.array_equal(host, old), kind
    assert np.array_equal(old, oracle.distance_rowwise(m1, m2, metric, kind, 2.0, True))


def test_nothing_outside_its_buffers(kpop, oracle):
    """64 sentinel rows behind `out` and 4 KiB of sentinel behind the workspace, at exactly dev_distance_workspace_bytes, stay as
    they were (the last block has 2 rows of its 64)"""
    import torch
    from kpop_amd import api
    r1, r2, d = 65, 130, 64
    m1, m2 = operands(r1, r2, d, 5)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    dev, t1, t2, tm = dev_buffers(m1, m2, metric)
    need = api.dev_distance_workspace_bytes(r1, r2, d)
    for normalize in (True, False):
        want = oracle.distance_rowwise(m1, m2, metric, EUCLIDEAN, 2.0, normalize)
        out = torch.full((r2 + 64, r1), -7.25, dtype=torch.float64, device=dev)
        work = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        with class_set(2):
            api.dev_distance_rowwise(t1.data_ptr(), r1, t2.data_ptr(), r2, d, tm.data_ptr(), work.data_ptr(), out.data_ptr(), normalize=normalize)
            torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:r2], want)
        assert np.all(got[r2:] == -7.25)
        assert np.all(work[need:].cpu().numpy() == 0xA5)


def test_two_streams_at_once(kpop, oracle):
    """the same call on two non-default streams at once, outputs and workspaces apart: both give the single call's bits"""
    import torch
    from kpop_amd import api
    r1, r2, d = 65, 3000, 64
    m1, m2 = operands(r1, r2, d, 6)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    dev, t1, t2, tm = dev_buffers(m1, m2, metric)
    need = api.dev_distance_workspace_bytes(r1, r2, d)
    single = torch.zeros(r2, r1, dtype=torch.float64, device=dev)
    work0 = torch.empty(need, dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    works = [torch.empty(need, dtype=torch.uint8, device=dev) for _ in range(2)]
    outs = [torch.zeros(r2, r1, dtype=torch.float64, device=dev) for _ in range(2)]
    with class_set(2):
        api.dev_distance_rowwise(t1.data_ptr(), r1, t2.data_ptr(), r2, d, tm.data_ptr(), work0.data_ptr(), single.data_ptr())
        torch.cuda.synchronize()
        for _ in range(3):
            for s, w, o in zip(streams, works, outs):
                api.dev_distance_rowwise(t1.data_ptr(), r1, t2.data_ptr(), r2, d, tm.data_ptr(), w.data_ptr(), o.data_ptr(), stream=s.cuda_stream)
        for s in streams:
            s.synchronize()
    want = single.cpu().numpy()
    assert np.array_equal(want, oracle.distance_rowwise(m1, m2, metric, EUCLIDEAN, 2.0, True))
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), want)


@pytest.mark.parametrize("r1,r2,d,kind,p", [(128, 100, 64, EUCLIDEAN, 2.0), (65, 100, 65, COSINE, 2.0), (65, 100, 64, MINKOWSKI, 1.5),
                                            (65, 1, 64, EUCLIDEAN, 2.0)])
def test_ineligible_shapes_still_answer(kpop, oracle, r1, r2, d, kind, p):
    """128 classes, 65 dimensions, a Minkowski distance, and a second operand too small to lend the room for the padded classes:
    under class_set = 2 each runs what it runs under class_set = 0"""
    m1, m2 = operands(r1, r2, d, r1 + r2 + d + kind)
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    for normalize in (True, False):
        with class_set(0):
            old = kpop.distance_rowwise(m1, m2, metric, kind, p, normalize)
        with class_set(2):
            new = kpop.distance_rowwise(m1, m2, metric, kind, p, normalize)
        assert np.array_equal(new, old)
        want = oracle.distance_rowwise(m1, m2, metric, kind, p, normalize)
        if kind == MINKOWSKI:  # tests/test_gpu_distance.py: pow() differs from libm by a few ulp
            assert np.max(np.abs(new - want)) <= 1e-11 * max(np.max(np.abs(want)), 1e-300)
        else:
            assert np.array_equal(new, want)


@pytest.mark.parametrize("r1,d", [(65, 64), (10, 9)])
def test_default_at_the_dispatch_boundary(kpop, oracle, r1, d):
    metric = oracle.metric_powers(oracle.synth_inertia(d))
    m1, m2_all = operands(r1, THRESHOLD + 1, d, r1 + d, decimals=2)
    for r2 in (THRESHOLD - 1, THRESHOLD, THRESHOLD + 1):
        m2 = m2_all[:r2]
        with class_set(0):
            old = kpop.distance_rowwise(m1, m2, metric)
        with class_set(1):
            new = kpop.distance_rowwise(m1, m2, metric)
        assert np.array_equal(new, old), r2


def test_headline_shape(kpop, oracle):
    """65 x 100,000 x 64, the flagship step's distance call: the default against class_set = 0 bit for bit, a few rows against the oracle"""
    r1, r2, d = 65, 100000, 64
    m1, m2 = operands(r1, r2, d, 2024, decimals=2)
    metric = kpop.metric_compute(oracle.synth_inertia(d))
    with class_set(0):
        old = kpop.distance_rowwise(m1, m2, metric)
    new = kpop.distance_rowwise(m1, m2, metric)  # the default
    assert np.array_equal(new, old)
    rows = sorted(set(list(range(0, r2, 9973)) + [r2 - 1]))
    assert np.array_equal(new[rows], oracle.distance_rowwise(m1, m2[rows], metric, EUCLIDEAN, 2.0, True))
