"""The concurrency contract of include/kpop_hip.h (conventions): device entry points on different streams may run at the same time
(the library's scratch is per stream), host entry points of one device slot run one at a time, kpop_last_error() is per thread, a host
thread works on the device slot it chose.

Every JOB is a fixed input on the device, a set of output tensors per use and a function that enqueues on a given stream.  A job has two
references: the SERIAL result -- the same call alone on the null stream, synchronised before and after, made twice and required to
return the same bits both times (every route here returns the same bits every call) -- and the ORACLE, applied to the serial
result once, with the assertion the single-call test of that route uses.  Whatever runs interleaved, back to back or from several
threads must then equal the serial result BIT FOR BIT; every instance of a job has its own seed, so another call's data in an output
is unmistakable.

  job        entry point                      scratch of the library it takes
  G-stream   dev_count_twist, < 16 genomes    segment tables, partial rows, the long sequences' counter (count_twist.hip)
  G-tile     dev_count_twist, assemblies      ... plus the tile route's tickets, lists and look-back scans
  G-packed   dev_count_twist_packed           the stream's SECOND block, then the first (packed.hip)
  T-long     dev_twist, very long spectra     the segments' partial rows
  S-wave/S-block/S-large  dev_distance_summary, 300 x 100 dimensions / 5,000 / 20,000 reference rows: distance rows, brackets, lists
  S-mfma     dev_distance_summary, 70,001 rows  the matrix-core chain's rows, scratch and candidate lists
  R-mfma     dev_distance_rowwise, 2^32 products and more: the normalised copies (distance_mfma.hip)
  C          dev_count_reads                  none: the caller's scratch (the control)

That calls on different streams did overlap is MEASURED (events around every call, one base event): a test of streams in which no round
shows an overlap ends in a skip, never in a pass.  Rounds are a fixed small number; threads are joined with a time limit."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import concat
from test_gpu_twist import _one_organism, assert_close

pytestmark = pytest.mark.gpu

ROUNDS = 5
JOIN_S = 300.0
K = 9  # every count -> twist job: all 131,072 canonical 9-mers


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(_dev())


def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device=_dev())


def _differs(got, want, loose=()):
    """None, or which field of two results differs (fields in `loose`: rtol 1e-10, atol 1e-13, tests/test_gpu_distance.py:667)"""
    assert got.keys() == want.keys()
    for f in want:
        a, b = got[f], want[f]
        if a.shape != b.shape:
            return "%s: shape %s against %s" % (f, a.shape, b.shape)
        if f in loose:
            if not np.allclose(a, b, rtol=1e-10, atol=1e-13, equal_nan=True):
                return "%s: beyond 1e-10" % f
        elif not np.array_equal(a, b, equal_nan=True):
            bad = ~((a == b) | ((a != a) & (b != b)))
            return "%s: %d of %d elements differ, the first at %s" % (f, int(bad.sum()), bad.size, tuple(int(x[0]) for x in np.nonzero(bad)))
    return None


class Job:
    """alloc() -> output tensors; call(outs, stream) enqueues; view(outs) -> {field: numpy array} holding what the call defines"""
    loose = ()  # fields compared at 1e-10 instead of bit for bit (none: see reference())

    def __init__(self, name, seed):
        self.name, self.seed, self.ref = name, seed, None

    def reference(self, W):
        """the serial result: alone on the null stream, twice, the same bits; then the oracle, once"""
        import torch
        if self.ref is None:
            res = []
            for _ in range(2):
                outs = self.alloc()
                torch.cuda.synchronize()
                self.call(outs, 0)
                torch.cuda.synchronize()
                res.append(self.view(outs))
            diff = _differs(res[1], res[0], self.loose)
            assert diff is None, "%s (seed %d) is not repeatable serially: %s" % (self.name, self.seed, diff)
            self.check(W.oracle, res[0])
            self.ref = res[0]
        return self.ref

    def differs(self, outs):
        return _differs(self.view(outs), self.ref, self.loose)


class CountTwistJob(Job):
    def __init__(self, W, name, seed, seqs, d, packed=False, per_row=True):
        super().__init__("%s(D=%d)" % (name, d), seed)
        self.api = W.api
        self.tw, self.T, self.cols = W.twister(K, d)
        self.d, self.per_row, self.packed = d, per_row, packed
        self.bases, self.offs = concat(seqs)
        self.n, self.n_bases, self.max_len = len(seqs), len(self.bases), max(len(s) for s in seqs)
        self.d_offs = _up(self.offs)
        if packed:
            codes, invalid = W.api.pack_bases(self.bases)
            self.d_in = (_up(codes), _up(invalid))
        else:
            self.d_in = (_up(self.bases),)

    def alloc(self):
        import torch
        return (_zeros((self.n, self.d), torch.float64),)

    def call(self, outs, stream):
        if self.packed:
            self.api.dev_count_twist_packed(self.tw, self.d_in[0].data_ptr(), self.d_in[1].data_ptr(), self.d_offs.data_ptr(), self.n, self.n_bases,
                                            self.max_len, outs[0].data_ptr(), stream=stream)
        else:
            self.api.dev_count_twist(self.tw, self.d_in[0].data_ptr(), self.d_offs.data_ptr(), self.n, self.n_bases, self.max_len, outs[0].data_ptr(),
                                     stream=stream)

    def view(self, outs):
        return {"rows": outs[0].cpu().numpy()}

    def check(self, oracle, res):
        h, c, o = oracle.count_reads(self.bases, self.offs, K)
        want = oracle.twist(self.T, self.cols, h, c.astype(np.float64), o)
        got = res["rows"]
        if self.per_row:  # (the streaming kernel: tests/test_gpu_twist.py, test_count_twist_long_sequences)
            for r in range(self.n):
                assert np.max(np.abs(got[r] - want[r])) <= 1e-12 * max(np.max(np.abs(want[r])), 1e-300), (self.name, r)
        else:  # (regrouped additions: RTOL of tests/test_gpu_twist.py)
            assert_close(got, want)
            plain = self._alone("dense", 0, 2)
            assert_close(plain, want)
            assert not np.array_equal(got, plain)  # (another order of additions: the tile kernel did run)

    def _alone(self, knob, value, back):
        """the serial call under another setting of a knob (nothing else is in flight when a reference is taken)"""
        import torch
        outs = self.alloc()
        torch.cuda.synchronize()
        self.api.tune(knob, value)
        try:
            self.call(outs, 0)
            torch.cuda.synchronize()
        finally:
            self.api.tune(knob, back)
        return outs[0].cpu().numpy()


def _genomes(rng, n, lo, hi):
    seqs = []
    for i in range(n):
        s = rng.choice(list("ACGT"), size=int(rng.randint(lo, hi)))
        if i % 2:
            cut = int(rng.randint(1000, lo - 1000))
            s[cut:cut + 37] = "N"
        seqs.append("".join(s))
    return seqs


def g_stream(W, seed, d=64, n=6):
    """a handful of unrelated 60-120 kb sequences: fewer than the tile route asks for, the streaming kernel's"""
    return CountTwistJob(W, "G-stream", seed, _genomes(np.random.RandomState(seed), n, 60000, 120000), d)


def g_tile(W, seed, d=64):
    """24 mutants of one 9 kb sequence, some strangers and short reads: the tile route"""
    return CountTwistJob(W, "G-tile", seed, _one_organism(np.random.RandomState(seed), 24, 9000, 0.003, unrelated=6), d, per_row=False)


def g_packed(W, seed, d=64):
    return CountTwistJob(W, "G-packed", seed, _genomes(np.random.RandomState(seed), 5, 30000, 60000), d, packed=True)


class TwistLongJob(Job):
    """a few very long spectra in segments (test_twist_few_very_long_spectra_in_segments): ragged, one empty, unknown k-mers, fractions"""

    def __init__(self, W, seed, d=64):
        super().__init__("T-long(D=%d)" % d, seed)
        self.api, self.d = W.api, d
        rng = np.random.RandomState(seed)
        self.tw, self.T, self.cols = W.twister(K, d, frac=0.9)
        allk = W.oracle.enumerate_kmers(K)
        lens = [len(allk), 70000, 0, 16384, 33333, 5]
        hs, vs, offs = [], [], [0]
        for n in lens:
            hh = np.sort(rng.choice(allk, size=n, replace=False)) if n else np.zeros(0, dtype=np.uint64)
            hs.append(hh)
            vs.append(np.round(rng.rand(len(hh)) * 50, 3) + 0.125)
            offs.append(offs[-1] + len(hh))
        self.h, self.v, self.o = np.concatenate(hs).astype(np.uint64), np.concatenate(vs), np.array(offs, dtype=np.uint64)
        self.n, self.max_lines = len(lens), max(lens)
        self.d_in = (_up(self.h), _up(self.v), _up(self.o))

    def alloc(self):
        import torch
        return (_zeros((self.n, self.d), torch.float64),)

    def call(self, outs, stream):
        self.api.dev_twist(self.tw, self.d_in[0].data_ptr(), self.d_in[1].data_ptr(), self.d_in[2].data_ptr(), self.n, self.max_lines, outs[0].data_ptr(),
                           normalize=True, stream=stream)

    def view(self, outs):
        return {"rows": outs[0].cpu().numpy()}

    def check(self, oracle, res):
        want = oracle.twist(self.T, self.cols, self.h, self.v, self.o, normalize=True)
        assert np.max(np.abs(res["rows"] - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))


class SummaryJob(Job):
    def __init__(self, W, name, seed, r1, r2, d, kind, keep, cap, grid, oracle_rows=None):
        super().__init__("%s(%d x %d x %d, kind %d, keep %d)" % (name, r2, r1, d, kind, keep), seed)
        import torch
        self.api = W.api
        rng = np.random.RandomState(seed)
        self.r1, self.r2, self.d, self.kind, self.keep, self.cap = r1, r2, d, kind, keep, cap
        m1, m2 = rng.normal(size=(r1, d)), rng.normal(size=(r2, d))
        if grid:  # (a coarse grid: exact ties between distances do occur)
            m1, m2 = np.round(m1, 1), np.round(m2, 1)
            m1[7] = m1[3]
            m2[5] = m1[11]  # a zero distance
        elif oracle_rows is not None:
            m2[::7] = m1[rng.randint(0, r1, size=len(m2[::7]))]
        else:
            m2[1] = m1[5]
            m1[77] = m1[5]
        self.m1, self.m2, self.metric = m1, m2, W.oracle.metric_powers(W.oracle.synth_inertia(d))
        self.oracle_rows = oracle_rows
        self.d_in = (_up(m1), _up(m2), _up(self.metric))
        self.work = torch.empty(max(W.api.dev_distance_workspace_bytes(r1, r2, d), 8), dtype=torch.uint8, device=_dev())  # (the caller's)
        self.filled = min(cap, 2048) if r1 > 4096 else cap  # (against more than 4,096 rows the device entry points fill 2,048 entries at most)

    def alloc(self):
        import torch
        r2, cap = self.r2, self.cap
        return (_zeros((r2, 4), torch.float64), _zeros(r2, torch.int32), _zeros((r2, cap), torch.int32), _zeros((r2, cap), torch.float64),
                _zeros((r2, cap), torch.float64))

    def call(self, outs, stream):
        st, n, idx, dist, z = outs
        self.api.dev_distance_summary(self.d_in[0].data_ptr(), self.r1, self.d_in[1].data_ptr(), self.r2, self.d, self.d_in[2].data_ptr(), self.work.data_ptr(),
                                      st.data_ptr(), n.data_ptr(), idx.data_ptr(), dist.data_ptr(), z.data_ptr(), keep_at_most=self.keep,
                                      max_neighbours=self.cap, kind=self.kind, p=2.0, normalize=True, stream=stream)

    def view(self, outs):
        st, n, idx, dist, z = (t.cpu().numpy() for t in outs)
        n = n.view(np.uint32)
        keep = np.arange(self.cap)[None, :] < np.minimum(n, self.filled)[:, None]  # (entries past a row's list are not the call's)
        return {"mean_sd": st[:, :2], "median_mad": st[:, 2:], "n": n, "idx": idx.view(np.uint32)[keep], "dist": dist[keep], "z": z[keep]}

    def check(self, oracle, res):
        rows = np.arange(self.r2) if self.oracle_rows is None else np.array(self.oracle_rows)
        st_o, offs, idx_o, dist_o, z_o = oracle.distance_summary(self.m1, self.m2[rows], self.metric, self.kind, 2.0, True, self.keep)
        n = res["n"]
        start = np.concatenate([[0], np.cumsum(np.minimum(n, self.filled))]).astype(np.int64)
        for t, j in enumerate(rows):
            a, b = int(offs[t]), int(offs[t + 1])
            assert n[j] == b - a, (self.name, j)
            m = int(min(n[j], self.filled))
            lo = int(start[j])
            assert res["idx"][lo:lo + m].tolist() == idx_o[a:a + m].tolist() and np.array_equal(res["dist"][lo:lo + m], dist_o[a:a + m]), (self.name, j)
            assert np.array_equal(res["median_mad"][j], st_o[t, 2:]) or self.r1 <= 65536, (self.name, j)
            if self.oracle_rows is None:
                np.testing.assert_allclose(res["z"][lo:lo + m], z_o[a:a + m], rtol=1e-8, atol=1e-10 if self.r1 <= 4096 else 1e-9)
        if self.oracle_rows is None:
            st = np.concatenate([res["mean_sd"], res["median_mad"]], axis=1)
            np.testing.assert_allclose(st, st_o, rtol=1e-10, atol=1e-13)


def s_wave(W, seed):
    """300 reference rows of 100 dimensions do not fit LDS: distance rows of a chunk in the workspace, a wavefront a row over them"""
    return SummaryJob(W, "S-wave", seed, 300, 600, 100, 0, 300, 300, grid=True)


def s_block(W, seed):
    return SummaryJob(W, "S-block", seed, 5000, 12, 16, 0, 2, 2048, grid=True)


def s_large(W, seed):
    return SummaryJob(W, "S-large", seed, 20000, 12, 16, 0, 300, 2048, grid=True)


def s_mfma(W, seed, kind=0):
    return SummaryJob(W, "S-mfma", seed, 70001, 9, 64, kind, 300, 512, grid=False)


def s_mfma_many(W, seed, kind, d, r2):
    """hundreds of query rows against 70,001 (test_distance_summary_on_the_matrix_cores_many_query_rows): 512 and more take two lanes
    under kpop_tune("summary_lanes", 2); a handful of rows against the oracle"""
    return SummaryJob(W, "S-mfma-many", seed, 70001, r2, d, kind, 20, 32, grid=False, oracle_rows=[0, 1, 7, 255, 256, r2 - 1])


class RowwiseJob(Job):
    """2^32 products and more: the tiled contraction on the matrix cores (test_distance_rowwise_on_the_matrix_cores)"""

    def __init__(self, W, seed, r1=1636, r2=1700, d=1635, kind=1):
        super().__init__("R-mfma(%d x %d x %d, kind %d)" % (r2, r1, d, kind), seed)
        import torch
        assert r1 * r2 * d >= 1 << 32
        self.api = W.api
        rng = np.random.RandomState(seed)
        self.r1, self.r2, self.d, self.kind = r1, r2, d, kind
        self.m1, self.m2 = rng.normal(size=(r1, d)), rng.normal(size=(r2, d))
        self.m2[1] = self.m1[5]
        self.metric = W.oracle.metric_powers(W.oracle.synth_inertia(d))
        self.sub = np.unique(np.concatenate([np.arange(64), rng.randint(0, r2, size=200)]))
        self.d_in = (_up(self.m1), _up(self.m2), _up(self.metric))
        self.work = torch.empty(W.api.dev_distance_workspace_bytes(r1, r2, d), dtype=torch.uint8, device=_dev())

    def alloc(self):
        import torch
        return (_zeros((self.r2, self.r1), torch.float64),)

    def call(self, outs, stream):
        self.api.dev_distance_rowwise(self.d_in[0].data_ptr(), self.r1, self.d_in[1].data_ptr(), self.r2, self.d, self.d_in[2].data_ptr(), self.work.data_ptr(),
                                      outs[0].data_ptr(), kind=self.kind, p=2.0, normalize=True, stream=stream)

    def view(self, outs):
        return {"distances": outs[0].cpu().numpy()}

    def check(self, oracle, res):
        want = oracle.distance_rowwise(self.m1, self.m2[self.sub], self.metric, self.kind, 2.0, True)
        g = res["distances"][self.sub]
        err = np.abs(g - want) / np.maximum(np.abs(want), 1e-300)
        err[want == g] = 0.0
        assert err.max() <= 1e-12, (self.name, err.max())
        assert g[1, 5] == want[1, 5] == 0.0
        exact = self._alone("distance_mfma", 0, 1)
        assert np.array_equal(exact[self.sub], want)
        assert not np.array_equal(exact, res["distances"])  # (the matrix cores did run)

    _alone = CountTwistJob._alone


class CountReadsJob(Job):
    """-L counting into the caller's buffers with the caller's scratch: nothing of the library's"""

    def __init__(self, W, seed, n=3000, L=150, k=10):
        super().__init__("C(%d reads)" % n, seed)
        import torch
        self.api, self.n, self.L, self.k = W.api, n, L, k
        self.bases, self.offs = W.oracle.synth_reads(seed, n, L)
        self.d_in = (_up(self.bases), _up(self.offs))
        self.scratch = torch.empty(max(W.api.dev_count_reads_scratch_bytes(n, L, k), 8), dtype=torch.uint8, device=_dev())

    def alloc(self):
        import torch
        return (_zeros(self.n * self.L, torch.int64), _zeros(self.n * self.L, torch.int32), _zeros(self.n + 1, torch.int64))

    def call(self, outs, stream):
        self.api.dev_count_reads(self.d_in[0].data_ptr(), self.d_in[1].data_ptr(), self.n, self.L, self.k, self.scratch.data_ptr(), outs[0].data_ptr(),
                                 outs[1].data_ptr(), outs[2].data_ptr(), stream=stream)

    def view(self, outs):
        h, c, o = (t.cpu().numpy() for t in outs)
        o = o.view(np.uint64)
        t = min(int(o[-1]), len(h))
        return {"hash": h.view(np.uint64)[:t], "count": c.view(np.uint32)[:t], "offsets": o}

    def check(self, oracle, res):
        h, c, o = oracle.count_reads(self.bases, self.offs, self.k)
        assert np.array_equal(res["hash"], h) and np.array_equal(res["count"], c) and np.array_equal(res["offsets"], o)


class HostJob:
    """the host entry points a thread loops over: count_reads per read and merged, Twister.count_twist on a genome batch,
    distance_summary against 5,000 rows -- null stream, the slot's arena, one at a time under the slot's lock"""

    def __init__(self, W, seed):
        self.kpop, self.seed = W.kpop, seed
        rng = np.random.RandomState(seed)
        self.reads = W.oracle.synth_reads(seed, 2000, 150)
        self.genomes = concat(_genomes(rng, 4, 20000, 40000))
        self.m1, self.m2 = np.round(rng.normal(size=(5000, 16)), 1), np.round(rng.normal(size=(12, 16)), 1)
        self.m2[5] = self.m1[11]
        self.metric = W.oracle.metric_powers(W.oracle.synth_inertia(16))
        self.tw, self.T, self.cols = W.twister(K, 64)
        self.ref = self.run(self.tw)
        # the oracle on the serial result, as the single-call tests of these entry points have it
        for per_read in (True, False):
            h, c, o = W.oracle.count_reads(self.reads[0], self.reads[1], 10, per_read=per_read)
            name = "per_read" if per_read else "merged"
            assert np.array_equal(self.ref[name + ".hash"], h) and np.array_equal(self.ref[name + ".count"], c) and np.array_equal(self.ref[name + ".offsets"], o)
        h, c, o = W.oracle.count_reads(self.genomes[0], self.genomes[1], K)
        want = W.oracle.twist(self.T, self.cols, h, c.astype(np.float64), o)
        for r in range(len(want)):
            assert np.max(np.abs(self.ref["genomes"][r] - want[r])) <= 1e-12 * np.max(np.abs(want[r]))
        st_o, offs, idx_o, dist_o, _ = W.oracle.distance_summary(self.m1, self.m2, self.metric, 0, 2.0, True, 2)
        np.testing.assert_allclose(self.ref["summary.stats"], st_o, rtol=1e-10, atol=1e-13)
        for j in range(12):
            a, b = int(offs[j]), int(offs[j + 1])
            assert self.ref["summary.n"][j] == b - a and self.ref["summary.idx"][j, :b - a].tolist() == idx_o[a:b].tolist()
            assert np.array_equal(self.ref["summary.dist"][j, :b - a], dist_o[a:b])

    def run(self, tw):
        kpop, res = self.kpop, {}
        for per_read in (True, False):
            h, c, o = kpop.count_reads(self.reads[0], self.reads[1], 10, per_read=per_read)
            name = "per_read" if per_read else "merged"
            res[name + ".hash"], res[name + ".count"], res[name + ".offsets"] = h, c, o
        res["genomes"] = tw.count_twist(self.genomes[0], self.genomes[1])
        st, n, idx, dist, z = kpop.distance_summary(self.m1, self.m2, self.metric, 0, 2.0, True, 2, max_neighbours=64)
        keep = np.arange(64)[None, :] < np.minimum(n, 64)[:, None]
        res["summary.stats"], res["summary.n"] = st, n
        res["summary.idx"], res["summary.dist"], res["summary.z"] = np.where(keep, idx, 0), np.where(keep, dist, 0.0), np.where(keep, z, 0.0)
        return res

    def loop(self, times, tw=None, who=""):
        for t in range(times):
            diff = _differs(self.run(tw or self.tw), self.ref)
            assert diff is None, "%s host job (seed %d), pass %d: %s" % (who, self.seed, t, diff)


class World:
    """what the tests of this file share: twisters, the jobs with their serial references, the work that keeps a stream busy"""

    def __init__(self, kpop, oracle):
        from kpop_amd import _lib, api
        self.kpop, self.oracle, self.api, self.lib = kpop, oracle, api, _lib.load()
        self._tw, self._jobs, self._fill = {}, {}, None

    def twister(self, k, d, seed=3, frac=1.0):
        key = (k, d, seed, frac)
        if key not in self._tw:
            cols = self.oracle.enumerate_kmers(k)
            if frac < 1.0:
                cols = cols[np.random.RandomState(seed).rand(len(cols)) < frac]
            T = self.oracle.synth_twister(seed, d, cols)
            self._tw[key] = (self.kpop.Twister.load(T, cols, k), T, cols)
        return self._tw[key]

    def job(self, make, seed, *args, **kw):
        """the instance of a job with that seed, its serial reference taken and checked against the oracle"""
        key = (make.__name__, seed, args, tuple(sorted(kw.items())))
        if key not in self._jobs:
            j = make(self, seed, *args, **kw)
            if isinstance(j, Job):
                j.reference(self)
            self._jobs[key] = j
        return self._jobs[key]

    def keep_busy(self):
        """some tens of milliseconds of work on torch's current stream: whatever is enqueued behind it, or behind an event recorded
        after it, is all in the queues before any of it starts"""
        import torch
        if self._fill is None:
            a = torch.randn((8192, 8192), dtype=torch.float64, device=_dev())
            self._fill = (a, torch.empty_like(a))
            torch.mm(a, a, out=self._fill[1])
            torch.cuda.synchronize()
        for _ in range(4):
            torch.mm(self._fill[0], self._fill[0], out=self._fill[1])

    def close(self):
        import torch
        torch.cuda.synchronize()
        self._jobs.clear()
        for tw, _, _ in self._tw.values():
            tw.free()
        self._tw.clear()
        self._fill = None


@pytest.fixture(scope="module")
def world(kpop, oracle):
    W = World(kpop, oracle)
    yield W
    W.close()


def _orders(n):
    """the order in which the streams get their next call, one per round"""
    fwd = list(range(n))
    swapped = [fwd[i ^ 1] if (i ^ 1) < n else fwd[i] for i in range(n)]
    return [fwd, fwd[::-1], swapped, fwd[1:] + fwd[:1], fwd[::2] + fwd[1::2]]


def _interleave(W, lanes, what):
    """lanes[s]: the jobs of stream s.  ROUNDS rounds, in each the streams' next calls enqueued round-robin in that round's order, no host
    synchronisation until the end; every call between two timing events.  Fails on the first output that is not the serial one;
    returns the share of rounds with a call that overlapped, in time, a call on another stream."""
    import torch
    streams = [torch.cuda.Stream(device=_dev()) for _ in lanes]
    outs = {(s, i, r): job.alloc() for s, lane in enumerate(lanes) for i, job in enumerate(lane) for r in range(ROUNDS)}
    torch.cuda.synchronize()
    base, gate = torch.cuda.Event(enable_timing=True), torch.cuda.Event()
    with torch.cuda.stream(streams[0]):
        base.record()
        W.keep_busy()
        gate.record()
    for s in streams[1:]:
        s.wait_event(gate)
    calls = []
    for r, order in enumerate(_orders(len(lanes))[:ROUNDS]):
        for i in range(max(len(lane) for lane in lanes)):
            for s in order:
                if i < len(lanes[s]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(streams[s])
                    lanes[s][i].call(outs[(s, i, r)], streams[s].cuda_stream)
                    e1.record(streams[s])
                    calls.append((r, s, i, e0, e1))
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for r, s, i, _, _ in calls:
        diff = lanes[s][i].differs(outs[(s, i, r)])
        if diff is not None:
            pytest.fail("%s: stream %d of %d, job %s (seed %d), round %d: not the serial result -- %s"
                        % (what, s, len(lanes), lanes[s][i].name, lanes[s][i].seed, r, diff))
    spans = [(r, s, base.elapsed_time(e0), base.elapsed_time(e1)) for r, s, _, e0, e1 in calls]
    hit = set()  # (a round counts when one of ITS calls ran while a call on another stream did)
    for r, s, t0, t1 in spans:
        for _, s_, u0, u1 in spans:
            if s_ != s and max(t0, u0) < min(t1, u1):
                hit.add(r)
    share = len(hit) / float(ROUNDS)
    print("\n[concurrency] %s: %d streams, %d calls, rounds with a call that overlapped a call on another stream: %d of %d"
          % (what, len(lanes), len(calls), len(hit), ROUNDS))
    return share


MIXES = {
    # G-tile beside G-tile, different batches and widths; the control beside them
    "tile_tile": lambda W: [[W.job(g_tile, 101, d=64), W.job(CountReadsJob, 102)], [W.job(g_tile, 103, d=100)]],
    "stream_large_long": lambda W: [[W.job(g_stream, 111, d=64), W.job(g_stream, 112, d=100)],
                                    [W.job(s_large, 113), W.job(s_block, 114), W.job(s_wave, 115)],
                                    [W.job(TwistLongJob, 116), W.job(CountReadsJob, 117)]],
    "mfma_mfma": lambda W: [[W.job(s_mfma, 121, kind=0)], [W.job(s_mfma, 122, kind=1)]],
    "rmfma_packed": lambda W: [[W.job(RowwiseJob, 131)], [W.job(g_packed, 132), W.job(CountReadsJob, 133)]],
    "four_streams": lambda W: [[W.job(g_tile, 141, d=64)], [W.job(s_large, 142), W.job(g_stream, 143, d=64)],
                               [W.job(TwistLongJob, 144), W.job(s_mfma, 145, kind=0)], [W.job(g_packed, 146), W.job(CountReadsJob, 147)]],
}


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_different_streams_one_host_thread(world, mix):
    """2, 3 and 4 streams, each with a job mix of its own, enqueued round-robin from one host thread in five interleavings and
    synchronised once at the end: every output of every round is the serial result, bit for bit.  A scratch block, a ticket or a
    counter shared between streams by accident shows here; a run in which nothing overlapped is skipped, not passed."""
    lanes = MIXES[mix](world)
    assert 2 <= len(lanes) <= 4 and len({id(j) for lane in lanes for j in lane}) == sum(len(lane) for lane in lanes)
    share = _interleave(world, lanes, mix)
    if share == 0.0:
        pytest.skip("%s: no two calls on different streams overlapped in any of the %d rounds: the run proves nothing" % (mix, ROUNDS))


def _back_to_back(W, jobs, stream, what):
    """the jobs enqueued on one stream behind work that keeps it busy, no synchronisation between them -> (outputs, whether that work was
    still running when the last call had returned)"""
    import torch
    outs = [j.alloc() for j in jobs]
    torch.cuda.synchronize()
    busy = torch.cuda.Event()
    with torch.cuda.stream(stream):
        W.keep_busy()
        busy.record()
    for j, o in zip(jobs, outs):
        j.call(o, stream.cuda_stream)
    still_busy = not busy.query()
    stream.synchronize()
    torch.cuda.synchronize()
    for t, (j, o) in enumerate(zip(jobs, outs)):
        diff = j.differs(o)
        assert diff is None, "%s: call %d, job %s (seed %d): not the serial result -- %s" % (what, t, j.name, j.seed, diff)
    return still_busy


def test_one_stream_back_to_back_routes_that_share_its_block(world):
    """G-tile -> S-large -> T-long -> G-stream (a smaller batch) -> S-mfma -> G-tile again on ONE stream with nothing between them: every
    route carves the stream's one block its own way and must leave nothing the next one trips over (a counter assumed zero, a ticket).
    Once after kpop_dev_workspace_reserve_stream: the calls then only enqueue -- they return while the work put in front of them is
    still running, which a call that grows the block cannot (it synchronises the device first).  Once on a fresh stream, small to
    large: the block grows while the stream is busy (Workspace::ensure: synchronise, free, allocate).  Once on the null stream after
    kpop_dev_workspace_reserve."""
    import torch
    W = world
    tile, large, long_, small, mfma = W.job(g_tile, 201), W.job(s_large, 202), W.job(TwistLongJob, 203), W.job(g_stream, 204, n=3), W.job(s_mfma, 205)
    jobs = [tile, large, long_, small, mfma, tile]
    reserved = torch.cuda.Stream(device=_dev())
    W.api.check(W.lib.kpop_dev_workspace_reserve_stream(1 << 30, reserved.cuda_stream))  # (1 GiB: far more than any of these calls takes)
    assert _back_to_back(W, jobs, reserved, "reserved"), "a call on a stream whose workspace was reserved waited for the device"
    assert _back_to_back(W, jobs, reserved, "reserved, again")
    fresh = torch.cuda.Stream(device=_dev())
    waited = not _back_to_back(W, [long_, small, large, tile, mfma, tile], fresh, "growing")
    assert waited, "no call grew the workspace of a fresh stream: the growth path did not run"
    assert _back_to_back(W, jobs, fresh, "grown"), "the block had grown to the largest call's size and a call still waited"
    W.api.check(W.lib.kpop_dev_workspace_reserve(1 << 28))
    outs = [j.alloc() for j in jobs]
    torch.cuda.synchronize()
    for j, o in zip(jobs, outs):
        j.call(o, 0)
    torch.cuda.synchronize()
    for t, (j, o) in enumerate(zip(jobs, outs)):
        assert j.differs(o) is None, ("null stream", t, j.name, j.differs(o))


def test_two_summary_lanes_on_two_caller_streams(world):
    """kpop_tune("summary_lanes", 2): 640 and 515 query rows against 70,001 on two caller streams at once, each with a second stream of
    the library's own beside it (Context::aux_for: one lane, four events per caller stream).  Equal to the one-lane serial result bit
    for bit, mean and standard deviation included (the lanes change nothing)."""
    import torch
    W = world
    a, b = W.job(s_mfma_many, 301, 0, 24, 640), W.job(s_mfma_many, 302, 1, 64, 515)  # (serial references: one lane)
    torch.cuda.synchronize()
    W.api.tune("summary_lanes", 2)
    try:
        share = _interleave(W, [[a], [b]], "summary_lanes=2")
    finally:
        torch.cuda.synchronize()
        W.api.tune("summary_lanes", 1)
    if share == 0.0:
        pytest.skip("the two streams' calls overlapped in none of the %d rounds: the run proves nothing" % ROUNDS)


def _run_threads(fns):
    """every function in a thread of its own, started together; joined with a time limit (a thread still alive is a failure, not a
    wait); a worker's exception is raised here"""
    errors = [None] * len(fns)
    start = threading.Barrier(len(fns))

    def work(i):
        try:
            start.wait(JOIN_S)
            fns[i]()
        except BaseException as e:  # noqa: BLE001
            errors[i] = e

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(fns))]
    for t in threads:
        t.start()
    for i, t in enumerate(threads):
        t.join(JOIN_S)
        if t.is_alive():
            pytest.fail("thread %d of %d is still running after %d s" % (i, len(fns), JOIN_S))
    for e in errors:
        if e is not None:
            raise e


@pytest.mark.parametrize("n_threads", [2, 4])
def test_host_entry_points_from_several_threads_on_one_slot(world, n_threads):
    """ctypes releases the GIL: the threads' calls meet inside the library, where the slot's lock lets one host entry point run at a time
    and every one of them rewinds the arena to where IT found it.  Three passes a thread; all results are the serial ones."""
    jobs = [world.job(HostJob, 400 + i) for i in range(n_threads)]
    _run_threads([lambda j=j, i=i: j.loop(3, who="thread %d" % i) for i, j in enumerate(jobs)])


def test_host_entry_points_beside_a_thread_on_a_stream_of_its_own(world):
    """thread A loops host entry points (null stream, the arena); thread B meanwhile loads a twister, makes, queries and frees a RefSet
    -- outside any arena scope of its own: memory of its own, never what A's scope is about to rewind (common.h, DevBuf) -- and runs
    device jobs on a stream of its own.  Both see the serial results."""
    import torch
    W, kpop = world, world.kpop
    host = W.job(HostJob, 501)
    dev_jobs = [W.job(g_stream, 502, n=3), W.job(s_large, 503), W.job(CountReadsJob, 504), W.job(g_tile, 505)]
    rng = np.random.RandomState(506)
    cols = W.oracle.enumerate_kmers(7)
    T = W.oracle.synth_twister(506, 9, cols)
    reads = W.oracle.synth_reads(506, 500, 150)
    m1, m2 = host.m1, rng.normal(size=(33, 16))
    tw0 = kpop.Twister.load(T, cols, 7)
    want_rows = tw0.count_twist(*reads)
    tw0.free()
    want_dist = kpop.distance_rowwise(m1, m2, host.metric, 0, 2.0, True)
    h, c, o = W.oracle.count_reads(reads[0], reads[1], 7)
    assert_close(want_rows, W.oracle.twist(T, cols, h, c.astype(np.float64), o))

    def thread_b():
        stream = torch.cuda.Stream(device=_dev())
        for t in range(3):
            tw = kpop.Twister.load(T, cols, 7)
            rs = kpop.RefSet(m1, host.metric, 0, 2.0, True)
            outs = [j.alloc() for j in dev_jobs]
            torch.cuda.current_stream().synchronize()  # (the outputs are zeroed on torch's stream of this thread)
            for j, o_ in zip(dev_jobs, outs):
                j.call(o_, stream.cuda_stream)
            rows = tw.count_twist(*reads)
            dist = rs.distance_rowwise(m2)
            stream.synchronize()
            rs.free()
            tw.free()
            assert np.array_equal(rows, want_rows), ("thread B, twister of its own", t)
            assert np.array_equal(dist, want_dist), ("thread B, RefSet", t)
            for j, o_ in zip(dev_jobs, outs):
                diff = j.differs(o_)
                assert diff is None, "thread B, pass %d, job %s: not the serial result -- %s" % (t, j.name, diff)

    _run_threads([lambda: host.loop(4, who="thread A"), thread_b])


def test_threads_on_device_slots_of_their_own(world):
    """kpop_init_devices([0, 0, 0]): three slots on one GPU, a lock and an arena each.  Three threads choose a slot each
    (kpop_use_device), take a handle on the twister for their slot (kpop_twister_replicate) and run host entry points at the same time;
    results are the serial ones.  The copy of a hash-range SLICE that keeps its rows at their hashes reports bytes that make sense:
    kpop_twister_replicate used to take the whole 4^k-row table off a count that held the slice's range only -- an unsigned wrap-around
    (on one GPU the copy is a second handle on the same arrays and reports the source's bytes; between two GPUs it is the subtraction)."""
    import torch
    from kpop_amd.shard import kmer_slice_bounds
    W, kpop, api = world, world.kpop, world.api
    hosts = [W.job(HostJob, 600 + s) for s in range(3)]
    k, d = 9, 16
    api.tune("direct", 1)
    try:
        sl = kpop.Twister.synth(11, k, d, hash_range=kmer_slice_bounds(k, 1, 3), acc_dim=True)
    finally:
        api.tune("direct", 2)
    reads = W.oracle.synth_reads(0x4B506F70, 400, 150)
    want_slice = sl.count_twist(*reads, normalize=False)
    src = sl.info()
    lo, hi = kmer_slice_bounds(k, 1, 3)
    assert src["direct_bytes"] == (hi - lo) * ((d + 1 + 15) // 16 * 16) * 8
    total = torch.cuda.get_device_properties(0).total_memory

    def replicate(tw, slot):
        h = C.c_void_p()
        api.check(W.lib.kpop_twister_replicate(tw.handle, slot, C.byref(h)))
        return kpop.Twister(h)

    infos = [None] * 3

    def on_slot(s):
        api.use_device(s)
        tw, slc = replicate(hosts[s].tw, s), replicate(sl, s)
        try:
            infos[s] = slc.info()
            for t in range(2):
                hosts[s].loop(1, tw=tw, who="slot %d" % s)
                assert np.array_equal(slc.count_twist(*reads, normalize=False), want_slice), ("slot", s, t)
        finally:
            tw.free()
            slc.free()

    torch.cuda.synchronize()
    kpop.init_devices([0, 0, 0])
    try:
        assert kpop.device_slots() == 3
        _run_threads([lambda s=s: on_slot(s) for s in range(3)])
    finally:
        kpop.init(0)
    for s, info in enumerate(infos):
        rows = info["n_cols"] * (d + 1) * 8
        assert rows <= info["device_bytes"] < total, (s, info)
        assert info["direct_bytes"] <= info["device_bytes"] - rows, (s, info)
        assert (info["n_cols"], info["n_dims"], info["k"]) == (src["n_cols"], src["n_dims"], src["k"])
    sl.free()


def test_a_pipeline_comes_and_goes_while_another_stream_is_busy(world):
    """kpop_pipeline_destroy erases its compute stream's workspace from the slot's map (under the map's lock) while a G-stream call on a
    caller's stream is in flight, its own block taken from the same map: both see their serial results."""
    import torch
    W, kpop = world, world.kpop
    job = W.job(g_stream, 701, d=64)
    tw, T, cols = W.twister(K, 64)
    bases, offs = concat(_genomes(np.random.RandomState(702), 5, 20000, 50000))

    def pipeline():
        pl = kpop.Pipeline(tw, outputs=kpop.OUT_TWISTED)
        rows = pl.run(bases, offs)["twisted"].copy()
        return pl, rows

    pl, want = pipeline()
    pl.close()
    h, c, o = W.oracle.count_reads(bases, offs, K)
    want_o = W.oracle.twist(T, cols, h, c.astype(np.float64), o)
    for r in range(len(want_o)):
        assert np.max(np.abs(want[r] - want_o[r])) <= 1e-12 * np.max(np.abs(want_o[r]))
    stream = torch.cuda.Stream(device=_dev())
    outs = [job.alloc() for _ in range(4)]
    torch.cuda.synchronize()
    last = torch.cuda.Event()

    def enqueue(these):
        with torch.cuda.stream(stream):
            W.keep_busy()
        for o_ in these:
            job.call(o_, stream.cuda_stream)
        last.record(stream)

    enqueue(outs[:2])
    pl, rows = pipeline()  # (created and used beside the caller's stream ...)
    enqueue(outs[2:])
    in_flight = not last.query()
    pl.close()             # (... and destroyed under it)
    stream.synchronize()
    assert in_flight, "the caller's stream was idle when the pipeline went: nothing was tested"
    assert np.array_equal(rows, want)
    for t, o_ in enumerate(outs):
        diff = job.differs(o_)
        assert diff is None, "call %d beside the pipeline: not the serial result -- %s" % (t, diff)
