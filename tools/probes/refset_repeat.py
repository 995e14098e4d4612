"""The same query batch against the same database, again and again: the unprepared call (kpop_dev_distance_summary /
kpop_distance_summary) beside the call on a resident set (kpop_refset), ALTERNATED in one process on the same rows.

    python tools/probes/refset_repeat.py [--calls 20] [--small]        the table kept as profiles/refset_repeat.txt
    rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/probes/refset_repeat.py --trace
                                                                        one create, eight prepared summaries of 256 x 1M x 64

Device calls are timed with device events around a call that ends in a synchronise; host calls (which synchronise inside, on
the null stream) with the host's clock.  Every shape is warmed first.  Rows are synthetic, from a seed, generated on the device."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import kpop_amd  # noqa: E402
from kpop_amd import api  # noqa: E402

STREAM_TBS = 6.29  # TB/s: the measured streaming rate of HBM on this part (MI355X_MICROARCH.md)
KEEP, CAP = 300, 304


def quartiles(ms):
    q1, q2, q3 = np.percentile(ms, [25, 50, 75])
    return q1, q2, q3


def verdict(plain, prep):
    a, b = quartiles(plain), quartiles(prep)
    if a[0] <= b[1] <= a[2] and b[0] <= a[1] <= b[2]:
        return "level"
    return "prepared faster" if b[1] < a[1] else "PREPARED SLOWER"


def line(what, plain, prep, extra=""):
    a, b = quartiles(plain), quartiles(prep)
    print("%-34s unprepared %9.3f [%9.3f %9.3f]  prepared %9.3f [%9.3f %9.3f] ms  %-16s %s" % (what, a[1], a[0], a[2], b[1], b[0], b[2], verdict(plain, prep), extra),
          flush=True)


def device_timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def database(r1, d, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m1 = torch.randn(r1, d, dtype=torch.float64, device=dev, generator=g)
    metric = torch.rand(d, dtype=torch.float64, device=dev, generator=g) + 0.1
    metric /= metric.sum()
    queries = m1[torch.randperm(r1, device=dev, generator=g)[:1024]] + 0.05 * torch.randn(1024, d, dtype=torch.float64, device=dev, generator=g)
    return m1, metric, queries.contiguous()


def outputs(r2, dev):
    return (torch.zeros(r2, 4, dtype=torch.float64, device=dev), torch.zeros(r2, dtype=torch.int32, device=dev), torch.zeros(r2, CAP, dtype=torch.int32, device=dev),
            torch.zeros(r2, CAP, dtype=torch.float64, device=dev), torch.zeros(r2, CAP, dtype=torch.float64, device=dev))


def device_calls(r1, d, m1, metric, queries, calls, dev):
    st = torch.cuda.current_stream().cuda_stream
    rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, True, stream=st, keep=(m1, metric))
    try:
        for r2 in (1, 16, 256, 1024):
            q = queries[:r2].contiguous()
            work = torch.empty(api.dev_distance_workspace_bytes(r1, r2, d), dtype=torch.uint8, device=dev)
            work_rs = torch.empty(api.dev_refset_workspace_bytes(rs, r2), dtype=torch.uint8, device=dev)
            a, b = outputs(r2, dev), outputs(r2, dev)

            def plain():
                api.dev_distance_summary(m1.data_ptr(), r1, q.data_ptr(), r2, d, metric.data_ptr(), work.data_ptr(), *[t.data_ptr() for t in a], keep_at_most=KEEP,
                                         max_neighbours=CAP, stream=st)

            def prepared():
                api.dev_refset_distance_summary(rs, q.data_ptr(), r2, work_rs.data_ptr(), *[t.data_ptr() for t in b], keep_at_most=KEEP, max_neighbours=CAP, stream=st)

            for _ in range(2):
                plain()
                prepared()
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])), "the prepared call answers differently"
            t_plain, t_prep = [], []
            for _ in range(calls):
                t_plain.append(device_timed(plain))
                t_prep.append(device_timed(prepared))
            floor = r1 * d * 8 / (STREAM_TBS * 1e12) * 1e3
            line("device %4d x %d x %d" % (r2, r1, d), t_plain, t_prep, "(reading the rows once at %.2f TB/s: %.3f ms)" % (STREAM_TBS, floor) if r2 <= 16 else "")
            del work, work_rs
    finally:
        rs.free()


def host_calls(r1, d, m1, metric, queries, calls):
    h1, hm, hq = m1.cpu().numpy(), metric.cpu().numpy(), queries[:256].cpu().numpy()
    extra = np.ascontiguousarray(h1[:1000])
    t0 = time.perf_counter()
    rs = kpop_amd.RefSet(h1, hm, api.EUCLIDEAN, 2.0, True, capacity=r1 + 1000 * (calls + 2))
    print("%-34s kpop_refset_create, once: %.1f ms (%d bytes on the device)" % ("host %d x %d" % (r1, d), (time.perf_counter() - t0) * 1e3, rs.info()["device_bytes"]), flush=True)
    try:
        plain = lambda: kpop_amd.distance_summary(h1, hq, hm, api.EUCLIDEAN, 2.0, True, KEEP, max_neighbours=CAP)  # noqa: E731
        prepared = lambda: rs.distance_summary(hq, KEEP, max_neighbours=CAP)  # noqa: E731
        want, got = plain(), prepared()
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), "the prepared call answers differently"
        t_plain, t_prep = [], []
        for _ in range(calls):
            t_plain.append(host_timed(plain))
            t_prep.append(host_timed(prepared))
        line("host    256 x %d x %d" % (r1, d), t_plain, t_prep)
        rs.append(extra)  # (warm)
        t_app = [host_timed(lambda: rs.append(extra)) for _ in range(calls)]
        q = quartiles(t_app)
        print("%-34s kpop_refset_append of 1,000 rows: %.3f [%.3f %.3f] ms" % ("host %d x %d" % (r1, d), q[1], q[0], q[2]), flush=True)
    finally:
        rs.free()


def trace(dev):
    r1, d, r2 = 1000000, 64, 256
    m1, metric, queries = database(r1, d, dev, 1)
    h1, hm = m1.cpu().numpy(), metric.cpu().numpy()
    q = queries[:r2].contiguous()
    out = outputs(r2, dev)
    st = torch.cuda.current_stream().cuda_stream
    rs = kpop_amd.RefSet(h1, hm, api.EUCLIDEAN, 2.0, True)
    work = torch.empty(api.dev_refset_workspace_bytes(rs, r2), dtype=torch.uint8, device=dev)
    for _ in range(8):
        api.dev_refset_distance_summary(rs, q.data_ptr(), r2, work.data_ptr(), *[t.data_ptr() for t in out], keep_at_most=KEEP, max_neighbours=CAP, stream=st)
    torch.cuda.synchronize()
    rs.free()
    print("trace: one create, eight prepared summaries of %d x %d x %d" % (r2, r1, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a quick look)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    if args.trace:
        return trace(dev)
    calls = max(args.calls, 20)
    print("euclidean, normalised, %d neighbours; %d timed calls a variant, the two variants alternated; median [quartiles]" % (KEEP, calls))
    for r1, d in ((1000000, 64), (650000, 1635)):
        if args.small:
            r1 //= 10
        m1, metric, queries = database(r1, d, dev, r1 + d)
        device_calls(r1, d, m1, metric, queries, calls, dev)
        if not args.no_host:
            host_calls(r1, d, m1, metric, queries, calls)
        del m1, metric, queries
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
