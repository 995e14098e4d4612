#!/usr/bin/env python3
"""Times the local outlier factor of a resident set (kpop_dev_lof) beside two calls that were there before it, on the same resident
set and the same build, and the query form against the same set.  One JSON line per number of dimensions:

    python tools/time_lof.py [--rows 100000] [--dims 64 1635] [--k 20] [--queries 4096] [--repeat 5]

The rows are the synthetic lineages of tools/time_kmedoids.py.  Inside one process, each call between two HIP events on the stream it
is enqueued on, after --warmup-s seconds of the same alternation untimed:
    lof          kpop_dev_lof at k, the four outputs: the lists of the k-distances, then the two sweeps
    core         kpop_dev_core_distances at min_pts = k + 1: the lists alone (the call's first third)
    silhouette   kpop_dev_silhouette with ONE class: the same full rectangle with a plain row sum, its columns gathered
    score        kpop_dev_lof_score of --queries rows (the set's first rows, displaced) with the set's arrays (only where dims <= --score-dims)
THE YARDSTICK is core + 2 silhouette; ratio = lof / yardstick (profiles/lof.md).  The split of the call into its kernels is read from a
run under rocprofv3 --kernel-trace --stats (--repeat 1 --warmup-s 0).  Before the timing kdist is checked against core_distances' bit
for bit, and a second run of lof against the first."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 1635])
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--score-dims", type=int, default=64, help="the query form is timed where the rows have at most this many dimensions")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1, k, r2 = args.rows, args.k, args.queries
    for d in args.dims:
        gen = torch.Generator(device=dev)
        gen.manual_seed(r1 + d)
        n_lin, n_sub = max(r1 // 100, 1), max(r1 // 5, 1)
        centres = torch.randn((n_lin, d), dtype=torch.float64, device=dev, generator=gen)
        lin_of_sub = torch.randint(n_lin, (n_sub,), device=dev, generator=gen)
        sub_of_row = torch.randint(n_sub, (r1,), device=dev, generator=gen)
        m1 = torch.empty((r1, d), dtype=torch.float64, device=dev)
        subs = centres[lin_of_sub] + 0.05 * torch.randn((n_sub, d), dtype=torch.float64, device=dev, generator=gen)
        for lo in range(0, r1, 65536):
            hi = min(lo + 65536, r1)
            m1[lo:hi] = subs[sub_of_row[lo:hi]] + 0.001 * torch.randn((hi - lo, d), dtype=torch.float64, device=dev, generator=gen)
        del subs, centres
        m2 = (m1[:r2] + 0.01 * torch.randn((min(r2, r1), d), dtype=torch.float64, device=dev, generator=gen)).contiguous()
        n_q = m2.shape[0]
        metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, False, stream=stream.cuda_stream, keep=(m1, metric))

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        def f64(n):
            return torch.zeros(n, dtype=torch.float64, device=dev)

        kdist, lrd, lof_, core, own, kdist2 = (f64(r1) for _ in range(6))
        q_kdist, q_lrd, q_lof = (f64(n_q) for _ in range(3))
        n_neigh, one_class = (torch.zeros(r1, dtype=torch.int32, device=dev) for _ in range(2))
        q_n = torch.zeros(n_q, dtype=torch.int32, device=dev)
        work = torch.empty(api.dev_lof_workspace_bytes(rs, k), dtype=torch.uint8, device=dev)
        work_c = torch.empty(api.dev_core_distances_workspace_bytes(rs, k + 1), dtype=torch.uint8, device=dev)
        work_s = torch.empty(api.dev_silhouette_workspace_bytes(rs, 1), dtype=torch.uint8, device=dev)
        work_q = torch.empty(api.dev_lof_score_workspace_bytes(rs, n_q, k), dtype=torch.uint8, device=dev)
        with_score = d <= args.score_dims

        def lof(out=kdist):
            api.dev_lof(rs, k, work.data_ptr(), out.data_ptr(), n_neigh.data_ptr(), lrd.data_ptr(), lof_.data_ptr(), stream=stream.cuda_stream)

        def core_distances():
            api.dev_core_distances(rs, k + 1, work_c.data_ptr(), core.data_ptr(), stream=stream.cuda_stream)

        def silhouette():
            api.dev_silhouette(rs, one_class.data_ptr(), 1, work_s.data_ptr(), own.data_ptr(), stream=stream.cuda_stream)

        def score():
            api.dev_lof_score(rs, k, kdist.data_ptr(), lrd.data_ptr(), m2.data_ptr(), n_q, work_q.data_ptr(), q_kdist.data_ptr(), q_n.data_ptr(), q_lrd.data_ptr(),
                              q_lof.data_ptr(), stream=stream.cuda_stream)

        calls = [("lof", lof), ("core", core_distances), ("silhouette", silhouette)] + ([("score", score)] if with_score else [])
        timed(lof)
        first = lof_.clone()
        timed(core_distances)
        assert bool(torch.equal(kdist.view(torch.int64), core.view(torch.int64))), "kdist is not core_distances(k + 1)"
        timed(lambda: lof(kdist2))
        assert bool(torch.equal(first.view(torch.int64), lof_.view(torch.int64))), "a second run gave other bits"
        t = {name: [] for name, _ in calls}
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            for _, fn in calls:
                timed(fn)
        for _ in range(args.repeat):
            for name, fn in calls:
                t[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in t.items()}
        yard = med["core"] + 2 * med["silhouette"]
        factors = lof_.cpu().numpy()
        line = {"rows": r1, "dims": d, "k": k, "lof_ms": [round(x, 3) for x in t["lof"]], "core_ms": [round(x, 3) for x in t["core"]],
                "silhouette_ms": [round(x, 3) for x in t["silhouette"]], "lof_median_ms": round(med["lof"], 3), "core_median_ms": round(med["core"], 3),
                "silhouette_median_ms": round(med["silhouette"], 3), "yardstick_ms": round(yard, 3), "ratio": round(med["lof"] / yard, 4),
                "max_n_neigh": int(n_neigh.max().item()), "lof_median": float(np.nanmedian(factors)), "lof_max": float(np.nanmax(factors)),
                "workspace_bytes": int(work.numel())}
        if with_score:
            line.update({"queries": n_q, "score_ms": [round(x, 3) for x in t["score"]], "score_median_ms": round(med["score"], 3),
                         "score_workspace_bytes": int(work_q.numel())})
        print(json.dumps(line), flush=True)
        rs.free()
        del m1, m2, rs


if __name__ == "__main__":
    main()
