#!/usr/bin/env python3
"""Times the representatives at a distance (kpop_dev_representatives_within) against the clusters at the same distance
(kpop_dev_clusters_within) on the same resident set and the same build.  One JSON line per case:

    python tools/time_representatives.py [--rows 100000] [--dims 64] [--repeat 5]

The rows are synthetic lineages on two levels: rows // 100 lineage centres (standard normal), rows // 5 sub-lineages at 0.05 of their
lineage's centre, and every row at 0.001 of a sub-lineage drawn at random.  Two thresholds, in units of the root of the metric's sum:
0.3 keeps about one row a lineage (about 1 % of the rows), 0.01 about one a sub-lineage that was drawn (about 20 %).  The two calls
alternate inside one process, each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the same
alternation untimed (tools/time_clusters.py).  kpop_clusters_within examines r1 (r1 - 1) / 2 pairs; this call about r1 n_reps +
r1 kRepStep / 2 (kRepStep = 2048, representatives.hip) when no row tile of a step is skipped: the ratio of the two times is listed
beside that ratio of the pair counts.  Before the timing the result is checked: its invariants, the count, every row in its
representative's cluster, no fewer representatives than clusters, and for a sample of rows -- from the rowwise matrix on the vector
pipe -- that a representative has no representative below it within the threshold and that any other row has the nearest one below
it.  A run under rocprofv3 --kernel-trace --stats (--repeat 1 --warmup-s 0) gives the split by kernel, the resolve kernel's among
them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP = 2048  # kRepStep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.3, 0.01], help="in units of the root of the metric's sum")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1, d = args.rows, args.dims
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
    del subs
    metric_h = np.linspace(1.0, 0.25, d)
    unit = float(np.sqrt(metric_h.sum()))
    metric = torch.from_numpy(metric_h).to(dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, False, stream=stream.cuda_stream, keep=(m1, metric))
    sample = torch.arange(0, r1, max(r1 // 64, 1), device=dev)[:64]
    q = m1[sample].contiguous()
    out = torch.empty((len(sample), r1), dtype=torch.float64, device=dev)
    work_r = torch.empty(api.dev_refset_workspace_bytes(rs, len(sample)), dtype=torch.uint8, device=dev)
    api.tune("distance_mfma", 0)
    api.dev_refset_distance_rowwise(rs, q.data_ptr(), len(sample), work_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    api.tune("distance_mfma", 1)
    work_c = torch.empty(max(api.dev_clusters_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
    work_p = torch.empty(max(api.dev_representatives_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
    labels = torch.zeros(r1, dtype=torch.int32, device=dev)
    rep_of = torch.zeros(r1, dtype=torch.int32, device=dev)
    rep_dist = torch.zeros(r1, dtype=torch.float64, device=dev)
    count_c = torch.zeros(1, dtype=torch.int32, device=dev)
    count_p = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = torch.arange(r1, device=dev)
    for t_units in args.thresholds:
        T = t_units * unit

        def clusters():
            api.dev_clusters_within(rs, T, work_c.data_ptr(), labels.data_ptr(), count_c.data_ptr(), stream=stream.cuda_stream)

        def representatives():
            api.dev_representatives_within(rs, T, work_p.data_ptr(), rep_of.data_ptr(), rep_dist.data_ptr(), count_p.data_ptr(), stream=stream.cuda_stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        timed(clusters)
        timed(representatives)
        lab, rep = labels.to(torch.int64), rep_of.to(torch.int64)
        n_clusters, n_reps = int(count_c.item()), int(count_p.item())
        is_rep = rep == rows
        assert bool(torch.all(rep <= rows)) and bool(torch.equal(rep[rep], rep)) and n_reps == int(torch.sum(is_rep))
        assert bool(torch.equal(lab[rep], lab)) and n_reps >= n_clusters
        assert not bool(torch.any(rep_dist[is_rep] != 0.0)) and bool(torch.all(rep_dist[~is_rep] <= T))
        for s, j in enumerate(sample.tolist()):  # against the rowwise matrix: what decides row j is the representatives below it
            below = is_rep & (rows < j) & (out[s] <= T)
            if bool(is_rep[j]):
                assert not bool(torch.any(below)), j
            else:
                cand = torch.nonzero(below).flatten()
                best = cand[torch.argmin(out[s][cand])]  # (the first of the least)
                assert int(best) == int(rep[j]) and float(out[s][best]) == float(rep_dist[j]), j
        t_c, t_p = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(clusters)
            timed(representatives)
        for _ in range(args.repeat):
            t_c.append(timed(clusters))
            t_p.append(timed(representatives))
        pairs_c = r1 * (r1 - 1) / 2.0
        pairs_p = float(r1) * n_reps + float(r1) * min(STEP, r1) / 2.0
        line = {"rows": r1, "dims": d, "threshold_units": t_units, "max_distance": T, "n_reps": n_reps, "reps_fraction": round(n_reps / r1, 4),
                "n_clusters": n_clusters, "steps": (r1 + STEP - 1) // STEP,
                "clusters_ms": [round(t, 3) for t in t_c], "representatives_ms": [round(t, 3) for t in t_p],
                "clusters_median_ms": round(float(np.median(t_c)), 3), "representatives_median_ms": round(float(np.median(t_p)), 3),
                "clusters_spread_ms": round(max(t_c) - min(t_c), 3), "representatives_spread_ms": round(max(t_p) - min(t_p), 3),
                "time_ratio": round(float(np.median(t_p) / np.median(t_c)), 4), "pair_ratio": round(pairs_p / pairs_c, 4),
                "representatives_ms_per_step": round(float(np.median(t_p)) / ((r1 + STEP - 1) // STEP), 4)}
        print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
