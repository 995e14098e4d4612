#!/usr/bin/env python3
"""Times the clusters at a distance (kpop_dev_clusters_within) against what could answer the same question before it existed, on the
same resident set: the count-only range query with the set's own rows as the queries (kpop_dev_neighbours_within, NULL lists), in
batches of --batch query rows.  One JSON line per case:

    python tools/time_clusters.py [--rows 100000] [--dims 64] [--hits 300] [--lineage 10000] [--repeat 7]

Two cases: random rows with a threshold that gives about --hits neighbours a row, and the same with one planted lineage of --lineage
near-identical rows.  The two calls alternate inside one process, each between two HIP events on the stream it is enqueued on, after
--warmup-s seconds of the same alternation untimed (tools/time_within.py).  Every timing is listed with the baseline's own spread (max
- min over its repeats): the clusters call examines half the pairs with the same tile loop and writes no pool, and is expected to be
no slower than the baseline by more than that spread.  Before the timing the labels are checked: their two invariants and the count,
one label for all rows of the lineage, and for a sample of rows that every neighbour within the threshold (from the rowwise matrix on
the vector pipe) carries the row's label.  A run under rocprofv3 --kernel-trace --stats (--repeat 2) gives the split
by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--hits", type=int, default=300, help="neighbours a row the threshold aims at")
    ap.add_argument("--lineage", type=int, default=10000, help="rows of the planted lineage of the second case")
    ap.add_argument("--batch", type=int, default=4096, help="query rows a call of the baseline")
    ap.add_argument("--repeat", type=int, default=7, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=2.0, help="seconds of untimed alternating calls before the timed series")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1, d = args.rows, args.dims
    for case in ("random rows", "a lineage of %d" % args.lineage):
        gen = torch.Generator(device=dev)
        gen.manual_seed(r1 + d)
        m1 = torch.empty((r1, d), dtype=torch.float64, device=dev)
        for lo in range(0, r1, 65536):
            m1[lo:lo + 65536] = torch.randn((min(65536, r1 - lo), d), dtype=torch.float64, device=dev, generator=gen)
        lin_lo = r1 // 3
        planted = case != "random rows"
        if planted:
            point = torch.randn((d,), dtype=torch.float64, device=dev, generator=gen)
            m1[lin_lo:lin_lo + args.lineage] = point + 1e-4 * torch.randn((args.lineage, d), dtype=torch.float64, device=dev, generator=gen)
        metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, True, stream=stream.cuda_stream, keep=(m1, metric))
        # the threshold: the median over a sample of rows (outside the lineage) of their (--hits + 1)-th smallest distance (a row is its own neighbour)
        sample = torch.arange(0, r1, max(r1 // 256, 1), device=dev)[:256]
        if planted:
            sample = sample[(sample < lin_lo) | (sample >= lin_lo + args.lineage)]
        q = m1[sample].contiguous()
        out = torch.empty((len(sample), r1), dtype=torch.float64, device=dev)
        work_r = torch.empty(api.dev_refset_workspace_bytes(rs, len(sample)), dtype=torch.uint8, device=dev)
        api.tune("distance_mfma", 0)
        api.dev_refset_distance_rowwise(rs, q.data_ptr(), len(sample), work_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        api.tune("distance_mfma", 1)
        T = float(torch.median(torch.kthvalue(out, min(args.hits + 1, r1), dim=1).values))
        batch = min(args.batch, r1)
        work_w = torch.empty(api.dev_neighbours_within_workspace_bytes(rs, batch, 0), dtype=torch.uint8, device=dev)
        offs = torch.zeros((div_up(r1, batch), batch + 1), dtype=torch.int64, device=dev)
        work_c = torch.empty(max(api.dev_clusters_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
        labels = torch.zeros(r1, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)

        def baseline():
            for k, lo in enumerate(range(0, r1, batch)):
                n = min(batch, r1 - lo)
                api.dev_neighbours_within(rs, m1.data_ptr() + lo * d * 8, n, T, 0, work_w.data_ptr(), offs[k].data_ptr(), None, None, stream=stream.cuda_stream)

        def clusters():
            api.dev_clusters_within(rs, T, work_c.data_ptr(), labels.data_ptr(), count.data_ptr(), stream=stream.cuda_stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        timed(baseline)
        timed(clusters)
        neighbours = int(sum(int(offs[k, min(batch, r1 - lo)]) for k, lo in enumerate(range(0, r1, batch))))
        lab = labels.to(torch.int64)
        n_clusters = int(count.item())
        assert n_clusters == int(torch.sum(lab == torch.arange(r1, device=dev)))
        assert bool(torch.all(lab <= torch.arange(r1, device=dev))) and bool(torch.equal(lab[lab], lab))
        for s, j in enumerate(sample.tolist()):  # a row's neighbours carry its label
            assert bool(torch.all(lab[out[s] <= T] == lab[j])), j
        if planted:
            assert bool(torch.all(lab[lin_lo:lin_lo + args.lineage] == lab[lin_lo])) and int(lab[lin_lo]) <= lin_lo
        largest = int(torch.bincount(lab).max())
        t_b, t_c = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(baseline)
            timed(clusters)
        for _ in range(args.repeat):
            t_b.append(timed(baseline))
            t_c.append(timed(clusters))
        ops_b, ops_c = 4.0 * r1 * r1 * d, 4.0 * r1 * (r1 - 1) / 2 * d
        line = {"case": case, "rows": r1, "dims": d, "max_distance": T, "neighbours_a_row": round(neighbours / r1, 1), "n_clusters": n_clusters,
                "largest_cluster": largest, "baseline_ms": [round(t, 3) for t in t_b], "clusters_ms": [round(t, 3) for t in t_c],
                "baseline_median_ms": round(float(np.median(t_b)), 3), "clusters_median_ms": round(float(np.median(t_c)), 3),
                "baseline_min_ms": round(min(t_b), 3), "clusters_min_ms": round(min(t_c), 3),
                "baseline_spread_ms": round(max(t_b) - min(t_b), 3), "clusters_spread_ms": round(max(t_c) - min(t_c), 3),
                "clusters_minus_baseline_median_ms": round(float(np.median(t_c) - np.median(t_b)), 3),
                "baseline_f64_valu_fraction": round(ops_b / (min(t_b) * 1e-3) / F64_OPS_PER_S, 4),
                "clusters_f64_valu_fraction": round(ops_c / (min(t_c) * 1e-3) / F64_OPS_PER_S, 4)}
        print(json.dumps(line), flush=True)
        rs.free()
        del m1, out, work_r, work_w, offs, labels
        torch.cuda.empty_cache()


def div_up(a, b):
    return (a + b - 1) // b


if __name__ == "__main__":
    main()
