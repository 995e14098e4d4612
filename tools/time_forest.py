#!/usr/bin/env python3
"""Times the single-linkage tree (kpop_dev_spanning_forest, max_distance = +inf: the whole tree) against one pass of the same
arithmetic on the same resident set: the clusters at a distance (kpop_dev_clusters_within) at a threshold that gives about --hits
neighbours a row.  One JSON line:

    python tools/time_forest.py [--rows 100000] [--dims 64] [--centres 1000] [--hits 30] [--repeat 5]

The set is clustered: --centres points, every row one of them plus noise of a twentieth.  The two calls alternate inside one process,
each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the same alternation untimed
(tools/time_clusters.py).  The forest's cost model is rounds x passes: a round computes every pair from both ends (two of the clusters'
half passes) less the tiles it skips.  The rounds that ran are read from the head of the workspace, where the call keeps what each
round added.  Before the timing the forest is checked: r1 - 1 edges in ascending order, one component, and its cut at the threshold
(kpop_forest_cut) against the clusters' labels."""
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
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--hits", type=int, default=30, help="neighbours a row the clusters' threshold aims at")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=2.0, help="seconds of untimed alternating calls before the timed series")
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
    centres = torch.randn((args.centres, d), dtype=torch.float64, device=dev, generator=gen)
    which = torch.randint(args.centres, (r1,), device=dev, generator=gen)
    m1 = centres[which] + 0.05 * torch.randn((r1, d), dtype=torch.float64, device=dev, generator=gen)
    metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, False, stream=stream.cuda_stream, keep=(m1, metric))
    sample = torch.arange(0, r1, max(r1 // 256, 1), device=dev)[:256]
    q = m1[sample].contiguous()
    out = torch.empty((len(sample), r1), dtype=torch.float64, device=dev)
    work_r = torch.empty(api.dev_refset_workspace_bytes(rs, len(sample)), dtype=torch.uint8, device=dev)
    api.tune("distance_mfma", 0)
    api.dev_refset_distance_rowwise(rs, q.data_ptr(), len(sample), work_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    api.tune("distance_mfma", 1)
    T = float(torch.median(torch.kthvalue(out, min(args.hits + 1, r1), dim=1).values))
    work_c = torch.empty(max(api.dev_clusters_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
    labels_c = torch.zeros(r1, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    work_f = torch.empty(api.dev_spanning_forest_workspace_bytes(rs), dtype=torch.uint8, device=dev)
    n_edges = torch.zeros(1, dtype=torch.int32, device=dev)
    ei, ej = torch.zeros(r1 - 1, dtype=torch.int32, device=dev), torch.zeros(r1 - 1, dtype=torch.int32, device=dev)
    ed = torch.zeros(r1 - 1, dtype=torch.float64, device=dev)
    labels_f = torch.zeros(r1, dtype=torch.int32, device=dev)

    def clusters():
        api.dev_clusters_within(rs, T, work_c.data_ptr(), labels_c.data_ptr(), count.data_ptr(), stream=stream.cuda_stream)

    def forest():
        api.dev_spanning_forest(rs, float("inf"), work_f.data_ptr(), n_edges.data_ptr(), ei.data_ptr(), ej.data_ptr(), ed.data_ptr(), labels_f.data_ptr(),
                                stream=stream.cuda_stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    timed(clusters)
    timed(forest)
    added = work_f[:4 * 33].cpu().numpy().view(np.uint32)
    enqueued = int(np.ceil(np.log2(r1)))
    rounds = min(int(np.count_nonzero(added)) + 1, enqueued)  # (the round that finds nothing to add runs too, unless none is left)
    hi, hj, hd = ei.cpu().numpy().view(np.uint32), ej.cpu().numpy().view(np.uint32), ed.cpu().numpy()
    assert int(n_edges.item()) == r1 - 1 and int(added.sum()) == r1 - 1 and not bool(labels_f.any())
    assert np.all(hi < hj) and np.array_equal(np.lexsort((hj, hi, hd)), np.arange(r1 - 1))
    cut = kpop_amd.forest_cut(r1, hi, hj, hd, T)
    assert np.array_equal(cut[0], labels_c.cpu().numpy().view(np.uint32)) and cut[1] == int(count.item())
    t_c, t_f = [], []
    t_end = time.perf_counter() + args.warmup_s
    while time.perf_counter() < t_end:
        timed(clusters)
        timed(forest)
    for _ in range(args.repeat):
        t_c.append(timed(clusters))
        t_f.append(timed(forest))
    try:
        clock_mhz = int(torch.cuda.clock_rate())  # (right after the timed series: the clock under load)
    except Exception:
        clock_mhz = None
    line = {"rows": r1, "dims": d, "centres": args.centres, "clusters_max_distance": T, "n_clusters_at_it": int(count.item()),
            "edges_added_a_round": [int(a) for a in added[:rounds]], "rounds": rounds, "rounds_enqueued": enqueued,
            "clusters_ms": [round(t, 3) for t in t_c], "forest_ms": [round(t, 3) for t in t_f],
            "clusters_median_ms": round(float(np.median(t_c)), 3), "forest_median_ms": round(float(np.median(t_f)), 3),
            "clusters_spread_ms": round(max(t_c) - min(t_c), 3), "forest_spread_ms": round(max(t_f) - min(t_f), 3),
            "forest_over_clusters": round(float(np.median(t_f) / np.median(t_c)), 2),
            "forest_over_clusters_a_round": round(float(np.median(t_f) / np.median(t_c)) / rounds, 2), "clock_mhz": clock_mhz}
    print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
