#!/usr/bin/env python3
"""Times the silhouette and the medoids of a labelled resident set (kpop_dev_silhouette) against the clusters at a distance
(kpop_dev_clusters_within) on the same resident set and the same build.  One JSON line per labelling:

    python tools/time_silhouette.py [--rows 100000] [--dims 64] [--repeat 5]

The rows are the synthetic lineages of tools/time_representatives.py and tools/time_dbscan.py: rows // 100 lineage centres (standard
normal), rows // 5 sub-lineages at 0.05 of their lineage's centre, and every row at 0.001 of a sub-lineage drawn at random, in random
order.  Two labellings: the lineage a row was drawn from (rows // 100 classes of about a hundred rows), and the labels of
kpop_dev_clusters_within at 0.3 (in units of the root of the metric's sum) made dense.  The two calls alternate inside one process,
each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the same alternation untimed
(tools/time_clusters.py).  kpop_clusters_within examines r1 (r1 - 1) / 2 pairs once; this call the full rectangle, r1^2: a ratio of 2
by pair count.  Before the timing the result is checked for a sample of rows against sums over the rowwise matrix on the vector pipe
(any order of a sum of r1 terms: within r1 2^-53 relative), the class sizes against a count, and each medoid against the least own_mean
of its class.  A run under rocprofv3 --kernel-trace --stats (--repeat 1 --warmup-s 0) gives the split by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NO_CLASS = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    ap.add_argument("--eps", type=float, default=0.3, help="the clusters' distance, in units of the root of the metric's sum")
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
    eps = args.eps * float(np.sqrt(metric_h.sum()))
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
    labels_c = torch.zeros(r1, dtype=torch.int32, device=dev)
    count_c = torch.zeros(1, dtype=torch.int32, device=dev)

    def clusters():
        api.dev_clusters_within(rs, eps, work_c.data_ptr(), labels_c.data_ptr(), count_c.data_ptr(), stream=stream.cuda_stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    timed(clusters)
    dense, n_dense, _ = api.dense_labels(labels_c.cpu().numpy().view(np.uint32))
    labellings = [("lineages", lin_of_sub[sub_of_row].cpu().numpy().astype(np.uint32), n_lin)]
    if 0 < n_dense <= 65535:
        labellings.append(("clusters_within_%g" % args.eps, dense, n_dense))
    own, other, sil = (torch.zeros(r1, dtype=torch.float64, device=dev) for _ in range(3))
    ocls = torch.zeros(r1, dtype=torch.int32, device=dev)
    tol = (r1 + 2) * 2.0 ** -52
    for name, class_h, n_classes in labellings:
        class_of = torch.from_numpy(class_h.view(np.int32)).to(dev)
        cls64 = class_of.to(torch.int64) & 0xFFFFFFFF
        work_bytes = api.dev_silhouette_workspace_bytes(rs, n_classes)
        work_s = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=dev)
        class_rows, medoid = (torch.zeros(n_classes, dtype=torch.int32, device=dev) for _ in range(2))
        medoid_mean = torch.zeros(n_classes, dtype=torch.float64, device=dev)

        def silhouette():
            api.dev_silhouette(rs, class_of.data_ptr(), n_classes, work_s.data_ptr(), own.data_ptr(), other.data_ptr(), ocls.data_ptr(), sil.data_ptr(),
                               class_rows.data_ptr(), medoid.data_ptr(), medoid_mean.data_ptr(), stream=stream.cuda_stream)

        timed(silhouette)
        sizes = torch.bincount(cls64, minlength=n_classes).to(torch.float64)
        assert bool(torch.equal(class_rows.to(torch.float64), sizes))
        for s, j in enumerate(sample.tolist()):  # against the rowwise matrix
            c = int(cls64[j])
            row = out[s].clone()
            row[j] = 0.0  # the pair of the row with itself is never examined
            sums = torch.zeros(n_classes, dtype=torch.float64, device=dev).index_add_(0, cls64, row)
            n_own = float(sizes[c]) - 1
            want_own = float(sums[c]) / n_own if n_own else 0.0
            means = sums / sizes
            means[c] = float("inf")
            means[sizes == 0] = float("inf")
            want_other = float(means.min())
            assert abs(float(own[j]) - want_own) <= tol * want_own, (name, j)
            if n_classes > 1:
                assert abs(float(other[j]) - want_other) <= tol * want_other, (name, j)
                assert abs(float(means[int(ocls[j])]) - want_other) <= 2 * tol * want_other, (name, j)
        med = medoid.to(torch.int64) & 0xFFFFFFFF
        least = torch.full((n_classes,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, cls64, own, reduce="amin")
        assert bool(torch.equal(cls64[med], torch.arange(n_classes, device=dev))) and bool(torch.equal(own[med], least))
        assert bool(torch.equal(medoid_mean, least))
        t_c, t_s = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(clusters)
            timed(silhouette)
        for _ in range(args.repeat):
            t_c.append(timed(clusters))
            t_s.append(timed(silhouette))
        # a column tile holds one class: w positions in the shape of the set's length (32 from 65,536 rows on, 64 below)
        w = 32 if r1 >= 65536 else 64
        column_tiles = int(torch.ceil(sizes / w).sum())
        line = {"rows": r1, "dims": d, "labelling": name, "n_classes": n_classes, "smallest_class": int(sizes.min()), "largest_class": int(sizes.max()),
                "column_tiles": column_tiles, "column_tile_fill": round(r1 / (column_tiles * w), 4), "mean_silhouette": round(float(torch.nanmean(sil)), 4),
                "workspace_bytes": work_bytes, "clusters_eps_units": args.eps, "clusters_ms": [round(t, 3) for t in t_c], "silhouette_ms": [round(t, 3) for t in t_s],
                "clusters_median_ms": round(float(np.median(t_c)), 3), "silhouette_median_ms": round(float(np.median(t_s)), 3),
                "clusters_spread_ms": round(max(t_c) - min(t_c), 3), "silhouette_spread_ms": round(max(t_s) - min(t_s), 3),
                "time_ratio": round(float(np.median(t_s) / np.median(t_c)), 4)}
        print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
