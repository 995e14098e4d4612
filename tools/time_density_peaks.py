#!/usr/bin/env python3
"""Times the density peaks of a resident set (kpop_dev_density_peaks) beside two calls that were there before it, on the same resident
set and the same build.  One JSON line per number of dimensions:

    python tools/time_density_peaks.py [--rows 100000] [--dims 64 1635] [--eps-quantile 0.002] [--repeat 5]

The rows are the synthetic lineages of tools/time_kmedoids.py.  Inside one process, each call between two HIP events on the stream it
is enqueued on, after --warmup-s seconds of the same alternation untimed:
    degree       kpop_dev_density_peaks with no density: the degree pass at eps, the sort, the triangle in rank order, the cut
    given        kpop_dev_density_peaks with a density given (the degrees of the call above): the sort, the triangle, the cut
    clusters     kpop_dev_clusters_within at the same eps: one folded triangle, the degree pass's kin
    silhouette   kpop_dev_silhouette with ONE class: the full rectangle, its columns gathered
THE YARDSTICKS (profiles/density_peaks.md): by pair count `given` is half a one-class silhouette plus the sort, `degree` that plus one
clusters_within.  ratio_given = given / silhouette; ratio_degree = degree / (0.5 silhouette + clusters).  eps is the --eps-quantile
quantile of the distances of 2,000 sampled rows.  The split of the call into its kernels is read from a run under rocprofv3
--kernel-trace --stats (--repeat 1 --warmup-s 0).  Before the timing the two forms are checked against each other bit for bit, the
density against kpop_dev_dbscan's degree, and a second run against the first."""
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
    ap.add_argument("--eps-quantile", type=float, default=0.002)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1 = args.rows
    inf = float("inf")
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
        metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
        sample = m1[torch.randperm(r1, device=dev, generator=gen)[:min(2000, r1)]] * metric.sqrt()
        dist = torch.cdist(sample, sample)
        eps = float(torch.quantile(dist[dist > 0][:1 << 22], args.eps_quantile).item())
        del sample, dist
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

        def u32(n):
            return torch.zeros(n, dtype=torch.int32, device=dev)

        density, delta, delta2, own = (f64(r1) for _ in range(4))
        parent, parent2, labels, labels2, one_class, comp, degree, db_labels = (u32(r1) for _ in range(8))
        counts, counts2, n_comp, db_counts = (u32(64) for _ in range(4))
        work = torch.empty(api.dev_density_peaks_workspace_bytes(rs), dtype=torch.uint8, device=dev)
        work_c = torch.empty(max(api.dev_clusters_within_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
        work_s = torch.empty(api.dev_silhouette_workspace_bytes(rs, 1), dtype=torch.uint8, device=dev)
        work_d = torch.empty(api.dev_dbscan_workspace_bytes(rs), dtype=torch.uint8, device=dev)

        def by_degree():
            api.dev_density_peaks(rs, eps, work.data_ptr(), None, -inf, eps, density.data_ptr(), delta.data_ptr(), parent.data_ptr(), labels.data_ptr(),
                                  counts.data_ptr(), stream=stream.cuda_stream)

        def given():
            api.dev_density_peaks(rs, eps, work.data_ptr(), density.data_ptr(), -inf, eps, None, delta2.data_ptr(), parent2.data_ptr(), labels2.data_ptr(),
                                  counts2.data_ptr(), stream=stream.cuda_stream)

        def clusters():
            api.dev_clusters_within(rs, eps, work_c.data_ptr(), comp.data_ptr(), n_comp.data_ptr(), stream=stream.cuda_stream)

        def silhouette():
            api.dev_silhouette(rs, one_class.data_ptr(), 1, work_s.data_ptr(), own.data_ptr(), stream=stream.cuda_stream)

        calls = [("degree", by_degree), ("given", given), ("clusters", clusters), ("silhouette", silhouette)]
        timed(by_degree)
        first = (delta.clone(), parent.clone(), labels.clone())
        timed(given)
        assert bool(torch.equal(delta.view(torch.int64), delta2.view(torch.int64))) and bool(torch.equal(parent, parent2)) and bool(torch.equal(labels, labels2)), \
            "the two forms disagree"
        with torch.cuda.stream(stream):
            api.dev_dbscan(rs, eps, 1, work_d.data_ptr(), db_labels.data_ptr(), None, degree.data_ptr(), db_counts.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert bool(torch.equal(density, degree.to(torch.float64))), "the density is not dbscan's degree"
        timed(by_degree)
        assert all(bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b))
                   for a, b in zip(first, (delta, parent, labels))), "a second run gave other bits"
        t = {name: [] for name, _ in calls}
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            for _, fn in calls:
                timed(fn)
        for _ in range(args.repeat):
            for name, fn in calls:
                t[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in t.items()}
        n = counts.cpu().numpy()
        line = {"rows": r1, "dims": d, "eps": eps}
        for name, _ in calls:
            line[name + "_ms"] = [round(x, 3) for x in t[name]]
            line[name + "_median_ms"] = round(med[name], 3)
        line.update({"ratio_given": round(med["given"] / med["silhouette"], 4),
                     "ratio_degree": round(med["degree"] / (0.5 * med["silhouette"] + med["clusters"]), 4),
                     "mean_density": float(density.mean().item()), "max_density": float(density.max().item()), "centres": int(n[0]), "roots": int(n[1]),
                     "components_at_eps": int(n_comp[0].item()), "workspace_bytes": int(work.numel())})
        print(json.dumps(line), flush=True)
        rs.free()
        del m1, rs


if __name__ == "__main__":
    main()
