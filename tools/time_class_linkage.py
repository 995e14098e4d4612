#!/usr/bin/env python3
"""Times the class linkage of a labelled resident set (kpop_dev_class_linkage) against the silhouette (kpop_dev_silhouette) on the same
resident set, the same build and the same labelling.  One JSON line per number of dimensions:

    python tools/time_class_linkage.py [--rows 100000] [--dims 64 1635] [--repeat 5]

The rows are the synthetic lineages of tools/time_silhouette.py: rows // 100 lineage centres (standard normal), rows // 5 sub-lineages
at 0.05 of their lineage's centre, and every row at 0.001 of a sub-lineage drawn at random, in random order; the labelling is the
lineage a row was drawn from.  The two calls alternate inside one process, each between two HIP events on the stream it is enqueued
on, after --warmup-s seconds of the same alternation untimed.  The silhouette examines the full rectangle, r1^2 pairs; this call the
triangle of the class pairs and both orders inside a diagonal block: 0.5 + sum n_c^2 / (2 r1^2) of the rectangle (pair_ratio).
Before the timing the result is checked: class_rows against a count, the tables' symmetry and a second run bit for bit, and --check
class pairs (the diagonal among them) against the distances of their rows computed with torch in f64 (means within 1e-12 relative,
minima and maxima within 1e-13: torch's chain is not the reference's).  A run under rocprofv3 --kernel-trace --stats (--repeat 1
--warmup-s 0) gives the split by kernel: the grouping, class_linkage_sweep_kernel and class_linkage_combine_kernel."""
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
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    ap.add_argument("--check", type=int, default=6, help="class pairs checked against torch before the timing")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1 = args.rows
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
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, False, stream=stream.cuda_stream, keep=(m1, metric))
        n_classes = n_lin
        cls64 = lin_of_sub[sub_of_row].to(torch.int64)
        class_of = cls64.to(torch.int32)
        nn = n_classes * n_classes

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        work_bytes = api.dev_class_linkage_workspace_bytes(rs, n_classes)
        work_l = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=dev)
        work_s = torch.empty(max(api.dev_silhouette_workspace_bytes(rs, n_classes), 1), dtype=torch.uint8, device=dev)
        class_rows = torch.zeros(n_classes, dtype=torch.int32, device=dev)
        mean, lo_, hi_, mean2 = (torch.zeros(nn, dtype=torch.float64, device=dev) for _ in range(4))
        min_i, min_j = (torch.zeros(nn, dtype=torch.int32, device=dev) for _ in range(2))
        own, other, sil = (torch.zeros(r1, dtype=torch.float64, device=dev) for _ in range(3))
        ocls = torch.zeros(r1, dtype=torch.int32, device=dev)
        s_rows, s_med = (torch.zeros(n_classes, dtype=torch.int32, device=dev) for _ in range(2))
        s_mm = torch.zeros(n_classes, dtype=torch.float64, device=dev)

        def linkage(out=mean):
            api.dev_class_linkage(rs, class_of.data_ptr(), n_classes, work_l.data_ptr(), class_rows.data_ptr(), out.data_ptr(), lo_.data_ptr(), hi_.data_ptr(),
                                  min_i.data_ptr(), min_j.data_ptr(), stream=stream.cuda_stream)

        def silhouette():
            api.dev_silhouette(rs, class_of.data_ptr(), n_classes, work_s.data_ptr(), own.data_ptr(), other.data_ptr(), ocls.data_ptr(), sil.data_ptr(),
                               s_rows.data_ptr(), s_med.data_ptr(), s_mm.data_ptr(), stream=stream.cuda_stream)

        timed(linkage)
        timed(lambda: linkage(mean2))
        assert bool(torch.equal(mean.view(torch.int64), mean2.view(torch.int64))), "a second run gave other bits"
        sizes = torch.bincount(cls64, minlength=n_classes)
        assert bool(torch.equal(class_rows.to(torch.int64), sizes))
        for t in (mean, lo_, hi_):
            t2 = t.view(torch.int64).reshape(n_classes, n_classes)
            assert bool(torch.equal(t2, t2.T)), "a table is not symmetric"
        pick = np.random.RandomState(d).randint(0, n_classes, size=(args.check, 2))
        pick[0, 1] = pick[0, 0]  # a diagonal block
        for a, b in pick.tolist():
            xa, xb = m1[cls64 == a], m1[cls64 == b]
            dd = torch.sqrt((((xa[:, None, :] - xb[None, :, :]) ** 2) * metric).sum(-1))
            if a == b:
                dd = dd[torch.triu(torch.ones_like(dd, dtype=torch.bool), 1)]
            if dd.numel() == 0:
                continue
            e = a * n_classes + b
            assert abs(float(mean[e]) - float(dd.mean())) <= 1e-12 * float(dd.mean()), (a, b)
            assert abs(float(lo_[e]) - float(dd.min())) <= 1e-13 * float(dd.max()) and abs(float(hi_[e]) - float(dd.max())) <= 1e-13 * float(dd.max()), (a, b)
        t_l, t_s = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(linkage)
            timed(silhouette)
        for _ in range(args.repeat):
            t_l.append(timed(linkage))
            t_s.append(timed(silhouette))
        pair_ratio = 0.5 + float((sizes.to(torch.float64) ** 2).sum()) / (2.0 * r1 * r1)
        off = ~torch.eye(n_classes, dtype=torch.bool, device=dev).reshape(-1)
        line = {"rows": r1, "dims": d, "n_classes": n_classes, "smallest_class": int(sizes.min()), "largest_class": int(sizes.max()),
                "workspace_bytes": work_bytes, "class_linkage_ms": [round(t, 3) for t in t_l], "silhouette_ms": [round(t, 3) for t in t_s],
                "class_linkage_median_ms": round(float(np.median(t_l)), 3), "silhouette_median_ms": round(float(np.median(t_s)), 3),
                "class_linkage_spread_ms": round(max(t_l) - min(t_l), 3), "silhouette_spread_ms": round(max(t_s) - min(t_s), 3),
                "time_ratio": round(float(np.median(t_l) / np.median(t_s)), 4), "pair_ratio": round(pair_ratio, 4),
                "least_distance_between_classes": float(lo_[off].min()), "largest_diameter": float(torch.nan_to_num(hi_[~off], nan=0.0).max())}
        print(json.dumps(line), flush=True)
        rs.free()
        del m1, rs


if __name__ == "__main__":
    main()
