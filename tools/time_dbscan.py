#!/usr/bin/env python3
"""Times DBSCAN on a resident set (kpop_dev_dbscan) against the clusters at the same distance (kpop_dev_clusters_within) on the same
resident set and the same build.  One JSON line per case:

    python tools/time_dbscan.py [--rows 100000] [--dims 64] [--repeat 5] [--min-pts 5]

The rows are the synthetic lineages of tools/time_representatives.py: rows // 100 lineage centres (standard normal), rows // 5
sub-lineages at 0.05 of their lineage's centre, and every row at 0.001 of a sub-lineage drawn at random, in random order.  Two radii,
in units of the root of the metric's sum: 0.01 joins the rows of a sub-lineage (a sparse graph: about five rows within eps of a row),
0.3 those of a lineage (a dense one: about a hundred).  The two calls alternate inside one process, each between two HIP events on the
stream it is enqueued on, after --warmup-s seconds of the same alternation untimed (tools/time_clusters.py).
kpop_clusters_within examines r1 (r1 - 1) / 2 pairs once; this call examines them once for the degrees, a second time in the tiles
that held a hit (the first bitmap: `tiles_hit` of `tiles` below) and a third time in the tiles that held a hit with one core end (the
second bitmap: `tiles_mixed`): two full passes would be a ratio of 2 by pair count.  Before the timing the result is checked: its
invariants and counts, min_pts = 1 against the clusters' labels, and for a sample of rows -- from the rowwise matrix on the vector
pipe -- the degree, the core flag of every row within eps, and the border row's choice.  A run under rocprofv3 --kernel-trace --stats (--repeat 1
--warmup-s 0) gives the split by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOISE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    ap.add_argument("--eps", type=float, nargs="+", default=[0.01, 0.3], help="in units of the root of the metric's sum")
    ap.add_argument("--min-pts", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1, d, min_pts = args.rows, args.dims, args.min_pts
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
    work_bytes = api.dev_dbscan_workspace_bytes(rs)
    work_d = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=dev)
    labels_c = torch.zeros(r1, dtype=torch.int32, device=dev)
    labels_d, core_of, degree = (torch.zeros(r1, dtype=torch.int32, device=dev) for _ in range(3))
    count_c = torch.zeros(1, dtype=torch.int32, device=dev)
    counts_d = torch.zeros(3, dtype=torch.int32, device=dev)
    rows = torch.arange(r1, device=dev)
    # the tiles of the call's grid: 32 columns x 256 rows from 65,536 rows on, 64 x 64 below; the two bitmaps (tiles with a hit, tiles
    # with a hit that has one core end) are the workspace's second and third part
    big = r1 >= 65536
    w, tj = (32, 256) if big else (64, 64)
    n_rt = (r1 + tj - 1) // tj
    n_ct = n_rt * (tj // w)
    bitmap_at = ((r1 * 4 + 255) // 256) * 256
    bitmap_words = (n_rt * n_ct + 31) // 32
    tiles = sum(min(n_ct, ((by + 1) * tj + w - 1) // w) for by in range(n_rt))  # (column tiles with a column below the row tile's end)

    def u32(t):
        return t.to(torch.int64) & 0xFFFFFFFF

    for eps_units in args.eps:
        eps = eps_units * unit

        def clusters():
            api.dev_clusters_within(rs, eps, work_c.data_ptr(), labels_c.data_ptr(), count_c.data_ptr(), stream=stream.cuda_stream)

        def dbscan(mp=min_pts):
            api.dev_dbscan(rs, eps, mp, work_d.data_ptr(), labels_d.data_ptr(), core_of.data_ptr(), degree.data_ptr(), counts_d.data_ptr(), stream=stream.cuda_stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        timed(clusters)
        lab_c = u32(labels_c)
        # min_pts = 1: the clusters' labels, bit for bit, and no noise
        timed(lambda: dbscan(1))
        assert bool(torch.equal(u32(labels_d), lab_c)) and counts_d.tolist() == [int(count_c.item()), r1, 0]
        timed(dbscan)
        lab, cof, deg = u32(labels_d), u32(core_of), u32(degree)
        n_clusters, n_core, n_noise = (int(v) for v in counts_d.tolist())
        core, noise = deg >= min_pts, lab == NOISE
        live = ~noise
        assert bool(torch.all(deg >= 1)) and n_core == int(core.sum()) and n_noise == int(noise.sum())
        assert bool(torch.equal(cof[core], rows[core])) and bool(torch.all(lab[core] <= rows[core])) and not bool(torch.any(noise & core))
        assert bool(torch.equal(noise, cof == NOISE)) and n_clusters == int(torch.sum(core & (lab == rows)))
        assert bool(torch.all(core[lab[live]])) and bool(torch.equal(lab[lab[live]], lab[live]))
        assert bool(torch.all(core[cof[live]])) and bool(torch.equal(lab[cof[live]], lab[live]))
        assert bool(torch.equal(lab_c[lab[live]], lab_c[live]))  # a cluster lies inside one component of the whole graph
        for s, j in enumerate(sample.tolist()):  # against the rowwise matrix (the row itself is in its list, at distance 0)
            near = out[s] <= eps
            assert int(near.sum()) == int(deg[j]), j
            cand = torch.nonzero(near & core).flatten()
            if bool(core[j]):
                assert bool(torch.all(lab[cand] == lab[j])), j  # core rows within eps of each other share a cluster
            elif len(cand):
                best = cand[torch.argmin(out[s][cand])]  # (the first of the least)
                assert int(best) == int(cof[j]) and int(lab[j]) == int(lab[best]), j
            else:
                assert bool(noise[j]), j
        def bits_set(at):
            words = work_d[at:at + 4 * bitmap_words].view(torch.int32).cpu().numpy().view(np.uint32)
            return int(np.unpackbits(words.view(np.uint8)).sum())

        tiles_hit, tiles_mixed = bits_set(bitmap_at), bits_set(bitmap_at + ((4 * bitmap_words + 255) // 256) * 256)
        n_border = r1 - n_core - n_noise
        t_c, t_d = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(clusters)
            timed(dbscan)
        for _ in range(args.repeat):
            t_c.append(timed(clusters))
            t_d.append(timed(dbscan))
        line = {"rows": r1, "dims": d, "eps_units": eps_units, "eps": eps, "min_pts": min_pts, "mean_degree": round(float(deg.double().mean()), 2),
                "n_core": n_core, "n_border": n_border, "n_noise": n_noise, "n_clusters": n_clusters, "n_components": int(count_c.item()),
                "tiles": tiles, "tiles_hit": tiles_hit, "tiles_hit_fraction": round(tiles_hit / max(tiles, 1), 4),
                "tiles_mixed": tiles_mixed, "tiles_mixed_fraction": round(tiles_mixed / max(tiles, 1), 4), "workspace_bytes": work_bytes,
                "clusters_ms": [round(t, 3) for t in t_c], "dbscan_ms": [round(t, 3) for t in t_d],
                "clusters_median_ms": round(float(np.median(t_c)), 3), "dbscan_median_ms": round(float(np.median(t_d)), 3),
                "clusters_spread_ms": round(max(t_c) - min(t_c), 3), "dbscan_spread_ms": round(max(t_d) - min(t_d), 3),
                "time_ratio": round(float(np.median(t_d) / np.median(t_c)), 4)}
        print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
