#!/usr/bin/env python3
"""Times the mutual-reachability forest (kpop_dev_reachability_tree) beside the two calls it is made of, on the same resident set in the
same process: the single-linkage tree (kpop_dev_spanning_forest, the same cap) and the leave-one-out pass of the k-NN validation
(kpop_dev_knn_validate at k = min_pts - 1, two classes), and beside its own first half (kpop_dev_core_distances).  One JSON line per
(min_pts, cap):

    python tools/time_reachability.py [--rows 100000] [--dims 64] [--centres 1000] [--min-pts 5 33] [--hits 30] [--repeat 5]

The set is tools/time_forest.py's: --centres points, every row one of them plus noise of a twentieth.  Two caps: +inf (the whole tree)
and the distance that gives about --hits neighbours a row (a small quantile of the matrix).  The calls alternate inside one process,
each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the same alternation untimed.  The
expectation under test: the forest part (the call less its core distances) costs what the plain forest costs a round.  The rounds that
ran are read from the workspaces, where the rounds keep what each added.  Before the timing the results are checked: min_pts = 1
against the plain forest array for array, the core distances of a sample of rows against the rowwise matrix on the vector pipe, the
edges ascending and no lighter than their ends' core distances, and the cut at the cap (kpop_reachability_cut) against
kpop_dev_dbscan's labels on the core rows."""
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
    ap.add_argument("--min-pts", type=int, nargs="+", default=[5, 33])
    ap.add_argument("--hits", type=int, default=30, help="neighbours a row the finite cap aims at")
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
    work_f = torch.empty(api.dev_spanning_forest_workspace_bytes(rs), dtype=torch.uint8, device=dev)
    work_d = torch.empty(max(api.dev_dbscan_workspace_bytes(rs), 1), dtype=torch.uint8, device=dev)
    n_edges = torch.zeros(1, dtype=torch.int32, device=dev)
    ei, ej = torch.zeros(r1 - 1, dtype=torch.int32, device=dev), torch.zeros(r1 - 1, dtype=torch.int32, device=dev)
    ed = torch.zeros(r1 - 1, dtype=torch.float64, device=dev)
    labels = torch.zeros(r1, dtype=torch.int32, device=dev)
    core = torch.zeros(r1, dtype=torch.float64, device=dev)
    core_alone = torch.zeros(r1, dtype=torch.float64, device=dev)
    db_labels, db_degree = torch.zeros(r1, dtype=torch.int32, device=dev), torch.zeros(r1, dtype=torch.int32, device=dev)
    db_counts = torch.zeros(3, dtype=torch.int32, device=dev)
    class_of = (which % 2).to(torch.int32)
    knn_out = [torch.zeros(r1, dtype=torch.int32, device=dev) for _ in range(3)]
    knn_correct = torch.zeros(1, dtype=torch.int64, device=dev)
    enqueued = int(np.ceil(np.log2(r1)))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    def rounds_of(work, at):
        added = work[at:at + 4 * 33].cpu().numpy().view(np.uint32)
        return min(int(np.count_nonzero(added)) + 1, enqueued), added  # (the round that finds nothing to add runs too, unless none is left)

    def host(t):
        return t.cpu().numpy()

    for min_pts in args.min_pts:
        k = min_pts - 1
        work_bytes = api.dev_reachability_forest_workspace_bytes(rs, min_pts)
        core_bytes = api.dev_core_distances_workspace_bytes(rs, min_pts)
        work_m = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
        work_c = torch.empty(core_bytes, dtype=torch.uint8, device=dev)
        work_k = torch.empty(api.dev_knn_validate_workspace_bytes(rs, r1, k, 2), dtype=torch.uint8, device=dev)
        words_at = ((r1 * 8 + 255) // 256) * 256  # the rounds' words: behind the workspace's core distances

        def reach(mp=min_pts, cap=float("inf")):
            api.dev_reachability_forest(rs, mp, cap, work_m.data_ptr(), n_edges.data_ptr(), ei.data_ptr(), ej.data_ptr(), ed.data_ptr(), core.data_ptr(),
                                        labels.data_ptr(), stream=stream.cuda_stream)

        def forest(cap=float("inf")):
            api.dev_spanning_forest(rs, cap, work_f.data_ptr(), n_edges.data_ptr(), ei.data_ptr(), ej.data_ptr(), ed.data_ptr(), labels.data_ptr(),
                                    stream=stream.cuda_stream)

        def cores():
            api.dev_core_distances(rs, min_pts, work_c.data_ptr(), core_alone.data_ptr(), stream=stream.cuda_stream)

        def leave_one_out():
            api.dev_knn_validate(rs, class_of.data_ptr(), 2, None, 0, r1, (k,), work_k.data_ptr(), knn_out[0].data_ptr(), knn_out[1].data_ptr(),
                                 knn_out[2].data_ptr(), None, knn_correct.data_ptr(), stream=stream.cuda_stream)

        # min_pts = 1 is the plain forest, array for array
        timed(forest)
        plain = [host(t).copy() for t in (n_edges, ei, ej, ed, labels)]
        timed(lambda: reach(1))
        assert all(np.array_equal(a, host(t)) for a, t in zip(plain, (n_edges, ei, ej, ed, labels))) and not bool(core.any())
        for cap_name, cap in (("inf", float("inf")), ("hits", T)):
            timed(lambda: forest(cap))
            rounds_f, _ = rounds_of(work_f, 0)
            edges_f = int(n_edges.item())
            timed(lambda: reach(cap=cap))
            rounds_m, added = rounds_of(work_m, words_at)
            n = int(n_edges.item())
            hi, hj, hd = host(ei).view(np.uint32)[:n], host(ej).view(np.uint32)[:n], host(ed)[:n]
            hc, hl = host(core), host(labels).view(np.uint32)
            timed(cores)
            assert np.array_equal(host(core_alone), hc) and np.isfinite(hc).all()
            # the sample's core distances from the rowwise matrix: the row itself is in its row, at distance 0, so the min_pts-th least
            assert np.array_equal(host(torch.kthvalue(out, min_pts, dim=1).values), hc[host(sample)])
            assert int(added.sum()) == n and n == r1 - int(np.sum(hl == np.arange(r1)))
            assert np.all(hi < hj) and np.array_equal(np.lexsort((hj, hi, hd)), np.arange(n))
            assert np.all(hd >= np.maximum(hc[hi], hc[hj])) and (n == 0 or hd[-1] <= cap)
            # the cut at T is DBSCAN* there: dbscan's labels on the core rows
            api.dev_dbscan(rs, T, min_pts, work_d.data_ptr(), db_labels.data_ptr(), None, db_degree.data_ptr(), db_counts.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            is_core = host(db_degree).view(np.uint32) >= min_pts
            cut, counts = kpop_amd.reachability_cut(r1, hi, hj, hd, hc, T)
            assert np.array_equal(hc <= T, is_core) and np.array_equal(cut[is_core], host(db_labels).view(np.uint32)[is_core])
            assert counts.tolist()[:2] == host(db_counts).tolist()[:2] and np.all(cut[~is_core] == 0xFFFFFFFF)
            series = {"forest": lambda: forest(cap), "reachability": lambda: reach(cap=cap), "core_distances": cores, "leave_one_out": leave_one_out}
            times = {name: [] for name in series}
            t_end = time.perf_counter() + args.warmup_s
            while time.perf_counter() < t_end:
                for fn in series.values():
                    timed(fn)
            for _ in range(args.repeat):
                for name, fn in series.items():
                    times[name].append(timed(fn))
            try:
                clock_mhz = int(torch.cuda.clock_rate())  # (right after the timed series: the clock under load)
            except Exception:
                clock_mhz = None
            med = {name: float(np.median(t)) for name, t in times.items()}
            line = {"rows": r1, "dims": d, "centres": args.centres, "min_pts": min_pts, "cap": cap_name, "max_distance": cap, "hits_distance": T,
                    "edges": n, "distinct_weights": int(len(np.unique(hd))), "plain_edges": edges_f, "core_rows_at_hits_distance": int(is_core.sum()),
                    "clusters_at_hits_distance": int(counts[0]), "rounds": rounds_m, "plain_rounds": rounds_f, "rounds_enqueued": enqueued,
                    "workspace_bytes": work_bytes, "core_workspace_bytes": core_bytes, "plain_workspace_bytes": int(work_f.numel())}
            for name, t in times.items():
                line[name + "_ms"] = [round(v, 3) for v in t]
                line[name + "_median_ms"] = round(med[name], 3)
                line[name + "_spread_ms"] = round(max(t) - min(t), 3)
            line["forest_part_ms"] = round(med["reachability"] - med["core_distances"], 3)
            line["forest_part_ms_a_round"] = round((med["reachability"] - med["core_distances"]) / rounds_m, 3)
            line["plain_ms_a_round"] = round(med["forest"] / rounds_f, 3)
            line["core_over_leave_one_out"] = round(med["core_distances"] / med["leave_one_out"], 3)
            line["clock_mhz"] = clock_mhz
            print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
