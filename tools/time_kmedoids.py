#!/usr/bin/env python3
"""Times k-medoids on a resident set (kpop_dev_kmedoids) beside the two one-shot calls whose halves it joins, on the same resident set
and the same build.  One JSON line per k:

    python tools/time_kmedoids.py [--rows 100000] [--dims 64] [--k 10 100 1000] [--repeat 5]

The rows are the synthetic lineages of tools/time_silhouette.py.  The initial medoids are the first k farthest-first picks.  Inside one
process, each call between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the same alternation untimed:
    round        kpop_dev_kmedoids at max_iter = 0: one assignment to the k picks, one within-class pass, one update
    silhouette   kpop_dev_silhouette on the labelling that round left: the full rectangle, r1^2 pairs, where the within-class pass
                 takes the sum of n_c^2 (pair_ratio)
    seeds        kpop_dev_farthest_first with the same k rows as forced seeds and max_picks = k: ceil(k / 32) passes over the set,
                 the pair count of the one assignment
    whole        kpop_kmedoids from the same picks to convergence (the host form: the done word read back every round)
    idle_round   the device form's cost per enqueued round behind the stop: (max_iter = 8 from a fixed point) - (max_iter = 0), over 8
The split of a round into its kernels (assignment, within-class pass) is read from a run under rocprofv3 --kernel-trace --stats
(--repeat 1 --warmup-s 0).  Before the timing the round's own_mean is checked against kpop_dev_silhouette's bit for bit."""
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
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
    ap.add_argument("--max-iter", type=int, default=100)
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

    k_max = max(args.k)
    picks = rs.farthest_first(max_picks=k_max).pick
    class_of = torch.zeros(r1, dtype=torch.int32, device=dev)
    dist, own, own_s = (torch.zeros(r1, dtype=torch.float64, device=dev) for _ in range(3))
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    for k in args.k:
        init_h = picks[:k].copy()
        d_init = torch.from_numpy(init_h.view(np.int32)).to(dev)
        medoid, class_rows = (torch.zeros(k, dtype=torch.int32, device=dev) for _ in range(2))
        work = {mi: torch.empty(api.dev_kmedoids_workspace_bytes(rs, k, mi), dtype=torch.uint8, device=dev) for mi in (0, 8)}
        work_s = torch.empty(api.dev_silhouette_workspace_bytes(rs, k), dtype=torch.uint8, device=dev)
        work_f = torch.empty(api.dev_farthest_first_workspace_bytes(rs, k), dtype=torch.uint8, device=dev)
        counts_f = torch.zeros(2, dtype=torch.int32, device=dev)

        def one_round(init=d_init, max_iter=0):
            api.dev_kmedoids(rs, k, init.data_ptr(), max_iter, work[max_iter].data_ptr(), counts.data_ptr(), medoid.data_ptr(), class_of.data_ptr(), dist.data_ptr(),
                             own.data_ptr(), class_rows.data_ptr(), stream=stream.cuda_stream)

        def silhouette():
            api.dev_silhouette(rs, class_of.data_ptr(), k, work_s.data_ptr(), own_s.data_ptr(), stream=stream.cuda_stream)

        def seeds():
            api.dev_farthest_first(rs, k, -1.0, work_f.data_ptr(), counts_f.data_ptr(), d_seeds=d_init.data_ptr(), n_seeds=k, stream=stream.cuda_stream)

        def whole():
            return rs.kmedoids(init_h, args.max_iter)

        timed(one_round)
        timed(silhouette)
        assert bool(torch.equal(own.view(torch.int64), own_s.view(torch.int64))), "own_mean is not the silhouette's"
        sizes = class_rows.cpu().numpy().astype(np.float64)
        assert sizes.sum() == r1
        t0 = time.perf_counter()
        res = whole()
        first_whole_ms = (time.perf_counter() - t0) * 1e3
        fixed = torch.from_numpy(res.medoid.view(np.int32).copy()).to(dev)
        t = {name: [] for name in ("round", "silhouette", "seeds", "whole", "idle0", "idle8")}
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            for fn in (one_round, silhouette, seeds):
                timed(fn)
        for _ in range(args.repeat):
            t["round"].append(timed(one_round))
            t["silhouette"].append(timed(silhouette))
            t["seeds"].append(timed(seeds))
            t["idle0"].append(timed(lambda: one_round(fixed, 0)))
            t["idle8"].append(timed(lambda: one_round(fixed, 8)))
            t0 = time.perf_counter()
            whole()
            t["whole"].append((time.perf_counter() - t0) * 1e3)
        timed(one_round)  # (class_of is the first round's again)
        med = {name: float(np.median(v)) for name, v in t.items()}
        line = {"rows": r1, "dims": d, "k": k, "smallest_class": int(sizes.min()), "largest_class": int(sizes.max()),
                "pair_ratio": round(float((sizes ** 2).sum()) / float(r1) ** 2, 5), "farthest_first_passes": -(-k // 32),
                "round_ms": [round(x, 3) for x in t["round"]], "silhouette_ms": [round(x, 3) for x in t["silhouette"]], "seeds_ms": [round(x, 3) for x in t["seeds"]],
                "round_median_ms": round(med["round"], 3), "silhouette_median_ms": round(med["silhouette"], 3), "seeds_median_ms": round(med["seeds"], 3),
                "round_over_silhouette": round(med["round"] / med["silhouette"], 4), "round_over_seeds": round(med["round"] / med["seeds"], 4),
                "whole_median_ms": round(med["whole"], 3), "first_whole_ms": round(first_whole_ms, 3), "rounds_to_convergence": int(res.n_iter),
                "converged": bool(res.converged), "cost_first": float(res.cost[0]), "cost_last": float(res.cost[-1]),
                "idle_round_ms": round((med["idle8"] - med["idle0"]) / 8, 4), "workspace_bytes": int(work[0].numel())}
        print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
