#!/usr/bin/env python3
"""Times the farthest-first traversal (kpop_farthest_first) beside the representatives at a distance (kpop_representatives_within) on
the same resident set and the same build.  One JSON line per case:

    python tools/time_farthest_first.py [--rows 100000] [--dims 64] [--repeat 5]

The rows are those of tools/time_representatives.py: rows // 100 lineage centres (standard normal), rows // 5 sub-lineages at 0.05 of
their lineage's centre, every row at 0.001 of a sub-lineage drawn at random; euclidean, not normalised, metric linspace(1, 0.25).  Two
runs: max_picks = --picks without a radius, and a cover_radius of --threshold (in units of the root of the metric's sum: 0.3 keeps
about one row a lineage) without a count; beside the second, kpop_representatives_within at that radius.  All three are the host forms,
timed by the wall clock around the call (they synchronise), alternating inside one process after --warmup-s seconds of the same
alternation untimed.  A pass reads every row and its key once: rows x (dims + 1) x 8 bytes, which with the kernel's share of a run
under rocprofv3 --kernel-trace --stats (--repeat 1 --warmup-s 0) gives the pass kernel's bytes a second.  Before the timing the result
is checked: the picks distinct, the radii falling, and for a sample of rows -- from the rowwise matrix on the vector pipe -- that
rep_dist is the least distance to a pick and rep_of the first pick at it."""
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
    ap.add_argument("--picks", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=0.3, help="in units of the root of the metric's sum")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=1.0, help="seconds of untimed alternating calls before the timed series")
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
    T = args.threshold * float(np.sqrt(metric_h.sum()))
    metric = torch.from_numpy(metric_h).to(dev)
    torch.cuda.synchronize()
    rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, False, keep=(m1, metric))
    rows_h = m1.cpu().numpy()

    def by_count():
        return rs.farthest_first(max_picks=args.picks)

    def by_radius():
        return rs.farthest_first(cover_radius=T)

    def representatives():
        return rs.representatives(T)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        return (time.perf_counter() - t0) * 1e3, res

    results = {}
    for name, fn in (("by_count", by_count), ("by_radius", by_radius)):
        got = timed(fn)[1]
        n = len(got.pick)
        assert n >= 1 and len(set(got.pick.tolist())) == n and 1 <= got.n_passes <= n
        assert np.all(got.pick_radius[2:] <= got.pick_radius[1:-1])
        sample = np.arange(0, r1, max(r1 // 64, 1))[:64]
        api.tune("distance_mfma", 0)
        Dp = kpop_amd.RefSet(rows_h[got.pick], metric_h, api.EUCLIDEAN, 2.0, False)
        try:
            D = Dp.distance_rowwise(rows_h[sample]) + 0.0  # [sample][pick]
        finally:
            Dp.free()
            api.tune("distance_mfma", 1)
        picked = np.isin(sample, got.pick)
        least = D.min(axis=1)
        first = got.pick[np.argmax(D == least[:, None], axis=1)]
        assert np.array_equal(got.rep_dist[sample][~picked], least[~picked]) and np.array_equal(got.rep_of[sample][~picked], first[~picked])
        if name == "by_radius":
            assert np.all(got.rep_dist <= T) and np.all(got.pick_radius > T)
        results[name] = got
    n_reps = representatives()[2]
    times = {"by_count": [], "by_radius": [], "representatives": []}
    calls = (("by_count", by_count), ("by_radius", by_radius), ("representatives", representatives))
    t_end = time.perf_counter() + args.warmup_s
    while time.perf_counter() < t_end:
        for _, fn in calls:
            timed(fn)
    for _ in range(args.repeat):
        for name, fn in calls:
            times[name].append(timed(fn)[0])
    pass_bytes = float(r1) * (d + 1) * 8
    line = {"rows": r1, "dims": d, "library": os.environ.get("KPOP_HIP_LIB", "built"), "max_distance": T, "pass_bytes": pass_bytes}
    for name in ("by_count", "by_radius"):
        got, t = results[name], times[name]
        line[name] = {"n_picks": len(got.pick), "n_passes": got.n_passes, "passes_per_pick": round(got.n_passes / len(got.pick), 4),
                      "last_radius": float(got.pick_radius[-1]), "ms": [round(x, 3) for x in t], "median_ms": round(float(np.median(t)), 3),
                      "spread_ms": round(max(t) - min(t), 3), "ms_per_pass": round(float(np.median(t)) / got.n_passes, 5)}
    t = times["representatives"]
    line["representatives"] = {"n_reps": n_reps, "ms": [round(x, 3) for x in t], "median_ms": round(float(np.median(t)), 3), "spread_ms": round(max(t) - min(t), 3)}
    print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
