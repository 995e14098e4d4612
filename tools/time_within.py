#!/usr/bin/env python3
"""Times the range query (kpop_dev_neighbours_within) against the call that does the same arithmetic and stores every distance
(kpop_dev_refset_distance_rowwise on the vector pipe, kpop_tune("distance_mfma", 0)), on the same device-resident operands, and prints
one JSON line per shape and threshold:

    python tools/time_within.py --shape 256x650000x64 [--shape 256x650000x1635] [--repeat 7] [--hits 300] [--host]

The two calls alternate inside one process, each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of
the same alternation untimed (the set's divided copy is made by the first call that needs it; the clock takes tens of calls of a
few milliseconds to settle, and a series that still drifts has a spread that says nothing).  Every timing is listed, with the rowwise call's own spread
(max - min over its repeats): the range query is expected to stay within that spread of the rowwise call.  Two thresholds: the
median over the query rows of their `--hits`-th smallest distance (about that many hits a row), and -1 (none).  --host adds the
host-to-host legs: RefSet.distance_rowwise + a numpy filter and sort against RefSet.within, wall clock.  The share of the vector
pipe's f64 rate counts 4 operations a pair and dimension (subtract, square, times the metric, add: nothing is fused) against
256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.  A run under rocprofv3 --kernel-trace --stats
(--repeat 2) gives the split by kernel."""
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
    ap.add_argument("--shape", action="append", required=True, help="QUERIESxROWSxDIMS, may be given several times")
    ap.add_argument("--repeat", type=int, default=25, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=2.0, help="seconds of untimed alternating calls before each timed series")
    ap.add_argument("--hits", type=int, default=300, help="hits a row the first threshold aims at")
    ap.add_argument("--host", action="store_true", help="also the host-to-host legs (the set is downloaded and made again from host memory)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    api.tune("distance_mfma", 0)  # the baseline on the vector pipe: the same arithmetic as the range query
    for shape in args.shape:
        r2, r1, d = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(r1 + d)
        m1 = torch.empty((r1, d), dtype=torch.float64, device=dev)
        for lo in range(0, r1, 65536):  # (a slab at a time: the generator's scratch stays small)
            m1[lo:lo + 65536] = torch.randn((min(65536, r1 - lo), d), dtype=torch.float64, device=dev, generator=gen)
        m2 = torch.randn((r2, d), dtype=torch.float64, device=dev, generator=gen)
        metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, True, stream=stream.cuda_stream, keep=(m1, metric))
        out = torch.empty((r2, r1), dtype=torch.float64, device=dev)
        work_r = torch.empty(api.dev_refset_workspace_bytes(rs, r2), dtype=torch.uint8, device=dev)
        capacity = 4 * args.hits * r2
        work_w = torch.empty(api.dev_neighbours_within_workspace_bytes(rs, r2, capacity), dtype=torch.uint8, device=dev)
        offs = torch.zeros(r2 + 1, dtype=torch.int64, device=dev)
        idx = torch.zeros(capacity, dtype=torch.int32, device=dev)
        dist = torch.zeros(capacity, dtype=torch.float64, device=dev)

        def rowwise():
            api.dev_refset_distance_rowwise(rs, m2.data_ptr(), r2, work_r.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)

        def within(T):
            api.dev_neighbours_within(rs, m2.data_ptr(), r2, T, capacity, work_w.data_ptr(), offs.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                                      stream=stream.cuda_stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        timed(rowwise)  # warm-up; and the distances the first threshold is read from
        kth = torch.kthvalue(out, min(args.hits, r1), dim=1).values
        thresholds = [("about %d hits a row" % args.hits, float(torch.median(kth))), ("no hit", -1.0)]
        for name, T in thresholds:
            timed(lambda: within(T))
            total = int(offs[r2])
            assert total <= capacity, (total, capacity)
            if total:  # the lists against the matrix, on the device: sorted hits of every row
                o = offs.cpu().numpy()
                for j in (0, r2 // 2, r2 - 1):
                    row = out[j]
                    want = torch.nonzero(row <= T).flatten()
                    want = want[torch.argsort(row[want], stable=True)]
                    got = idx[int(o[j]):int(o[j + 1])].to(torch.int64)
                    assert torch.equal(got, want) and torch.equal(dist[int(o[j]):int(o[j + 1])], row[want]), (name, j)
            t_r, t_w = [], []
            t_end = time.perf_counter() + args.warmup_s
            while time.perf_counter() < t_end:
                timed(rowwise)
                timed(lambda: within(T))
            for _ in range(args.repeat):
                t_r.append(timed(rowwise))
                t_w.append(timed(lambda: within(T)))
            ops = 4.0 * r1 * r2 * d
            line = {"queries": r2, "rows": r1, "dims": d, "threshold": name, "max_distance": T, "neighbours": total,
                    "rowwise_ms": [round(t, 4) for t in t_r], "within_ms": [round(t, 4) for t in t_w],
                    "rowwise_min_ms": round(min(t_r), 4), "within_min_ms": round(min(t_w), 4),
                    "rowwise_median_ms": round(float(np.median(t_r)), 4), "within_median_ms": round(float(np.median(t_w)), 4),
                    "rowwise_spread_ms": round(max(t_r) - min(t_r), 4), "within_spread_ms": round(max(t_w) - min(t_w), 4),
                    "rowwise_first_half_median_ms": round(float(np.median(t_r[:len(t_r) // 2])), 4),
                    "rowwise_second_half_median_ms": round(float(np.median(t_r[len(t_r) // 2:])), 4),
                    "within_minus_rowwise_median_ms": round(float(np.median(t_w) - np.median(t_r)), 4),
                    "rowwise_f64_valu_fraction": round(ops / (min(t_r) * 1e-3) / F64_OPS_PER_S, 4),
                    "within_f64_valu_fraction": round(ops / (min(t_w) * 1e-3) / F64_OPS_PER_S, 4),
                    "matrix_bytes_not_written": r1 * r2 * 8, "workspace_bytes": work_w.numel()}
            print(json.dumps(line), flush=True)
        if args.host:
            h1, h2, hm = m1.cpu().numpy(), m2.cpu().numpy(), metric.cpu().numpy()
            T = thresholds[0][1]
            rs.free()
            rs = kpop_amd.RefSet(h1, hm, api.EUCLIDEAN, 2.0, True)
            legs = {"rowwise_and_numpy_filter_s": [], "within_s": []}
            for it in range(1 + min(args.repeat, 3)):
                t0 = time.perf_counter()
                full = rs.distance_rowwise(h2)
                lists = []
                for j in range(r2):
                    hit = np.nonzero(full[j] <= T)[0]
                    lists.append(hit[np.lexsort((hit, full[j][hit]))])
                t1 = time.perf_counter()
                o, i, x = rs.within(h2, T)
                t2 = time.perf_counter()
                assert all(np.array_equal(i[int(o[j]):int(o[j + 1])], lists[j]) for j in range(r2))
                if it:
                    legs["rowwise_and_numpy_filter_s"].append(round(t1 - t0, 5))
                    legs["within_s"].append(round(t2 - t1, 5))
            print(json.dumps(dict({"queries": r2, "rows": r1, "dims": d, "leg": "host to host", "neighbours": int(o[r2])}, **legs)), flush=True)
        rs.free()
        del m1, m2, out, work_r, work_w, idx, dist
        torch.cuda.empty_cache()
    api.tune("distance_mfma", 1)


if __name__ == "__main__":
    main()
