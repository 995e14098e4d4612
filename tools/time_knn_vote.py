#!/usr/bin/env python3
"""Times the k-NN vote (kpop_dev_knn_vote) against the only way to the same answer without it: kpop_dev_refset_distance_summary with
keep_at_most = k (whose neighbour arrays the host then votes over), on the same device-resident operands, and prints one JSON line per
shape:

    python tools/time_knn_vote.py --shape 256x1000000x64 [--shape 4096x100000x64] [--duplicates 256x1000000x64] [--k 5] [--repeat 15]

The two calls alternate inside one process, each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of
the same alternation untimed (the set's divided copy and scalars are made by the first calls that need them).  Every timing is listed;
the medians and the spreads (max - min) are what to compare.  The summary call alone is the bar: the host vote over its arrays comes on
top of it and is timed apart (vote_host_ms, numpy, wall clock), as are the bytes a query row sends over the bus either way.  Before the
timing the two answers are compared (answers_agree): the same list lengths, the same classes and votes from the summary's idx arrays.
--duplicates QUERIESxROWSxDIMS: the duplicate-heavy set of tests/test_gpu_knn_vote.py at that size -- three rows in five are copies of
one row, and query row 0 is that row: its tie group is far longer than k, the second pass over the pairs runs for its strip.  There the
summary's list is cut at max_neighbours, and only the vote's own numbers are checked (the list length, the votes).  The share of the
vector pipe's f64 rate counts 4 operations a pair and dimension (subtract, square, times the metric, add: nothing is fused) against
256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.  A run under rocprofv3 --kernel-trace --stats (--repeat 2) gives the split by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9
N_CLASSES = 1000


def host_vote(idx, n, class_of):
    """the awk of the reference's README over the summary's arrays: the most frequent class, the first on a tie"""
    import numpy as np
    cls = np.zeros(len(n), dtype=np.uint32)
    votes = np.zeros(len(n), dtype=np.uint32)
    for j in range(len(n)):
        c = class_of[idx[j, :n[j]]]
        u, first, count = np.unique(c, return_index=True, return_counts=True)
        best = np.lexsort((first, -count))[0]
        cls[j], votes[j] = u[best], count[best]
    return cls, votes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", default=[], help="QUERIESxROWSxDIMS, may be given several times")
    ap.add_argument("--duplicates", action="append", default=[], help="QUERIESxROWSxDIMS of the duplicate-heavy set, may be given several times")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=15, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=2.0, help="seconds of untimed alternating calls before each timed series")
    args = ap.parse_args()
    if not args.shape and not args.duplicates:
        ap.error("a --shape or a --duplicates")
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    k = args.k
    for shape, dup in [(s, False) for s in args.shape] + [(s, True) for s in args.duplicates]:
        r2, r1, d = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(r1 + d)
        m1 = torch.empty((r1, d), dtype=torch.float64, device=dev)
        for lo in range(0, r1, 65536):  # (a slab at a time: the generator's scratch stays small)
            m1[lo:lo + 65536] = torch.randn((min(65536, r1 - lo), d), dtype=torch.float64, device=dev, generator=gen)
        m2 = torch.randn((r2, d), dtype=torch.float64, device=dev, generator=gen)
        class_np = (np.arange(r1, dtype=np.int64) * 7919 % N_CLASSES).astype(np.uint32)
        if dup:
            copies = torch.nonzero(torch.arange(r1, device=dev) % 5 < 3).flatten()
            row = m1[0].clone()
            m1[copies] = row
            m2[0] = row
            class_np[copies.cpu().numpy()] = 1 - np.arange(len(copies)) % 2
        class_of = torch.from_numpy(class_np.view(np.int32)).to(dev)
        metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, True, stream=stream.cuda_stream, keep=(m1, metric))
        mn = max(4 * k, 8)
        work_s = torch.empty(api.dev_refset_workspace_bytes(rs, r2), dtype=torch.uint8, device=dev)
        stats = torch.zeros((r2, 4), dtype=torch.float64, device=dev)
        s_n = torch.zeros(r2, dtype=torch.int32, device=dev)
        s_idx = torch.zeros((r2, mn), dtype=torch.int32, device=dev)
        s_dist = torch.zeros((r2, mn), dtype=torch.float64, device=dev)
        s_z = torch.zeros((r2, mn), dtype=torch.float64, device=dev)
        work_v = torch.empty(api.dev_knn_vote_workspace_bytes(rs, r2, k, N_CLASSES), dtype=torch.uint8, device=dev)
        v_cls, v_votes, v_n = (torch.zeros(r2, dtype=torch.int32, device=dev) for _ in range(3))
        v_first = torch.zeros(r2, dtype=torch.float64, device=dev)

        def summary():
            api.dev_refset_distance_summary(rs, m2.data_ptr(), r2, work_s.data_ptr(), stats.data_ptr(), s_n.data_ptr(), s_idx.data_ptr(), s_dist.data_ptr(),
                                            s_z.data_ptr(), keep_at_most=k, max_neighbours=mn, stream=stream.cuda_stream)

        def knn():
            api.dev_knn_vote(rs, class_of.data_ptr(), N_CLASSES, m2.data_ptr(), r2, k, work_v.data_ptr(), v_cls.data_ptr(), v_votes.data_ptr(), v_n.data_ptr(),
                             v_first.data_ptr(), stream=stream.cuda_stream)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        timed(summary)
        timed(knn)
        # the two answers
        n_s, idx_s = s_n.cpu().numpy().view(np.uint32), s_idx.cpu().numpy().view(np.uint32)
        cls_v, votes_v, n_v = (t.cpu().numpy().view(np.uint32) for t in (v_cls, v_votes, v_n))
        t0 = time.perf_counter()
        rows = slice(1, None) if dup else slice(None)
        cls_h, votes_h = host_vote(idx_s[rows], np.minimum(n_s[rows], mn), class_np)
        vote_host_ms = (time.perf_counter() - t0) * 1e3
        agree = bool(np.array_equal(n_s[rows], n_v[rows]) and np.array_equal(cls_h, cls_v[rows]) and np.array_equal(votes_h, votes_v[rows]))
        if dup:
            n_copies = int((np.arange(r1) % 5 < 3).sum())
            agree = agree and (int(n_v[0]), int(cls_v[0]), int(votes_v[0])) == (n_copies, 1, (n_copies + 1) // 2)
        t_s, t_v = [], []
        t_end = time.perf_counter() + args.warmup_s
        while time.perf_counter() < t_end:
            timed(summary)
            timed(knn)
        for _ in range(args.repeat):
            t_s.append(timed(summary))
            t_v.append(timed(knn))
        ops = 4.0 * r1 * r2 * d
        line = {"queries": r2, "rows": r1, "dims": d, "k": k, "duplicate_heavy": dup, "longest_list": int(n_v.max()), "answers_agree": agree,
                "summary_ms": [round(t, 4) for t in t_s], "knn_vote_ms": [round(t, 4) for t in t_v],
                "summary_median_ms": round(float(np.median(t_s)), 4), "knn_vote_median_ms": round(float(np.median(t_v)), 4),
                "summary_spread_ms": round(max(t_s) - min(t_s), 4), "knn_vote_spread_ms": round(max(t_v) - min(t_v), 4),
                "knn_vote_over_summary": round(float(np.median(t_v) / np.median(t_s)), 3),
                "knn_vote_f64_valu_fraction": round(ops / (float(np.median(t_v)) * 1e-3) / F64_OPS_PER_S, 4),
                "vote_host_ms": round(vote_host_ms, 3),
                "summary_bytes_per_query": 4 * 8 + 4 + mn * (4 + 8 + 8), "knn_vote_bytes_per_query": 3 * 4 + 8,
                "knn_vote_workspace_bytes": work_v.numel()}
        print(json.dumps(line), flush=True)
        rs.free()
        del m1, m2, work_s, work_v, s_idx, s_dist, s_z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
