#!/usr/bin/env python3
"""Times the k-NN validation (kpop_dev_knn_validate: every row of a labelled set against the other rows, a ladder of k from one pass
over the pairs) against the only way to a ladder without it, and prints one JSON line:

    python tools/time_knn_validate.py [--rows 100000] [--dims 64] [--ks 1,3,5,9,15,31] [--repeat 7] [--warmup-s 2]

  (a) validate      kpop_dev_knn_validate over all rows, leave-one-out, the whole ladder
  (b) vote_kmax     kpop_dev_knn_vote with the set's rows as the query rows at k = the ladder's last: the same arithmetic (it counts
                    the row itself, so it is a timing, not an answer)
  (c) vote_ladder   one such call for each k of the ladder

The three alternate inside one process, each between two HIP events on the stream it is enqueued on, after --warmup-s seconds of the
same alternation untimed (the set's divided copy is made by the first call that needs it).  Every timing is listed; the medians and
the spreads (max - min) are what to compare.  Euclidean, normalised rows, 1,000 classes.  With --groups F the validation leaves out
folds of rows (group_of = row % F) instead of the row alone.  A run under rocprofv3 --kernel-trace --stats (--repeat 2) gives the split
by kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CLASSES = 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--ks", default="1,3,5,9,15,31")
    ap.add_argument("--groups", type=int, default=0, help="leave out folds of rows (row %% GROUPS) instead of the row alone")
    ap.add_argument("--repeat", type=int, default=7, help="timed calls of each kind after the warm-up, alternating")
    ap.add_argument("--warmup-s", type=float, default=2.0, help="seconds of untimed alternating calls before the timed series")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    r1, d = args.rows, args.dims
    ks = tuple(int(v) for v in args.ks.split(","))
    n_ks, k_max = len(ks), max(ks)
    gen = torch.Generator(device=dev)
    gen.manual_seed(r1 + d)
    m1 = torch.empty((r1, d), dtype=torch.float64, device=dev)
    for lo in range(0, r1, 65536):  # (a slab at a time: the generator's scratch stays small)
        m1[lo:lo + 65536] = torch.randn((min(65536, r1 - lo), d), dtype=torch.float64, device=dev, generator=gen)
    class_np = (np.arange(r1, dtype=np.int64) * 7919 % N_CLASSES).astype(np.uint32)
    class_of = torch.from_numpy(class_np.view(np.int32)).to(dev)
    group_of = None
    if args.groups:
        group_of = torch.from_numpy((np.arange(r1, dtype=np.int64) % args.groups).astype(np.int32)).to(dev)
    metric = torch.from_numpy(np.linspace(1.0, 0.25, d)).to(dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rs = kpop_amd.RefSet.wrap(m1.data_ptr(), r1, d, metric.data_ptr(), api.EUCLIDEAN, 2.0, True, stream=stream.cuda_stream, keep=(m1, metric))
    work_a = torch.empty(api.dev_knn_validate_workspace_bytes(rs, r1, k_max, N_CLASSES), dtype=torch.uint8, device=dev)
    a_cls, a_votes, a_n = (torch.zeros(n_ks * r1, dtype=torch.int32, device=dev) for _ in range(3))
    a_first = torch.zeros(n_ks * r1, dtype=torch.float64, device=dev)
    a_correct = torch.zeros(n_ks, dtype=torch.int64, device=dev)
    work_v = torch.empty(max(api.dev_knn_vote_workspace_bytes(rs, r1, k, N_CLASSES) for k in ks), dtype=torch.uint8, device=dev)
    v_cls, v_votes, v_n = (torch.zeros(r1, dtype=torch.int32, device=dev) for _ in range(3))
    v_first = torch.zeros(r1, dtype=torch.float64, device=dev)

    def validate():
        api.dev_knn_validate(rs, class_of.data_ptr(), N_CLASSES, None if group_of is None else group_of.data_ptr(), 0, r1, ks, work_a.data_ptr(),
                             a_cls.data_ptr(), a_votes.data_ptr(), a_n.data_ptr(), a_first.data_ptr(), a_correct.data_ptr(), stream=stream.cuda_stream)

    def vote(k):
        api.dev_knn_vote(rs, class_of.data_ptr(), N_CLASSES, m1.data_ptr(), r1, k, work_v.data_ptr(), v_cls.data_ptr(), v_votes.data_ptr(), v_n.data_ptr(),
                         v_first.data_ptr(), stream=stream.cuda_stream)

    def vote_kmax():
        vote(k_max)

    def vote_ladder():
        for k in ks:
            vote(k)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    calls = (validate, vote_kmax, vote_ladder)
    for fn in calls:
        timed(fn)
    correct = a_correct.cpu().numpy().tolist()
    n_last = a_n.cpu().numpy().view(np.uint32).reshape(n_ks, r1)
    # the row itself is not in its list: with it the nearest member would be at distance 0 in every row
    first_k0 = a_first.cpu().numpy().reshape(n_ks, r1)[0]
    t = {fn.__name__: [] for fn in calls}
    t_end = time.perf_counter() + args.warmup_s
    while time.perf_counter() < t_end:
        for fn in calls:
            timed(fn)
    for _ in range(args.repeat):
        for fn in calls:
            t[fn.__name__].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in t.items()}
    line = {"rows": r1, "dims": d, "ks": list(ks), "groups": args.groups, "n_classes": N_CLASSES, "correct": correct,
            "shortest_list": [int(v) for v in n_last.min(axis=1)], "longest_list": [int(v) for v in n_last.max(axis=1)],
            "rows_with_a_neighbour_at_zero": int(np.count_nonzero(first_k0 == 0.0))}
    for name, v in t.items():
        line[name + "_ms"] = [round(x, 3) for x in v]
        line[name + "_median_ms"] = round(med[name], 3)
        line[name + "_spread_ms"] = round(max(v) - min(v), 3)
    line["validate_over_vote_kmax"] = round(med["validate"] / med["vote_kmax"], 4)
    line["validate_over_vote_ladder"] = round(med["validate"] / med["vote_ladder"], 4)
    line["validate_below_vote_ladder"] = bool(med["validate"] < med["vote_ladder"])
    line["validate_workspace_bytes"] = work_a.numel()
    print(json.dumps(line), flush=True)
    rs.free()


if __name__ == "__main__":
    main()
