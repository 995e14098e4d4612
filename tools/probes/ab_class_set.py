#!/usr/bin/env python3
"""kpop_dev_distance_rowwise against a class set: class_set.hip's kernel (kpop_tune("class_set", 2)) beside the tiled kernel
(kpop_tune("class_set", 0)) in one process -- ms a call (HIP events, median of 20 after 3 warm calls, as bench.py::_event_ms),
the outputs compared bit for bit.  AB_SHAPES="r1xr2xd,..." (default: the four shapes of profiles/class_set_distance.md);
AB_SWEEP=1 adds the sweep of second-operand rows at 65 x r2 x 64 and 10 x r2 x 9 the dispatch threshold comes from."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import kpop_amd
    from kpop_amd import api
    kpop_amd.init(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    rng = np.random.default_rng(5)
    shapes = [tuple(int(v) for v in s.split("x")) for s in
              os.environ.get("AB_SHAPES", "65x100000x64,65x1000000x64,10x100000x9,65x10000x64").split(",")]
    if os.environ.get("AB_SWEEP"):
        for r1, d in ((65, 64), (10, 9)):
            shapes += [(r1, r2, d) for r2 in (16, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 49152, 65536)]
    print("%22s %10s %10s %8s %s" % ("r1 x r2 x d", "old ms", "new ms", "old/new", "same bits"))
    for r1, r2, d in shapes:
        m1 = torch.from_numpy(rng.standard_normal((r1, d))).to(dev)
        m2 = torch.from_numpy(rng.standard_normal((r2, d))).to(dev)
        metric = torch.from_numpy(rng.random(d) + 0.1).to(dev)
        work = torch.empty(api.dev_distance_workspace_bytes(r1, r2, d) // 8 + 16, dtype=torch.float64, device=dev)
        outs = {}
        ms = {}
        for mode in (0, 2, 0, 2):  # (twice, alternating: the second figures are the ones kept)
            api.tune("class_set", mode)
            out = torch.zeros(r2, r1, dtype=torch.float64, device=dev)

            def run():
                api.dev_distance_rowwise(m1.data_ptr(), r1, m2.data_ptr(), r2, d, metric.data_ptr(), work.data_ptr(), out.data_ptr(),
                                         stream=st.cuda_stream)

            for _ in range(3):
                run()
            torch.cuda.synchronize()
            t = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                run()
                e1.record(st)
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1))
            ms[mode] = float(np.median(t))
            outs[mode] = out
        api.tune("class_set", 1)
        same = bool(torch.equal(outs[0], outs[2]))
        print("%22s %10.4f %10.4f %8.2f %s" % ("%d x %d x %d" % (r1, r2, d), ms[0], ms[2], ms[0] / ms[2], same), flush=True)


if __name__ == "__main__":
    main()
