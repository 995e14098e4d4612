#!/usr/bin/env python3
"""Times kpop_dev_counter_distill on a Poisson database made on the GPU and prints one JSON line per shape:

    python tools/time_distill.py --shape 96x8 [--kmers 8390656] [--lam 2.0] [--repeat 2]

The milliseconds are the library's own phase clocks (kpop_tune("distill_clock", 1): the stream is drained after every band,
cells / reduce / fit timed with events).  The fractions are against the rates of the MI355X the kernels were designed to:
256 CUs at 2.4 GHz; f64 vector operations at 16 lanes a clock a SIMD (half the f32 vector rate); ds_read_b64 at 256 bytes a
clock a CU.  A pair costs the cell kernel 3 f64 operations and half an 8-byte LDS read (8 reads serve a 4 x 4 tile)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9
LDS_BYTES_PER_S = 256 * 256 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", required=True, help="SPECTRAxCLASSES, may be given several times")
    ap.add_argument("--kmers", type=int, default=8390656)
    ap.add_argument("--lam", type=float, default=2.0)
    ap.add_argument("--repeat", type=int, default=2, help="timed calls after one warm-up; the fastest is reported")
    args = ap.parse_args()
    import numpy as np
    import torch

    import kpop_amd
    from kpop_amd import _lib, api
    kpop_amd.init(0)
    L = _lib.load()
    dev = torch.device("cuda", 0)
    K = args.kmers
    ld = int(L.kpop_dev_counter_ld(K))
    for shape in args.shape:
        S, n_classes = (int(v) for v in shape.split("x"))
        storage = torch.zeros((S, ld), dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        rate = torch.full((K,), args.lam, dtype=torch.float32, device=dev)
        for s in range(S):  # a spectrum at a time: one float vector of scratch
            storage[s, :K] = torch.poisson(rate, generator=gen).to(torch.int32)
        del rate
        classes = torch.tensor([s % n_classes for s in range(S)], dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.kpop_dev_counter_distill_workspace_bytes(S, K, n_classes)), dtype=torch.uint8, device=dev)
        out = torch.empty((18, K), dtype=torch.float64, device=dev)
        fits = np.zeros((6, 2))
        torch.cuda.synchronize()
        api.tune("distill_clock", 1)
        best = None
        for it in range(1 + args.repeat):
            t0 = time.perf_counter()
            rc = L.kpop_dev_counter_distill(storage.data_ptr(), ld, S, K, classes.data_ptr(), n_classes, ws.data_ptr(), out.data_ptr(),
                                            fits.ctypes.data_as(C.POINTER(C.c_double)), None)
            wall = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.kpop_last_error()
            ms = (C.c_double * 3)()
            assert L.kpop_debug_distill_clocks(ms) == 0
            if it > 0 and (best is None or ms[0] + ms[1] + ms[2] < sum(best[:3])):
                best = (ms[0], ms[1], ms[2], wall)
        api.tune("distill_clock", 0)
        pairs = K * S * (S - 1) / 2.0
        cell_s = best[0] * 1e-3
        print(json.dumps({"spectra": S, "classes": n_classes, "kmers": K, "lambda": args.lam, "cells_ms": round(best[0], 3),
                          "reduce_ms": round(best[1], 3), "fit_ms": round(best[2], 3), "call_wall_ms": round(best[3], 3),
                          "pairs_per_s": pairs / cell_s, "f64_valu_fraction": 3.0 * pairs / cell_s / F64_OPS_PER_S,
                          "lds_read_fraction": 4.0 * pairs / cell_s / LDS_BYTES_PER_S, "workspace_bytes": ws.numel(),
                          "fit_avgs_mean": [float(fits[0, 0]), float(fits[0, 1])]}), flush=True)
        del storage, ws, out


if __name__ == "__main__":
    main()
