"""bench.py's headline and its config 2 / 3 / 5 legs (the leg functions themselves, imported), then the host cost of enqueueing kpop_dev_count_twist:
1,000 calls on 64 reads and 200 calls on 64 assemblies of 4,000 bases, a host clock around each loop ending in a synchronise, seven loops each.
One JSON file; run it once a library (KPOP_HIP_LIB) and compare:   python tools/probes/count_twist_legs.py OUT.json [SECONDS]
SECONDS (default 280) is the time limit of the whole run.  The legs are bench.py's functions: a change there changes what this measures."""
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402

out_path = sys.argv[1]
signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 280)  # (SIGALRM ends the process)
args = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
R = bench.Rank(args)
t, api = R.torch, R.api
res = {}
h = R.run_headline(100000, 0, 20, 5)
res["headline_ms_per_step"] = h["elapsed"] / 20 * 1e3
res["headline_count_twist_ms"] = h["ms_fused"]
res["headline_distance_ms"] = h["ms_dist"]
c2 = bench.config2_leg(R)
res["config2_count_reads_ms"] = c2["kernels_ms"]["count_reads (-L, CSR out)"]
res["config2_count_twist_ms"] = c2["kernels_ms"]["count_twist (fused)"]
c3 = bench.config3_leg(R)
res["config3_unrelated_ms"] = c3["unrelated_genomes"]["ms_per_step"]
res["config3_unrelated_all"] = c3["unrelated_genomes"]["ms_all"]
res["config3_one_organism_ms"] = c3["one_organism_0.3pct"]["ms_per_step"]
res["config3_one_organism_all"] = c3["one_organism_0.3pct"]["ms_all"]
res["config3_one_organism_streaming_alone_ms"] = c3["one_organism_0.3pct"]["streaming_kernel_alone_ms"]
for dd in ("256", "1635"):
    res["config3_d%s_ms" % dd] = c3["one_organism_dims"][dd].get("ms")
c5 = bench.config5_leg(R)
res["config5_ms"] = c5.get("ms_per_step")
# enqueue cost
n, L = 64, 150
bases = t.empty(n * L, dtype=t.uint8, device=R.dev)
offs = t.empty(n + 1, dtype=t.int64, device=R.dev)
api.dev_synth_reads(7, n, L, bases.data_ptr(), offs.data_ptr(), stream=R.sp)
out = t.zeros(n, args.dims, dtype=t.float64, device=R.dev)
call = lambda: api.dev_count_twist(R.tw, bases.data_ptr(), offs.data_ptr(), n, n * L, L, out.data_ptr(), stream=R.sp)  # noqa: E731
for _ in range(200):
    call()
t.cuda.synchronize()
runs, host = [], []
for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(1000):
        call()
    host.append((time.perf_counter() - t0) * 1e3)  # (the host's share: the loop before the synchronise)
    t.cuda.synchronize()
    runs.append((time.perf_counter() - t0) * 1e3)
res["enqueue_1000_calls_ms_runs"] = runs
res["enqueue_1000_calls_host_ms_runs"] = host
res["enqueue_1000_calls_host_ms_median"] = sorted(host)[3]
res["enqueue_1000_calls_ms_median"] = sorted(runs)[3]
# ... and of a call with a long part (64 sequences of 4,000 bases: the tile route's dozen launches)
g = t.Generator(device=R.dev)
g.manual_seed(0x99)
acgt = t.tensor(list(b"ACGT"), dtype=t.uint8, device=R.dev)
ref = acgt[t.randint(0, 4, (4000,), device=R.dev, generator=g)]
gb = t.where(t.rand(64 * 4000, device=R.dev, generator=g) < 0.003, acgt[t.randint(0, 4, (64 * 4000,), device=R.dev, generator=g)], ref.repeat(64))
go = t.arange(65, dtype=t.int64, device=R.dev) * 4000
gout = t.zeros(64, args.dims, dtype=t.float64, device=R.dev)
gcall = lambda: api.dev_count_twist(R.tw, gb.data_ptr(), go.data_ptr(), 64, 64 * 4000, 4000, gout.data_ptr(), stream=R.sp)  # noqa: E731
for _ in range(50):
    gcall()
t.cuda.synchronize()
runs, host = [], []
for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(200):
        gcall()
    host.append((time.perf_counter() - t0) * 1e3)
    t.cuda.synchronize()
    runs.append((time.perf_counter() - t0) * 1e3)
res["long_200_calls_ms_runs"] = runs
res["long_200_calls_host_ms_runs"] = host
res["long_200_calls_host_ms_median"] = sorted(host)[3]
res["long_200_calls_ms_median"] = sorted(runs)[3]
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), file=sys.stderr)
