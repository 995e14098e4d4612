"""One SHA-256 per route of the count -> twist entry points (count_twist.hip, packed.hip): a fixed, seeded list of small batches, each
through the route its name ends in ("-> reads": no sequence of more than 512 windows), the output rows hashed.  check_digest_cases in
tests/host/count_twist_plan_check.cpp has the same list -- k, dimensions, sequences, longest sequence, knobs -- and holds plan_count_twist to
the route named here: a case changed or added here is changed or added there.
Two builds of the library print the same listing or they do not compute the same bits:

    python tools/probes/count_twist_routes_digest.py                     this tree's library
    KPOP_HIP_LIB=/path/to/another/libkpop_hip.so python tools/probes/count_twist_routes_digest.py

Twisters hold the k-mers the library's own kpop_count_reads finds in the batch (four fifths of them, shuffled) with seeded random rows.
One time limit on the whole run (--limit seconds); the first failing call ends it."""
import argparse
import hashlib
import os
import signal
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import kpop_amd  # noqa: E402
from kpop_amd import api  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYXBZ*", dtype=np.uint8)
DNA = np.frombuffer(b"ACGTN", dtype=np.uint8)


def concat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if len(seqs) else np.zeros(0, dtype=np.uint8)).astype(np.uint8), offs


def reads(rng, n, lo, hi, alphabet=DNA, p=(.245, .245, .245, .245, .02)):
    """n ragged sequences of lo..hi letters, an empty one and one of two letters among them"""
    p = np.asarray(p, dtype=np.float64)
    seqs = [alphabet[rng.choice(len(alphabet), size=int(rng.randint(lo, hi + 1)), p=p / p.sum())] for _ in range(n)]
    seqs[1], seqs[2] = seqs[1][:0], seqs[2][:2]
    seqs[0] = alphabet[rng.choice(len(alphabet), size=hi, p=p / p.sum())]  # (the longest: what picks R)
    return seqs


def mutants(rng, n, L, rate=0.01):
    ref = DNA[rng.choice(4, size=L)]
    out = []
    for i in range(n):
        m = ref.copy()
        hit = rng.rand(L) < rate
        m[hit] = DNA[rng.choice(5, size=int(hit.sum()), p=[.24, .24, .24, .24, .04])]
        out.append(m[:L - (i % 7) * 3] if L > 2000 else m)
    return out


def twister_for(rng, seqs, k, d, content=api.DNA_DS):
    bases, offs = concat(seqs)
    h, _, _ = api.count_reads(bases, offs, k, content)
    cols = np.unique(h)
    cols = cols[rng.rand(len(cols)) < 0.8]
    cols = cols[rng.permutation(len(cols))]
    T = rng.standard_normal((d, len(cols)))
    tw = kpop_amd.Twister.load(T, cols, k if content != api.PROTEIN else (5 * k + 1) // 2)
    if content == api.PROTEIN:
        tw.set_count_k(k)
    return tw


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dev_rows(tw, seqs, d, content=api.DNA_DS, packed=False):
    """kpop_dev_count_twist (or its packed form) on device buffers: the route is the plan's, whatever the host entry point would choose"""
    bases, offs = concat(seqs)
    n, n_bases, max_len = len(seqs), int(offs[-1]), int(max(len(s) for s in seqs))
    dev = torch.device("cuda", 0)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    out = torch.full((n, d), float("nan"), dtype=torch.float64, device=dev)
    if packed:
        codes, invalid = api.pack_bases(bases)
        d_codes = torch.from_numpy(np.concatenate([codes, np.zeros(2, np.uint32)]).view(np.int32)).to(dev)
        d_mask = torch.from_numpy(np.concatenate([invalid, np.zeros(2, np.uint32)]).view(np.int32)).to(dev)
        api.dev_count_twist_packed(tw, d_codes.data_ptr(), d_mask.data_ptr(), d_offs.data_ptr(), n, n_bases, max_len, out.data_ptr(), content=content)
    else:
        d_bases = torch.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])).to(dev)
        api.dev_count_twist(tw, d_bases.data_ptr(), d_offs.data_ptr(), n, n_bases, max_len, out.data_ptr(), content=content)
    torch.cuda.synchronize()
    return out.cpu().numpy()


class Tuned:
    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for key, (value, _) in self.knobs.items():
            api.tune(key, value)

    def __exit__(self, *exc):
        for key, (_, default) in self.knobs.items():
            api.tune(key, default)


def cases():
    k = 11
    # reads: one wavefront each, R rounds of 64 windows by the longest
    for R, hi in ((1, k + 63), (2, k + 127), (4, k + 255), (8, k + 511)):
        rng = np.random.RandomState(100 + R)
        seqs = reads(rng, 300, 20, hi)
        tw = twister_for(rng, seqs, k, 64)
        yield "reads R=%d -> reads" % R, lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64)
        if R == 2:
            yield "reads R=2 unroll 16 -> reads", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64), {"unroll": (16, 8)}
            yield "reads R=2 nt 1 -> reads", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64), {"nt": (1, 2)}
            yield "reads R=2 ldspad 16384 -> reads", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64), {"ldspad": (16384, 0)}
            yield "reads R=2 packed -> reads", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64, packed=True)
            yield "reads R=2 packed nt 1 -> reads", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64, packed=True), {"nt": (1, 2)}
            long_one = seqs + [DNA[rng.choice(4, size=3000)]]
            yield "packed, one long sequence among 300 reads (unpack) -> TilePipe", lambda tw=tw, s=long_one: dev_rows(tw, s, 64, packed=True)
    rng = np.random.RandomState(7)
    seqs = reads(rng, 300, 20, 150)
    tw16 = twister_for(rng, seqs, 16, 64)
    yield "reads hk 16 (64-bit keys) -> reads", lambda: dev_rows(tw16, seqs, 64)
    yield "reads hk 16 packed -> reads", lambda: dev_rows(tw16, seqs, 64, packed=True)
    for pk in (3, 7):
        rng = np.random.RandomState(30 + pk)
        prot = reads(rng, 200, 5, 400, AA, [1.0] * 20 + [.06, .03, .03, .03])
        twp = twister_for(rng, prot, pk, 64, api.PROTEIN)
        yield "protein k=%d -> reads" % pk, lambda twp=twp, prot=prot: dev_rows(twp, prot, 64, content=api.PROTEIN)
        prot_long = prot[:40] + [AA[rng.choice(20, size=n)] for n in (900, 2500, 4000)]
        if pk == 7:
            yield "protein k=7, three long among 40 -> Stream", lambda twp=twp, s=prot_long: dev_rows(twp, s, 64, content=api.PROTEIN)
        else:
            yield "protein k=3, three long among 40 -> Stream", lambda twp=twp, s=prot_long: dev_rows(twp, s, 64, content=api.PROTEIN)
    # the streaming kernel alone: three long sequences among ten reads (fewer than 16 sequences: no tile route)
    for d in (9, 100, 300):
        rng = np.random.RandomState(200 + d)
        seqs = reads(rng, 10, 20, 150) + [DNA[rng.choice(5, size=n, p=[.245, .245, .245, .245, .02])] for n in (700, 20000, 45000)]
        tw = twister_for(rng, seqs, k, d)
        yield "three long among 10 reads, d=%d -> Stream" % d, lambda tw=tw, seqs=seqs, d=d: dev_rows(tw, seqs, d)
        if d == 100:
            yield "three long among 10 reads, d=100 seg 2048 -> Stream", lambda tw=tw, seqs=seqs, d=d: dev_rows(tw, seqs, d), {"seg": (2048, 0)}
            yield "three long among 10 reads, d=100 nt 1 -> Stream", lambda tw=tw, seqs=seqs, d=d: dev_rows(tw, seqs, d), {"nt": (1, 2)}
    rng = np.random.RandomState(16)
    seqs = reads(rng, 10, 20, 150) + [DNA[rng.choice(4, size=n)] for n in (700, 20000, 45000)]
    tw = twister_for(rng, seqs, 16, 64)
    yield "three long among 10 reads, hk 16 -> Stream", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 64)
    # the tile routes: 64 mutants of one sequence
    for d in (64, 72, 130):
        rng = np.random.RandomState(300 + d)
        seqs = mutants(rng, 64, 4000) + reads(rng, 10, 20, 150)
        tw = twister_for(rng, seqs, k, d)
        run = lambda tw=tw, seqs=seqs, d=d: dev_rows(tw, seqs, d)  # noqa: E731
        if d == 64:
            yield "mutants d=64 -> TilePipe", run
            yield "mutants d=64 tilewide 1 -> TilePipeWide", run, {"tilewide": (1, 0)}
            yield "mutants d=64 tilepipe 0 tileg 32 -> TileRound4", run, {"tilepipe": (0, 1), "tileg": (32, 64)}
            yield "mutants d=64 tilepipe 0 tileg 64 -> TileRound4", run, {"tilepipe": (0, 1), "tileg": (64, 64)}
            yield "mutants d=64 dense 0 -> Stream", run, {"dense": (0, 2)}
        elif d == 72:
            yield "mutants d=72 -> TilePipeWide", run
        else:
            yield "mutants d=130 tilepipe 0 -> TileRound4Residual", run, {"tilepipe": (0, 1)}
            yield "mutants d=130 tilepipe 0 nt 1 -> TileRound4Residual", run, {"tilepipe": (0, 1), "nt": (1, 2)}
    # sub-batches: (8 << 20) / ((1023 / 512 + 2) * (72 * 8 + 16)) = 4,723 sequences a call
    rng = np.random.RandomState(4800)
    seqs = mutants(rng, 4800, 1023, 0.004)
    tw = twister_for(rng, seqs[:200], k, 72)
    yield "4800 x 1023 at d=72, tilecap_mb 8 -> sub-batches of 4723", lambda tw=tw, seqs=seqs: dev_rows(tw, seqs, 72), {"tilecap_mb": (8, 0)}
    # the host-buffer entry points
    rng = np.random.RandomState(5)
    seqs = reads(rng, 200, 20, 300)
    bases, offs = concat(seqs)
    yield "kpop_count_reads per read", lambda: np.concatenate([x.view(np.uint8).ravel() for x in api.count_reads(bases, offs, k)])
    yield "kpop_count_reads whole", lambda: np.concatenate([x.view(np.uint8).ravel() for x in api.count_reads(bases, offs, k, per_read=False)])
    with_genome = seqs + [DNA[rng.choice(4, size=5000)]]
    gb, go = concat(with_genome)
    yield "kpop_count_reads per read, a genome among them", lambda: np.concatenate([x.view(np.uint8).ravel() for x in api.count_reads(gb, go, k)])
    for d in (16, 64):
        tw = twister_for(rng, seqs, k, d)
        yield "kpop_spectra_twist d=%d -> spectra (d=16), reads (d=64)" % d, lambda tw=tw: tw.spectra_twist(bases, offs, k)
        yield "kpop_spectra_twist d=%d, a genome among them" % d, lambda tw=tw: tw.spectra_twist(gb, go, k)
        yield "kpop_count_twist d=%d, a genome among 200 reads -> TilePipe" % d, lambda tw=tw: tw.count_twist(gb, go)
    h, c, o = api.count_reads(bases, offs, k)
    yield "kpop_twist", lambda tw=tw: tw.twist(h, c.astype(np.float64), o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=240, help="seconds the whole run may take")
    args = ap.parse_args()
    signal.alarm(args.limit)  # (SIGALRM ends the process)
    kpop_amd.init(0)
    print("library: %s" % ("KPOP_HIP_LIB" if "KPOP_HIP_LIB" in os.environ else "this tree's"), flush=True)
    n = 0
    for case in cases():
        name, run = case[0], case[1]
        with Tuned(**(case[2] if len(case) > 2 else {})):
            rows = run()  # (a failing call raises: the run ends here)
        print("%s  %s  %s" % (digest(rows), "x".join(map(str, rows.shape)), name), flush=True)
        n += 1
    print("count_twist_routes_digest: %d cases" % n)


if __name__ == "__main__":
    main()
