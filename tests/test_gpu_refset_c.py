"""The resident reference set from a plain C99 host (examples/c_refset.c): compiled with gcc against include/kpop_hip.h and the
shared library as tests/test_gpu_abi_c.py compiles examples/c_host.c, run on the GPU, its neighbours compared with the oracle."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

D, ROWS, MORE, QUERIES, NB = 4, 6, 3, 2, 2


def ref_value(i, c):
    return ((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (0.5 if c == i % D else 0.0)


def test_c_refset_program(tmp_path, oracle):
    exe = tmp_path / "c_refset"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_refset.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[ref_value(i, c) for c in range(D)] for i in range(ROWS + MORE)])
    queries = [np.array([[ref_value(2 * b + j + 1, c) + (c + 1 + b) / 16.0 for c in range(D)] for j in range(QUERIES)]) for b in range(2)]
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    at = 0
    for what, r1, q in (("first", ROWS, queries[0]), ("second", ROWS, queries[1]), ("grown", ROWS + MORE, queries[1])):
        st, offs, idx, dist, _ = oracle.distance_summary(rows[:r1], q, metric, 0, 2.0, True, NB)
        for j in range(QUERIES):
            a = int(offs[j])
            assert int(offs[j + 1]) - a == NB  # (no ties among these rows: two neighbours each)
            assert lines[at] == "%s: %u rows, query %d: mean %.15g nearest %u at %.15g then %u at %.15g" % (
                what, r1, j, st[j, 0], idx[a], dist[a], idx[a + 1], dist[a + 1]), (lines[at], st[j], idx[a:a + 2], dist[a:a + 2])
            at += 1
    assert lines[at] == "full: append returned -2, %u of %u rows, device memory reported" % (ROWS + MORE, ROWS + MORE)
    want = oracle.distance_rowwise(rows, queries[1], metric, 0, 2.0, True)
    for j in range(QUERIES):
        assert lines[at + 1 + j] == "distances %d: %s" % (j, " ".join("%.15g" % x for x in want[j]))
    assert len(lines) == at + 1 + QUERIES
