"""The range query from a plain C99 host (examples/c_within.c): compiled with gcc against include/kpop_hip.h and the shared library as
tests/test_gpu_refset_c.py compiles examples/c_refset.c, run on the GPU, its printed lists compared with tests/within_ref.py on the
oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from within_ref import rows_of, within_ref

pytestmark = pytest.mark.gpu

D, ROWS, QUERIES = 4, 9, 3


def ref_value(i, c):
    return ((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (0.5 if c == i % D else 0.0)


def test_c_within_program(tmp_path, oracle):
    exe = tmp_path / "c_within"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_within.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[ref_value(i, c) for c in range(D)] for i in range(ROWS)])
    queries = np.array([[ref_value(4, c) if j == 2 else ref_value(j + 1, c) + (c + 1) / 16.0 for c in range(D)] for j in range(QUERIES)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    dist = oracle.distance_rowwise(rows, queries, metric, 0, 2.0, True)
    at = 0
    for T in (0.0, 0.5, 1e300):
        want = within_ref(dist, T)
        total = int(want[0][-1])
        calls = 1 if total <= 2 else 2  # (the program starts with room for two entries and grows once, to the exact size)
        assert lines[at] == "within %.15g: %d neighbours in %d call%s" % (T, total, calls, "" if calls == 1 else "s"), lines[at]
        for j, (idx, dd) in enumerate(rows_of(want)):
            assert lines[at + 1 + j] == "query %d:" % j + "".join(" %u at %.15g" % (i, x) for i, x in zip(idx, dd)), (T, lines[at + 1 + j])
        at += 1 + QUERIES
    assert rows_of(within_ref(dist, 0.0))[2][0].tolist() == [4]  # query 2 is row 4
    assert int(within_ref(dist, 0.5)[0][-1]) > 2 and int(within_ref(dist, 1e300)[0][-1]) == ROWS * QUERIES
    counts = np.diff(within_ref(dist, 0.25)[0].astype(np.int64))
    assert lines[at] == "count within 0.25:" + "".join(" %d" % n for n in counts)
    assert len(lines) == at + 1
