"""Representatives at a distance from a plain C99 host (examples/c_representatives.c): compiled with gcc against include/kpop_hip.h and
the shared library as tests/test_gpu_clusters_c.py compiles examples/c_clusters.c, run on the GPU, what it prints compared with
tests/representatives_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from representatives_ref import representatives_ref

pytestmark = pytest.mark.gpu

D, ROWS, MORE, T = 4, 24, 8, 0.375


def row_value(i, c):
    g = i % 5
    centre = [2.0 * g, float(g), 0.0, -float(g)][c]
    return centre + ((i // 5) / 8.0 if c == i % D else 0.0)


def more_value(k, c):
    if k == MORE - 1:
        return 40.0 if c == 3 else 0.0
    return [2.0, 1.0, 0.0, -1.0][c] * (k + 1) / 8.0


def report(what, rep_of, n):
    return "%s: %d rows, %d representatives:" % (what, len(rep_of), n) + "".join(" %d" % i for i in range(len(rep_of)) if rep_of[i] == i)


def test_c_representatives_program(tmp_path, oracle):
    exe = tmp_path / "c_representatives"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "c_representatives.c"), "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm",
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[row_value(i, c) for c in range(D)] for i in range(ROWS)])
    more = np.array([[more_value(k, c) for c in range(D)] for k in range(MORE)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    first = representatives_ref(oracle.distance_rowwise(rows, rows, metric, 0, 2.0, False), T)
    both = np.vstack([rows, more])
    D2 = oracle.distance_rowwise(both, both, metric, 0, 2.0, False)
    grown = representatives_ref(D2, T)
    # what the example is about: rows that are dropped, appended rows of both kinds, a row that stays alone
    assert 5 <= first[2] < ROWS
    new = grown[0][ROWS:] == np.arange(ROWS, ROWS + MORE)
    assert new.any() and not new.all() and new[MORE - 1] and grown[2] == first[2] + int(new.sum())
    assert np.array_equal(grown[0][:ROWS], first[0])  # the prefix property
    assert np.array_equal(representatives_ref(D2, T, known=first[0])[0], grown[0])
    assert lines[0] == report("created", first[0], first[2]), lines[0]
    assert lines[1] == report("grown", grown[0], grown[2]), lines[1]
    assert lines[2] == "from scratch: the same result"
    assert lines[3] == "rep_of:" + "".join(" %d" % v for v in grown[0]), lines[3]
    assert lines[4] == "rep_dist:" + "".join(" %.17g" % v for v in grown[1]), lines[4]
    everything = representatives_ref(oracle.distance_rowwise(rows, rows, metric, 0, 2.0, False), 1e300)
    assert everything[2] == 1
    assert lines[5] == report("one neighbourhood", everything[0], everything[2]), lines[5]
    assert len(lines) == 6
