"""Clusters at a distance from a plain C99 host (examples/c_clusters.c): compiled with gcc against include/kpop_hip.h and the shared
library as tests/test_gpu_within_c.py compiles examples/c_within.c, run on the GPU, its printed sizes and labels compared with
tests/clusters_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from clusters_ref import clusters_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

D, ROWS, MORE, TOP, T = 4, 24, 8, 3, 0.375


def row_value(i, c):
    g = i % 5
    centre = [2.0 * g, float(g), 0.0, -float(g)][c]
    return centre + ((i // 5) / 8.0 if c == i % D else 0.0)


def more_value(k, c):
    if k == MORE - 1:
        return 40.0 if c == 3 else 0.0
    return [2.0, 1.0, 0.0, -1.0][c] * (k + 1) / 8.0


def report(what, labels, n):
    size = np.bincount(labels.astype(np.int64), minlength=len(labels))
    line = "%s: %d rows in %d clusters; largest:" % (what, len(labels), n)
    for _ in range(TOP):
        if not size.any():
            break
        best = int(np.argmax(size))  # (the first of the largest: by size, then by label)
        line += " %d rows under label %d;" % (size[best], best)
        size[best] = 0
    return line


def test_c_clusters_program(tmp_path, oracle):
    exe = tmp_path / "c_clusters"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_clusters.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[row_value(i, c) for c in range(D)] for i in range(ROWS)])
    more = np.array([[more_value(k, c) for c in range(D)] for k in range(MORE)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    first = clusters_ref(oracle.distance_rowwise(rows, rows, metric, 0, 2.0, False), T)
    both = np.vstack([rows, more])
    D2 = oracle.distance_rowwise(both, both, metric, 0, 2.0, False)
    grown = clusters_ref(D2, T)
    # what the example is about: groups of several rows, a bridge that joins two of them, a row that stays alone
    assert first[1] == 5 and sorted(np.bincount(first[0]).tolist())[-1] == 5
    assert grown[1] == first[1] - 1 + 1 and grown[0][ROWS + MORE - 1] == ROWS + MORE - 1
    assert np.array_equal(clusters_ref(D2, T, known=first[0])[0], grown[0])
    assert lines[0] == report("created", first[0], first[1]), lines[0]
    assert lines[1] == report("grown", grown[0], grown[1]), lines[1]
    assert lines[2] == "from scratch: the same labels"
    assert lines[3] == "labels:" + "".join(" %d" % v for v in grown[0]), lines[3]
    everything = clusters_ref(oracle.distance_rowwise(rows, rows, metric, 0, 2.0, False), 1e300)
    assert everything[1] == 1
    assert lines[4] == report("everything joined", everything[0], everything[1]), lines[4]
    assert len(lines) == 5
