"""The single-linkage tree from a plain C99 host (examples/c_forest.c): compiled with gcc against include/kpop_hip.h and the shared
library as tests/test_gpu_clusters_c.py compiles examples/c_clusters.c, run on the GPU, its printed edges and cuts compared with
tests/forest_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from clusters_ref import clusters_ref
from conftest import ROOT
from forest_ref import cut_ref, forest_ref

pytestmark = pytest.mark.gpu

D, GROUPED, ROWS, CUT_A, CUT_B = 4, 24, 32, 0.25, 0.375


def row_value(i, c):
    if i == ROWS - 1:
        return 40.0 if c == 3 else 0.0
    if i >= GROUPED:
        return [2.0, 1.0, 0.0, -1.0][c] * (i - GROUPED + 1) / 8.0
    g = i % 5
    centre = [2.0 * g, float(g), 0.0, -float(g)][c]
    return centre + ((i // 5) / 8.0 if c == i % D else 0.0)


def labels_line(what, labels, n):
    return "%s: %d clusters; labels:" % (what, n) + "".join(" %d" % v for v in labels)


def test_c_forest_program(tmp_path, oracle):
    exe = tmp_path / "c_forest"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_forest.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[row_value(i, c) for c in range(D)] for i in range(ROWS)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    dist = oracle.distance_rowwise(rows, rows, metric, 0, 2.0, False)
    ei, ej, ed, labels = forest_ref(dist, float("inf"))
    cut_a, cut_b = cut_ref(ROWS, ei, ej, ed, CUT_A), cut_ref(ROWS, ei, ej, ed, CUT_B)
    # what the example is about: one tree with many equal distances in it, two cuts that differ, the second the clusters at its distance
    assert len(ei) == ROWS - 1 and not labels.any() and len(np.unique(ed)) <= len(ed) // 2
    assert cut_a[1] > cut_b[1] > 1
    want_b = clusters_ref(dist, CUT_B)
    assert np.array_equal(cut_b[0], want_b[0]) and cut_b[1] == want_b[1]
    assert lines[0] == "forest: %d edges on %d rows" % (ROWS - 1, ROWS), lines[0]
    for e in range(ROWS - 1):
        assert lines[1 + e] == "edge %d: %d - %d at %.17g" % (e, ei[e], ej[e], ed[e]), lines[1 + e]
    assert lines[ROWS] == labels_line("cut at 0.25", *cut_a), lines[ROWS]
    assert lines[ROWS + 1] == labels_line("cut at 0.375", *cut_b), lines[ROWS + 1]
    assert lines[ROWS + 2] == "the cut at 0.375 and kpop_clusters_within at 0.375: the same labels"
    assert len(lines) == ROWS + 3
