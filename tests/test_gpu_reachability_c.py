"""The mutual-reachability forest from a plain C99 host (examples/c_reachability.c): compiled with gcc against include/kpop_hip.h and the
shared library as tests/test_gpu_forest_c.py compiles examples/c_forest.c, run on the GPU, its printed core distances, edges, cuts and
argument errors compared with tests/reachability_ref.py on the oracle's distances -- the worked case of INTEGRATION.md 6j."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import NOISE, dbscan_ref
from reachability_ref import reachability_cut_ref, reachability_forest_ref

pytestmark = pytest.mark.gpu

D, ROWS, MIN_PTS = 3, 10, 4
X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]


def cut_lines(ei, ej, ed, core, dist, T):
    labels, counts = reachability_cut_ref(ROWS, ei, ej, ed, core, T)
    want = dbscan_ref(dist, T, MIN_PTS)
    is_core = want[2] >= MIN_PTS
    assert np.array_equal(labels[is_core], want[0][is_core]) and np.all(labels[~is_core] == NOISE) and counts.tolist()[:2] == want[3].tolist()[:2]
    return ["cut at %g: %d clusters, %d core rows, %d noise rows; labels:" % ((T,) + tuple(counts.tolist()))
            + "".join(" -" if v == NOISE else " %d" % v for v in labels),
            "the cut at %g and kpop_dbscan at %g: the same labels on the core rows" % (T, T)]


def test_c_reachability_program(tmp_path, oracle):
    exe = tmp_path / "c_reachability"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_reachability.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    rows = np.zeros((ROWS, D))
    rows[:, 0] = X
    dist = oracle.distance_rowwise(rows, rows, np.ones(D), 0, 2.0, False)
    ei, ej, ed, core, labels = reachability_forest_ref(dist, MIN_PTS)
    # what the example is about: the section's numbers, one tree with equal weights in it, two cuts that differ
    assert core.tolist() == [.375, .25, .25, .375, .25, .25, .375, .5, 3.75, .375]
    assert len(ei) == ROWS - 1 and not labels.any() and len(np.unique(ed)) <= len(ed) // 2
    want = ["core distances at min_pts = %d:" % MIN_PTS + "".join(" %.17g" % v for v in core), "forest: %d edges on %d rows" % (ROWS - 1, ROWS)]
    want += ["edge %d: %d - %d at %.17g" % (e, ei[e], ej[e], ed[e]) for e in range(ROWS - 1)]
    want += cut_lines(ei, ej, ed, core, dist, 0.25) + cut_lines(ei, ej, ed, core, dist, 0.375)
    assert want[-4].endswith("labels: - 1 1 - 4 4 - - - -") and want[-2].endswith("labels: 0 0 0 3 3 3 3 - - 0")
    want += ["min_pts = 0: -1", "min_pts = 130: -3", "max_distance = NaN: -1", "no room for the edges: -1", "a cut without core distances: -1", "a cut at NaN: -1"]
    for k, line in enumerate(want):
        assert lines[k] == line, (k, lines[k], line)
    assert len(lines) == len(want)
