"""DBSCAN on a resident set from a plain C99 host (examples/c_dbscan.c): compiled with gcc against include/kpop_hip.h and the shared
library as tests/test_gpu_clusters_c.py compiles examples/c_clusters.c, run on the GPU, its printed labels, core rows, degrees and
counts compared with tests/dbscan_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import NOISE, dbscan_ref

pytestmark = pytest.mark.gpu

X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
EPS, MIN_PTS = 0.375, 4


def printed(what, values):
    return what + ":" + "".join(" noise" if v == NOISE else " %d" % v for v in values)


def test_c_dbscan_program(tmp_path, oracle):
    exe = tmp_path / "c_dbscan"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_dbscan.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(X), 3))
    rows[:, 0] = X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    labels, core_of, degree, counts = dbscan_ref(D, EPS, MIN_PTS)
    # what the example is about: two clusters, a border row between them that goes to the smaller row index, a noise row
    assert counts.tolist() == [2, 8, 1] and degree[7] < MIN_PTS and core_of[7] == 3 and labels[8] == NOISE
    assert lines[0] == printed("labels", labels), lines[0]
    assert lines[1] == printed("core_of", core_of), lines[1]
    assert lines[2] == printed("degree", degree), lines[2]
    assert lines[3] == "counts: %d clusters, %d core rows, %d noise rows" % tuple(counts), lines[3]
    assert lines[4] == "resident set: the same labels"
    joined = dbscan_ref(D, EPS, 3)
    assert joined[3].tolist() == [1, 9, 1]
    assert lines[5] == printed("labels at min_pts 3", joined[0]), lines[5]
    assert lines[6] == "counts at min_pts 3: %d clusters, %d core rows, %d noise rows" % tuple(joined[3]), lines[6]
    assert len(lines) == 7
