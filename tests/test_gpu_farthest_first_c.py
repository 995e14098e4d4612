"""The farthest-first traversal from a plain C99 host (examples/c_farthest_first.c): compiled with gcc against include/kpop_hip.h and
the shared library as tests/test_gpu_dbscan_c.py compiles examples/c_dbscan.c, run on the GPU, its printed lines held to the worked
case of INTEGRATION.md section 6l -- tests/farthest_first_ref.py on the oracle's distances, and the values worked out by hand."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from farthest_first_ref import NOISE, farthest_first_ref

pytestmark = pytest.mark.gpu

X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
COVER_RADIUS = 0.375


def printed(what, values):
    return what + ":" + "".join(" none" if v == NOISE else " %d" % v for v in values)


def printed_doubles(what, values):
    return what + ":" + "".join(" %s" % ("inf" if v == float("inf") else "%.17g" % v) for v in values)


def test_c_farthest_first_program(tmp_path, oracle):
    exe = tmp_path / "c_farthest_first"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_farthest_first.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(X), 3))
    rows[:, 0] = X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    full = farthest_first_ref(D)
    # what the example is about: the order by hand, a tie that keeps the earlier pick, a tie that goes to the smaller row
    assert full.pick.tolist() == [0, 8, 6, 7, 3, 9, 1, 2, 4, 5] and full.pick_parent[3] == 0 and full.pick_radius[4] == full.pick_radius[5] == 0.375
    assert lines[0] == printed("pick", full.pick), lines[0]
    assert lines[1] == printed_doubles("pick_radius", full.pick_radius), lines[1]
    assert lines[2] == printed("pick_parent", full.pick_parent), lines[2]
    assert lines[3] == "from three seeds: the same picks"
    cut = farthest_first_ref(D, cover_radius=COVER_RADIUS)
    assert cut.pick.tolist() == [0, 8, 6, 7] and cut.rep_of.tolist() == [0, 0, 0, 6, 6, 6, 6, 7, 8, 0]
    assert lines[4] == printed("pick at 0.375", cut.pick), lines[4]
    assert lines[5] == printed("rep_of", cut.rep_of), lines[5]
    assert lines[6] == printed_doubles("rep_dist", cut.rep_dist), lines[6]
    assert len(lines) == 7
