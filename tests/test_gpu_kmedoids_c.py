"""k-medoids from a plain C99 host (examples/c_kmedoids.c): compiled with gcc against include/kpop_hip.h and the shared library as
tests/test_gpu_farthest_first_c.py compiles examples/c_farthest_first.c, run on the GPU, its printed lines held to the worked case of
INTEGRATION.md section 6m -- tests/kmedoids_ref.py on the oracle's distances, and the values worked out by hand."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from farthest_first_ref import farthest_first_ref
from kmedoids_ref import NO_CLASS, kmedoids_ref

pytestmark = pytest.mark.gpu

X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]


def printed(what, values):
    return what + ":" + "".join(" none" if v == NO_CLASS else " %d" % v for v in values)


def printed_doubles(what, values):
    return what + ":" + "".join(" %.17g" % v for v in values)


def test_c_kmedoids_program(tmp_path, oracle):
    exe = tmp_path / "c_kmedoids"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_kmedoids.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(X), 3))
    rows[:, 0] = X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    init = farthest_first_ref(D, max_picks=3).pick
    assert init.tolist() == [0, 8, 6]
    plain, full = kmedoids_ref(D, init, 0), kmedoids_ref(D, init, 10)
    # what the example is about, by hand: the classes, a medoid tie that goes to the smaller row, the two costs
    assert plain.class_of.tolist() == [0, 0, 0, 2, 2, 2, 2, 0, 1, 0] and plain.cost.tolist() == [2.25] and not plain.converged
    assert full.medoid.tolist() == [2, 8, 4] and full.own_mean[4] == full.own_mean[5] and full.cost.tolist() == [2.25, 1.5]
    assert full.dist.tolist() == [.25, .125, 0, .125, 0, .125, .25, .5, 0, .125] and full.n_iter == 1 and full.converged
    assert lines[0] == printed("init", init), lines[0]
    assert lines[1] == printed("class_of, round 0", plain.class_of), lines[1]
    assert lines[2] == printed_doubles("own_mean, round 0", plain.own_mean), lines[2]
    assert lines[3] == "cost[0] = 2.25, a fixed point: no", lines[3]
    assert lines[4] == printed("medoid", full.medoid), lines[4]
    assert lines[5] == printed("class_of", full.class_of), lines[5]
    assert lines[6] == printed_doubles("dist", full.dist), lines[6]
    assert lines[7] == printed("class_rows", full.class_rows), lines[7]
    assert lines[8] == printed_doubles("cost", full.cost), lines[8]
    assert lines[9] == "n_iter = 1, converged = 1", lines[9]
    assert lines[10] == "continued from the first round: the same result"
    assert len(lines) == 11
