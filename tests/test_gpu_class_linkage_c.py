"""The class linkage and the classes' tree from a plain C99 host (examples/c_class_linkage.c): compiled with gcc against
include/kpop_hip.h and the shared library as tests/test_gpu_lof_c.py compiles examples/c_lof.c, run on the GPU, its printed lines held to
the worked case of INTEGRATION.md section 6o -- tests/class_linkage_ref.py on the oracle's distances, and the table's values as
literals."""
import os
import subprocess

import numpy as np
import pytest

from class_linkage_ref import class_linkage_ref, class_tree_ref
from conftest import ROOT
from test_class_linkage_ref import HAND_CLASS, HAND_MAX, HAND_MEAN, HAND_MIN, HAND_MIN_I, HAND_MIN_J, HAND_N, HAND_ROWS, HAND_TREES, HAND_X

pytestmark = pytest.mark.gpu


def pair_line(a, b, mean, lo, hi, mi, mj):
    return "classes %d %d: mean %.17g min %.17g (rows %d %d) max %.17g" % (a, b, mean[a][b], lo[a][b], mi[a][b], mj[a][b], hi[a][b])


def test_c_class_linkage_program(tmp_path, oracle):
    exe = tmp_path / "c_class_linkage"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_class_linkage.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(HAND_X), 3))
    rows[:, 0] = HAND_X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    want = class_linkage_ref(D, HAND_CLASS, HAND_N)
    assert lines[0] == "class_rows:" + "".join(" %d" % n for n in want[0]) == "class_rows:" + "".join(" %d" % n for n in HAND_ROWS)
    k = 1
    for a in range(3):
        for b in range(a, 3):
            # the reference on the oracle's distances, and the table of the section by literal value
            assert lines[k] == pair_line(a, b, *want[1:]) == pair_line(a, b, HAND_MEAN, HAND_MIN, HAND_MAX, HAND_MIN_I, HAND_MIN_J), (lines[k], a, b)
            k += 1
    assert lines[7] == "class 3: empty" and lines[8] == "without a set: the same bits"
    k = 9
    for linkage, name, table in ((0, "single", want[2]), (1, "complete", want[3]), (2, "average", want[1])):
        ref, hand = class_tree_ref(want[0], table, linkage), HAND_TREES[linkage]
        for t in range(2):
            show = lambda tr: "%s merge %d: nodes %d %d -> node %d at %.17g, %d rows" % (name, t, tr[0][t], tr[1][t], HAND_N + t, tr[2][t], tr[3][t])  # noqa: E731
            assert lines[k] == show(ref) == show(hand), (lines[k], show(hand))
            k += 1
    assert len(lines) == 15
