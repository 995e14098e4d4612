"""Density peaks from a plain C99 host (examples/c_density_peaks.c): compiled with gcc against include/kpop_hip.h and the shared library
as tests/test_gpu_lof_c.py compiles examples/c_lof.c, run on the GPU, its printed lines held to the worked case of INTEGRATION.md
section 6p -- tests/density_peaks_ref.py on the oracle's distances, and the table's values as literals."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from density_peaks_ref import density_peaks_ref
from test_density_peaks_ref import HAND_CUTS, HAND_DELTA, HAND_DENSITY, HAND_EPS, HAND_PARENT, HAND_X

pytestmark = pytest.mark.gpu


def printed(what, values):
    return what + ":" + "".join(" %d" % v for v in values)


def printed_doubles(what, values):
    return what + ":" + "".join(" %.17g" % v for v in values)


def test_c_density_peaks_program(tmp_path, oracle):
    exe = tmp_path / "c_density_peaks"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_density_peaks.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(HAND_X), 3))
    rows[:, 0] = HAND_X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    want = density_peaks_ref(D, eps=HAND_EPS)
    # the reference on the oracle's distances, and the table of the section by literal value
    for i, (name, ref, hand) in enumerate((("density", want.density, HAND_DENSITY), ("delta", want.delta, HAND_DELTA), ("parent", want.parent, HAND_PARENT))):
        show = printed if name == "parent" else printed_doubles
        assert lines[i] == show(name, ref) == show(name, hand), (lines[i], show(name, hand))
    for i, (at, ((min_density, min_delta), labels, counts)) in enumerate(zip(("(-inf, 2)", "(2, 2)"), HAND_CUTS)):
        cut = density_peaks_ref(D, eps=HAND_EPS, min_density=min_density, min_delta=min_delta)
        assert lines[3 + 2 * i] == printed("labels at " + at, cut.labels) == printed("labels at " + at, labels)
        assert lines[4 + 2 * i] == printed("counts at " + at, cut.counts) == printed("counts at " + at, counts)
    assert lines[7] == "the cut in the call: the same labels"
    assert lines[8] == "without a set: the same result"
    assert lines[9] == "no eps: -1, a NaN threshold: -1, a parent below its child: -1"
    assert len(lines) == 10
