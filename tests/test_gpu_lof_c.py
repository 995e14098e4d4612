"""The local outlier factor from a plain C99 host (examples/c_lof.c): compiled with gcc against include/kpop_hip.h and the shared
library as tests/test_gpu_kmedoids_c.py compiles examples/c_kmedoids.c, run on the GPU, its printed lines held to the worked case of
INTEGRATION.md section 6n -- tests/lof_ref.py on the oracle's distances, and the table's values as literals."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lof_ref import lof_ref, lof_score_ref
from test_lof_ref import (HAND_K, HAND_KDIST, HAND_LOF, HAND_LRD, HAND_N, HAND_Q, HAND_Q_KDIST, HAND_Q_LOF, HAND_Q_LRD, HAND_Q_N, HAND_X)

pytestmark = pytest.mark.gpu


def printed(what, values):
    return what + ":" + "".join(" %d" % v for v in values)


def printed_doubles(what, values):
    return what + ":" + "".join(" %.17g" % v for v in values)


def test_c_lof_program(tmp_path, oracle):
    exe = tmp_path / "c_lof"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_lof.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows, queries = np.zeros((len(HAND_X), 3)), np.zeros((len(HAND_Q), 3))
    rows[:, 0], queries[:, 0] = HAND_X, HAND_Q
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    E = oracle.distance_rowwise(rows, queries, np.ones(3), 0, 2.0, False)
    assert E.shape == (len(HAND_Q), len(HAND_X))
    want = lof_ref(D, HAND_K)
    score = lof_score_ref(E, HAND_K, want.kdist, want.lrd)
    # the reference on the oracle's distances, and the table of the section by literal value
    for i, (name, ref, hand) in enumerate((("kdist", want.kdist, HAND_KDIST), ("n_neigh", want.n_neigh, HAND_N), ("lrd", want.lrd, HAND_LRD),
                                           ("lof", want.lof, HAND_LOF))):
        show = printed if name == "n_neigh" else printed_doubles
        assert lines[i] == show(name, ref) == show(name, hand), (lines[i], show(name, hand))
    assert lines[4] == "kdist is core_distances(k + 1): yes"
    for i, (name, ref, hand) in enumerate((("query kdist", score.kdist, HAND_Q_KDIST), ("query n_neigh", score.n_neigh, HAND_Q_N),
                                           ("query lrd", score.lrd, HAND_Q_LRD), ("query lof", score.lof, HAND_Q_LOF))):
        show = printed if name == "query n_neigh" else printed_doubles
        assert lines[5 + i] == show(name, ref) == show(name, hand), (lines[5 + i], show(name, hand))
    assert lines[9] == "without a set: the same result"
    assert lines[10] == "k = 0: -1, k = 129: -3"
    assert len(lines) == 11
