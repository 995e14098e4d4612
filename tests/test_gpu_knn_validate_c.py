"""The k-NN validation from a plain C99 host (examples/c_knn_validate.c): compiled with gcc against include/kpop_hip.h and the shared
library as tests/test_gpu_knn_vote_c.py compiles examples/c_knn_vote.c, run on the GPU, its printed accuracies and votes compared with
tests/knn_validate_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from knn_validate_ref import knn_validate_ref
from knn_vote_ref import NO_CLASS

pytestmark = pytest.mark.gpu

D, ROWS, CLASSES = 4, 10, 3
KS = (1, 3, 5, 8)


def ref_value(i, c):
    return ((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (0.5 if c == i % D else 0.0)


def test_c_knn_validate_program(tmp_path, oracle):
    exe = tmp_path / "c_knn_validate"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_knn_validate.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[ref_value(2 if i == ROWS - 1 else i, c) for c in range(D)] for i in range(ROWS)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    dist = oracle.distance_rowwise(rows, rows, metric, 0, 2.0, True)
    class_of = np.arange(ROWS) % CLASSES
    cls, votes, n, first, correct = knn_validate_ref(dist, class_of, KS)
    assert lines[0] == "leave-one-out"
    for t, k in enumerate(KS):
        assert lines[1 + t] == "k = %d: %d of %d correct" % (k, correct[t], ROWS), lines[1 + t]
    at = 1 + len(KS)
    assert not np.any(cls[1] == NO_CLASS)
    for j in range(ROWS):
        want = "row %d (class %u): class %u with %u of %u, nearest at %.15g" % (j, class_of[j], cls[1][j], votes[1][j], n[1][j], first[1][j])
        assert lines[at + j] == want, (lines[at + j], want)
    at += ROWS
    # the last row is row 2: each is the other's nearest neighbour, at 0 -- the duplicate stays, the row itself does not
    assert cls[0][2] == class_of[ROWS - 1] and cls[0][ROWS - 1] == class_of[2] and first[0][2] == first[0][ROWS - 1] == 0.0 and n[0][2] == 1
    assert lines[at] == "groups of three"
    correct_g = knn_validate_ref(dist, class_of, KS, np.arange(ROWS) // 3)[4]
    for t, k in enumerate(KS):
        assert lines[at + 1 + t] == "k = %d: %d of %d correct" % (k, correct_g[t], ROWS), lines[at + 1 + t]
    at += 1 + len(KS)
    assert lines[at:] == ["ks = 3, 1: invalid", "ks = 0, 2: invalid", "no k: invalid", "ks = 5, 129: unsupported"]
