"""The k-NN vote from a plain C99 host (examples/c_knn_vote.c): compiled with gcc against include/kpop_hip.h and the shared library as
tests/test_gpu_within_c.py compiles examples/c_within.c, run on the GPU, its printed votes compared with tests/knn_vote_ref.py on the
oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from knn_vote_ref import knn_vote_ref

pytestmark = pytest.mark.gpu

D, ROWS, QUERIES, CLASSES = 4, 9, 3, 3


def ref_value(i, c):
    return ((i * 7 + c * 3) % 11) / 4.0 - 1.0 + (0.5 if c == i % D else 0.0)


def test_c_knn_vote_program(tmp_path, oracle):
    exe = tmp_path / "c_knn_vote"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_knn_vote.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = np.array([[ref_value(i, c) for c in range(D)] for i in range(ROWS)])
    queries = np.array([[ref_value(4, c) if j == 2 else ref_value(j + 1, c) + (c + 1) / 16.0 for c in range(D)] for j in range(QUERIES)])
    metric = oracle.metric_powers(np.array([0.4, 0.3, 0.2, 0.1]))
    dist = oracle.distance_rowwise(rows, queries, metric, 0, 2.0, True)
    class_of = np.arange(ROWS) % CLASSES
    at = 0
    for k in (1, 5, 128):
        cls, votes, n, first = knn_vote_ref(dist, class_of, k)
        assert lines[at] == "k = %d" % k, lines[at]
        for j in range(QUERIES):
            assert lines[at + 1 + j] == "query %d: class %u with %u of %u, nearest at %.15g" % (j, cls[j], votes[j], n[j], first[j]), (k, lines[at + 1 + j])
        at += 1 + QUERIES
    one = knn_vote_ref(dist, class_of, 1)
    assert one[0][2] == 4 % CLASSES and one[3][2] == 0.0  # query 2 is row 4
    assert knn_vote_ref(dist, class_of, 128)[2].tolist() == [ROWS] * QUERIES
    assert lines[at] == "k = 3, classes alone:" + "".join(" %u" % c for c in knn_vote_ref(dist, class_of, 3)[0])
    assert lines[at + 1] == "k = 129: unsupported"
    assert len(lines) == at + 2
