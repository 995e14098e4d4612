"""The silhouette and the medoids from a plain C99 host (examples/c_silhouette.c): compiled with gcc against include/kpop_hip.h and the
shared library as tests/test_gpu_dbscan_c.py compiles examples/c_dbscan.c, run on the GPU, its printed lines compared with
tests/silhouette_ref.py on the oracle's distances."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dbscan_ref import dbscan_ref
from silhouette_ref import NO_CLASS, silhouette_ref, summary_ref

pytestmark = pytest.mark.gpu

X = [0.0, 0.125, 0.25, 1.125, 1.25, 1.375, 1.5, 0.75, 5.0, 0.375]
EPS, MIN_PTS = 0.375, 4


def test_c_silhouette_program(tmp_path, oracle):
    import kpop_amd
    exe = tmp_path / "c_silhouette"
    lib = os.path.join(ROOT, "kpop_amd")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_silhouette.c"),
                    "-L" + lib, "-lkpop_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    rows = np.zeros((len(X), 3))
    rows[:, 0] = X
    D = oracle.distance_rowwise(rows, rows, np.ones(3), 0, 2.0, False)
    class_of, n_classes, _ = kpop_amd.dense_labels(dbscan_ref(D, EPS, MIN_PTS)[0])
    own, other, ocls, sil, class_rows, medoid, medoid_mean = silhouette_ref(D, class_of, n_classes)
    # what the example is about: a border row with silhouette exactly 0, a noise row left out, a medoid on a tie
    assert n_classes == 2 and sil[7] == 0.0 and class_of[8] == NO_CLASS and medoid.tolist() == [1, 4] and own[1] == own[2]
    assert lines[0] == "classes: 2"
    for i in range(len(X)):
        if class_of[i] == NO_CLASS:
            assert lines[1 + i] == "row %d: left out" % i
        else:
            assert lines[1 + i] == "row %d: class %d own %.17g other %.17g (class %d) silhouette %.17g" % (i, class_of[i], own[i], other[i], ocls[i], sil[i]), lines[1 + i]
    for c in range(2):
        assert lines[11 + c] == "class %d: %d rows, medoid row %d at %.17g" % (c, class_rows[c], medoid[c], medoid_mean[c]), lines[11 + c]
    assert lines[13] == "without a set: the same bits"
    mean, overall = summary_ref(class_of, n_classes, sil)
    assert lines[14] == "mean silhouette: class 0 %.17g, class 1 %.17g, all rows %.17g" % (mean[0], mean[1], overall), lines[14]
    assert len(lines) == 15
