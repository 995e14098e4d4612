"""CPU tests of the resident reference set's boundary: include/kpop_hip.h declares its ten functions, the library exports them, the
Python table binds them, and without a GPU a set refuses to exist (no CPU fallback)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FUNCTIONS = ["kpop_refset_create", "kpop_dev_refset_wrap", "kpop_refset_append", "kpop_refset_info", "kpop_refset_free",
             "kpop_refset_distance_rowwise", "kpop_refset_distance_summary", "kpop_dev_refset_workspace_bytes",
             "kpop_dev_refset_distance_rowwise", "kpop_dev_refset_distance_summary"]


def test_header_declares_and_library_exports_the_ten_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    assert "typedef struct kpop_refset kpop_refset;" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_(?:dev_)?refset_[a-z0-9_]+)\s*\(", code))
    assert declared == set(FUNCTIONS)
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands in for, as the others do
    for name in FUNCTIONS[:3] + FUNCTIONS[5:7]:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment, name


def test_python_surface():
    import kpop_amd
    for name in ("RefSet", "dev_refset_workspace_bytes", "dev_refset_distance_rowwise", "dev_refset_distance_summary"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    for method in ("wrap", "append", "distance_rowwise", "distance_summary", "info", "free"):
        assert callable(getattr(kpop_amd.RefSet, method))
    with pytest.raises(ValueError):
        kpop_amd.RefSet(np.ones((3, 4)), np.ones(5))  # Incompatible_geometries before anything reaches the library


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.RefSet(np.ones((2, 3)), np.ones(3))
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.RefSet.wrap(0, 0, 3, 0)
