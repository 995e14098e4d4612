"""CPU tests of the boundary of the clusters at a distance: include/kpop_hip.h declares the four functions with the lines of the
reference they stand on, the library exports them, the Python table binds them, and the package offers them."""
import os
import re

from conftest import ROOT

FUNCTIONS = ["kpop_clusters_within", "kpop_dev_clusters_within_workspace_bytes", "kpop_dev_clusters_within", "kpop_distance_clusters"]


def test_header_declares_and_library_exports_the_four_functions():
    from kpop_amd import _lib
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kpop_[a-z0-9_]*clusters[a-z0-9_]*)\s*\(", code))
    assert declared == set(FUNCTIONS)
    assert code.index("kpop_distance_within(") < code.index("kpop_clusters_within(")  # the block after the range queries
    lib = _lib.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), "libkpop_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    # every declaration says which lines of the reference it stands on, as its neighbours do
    for name in FUNCTIONS:
        before = src[:src.index(name + "(")]
        comment = before[before.rindex("/*"):]
        assert "lib/Matrix.ml:" in comment or "lib/Space.ml:" in comment, name


def test_python_surface():
    import kpop_amd
    for name in ("distance_clusters", "dev_clusters_within_workspace_bytes", "dev_clusters_within"):
        assert hasattr(kpop_amd, name) and name in kpop_amd.__all__
    assert callable(kpop_amd.RefSet.clusters)


def test_the_kernels_are_built_from_their_own_file():
    mk = open(os.path.join(ROOT, "kpop_amd", "csrc", "Makefile")).read()
    assert "clusters.hip" in mk
    src = open(os.path.join(ROOT, "kpop_amd", "csrc", "clusters.hip")).read()
    for kernel in ("clusters_init_kernel", "clusters_tile_kernel", "clusters_flatten_kernel"):
        assert "void " + kernel in src
