"""CPU test of the large-reference summary's workspace layouts (kpop_amd/csrc/summary_layout.h): tests/host/summary_layout_check.cpp,
a program of its own built with AddressSanitizer + UBSan, runs every route's layout over a null and over a made-up base -- aligned,
disjoint regions inside the size, and a size no larger than the sums of byte counts the routes were written with before."""
import os
import subprocess

from conftest import ROOT


def test_summary_workspace_layouts(tmp_path):
    out = tmp_path / "summary_layout_check"
    src = os.path.join(ROOT, "tests", "host", "summary_layout_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(out), src], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "summary_layout_check: ok" in r.stdout, (r.stdout, r.stderr)
