"""CPU test of the plan of kpop_dev_count_twist (kpop_amd/csrc/count_twist_plan.h): tests/host/count_twist_plan_check.cpp, a program
of its own built with AddressSanitizer + UBSan, holds pick_R, the segment length, the route at every turn of the decision, the
sub-batch rule and the workspace of every route (aligned, disjoint regions inside a size equal to the sum it was written as) to the
logic as it stood inside kpop_dev_count_twist, restated there."""
import os
import subprocess

from conftest import ROOT


def test_count_twist_plan_and_workspace(tmp_path):
    out = tmp_path / "count_twist_plan_check"
    src = os.path.join(ROOT, "tests", "host", "count_twist_plan_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(out), src], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "count_twist_plan_check: ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
