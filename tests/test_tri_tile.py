"""The folded upper triangle of a self-join (kpop_amd/csrc/tri_tile.h) apart from the kernels that walk it: which tile a block owns,
for 1 .. 12 row tiles, both tile shapes and every first row tile.  tools/probes/src/tri_tile_check.cpp includes the header alone and
is built with the host compiler; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tile_of_the_triangle_has_one_owner(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "tools", "probes", "src", "tri_tile_check.cpp")
    exe = str(tmp_path / "tri_tile_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True, timeout=300)
    run = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert run.returncode == 0 and len(lines) == 2 and all(l.endswith("bad 0") for l in lines), run.stdout + run.stderr
    assert "kf 1" in lines[0] and "kf 8" in lines[1], run.stdout
