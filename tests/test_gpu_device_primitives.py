"""The header primitives every kernel rests on (kpop_amd/csrc/scan.h, radix_sort.h, lookback.h, wave_select.h and the parts of
wave_sort.h that test_gpu_wave_sort.py leaves out), each on its own against the standard library on the host:
tools/probes/src/device_primitives_check.hip is built once and each of its sub-commands runs as a process of its own.  The case
names are spelt out here, so a case that silently leaves the program fails its test; every case must end in `bad 0`, and the
self-test must show every sub-command's comparison failing on a perturbed host copy."""
import itertools
import os
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_TIMEOUT = 600
RUN_TIMEOUT = 60  # a sub-command takes a few seconds; if one needs more than ~10 s, shrink its largest case, not this

# a child that ended by a signal or at its time limit: nothing more of this module is started on the device
_stopped = []


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "tools", "probes", "src", "device_primitives_check.hip")
    exe = str(tmp_path_factory.mktemp("device_primitives") / "device_primitives_check")
    t0 = time.perf_counter()
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-o", exe, src], check=True, timeout=BUILD_TIMEOUT,
                   capture_output=True, text=True)
    print("device_primitives_check: built in %.1f s" % (time.perf_counter() - t0))
    return exe


def _run(exe, arg):
    if _stopped:
        pytest.fail("not started: %s" % _stopped[0])
    t0 = time.perf_counter()
    try:
        p = subprocess.run([exe, arg], timeout=RUN_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _stopped.append("`%s` was still running after %d s" % (arg, RUN_TIMEOUT))
        pytest.fail("%s\n%s" % (_stopped[0], e.stdout))
    print("device_primitives_check %s: %.2f s" % (arg, time.perf_counter() - t0))
    if p.returncode < 0:
        _stopped.append("`%s` ended by signal %d" % (arg, -p.returncode))
        pytest.fail("%s\n%s\n%s" % (_stopped[0], p.stdout[-4000:], p.stderr[-4000:]))
    return p


def _cases(out, prefix=""):
    found = {}
    for line in out.splitlines():
        if " bad " not in line or not line.startswith(prefix):
            continue
        name, bad = line[len(prefix):].rsplit(" bad ", 1)
        assert name not in found, "case printed twice: " + name
        found[name] = int(bad)
    return found


def _check(exe, sub, expected):
    assert len(set(expected)) == len(expected)
    p = _run(exe, sub)
    found = _cases(p.stdout)
    missing = sorted(set(expected) - set(found))
    extra = sorted(set(found) - set(expected))
    wrong = {n: b for n, b in found.items() if b != 0}
    assert not wrong, "%d of %d cases differ from the host: %s" % (len(wrong), len(found), dict(itertools.islice(wrong.items(), 20)))
    assert not missing and not extra, "missing %s, not expected %s" % (missing[:20], extra[:20])
    assert p.returncode == 0, (p.returncode, p.stderr[-4000:])


SCAN_TILE = 4096
RADIX_FAMILIES = ["random64", "three_values", "all_equal", "all_ones", "ones_in_last_wave", "ascending", "descending",
                  "equal_low_bits"]
SELECT_FAMILIES = ["distinct", "five_values", "all_equal", "mostly_zeros", "signed_zeros", "denormals_and_huge", "negatives"]
MERGE_FAMILIES = ["rise_fall", "fall_rise", "plateaus", "all_equal", "ascending", "descending"]
UNIQUE_FAMILIES = ["no_sentinel", "all_sentinel", "all_equal", "all_distinct", "runs_cross_lanes", "runs_end_at_lanes",
                   "partly_valid"]


@pytest.mark.gpu
def test_scan_against_partial_sum(check_exe):
    T = SCAN_TILE
    ns = [0, 1, 255, 256, T - 1, T, T + 1, 3 * T + 17, 1024 * T, 1024 * T + 1, 2049 * T + 5]
    expected = ["scan exclusive n=%d %s" % (n, f) for n in ns for f in ("zeros", "ones", "flags", "counts")]
    expected.append("scan exclusive n=%d tile_max" % (3 * T + 17))  # tile totals of 2^32 - 4096, a grand total beyond 2^32
    expected += ["scan block_sums nb=%d" % nb for nb in (0, 1, 63, 64, 65, 1023, 1024, 1025, 3000)]
    assert len(expected) == 54
    _check(check_exe, "scan", expected)


@pytest.mark.gpu
def test_radix_sort_against_stable_sort(check_exe):
    ns = [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1, 40000]
    bits = [0, 1, 8, 9, 20, 40, 63, 64]
    expected = ["radix %s n=%d bits=%d %s" % (kind, n, b, f)
                for kind in ("keys", "pairs") for n in ns for b in bits for f in RADIX_FAMILIES]
    assert len(expected) == 1280
    _check(check_exe, "radix", expected)


@pytest.mark.gpu
def test_lookback_against_prefix_sum_in_ticket_order(check_exe):
    expected = ["lookback %s tickets=%d %s naps=%d" % (kind, n, f, naps)
                for kind in ("one_level", "grouped") for n in (1, 2, 63, 64, 65, 128, 129, 197, 513, 1100)
                for f in ("zeros", "ones", "below_2p20", "below_2p40") for naps in (1, 16)]
    assert len(expected) == 160
    _check(check_exe, "lookback", expected)


@pytest.mark.gpu
def test_select_rank_against_sorted_copy(check_exe):
    expected = []
    for R in (1, 2, 4, 8, 16, 32):
        ms = sorted({m for m in (1, 2, 63, 64, 65, 64 * R - 1, 64 * R) if m <= 64 * R})
        expected += ["select R=%d m=%d %s %s" % (R, m, f, layout)
                     for m in ms for f in SELECT_FAMILIES for layout in ("in_order", "shuffled")]
    assert len(expected) == (4 + 5 * 7) * 7 * 2
    _check(check_exe, "select", expected)


@pytest.mark.gpu
def test_wave_networks_against_their_definitions(check_exe):
    expected = ["wave sort_pairs R=%d" % R for R in (1, 2, 4, 8)]
    expected += ["wave merge_striped RP=%d %s" % (RP, f) for RP in (1, 2, 4, 8, 16) for f in MERGE_FAMILIES]
    expected += ["wave unique K=%d R=%d %s" % (K, R, f) for K in (32, 64) for R in (1, 2, 4, 8) for f in UNIQUE_FAMILIES]
    expected += ["wave mirror G=%d K=%d" % (G, K) for G in (2, 4, 8, 16, 32, 64) for K in (32, 64)]
    expected += ["wave row_shift 0x%x K=%d" % (c, K) for c in (0x104, 0x114) for K in (32, 64)]
    assert len(expected) == 4 + 30 + 56 + 12 + 4
    _check(check_exe, "wave", expected)


@pytest.mark.gpu
def test_selftest_every_comparison_can_fail(check_exe):
    p = _run(check_exe, "--selftest")
    found = _cases(p.stdout, "selftest ")
    for sub in ("scan", "radix", "lookback", "select", "wave"):
        mine = {n: b for n, b in found.items() if n.startswith(sub + " ")}
        assert mine, "no perturbed case of " + sub
        assert all(b > 0 for b in mine.values()), mine
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
