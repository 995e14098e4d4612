"""CPU tests of the boundary: the C-ABI library loads, exports every symbol include/kpop_hip.h
declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "kpop_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kpop_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported():
    from kpop_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "libkpop_hip.so does not export %s" % n
    assert set(_lib.SIGNATURES) == set(names), "python binding and header disagree"


def test_library_is_in_tree():
    from kpop_amd import _lib
    assert os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "kpop_amd")


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under kpop_amd/ may import, link or read it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "kpop_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".c", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "kpop_oracle" not in text and "import oracle" not in text and "from oracle" not in text, (dirpath, f)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_cpu_fallback():
    import kpop_amd
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.init(0)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.count_reads(np.frombuffer(b"ACGTACGT", dtype=np.uint8), [0, 8], 3)
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.distance_rowwise(np.ones((1, 2)), np.ones((1, 2)), np.ones(2))


def test_metric_matches_oracle(oracle):
    """kpop_metric_compute is O(n_dims) host arithmetic inside the library (lib/Space.ml:88-105)."""
    import kpop_amd
    for n in (1, 9, 64):
        w = oracle.synth_inertia(n)
        assert np.array_equal(kpop_amd.metric_compute(w), oracle.metric_powers(w, 1.0, 1.0, 2.0))
        assert np.array_equal(kpop_amd.metric_compute(w, kpop_amd.METRIC_POWERS, 0.5, 0.7, 1.5),
                              oracle.metric_powers(w, 0.5, 0.7, 1.5))
        assert np.array_equal(kpop_amd.metric_compute(w, kpop_amd.METRIC_FLAT), oracle.metric_flat(n))
    with pytest.raises(kpop_amd.KPopError):
        kpop_amd.metric_compute([1.0], kpop_amd.METRIC_POWERS, -1.0, 1.0, 2.0)  # Negative_power, lib/Space.ml:124


def _last_error_is_per_thread():
    """(the body of the test below; runs in a process of its own, where no kpop_init has happened)"""
    import ctypes as C
    import threading
    from kpop_amd import _lib
    lib = _lib.load()
    assert lib.kpop_device_slots() == 0
    turn = [threading.Event() for _ in range(4)]
    seen, errors = {}, []

    def msg():
        return lib.kpop_last_error().decode()

    def thread_a():
        try:
            seen["a0"] = msg()
            rc = lib.kpop_dev_workspace_reserve_stream(4096, None)  # a device entry point without kpop_init
            seen["a_rc"], seen["a1"] = rc, msg()
            turn[0].set()
            assert turn[1].wait(30)
            seen["a2"] = msg()  # ... after B's failure
            rc = lib.kpop_dev_count_twist(None, None, None, 1, 0, 0, 0, 1, None, None)
            seen["a_rc2"], seen["a3"] = rc, msg()
            turn[2].set()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            for t in turn:
                t.set()

    def thread_b():
        try:
            assert turn[0].wait(30)
            seen["b0"] = msg()  # A has failed, B has not
            w, out = (C.c_double * 2)(1.0, 2.0), (C.c_double * 2)()
            rc = lib.kpop_metric_compute(1, w, 2, -1.0, 1.0, 2.0, out)  # Negative_power, lib/Space.ml:124: pure host arithmetic
            seen["b_rc"], seen["b1"] = rc, msg()
            turn[1].set()
            assert turn[2].wait(30)
            seen["b2"] = msg()  # ... after A's second failure
            turn[3].set()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            for t in turn:
                t.set()

    threads = [threading.Thread(target=thread_a), threading.Thread(target=thread_b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
        assert not t.is_alive(), "a thread did not finish"
    if errors:
        raise errors[0]
    assert seen["a0"] == "" and seen["b0"] == ""  # a thread that has not failed has no message, whatever the others did
    assert seen["a_rc"] == -5 and "kpop_init" in seen["a1"]  # KPOP_ERR_NOT_INIT
    assert seen["b_rc"] == -1 and "negative power" in seen["b1"]  # KPOP_ERR_INVALID
    assert seen["a2"] == seen["a1"] and seen["b2"] == seen["b1"]  # each its own, unchanged by the other's later failure
    assert seen["a_rc2"] == -5 and seen["a3"] == seen["a1"]
    assert lib.kpop_last_error().decode() == ""  # the main thread never failed


def test_last_error_is_per_thread():
    """kpop_last_error() is thread-local (include/kpop_hip.h, conventions): one thread takes KPOP_ERR_NOT_INIT from a device entry
    point, another the "negative power" failure of kpop_metric_compute (host arithmetic, lib/Space.ml:124); each reads its own
    message, before and after the other's later failure.  In a fresh process: no kpop_init has happened there, GPU or not."""
    import subprocess
    import sys
    code = "import sys; sys.path[:0] = [%r, %r]; import test_abi; test_abi._last_error_is_per_thread()" % (os.path.join(ROOT, "tests"), ROOT)
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_parse_distance():
    import kpop_amd
    assert kpop_amd.parse_distance("euclidean") == (kpop_amd.EUCLIDEAN, 2.0)
    assert kpop_amd.parse_distance("cosine")[0] == kpop_amd.COSINE
    assert kpop_amd.parse_distance("minkowski(1.5)") == (kpop_amd.MINKOWSKI, 1.5)
    for bad in ("manhattan", "minkowski(x)", "minkowski(-1)"):
        with pytest.raises(ValueError):
            kpop_amd.parse_distance(bad)


def test_pack_bases_on_the_host():
    """kpop_pack_bases needs no GPU: 2-bit codes (A0 C1 G2 T3, either case; base i in bits 2 (i % 16).. of word i / 16) and a bit a base
    that is none of ACGTacgt, whatever the number of threads and wherever the batch ends (bin/KPopCount.ml:242-245: Lint.dnaize)"""
    import numpy as np
    from kpop_amd import api
    rng = np.random.RandomState(3)
    lut = {ord(ch): i for i, ch in enumerate("ACGT")}
    lut.update({ord(ch): i for i, ch in enumerate("acgt")})
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 100003):
        b = np.frombuffer(bytes(rng.choice(list(b"ACGTacgtNnRYKM-*.x\x00\xff"), size=n).astype(np.uint8)), dtype=np.uint8) if n else np.zeros(0, np.uint8)
        c, m = api.pack_bases(b, threads=1)
        c3, m3 = api.pack_bases(b, threads=3)
        assert np.array_equal(c, c3) and np.array_equal(m, m3)
        assert len(c) == max((n + 15) // 16, 1) and len(m) == max((n + 31) // 32, 1)
        for i in range(n):
            code, inv = (int(c[i // 16]) >> (2 * (i % 16))) & 3, (int(m[i // 32]) >> (i % 32)) & 1
            if int(b[i]) in lut:
                assert inv == 0 and code == lut[int(b[i])], (n, i, chr(b[i]))
            else:
                assert inv == 1, (n, i, int(b[i]))
        if n % 32:
            assert (int(m[-1]) >> (n % 32)) == (1 << (32 - n % 32)) - 1  # (past the batch's end: no bases)
