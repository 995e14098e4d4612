"""The table of tests/tune_contract.py against the sources it mirrors, and kpop_tune itself (which needs no GPU: it does not ask
for an initialised device): a knob added to the library without a row, a default that moved, a knob the header does not name or a
value kpop_tune accepts that the table calls rejected fails here."""
import os
import re

import pytest

from conftest import ROOT
from tune_contract import KNOBS, tuned

KPOP_OK, KPOP_ERR_INVALID = 0, -1  # include/kpop_hip.h, enum kpop_status
EFFECTS = {"bits", "order", "approx", "none"}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _tune_body():
    src = _read("kpop_amd", "csrc", "runtime.hip")
    body = src[src.index('extern "C" int kpop_tune('):]
    return body[:body.index("\n}\n")]


def test_every_key_of_kpop_tune_has_a_row():
    keys = re.findall(r'!strcmp\(key, "(\w+)"\)', _tune_body())
    assert len(keys) == len(set(keys)) >= 28, keys
    assert set(keys) == set(KNOBS), (sorted(set(keys) - set(KNOBS)), sorted(set(KNOBS) - set(keys)))


def test_rows_are_well_formed():
    for key, row in KNOBS.items():
        assert row["effect"] in EFFECTS, key
        assert row["default"] in row["values"], key
        assert not set(row["values"]) & set(row["rejected"]), key
        assert row["rejected"] or key == "dbg", key  # (dbg takes any bit field)


def test_defaults_are_those_of_the_context():
    inits = dict(re.findall(r"^\s*int tune_(\w+) = (-?\d+);", _read("kpop_amd", "csrc", "common.h"), flags=re.M))
    assert set(inits) == set(KNOBS), (sorted(set(inits) ^ set(KNOBS)))
    for key, row in KNOBS.items():
        assert int(inits[key]) == row["default"], (key, inits[key], row["default"])


def test_the_header_names_every_knob():
    comments = " ".join(re.findall(r"/\*.*?\*/", _read("include", "kpop_hip.h"), flags=re.S))
    missing = [key for key in KNOBS if key != "dbg" and '"%s"' % key not in comments]
    assert not missing, missing


def test_the_header_names_the_three_classes_and_claims_no_blanket_identity():
    src = _read("include", "kpop_hip.h")
    comment = src[:src.index("int kpop_tune(")]
    comment = comment[comment.rindex("/*"):]
    assert "results are identical for every setting" not in comment
    for word in ("SAME BITS", "ORDER", "APPROXIMATION"):
        assert word in comment, word


def test_covered_by_names_a_file_that_sets_the_knob():
    for key, row in KNOBS.items():
        path = os.path.join(ROOT, "tests", row["covered_by"])
        assert os.path.exists(path), (key, path)
        text = open(path).read()
        assert 'tune("%s"' % key in text or re.search(r"tuned\([^()]*\b%s=" % key, text), (key, row["covered_by"])


@pytest.fixture(scope="module")
def lib():
    from kpop_amd import _lib
    return _lib.load()


def test_kpop_tune_accepts_the_values_and_refuses_the_rest(lib):
    try:
        for key, row in KNOBS.items():
            for value in row["values"]:
                assert lib.kpop_tune(key.encode(), value) == KPOP_OK, (key, value, lib.kpop_last_error())
            for value in row["rejected"]:
                assert lib.kpop_tune(key.encode(), value) == KPOP_ERR_INVALID, (key, value)
                assert b"unknown knob or value %s=%d" % (key.encode(), value) in lib.kpop_last_error(), (key, value)
        assert lib.kpop_tune(b"no_such_knob", 1) == KPOP_ERR_INVALID
        assert b"unknown knob or value no_such_knob=1" in lib.kpop_last_error()
        assert lib.kpop_tune(b"", 0) == KPOP_ERR_INVALID
        assert lib.kpop_tune(None, 0) == KPOP_ERR_INVALID
        assert b"null key" in lib.kpop_last_error()
    finally:
        for key, row in KNOBS.items():
            assert lib.kpop_tune(key.encode(), row["default"]) == KPOP_OK, key


def test_tuned_puts_every_knob_back_when_the_block_fails_or_a_value_is_refused(lib, monkeypatch):
    """no getter: what kpop_tune was last called with, per key, through api.tune"""
    from kpop_amd import api
    last = {}
    real = api.tune
    monkeypatch.setattr(api, "tune", lambda key, value: (real(key, value), last.__setitem__(key, value)))
    with pytest.raises(ZeroDivisionError):
        with tuned(unroll=16, seg=64):
            assert last == {"unroll": 16, "seg": 64}
            1 / 0
    assert last == {"unroll": 8, "seg": 0}
    last.clear()
    with pytest.raises(api.KPopError):
        with tuned(nt=1, tileg=48, pipeprio=3):
            pytest.fail("tileg = 48 was accepted")
    assert last == {"nt": 2, "tileg": 64, "pipeprio": 1}
