"""The SCF driver (qc_scf.cpp) computes what it computed before it was rewritten as a sequence of steps, bit for bit: the runs of the
second table of tools/record_small_bits.py (PASS_CASES) are replayed and every word - energy and rms of every pass, final orbital
energies, redos, passes - is compared with tests/golden/scf_pass_bits.json, recorded with the library of the commit before the rewrite.
The systems are the smallest (all n <= 64) at which each form of a pass can go wrong: the generic launch sequence for RHF, for UHF with
the spins side by side and one after the other, and for an open shell; the one-workgroup kernels of two spins side by side; the wait on
the event; stored mode; a one-rank communicator; and the repeat of an eigensolve on the generic, the side-by-side and the communicator
path."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_small_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded():
    return {"pass": _golden("scf_pass_bits.json"), "small": _golden("small_roothaan_bits.json")}


def test_every_case_is_recorded(recorded):
    assert sorted(recorded["pass"]) == sorted(rec.PASS_CASES)


def test_records_of_the_same_run_are_equal(recorded):
    """Spins one after the other against side by side, the event wait against the sequence word: the same words."""
    for name, table, twin in rec.SAME_AS:
        assert recorded["pass"][name] == recorded[table][twin], (name, twin)


def test_repeat_cases_repeated_when_recorded(recorded):
    for name in rec.REPEAT_CASES:
        if name in rec.PASS_CASES:
            assert recorded["pass"][name]["redos"] >= 1, name


@pytest.mark.parametrize("name", list(rec.PASS_CASES))
def test_scf_pass_bits(recorded, name):
    got, want = rec.run_case(name), recorded["pass"][name]
    assert got["n"] == want["n"] and got["passes"] == want["passes"] == rec.PASS_CASES[name][4]
    for k in ("energy", "rms"):
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b]
        assert len(got[k]) == len(want[k]) and not diff, "%s: %s differs first at pass %d: %s, recorded %s" % ((name, k) + diff[0])
    assert got["orbital_energies"] == want["orbital_energies"], name
    assert got["redos"] == want["redos"], name
    if name in rec.REPEAT_CASES:
        assert got["redos"] >= 1                                         # (the repeat branch ran)
    for case, table, twin in rec.SAME_AS:
        if case == name:
            assert got == recorded[table][twin], (name, twin)            # (and this run equals its twin's record word for word)
