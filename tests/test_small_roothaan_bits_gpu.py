"""The one-workgroup Roothaan kernel (qc_scf_small.hip) computes what it computed before its latency work, bit for bit: the runs of
tools/record_small_bits.py are replayed and every word - energy and rms of every pass, final orbital energies, redos, passes - is
compared with tests/golden/small_roothaan_bits.json, recorded with the library of the commit before that work.  The systems are the
smallest at which each form of the kernel can go wrong (one tile per wave at n = 7 and 24, 2 x 2 tiles with partial edge tiles at n = 50
and 58, the repeat after ROTATE, the rotation-only open-shell route with the generic-order dots)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_small_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "small_roothaan_bits.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(rec.CASES)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_small_roothaan_bits(recorded, name):
    got, want = rec.run_case(name), recorded[name]
    assert got["n"] == want["n"] and got["passes"] == want["passes"] == rec.CASES[name][4]
    for k in ("energy", "rms"):
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b]
        assert len(got[k]) == len(want[k]) and not diff, "%s: %s differs first at pass %d: %s, recorded %s" % ((name, k) + diff[0])
    assert got["orbital_energies"] == want["orbital_energies"], name
    assert got["redos"] == want["redos"], name
    if name == "h2o_tz_repeat":
        assert got["redos"] >= 1                                         # (the repeat branch ran)
