"""The body of the column Fock kernels (qc_fock_body, qc_fock_kernel.h) computes what it computed before the bra-run mode was taken out
of it and it was split into named pieces, bit for bit: the cases of tools/record_fock_bits.py are replayed and the class map, the SHA-256
of G (RHF), G_alpha and G_beta (UHF, Da != Db), the ERI tensor and the Schwarz factors, and each array's sum and max-abs word are compared
with tests/golden/fock_column_bits.json, recorded with the library of the commit before that work.  Each case is the smallest system in
the tree that reaches the piece it is there for (table in the recorder), and the class map is checked for that piece's class."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_fock_bits as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "fock_column_bits.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(rec.CASES)
    for name, want in recorded.items():
        rec.check_classes(name, {int(c): k for c, k in want["classes"].items()})


@pytest.mark.parametrize("name", list(rec.CASES))
def test_fock_column_bits(recorded, name):
    got, want = rec.run_case(name), recorded[name]                       # (run_case asserts the case's class forms)
    assert got["n"] == want["n"] == rec.CASES[name][4]
    assert got["classes"] == want["classes"], name
    assert got["schwarz_pairs"] == want["schwarz_pairs"], name
    for k in ("schwarz", "eri", "fock_rhf", "fock_uhf"):
        far = {w: (float.fromhex(got[k][w]), float.fromhex(want[k][w])) for w in ("sum", "maxabs")}
        assert got[k] == want[k], "%s: %s differs from the record; (got, recorded) %s" % (name, k, far)
