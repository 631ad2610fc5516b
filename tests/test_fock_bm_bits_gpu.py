"""The bra-major Fock kernels (qc_fock_bm_kernel<LCD, HI>, qc_fock_bm.hip) compute what they computed before their unused variants were
removed and qc_bm_pass / qc_bm_body were carved into named pieces, bit for bit: the bra-major cases of tools/record_fock_bits.py are
replayed and the class map, the quartets of each bra-major launch, the SHA-256 of G (RHF), G_alpha and G_beta (UHF, Da != Db), the ERI
tensor and the Schwarz factors, and each array's sum and max-abs word are compared with tests/golden/fock_bm_bits.json, recorded with the
library of the commit before that work.  Both builds are also replayed with QC_BM_NO_ROWBUF=1 (exchange contributions as global atomics:
another summation order, words of their own).  Each case is the smallest system in the tree that reaches the instance it is there for
(table in the recorder), and its class map and launch quartets are checked for that instance."""
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
    with open(os.path.join(ROOT, "tests", "golden", "fock_bm_bits.json")) as f:
        return json.load(f)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(rec.BM_CASES)
    for name, want in recorded.items():
        rec.check_bm_case(name, {int(c): k for c, k in want["classes"].items()}, want["units"])


def _same(name, k, got, want):
    far = {w: (float.fromhex(got[w]), float.fromhex(want[w])) for w in ("sum", "maxabs")}
    assert got == want, "%s: %s differs from the record; (got, recorded) %s" % (name, k, far)


@pytest.mark.parametrize("name", list(rec.BM_CASES))
def test_fock_bm_bits(recorded, name):
    got, want = rec.run_case(name, bm=True), recorded[name]              # (run_case asserts the case's instances)
    assert got["n"] == want["n"] == rec.BM_CASES[name][4]
    assert got["classes"] == want["classes"], name
    assert got["units"] == want["units"], name
    assert got["schwarz_pairs"] == want["schwarz_pairs"], name
    for k in ("schwarz", "eri", "fock_rhf", "fock_uhf"):
        _same(name, k, got[k], want[k])
    for k in ("fock_rhf", "fock_uhf"):
        _same(name, k + " without the row buffer", got["no_rowbuf"][k], want["no_rowbuf"][k])
