"""The one-workgroup Roothaan kernel (qc_scf_small.hip) at the shapes where its predication, its addressing and its per-shape, per-phase
instances can go wrong and that tests/test_small_roothaan_bits_gpu.py does not reach: n = 13 (odd, a single tile), n = 33 (odd, the first
size of the 2 x 2-tile form, one row and column into the second tile), n = 36, n = 50, an open-shell n = 60 through the per-spin
pre | Jacobi | post instances with the generic dot order, and n = 33 again with a repeated eigensolve.  The runs of SHAPE_CASES
(tools/record_small_bits.py) are replayed and every word of every pass - energy, rms, the final orbital energies, redos, passes - is
compared with tests/golden/small_roothaan_shapes_bits.json, recorded with the library of the commit before the kernel's instruction diet.
The step counts by route of qc_scf_counters show that each record holds the routes it is there for."""
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
    with open(os.path.join(ROOT, "tests", "golden", "small_roothaan_shapes_bits.json")) as f:
        return json.load(f)


def test_every_shape_is_recorded(recorded):
    assert sorted(recorded) == sorted(rec.SHAPE_CASES)
    assert sorted(r["n"] for r in recorded.values()) == [13, 33, 33, 36, 50, 60]


@pytest.mark.parametrize("name", list(rec.SHAPE_CASES))
def test_small_roothaan_shape_bits(recorded, name):
    got, want = rec.run_case(name), recorded[name]
    uhf, npass = rec.SHAPE_CASES[name][2], rec.SHAPE_CASES[name][4]
    assert got["n"] == want["n"] and got["passes"] == want["passes"] == npass <= 12
    for k in ("energy", "rms"):
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b]
        assert len(got[k]) == len(want[k]) and not diff, "%s: %s differs first at pass %d: %s, recorded %s" % ((name, k) + diff[0])
    assert got["orbital_energies"] == want["orbital_energies"], name
    assert got["redos"] == want["redos"], name
    # the routes the record is there for ran (one Roothaan step per spin and pass)
    steps = got["small_steps"]
    assert sum(steps.values()) == npass * (2 if uhf else 1), steps
    if uhf:
        assert steps["jacobi"] >= 1, steps
    elif got["n"] < 24:                                                  # (below the tridiagonal path's smallest n a cold pass is pre | Jacobi | post)
        assert steps["cold"] == 0 and steps["jacobi"] >= 1 and steps["warm"] >= 1, steps
    else:
        assert steps["cold"] >= 1 and steps["warm"] >= 1, steps
    if name.endswith("_repeat"):
        assert got["redos"] >= 1                                         # (the repeat branch ran)
