"""The values on points and the point-charge embedding, bit for bit: tools/record_points_bits.py's runs replayed against
tests/golden/points_embed_bits.json, which was recorded (device part on an MI355X, host part on a CPU-only machine) with the library of
the commit before the potential and the field became one record walk with one driver and one dispatch.  Every output is compared as the
SHA-256 of its bytes; the first eight words are kept for diagnosis.

Systems: water/cc-pVTZ (n = 58: all seven pair orders, a group of two LDS tiles with a partial second one, the order-7 tables of the
field and of the atoms' gradient), far (n = 32: both sides of the Boys switch), deep (n = 18: deep contractions); 300 points and 300
charges each.  Outputs: v_elec, e_elec, rho, V_pc (automatic and both forced orientations), the charges' gradient, the four terms of
gradient(D, W) with charges set; for water a UHF(5, 5) state's potential, field, gradient and charges' gradient after six passes; on the
host the potential and field matrices of three points and the embedding matrix."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_points_bits as REC

with open(os.path.join(ROOT, "tests", "golden", "points_embed_bits.json")) as _f:
    GOLD = json.load(_f)


def _compare(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key] == want[key], (what, key, got[key]["head"], want[key]["head"])


def test_the_record_holds_every_case():
    for part in ("gpu", "host"):
        assert sorted(GOLD[part]) == sorted(REC.SYSTEMS)
    assert len(GOLD["uhf"]) == 4 and all(len(GOLD["gpu"][name]) == 11 and len(GOLD["host"][name]) == 1 + 2 * REC.HOST_POINTS for name in REC.SYSTEMS)


@pytest.mark.parametrize("name", REC.SYSTEMS)
def test_host_matrices_keep_their_bits(name):
    _compare(REC.run_host(name), GOLD["host"][name], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REC.SYSTEMS)
def test_device_outputs_keep_their_bits(name):
    _compare(REC.run_gpu(name), GOLD["gpu"][name], name)


@pytest.mark.gpu
def test_uhf_state_outputs_keep_their_bits():
    _compare(REC.run_uhf(), GOLD["uhf"], "uhf")
