"""The CLI's --point-charges flag: the printed lines with a stubbed driver (no device), and end to end on the GPU against the oracle."""
import json

import numpy as np
import pytest

from conftest import data, load_system
import embed_reference as ER


def _charge_file(tmp_path):
    f = tmp_path / "charges.json"
    f.write_text(json.dumps([{"charge": float(c), "position": [float(x) for x in r]} for c, r in zip(ER.THREE_Q, ER.THREE_POS)]))
    return str(f)


def test_flag_parses_and_the_file_is_read_like_a_molecule_file(tmp_path):
    from qchem_rs_amd import cli
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    path = _charge_file(tmp_path)
    for sub in ("rhf", "uhf"):
        assert cli.parse_args([sub, "-b", B, "-m", M]).point_charges is None
        assert cli.parse_args([sub, "-b", B, "-m", M, "--point-charges", path, "--gradient"]).point_charges == path
        with pytest.raises(SystemExit):
            cli.parse_args([sub, "-b", B, "-m", M, "--point-charges", path, "--follow"])
    pos, q = cli.load_point_charges(path)
    assert np.array_equal(pos, ER.THREE_POS) and np.array_equal(q, ER.THREE_Q)


def test_printed_lines_with_a_stubbed_driver(monkeypatch, capsys, tmp_path):
    from qchem_rs_amd import cli, hf
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    m = load_system("water", "STO-3G")
    enq = ER.e_nq(m.coordinates(), np.asarray(m.atomic_numbers(), float), ER.THREE_POS, ER.THREE_Q)
    g = np.array([[0.0, 0.0, -0.1], [0.0, 0.05, 0.05], [0.0, -0.05, 0.05]])
    gc = np.array([[0.01, 0.0, 0.0], [0.0, -0.02, 0.0], [0.0, 0.0, 0.03]])
    seen = {}

    class State:
        def point_charge_count(self): return 3
        def point_charge_gradient(self): return gc
        def gradient(self): return g

    def stepped(system, cfg, uhf, after):
        seen["count"], seen["enq"] = system.point_charge_count(), system.point_charge_nuclear_energy()
        out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11, {}, seen["enq"])
        return out, after(State())

    monkeypatch.setattr(hf, "_stepped", stepped)
    assert cli.main(["rhf", "-b", B, "-m", M, "--gradient", "--json", "--point-charges", _charge_file(tmp_path)]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert seen["count"] == 3 and abs(seen["enq"] - enq) <= 1e-13 * abs(enq)
    assert lines[0] == "point charges: 3, nuclei-charges energy: " + cli.fmt_f(enq)
    assert lines[2] == "electronic energy: " + cli.fmt_f(-84.151059) and lines[3] == "nuclear repulsion energy: " + cli.fmt_f(9.188258)
    assert lines[4] == "hartree fock energy: " + cli.fmt_f(-84.151059 + 9.188258 + seen["enq"])
    assert lines[6].split()[2:] == ["0.0000000000", "0.0000000000", "-0.1000000000"]
    assert [l.split() for l in lines[9:12]] == [["q0", "0.0100000000", "0.0000000000", "0.0000000000"], ["q1", "0.0000000000", "-0.0200000000", "0.0000000000"],
                                                ["q2", "0.0000000000", "0.0000000000", "0.0300000000"]]
    doc = json.loads(lines[12])
    assert len(lines) == 13 and doc["point_charges"] == {"count": 3, "nuclear_energy": seen["enq"], "gradient": gc.tolist()}
    assert doc["gradient"] == g.tolist() and doc["total_energy"] == -84.151059 + 9.188258 + seen["enq"]
    # without the flag: the lines of before, no "point_charges" key, and the driver gets the molecule itself

    def plain(system, cfg, uhf, after):
        seen["plain"] = system
        return hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11), (None, g)

    monkeypatch.setattr(hf, "_stepped", plain)
    assert cli.main(["rhf", "-b", B, "-m", M, "--gradient", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert isinstance(seen["plain"], hf.MolecularSystem) and lines[0].startswith("hartree fock converged after 11 iterations")
    assert len(lines) == 9 and "point_charges" not in json.loads(lines[8]) and lines[3] == "hartree fock energy: " + cli.fmt_f(-84.151059 + 9.188258)


@pytest.mark.gpu
@pytest.mark.parametrize("sub", ["rhf", "uhf"])
def test_cli_end_to_end_matches_the_oracle(sub, capsys, tmp_path):
    from oracle.oracle import Oracle
    from qchem_rs_amd import cli
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    m = load_system("water", "STO-3G")
    argv = [sub, "-b", B, "-m", M, "--gradient", "--json", "--epsilon", "1e-10", "--point-charges", _charge_file(tmp_path)]
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    doc = json.loads(lines[-1])
    ref = Oracle(ER.embedded_ghost(m, ER.THREE_POS, ER.THREE_Q)).uhf(200, 1e-10, 5, 5)
    want = ref["total_energy"] - ER.e_cc(ER.THREE_POS, ER.THREE_Q)
    enq = ER.e_nq(m.coordinates(), np.asarray(m.atomic_numbers(), float), ER.THREE_POS, ER.THREE_Q)
    assert lines[0] == "point charges: 3, nuclei-charges energy: " + cli.fmt_f(enq)
    assert abs(doc["total_energy"] - want) < 1e-8 and doc["point_charges"]["count"] == 3
    assert abs(doc["total_energy"] - (doc["electronic_energy"] + doc["nuclear_repulsion"] + doc["point_charges"]["nuclear_energy"])) < 1e-12
    g, gc = np.array(doc["gradient"]), np.array(doc["point_charges"]["gradient"])
    assert g.shape == (3, 3) and gc.shape == (3, 3) and np.abs(g.sum(axis=0) + gc.sum(axis=0)).max() <= 1e-8
    assert [l.split()[0] for l in lines[-4:-1]] == ["q0", "q1", "q2"]
