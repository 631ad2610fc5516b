"""`--dipole` and `--polarizability` of the `qchem-hip` front end (qchem-rs_amd/cli.py): the flags and their rejection with `--follow`, the
printed lines with stubbed drivers (CPU-only, as tests/test_cli.py), and one real run on the GPU against the Python API."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(ROOT, "data", "basis", "STO-3G.json")
M = os.path.join(ROOT, "data", "mol", "water.json")


def _cli():
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    return cli


def test_flags_default_off_and_are_rejected_with_follow(capsys):
    cli = _cli()
    for cmd in ("rhf", "uhf"):
        a = cli.parse_args([cmd, "-b", B, "-m", M])
        assert (a.dipole, a.polarizability) == (False, False)
        a = cli.parse_args([cmd, "-b", B, "-m", M, "--dipole", "--polarizability"])
        assert (a.dipole, a.polarizability) == (True, True)
        for flag in ("--dipole", "--polarizability"):
            with pytest.raises(SystemExit):
                cli.parse_args([cmd, "-b", B, "-m", M, "--follow", flag])
            assert "--follow cannot be combined" in capsys.readouterr().err


def _parse(lines):
    """the numbers of the property lines: (mu a.u., mu Debye, |mu| a.u., |mu| Debye, alpha rows, isotropic)"""
    i = next(k for k, l in enumerate(lines) if l.startswith("dipole moment (a.u.): "))
    mu = [float(x) for x in lines[i].split(": ")[1].split()]
    assert lines[i + 1].startswith("dipole moment (Debye): ")
    deb = [float(x) for x in lines[i + 1].split(": ")[1].split()]
    assert lines[i + 2].startswith("|mu|: ")
    w = lines[i + 2].split()
    assert w[2] == "a.u." and w[3] == "=" and w[5] == "Debye"
    j = lines.index("polarizability (a.u.):")
    rows = [[float(x) for x in lines[j + 1 + k].split()] for k in range(3)]
    assert lines[j + 4].startswith("isotropic polarizability: ")
    return np.array(mu), np.array(deb), float(w[1]), float(w[4]), np.array(rows), float(lines[j + 4].split(": ")[1])


def test_printed_lines_parse_with_stubbed_drivers(monkeypatch, capsys):
    cli = _cli()
    from qchem_rs_amd import hf
    out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11)
    alpha = np.array([[7.0, 0.0, 0.25], [0.0, 3.0, 0.0], [0.25, 0.0, 5.0]])

    class State:
        def dipole(self): return np.array([0.0, -0.3, 0.4])
        def polarizability(self): return hf.PolarizabilityOutput(alpha, 5.0, np.zeros(3), True, 4, 9, 1.5, 1.0)

    monkeypatch.setattr(hf, "_stepped", lambda system, cfg, uhf, after: (out, after(State())))
    assert cli.main(["rhf", "-b", B, "-m", M, "--dipole", "--polarizability", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[1:5] == ["electronic energy: -84.151", "nuclear repulsion energy: 9.188", "hartree fock energy: -74.963",
                          "orbital energies: [-20.243, -1.267, 0.606]"]
    mu, deb, n_au, n_deb, rows, iso = _parse(lines)
    assert np.allclose(mu, [0.0, -0.3, 0.4], atol=1e-8) and np.allclose(deb, mu * 2.541746473, atol=1e-7)
    assert abs(n_au - 0.5) < 1e-8 and abs(n_deb - 0.5 * 2.541746473) < 1e-7
    assert np.allclose(rows, alpha, atol=1e-8) and abs(iso - 5.0) < 1e-8
    doc = json.loads(lines[-1])
    assert doc["dipole"]["au"] == [0.0, -0.3, 0.4] and doc["polarizability"]["alpha"] == alpha.tolist()
    assert doc["polarizability"]["isotropic"] == 5.0 and doc["polarizability"]["builds"] == 9 and doc["polarizability"]["converged"] is True
    assert "stability" not in doc and "gradient" not in doc and "mp2" not in doc
    # without the flags the run is the plain one
    monkeypatch.setattr(hf, "restricted_hartree_fock", lambda system, cfg: out)
    assert cli.main(["rhf", "-b", B, "-m", M]) == 0
    assert len(capsys.readouterr().out.splitlines()) == 5


@pytest.mark.gpu
def test_json_and_lines_carry_the_values_of_the_python_api(capsys):
    import qchem_rs_amd as q
    cli = _cli()
    basis, mol = os.path.join(ROOT, "data", "basis", "cc-pVDZ.json"), M
    assert cli.main(["rhf", "-b", basis, "-m", mol, "--epsilon", "1e-9", "--dipole", "--polarizability", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    doc = json.loads(lines[-1])
    mu, deb, n_au, n_deb, rows, iso = _parse(lines)
    res = q.hf._stepped(q.MolecularSystem.load(mol, q.BasisSet.load(basis)), q.HartreeFockConfig(100, 1e-9), False,
                        lambda st: (st.dipole(), st.polarizability()))
    assert res is not None
    _, (mu_api, pol) = res
    # (the same deterministic path twice: the same bits)
    assert doc["dipole"]["au"] == mu_api.tolist() and doc["polarizability"]["alpha"] == pol.alpha.tolist()
    assert doc["polarizability"]["isotropic"] == pol.isotropic and doc["polarizability"]["converged"] is True
    assert doc["polarizability"]["builds"] == pol.builds and doc["polarizability"]["iterations"] == pol.iterations
    assert np.allclose(mu, mu_api, atol=1e-8) and np.allclose(deb, mu_api * 2.541746473, atol=1e-7) and abs(n_au - np.linalg.norm(mu_api)) < 1e-8
    assert abs(n_deb - n_au * 2.541746473) < 1e-7
    assert np.allclose(rows, pol.alpha, atol=1e-8) and abs(iso - pol.isotropic) < 1e-8

    assert cli.main(["uhf", "-b", basis, "-m", mol, "--epsilon", "1e-9", "--dipole", "--polarizability", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    doc_u = json.loads(lines[-1])
    assert np.allclose(doc_u["dipole"]["au"], mu_api, atol=1e-6) and np.allclose(doc_u["polarizability"]["alpha"], pol.alpha, atol=1e-4)
