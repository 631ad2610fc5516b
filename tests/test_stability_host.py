"""CPU tests of the stability surface.  The dense reference (tests/stability_reference.py) is pinned: fed with the oracle's converged
densities and ERI tensor it reproduces the recorded eigenvalues of (A + B) (tests/golden/stability_golden.json) to 1e-6, the precision they
are quoted to, and the second-order energy of a rotation along an eigenvector with the constants of DESIGN.md 3.8.  The new entry points are
declared, listed and exported; their argument checks answer on the host with no device present; the CLI parses --stability / --follow."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, data, load_system
import stability_reference as R

NEW = ("qc_scf_stability_dim", "qc_scf_stability", "qc_scf_rotated_density", "qc_scf_begin_rhf_from", "qc_scf_begin_uhf_from")
TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "stability_golden.json")) as f:
        return json.load(f)


def h2(R_bohr):
    import qchem_rs_amd as q
    b = q.BasisSet.load(data("basis", "6-31G.json"))
    return q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, float(R_bohr)])], b)


def _rhf_state(m):
    from oracle.oracle import Oracle
    o = Oracle(m)
    I = o.eri()
    r = o.rhf(500, 1e-10, eri=I)
    assert r["status"] == 0
    S, H = o.overlap(), o.kinetic() + o.nuclear()
    C, eps = R.orbitals(R.fock_rhf(I, H, r["density"]), S)
    return I, H, C, eps, m.n_electrons // 2, r


@pytest.mark.parametrize("dist", ["1.4", "2.0", "2.5", "3.0"])
def test_reference_reproduces_h2_eigenvalues(golden, dist):
    I, H, C, eps, no, r = _rhf_state(h2(float(dist)))
    want = golden["h2_631g"][dist]
    for kind, name in ((0, "singlet"), (1, "triplet")):
        if name in want:
            assert abs(np.linalg.eigvalsh(R.hessian_rhf(I, C, eps, no, kind))[0] - want[name]) < TOL, (dist, name)
    if "energy" in want:
        assert abs(r["total_energy"] - want["energy"]) < TOL


@pytest.mark.parametrize("mol,basis,key", [("water", "cc-pVDZ", "water_ccpvdz"), ("ethylene", "6-31G", "ethylene_631g")])
def test_reference_reproduces_closed_shell_eigenvalues(golden, mol, basis, key):
    I, H, C, eps, no, _ = _rhf_state(load_system(mol, basis))
    for kind, name in ((0, "singlet"), (1, "triplet")):
        assert abs(np.linalg.eigvalsh(R.hessian_rhf(I, C, eps, no, kind))[0] - golden[key][name]) < TOL, name


def test_reference_reproduces_the_oxygen_saddle(golden):
    from oracle.oracle import Oracle
    g = golden["oxygen_triplet_ccpvdz"]
    o = Oracle(load_system("oxygen", "cc-pVDZ"))
    I = o.eri()
    r = o.uhf(600, 1e-10, g["n_alpha"], g["n_beta"], eri=I)
    assert r["status"] == 0 and r["iterations"] == g["passes"] and abs(r["total_energy"] - g["energy"]) < TOL
    S, H = o.overlap(), o.kinetic() + o.nuclear()
    Fa, Fb = R.fock_uhf(I, H, r["density_alpha"], r["density_beta"])
    (Ca, ea), (Cb, eb) = R.orbitals(Fa, S), R.orbitals(Fb, S)
    w = np.linalg.eigvalsh(R.hessian_uhf(I, Ca, ea, g["n_alpha"], Cb, eb, g["n_beta"]))
    assert np.abs(w[:5] - np.array(g["lowest"])).max() < TOL
    assert (w < -1e-5).sum() == 3


def test_rotation_energy_follows_the_eigenvalue_with_the_documented_constant():
    """E(theta) - E(0) = c theta^2 lambda, c = 2 for an RHF vector (both spins rotate), checked by rotating the oracle's H2 R = 3.0
    determinant along the triplet eigenvector (alpha by +theta, beta by -theta) and along the singlet one."""
    I, H, C, eps, no, r = _rhf_state(h2(3.0))
    for kind in (0, 1):
        w, V = np.linalg.eigh(R.hessian_rhf(I, C, eps, no, kind))
        for theta in (0.01, 0.02):
            Ca, Cb = R.rotate(C, no, V[:, 0], theta), R.rotate(C, no, V[:, 0], -theta if kind == 1 else theta)
            Da, Db = Ca @ Ca.T, Cb @ Cb.T
            Fa, Fb = R.fock_uhf(I, H, Da, Db)
            e = 0.5 * (np.sum(Da * (H + Fa)) + np.sum(Db * (H + Fb)))
            assert abs((e - r["electronic_energy"]) / (R.ROTATION_C["rhf"] * theta ** 2 * w[0]) - 1.0) < 0.05, (kind, theta)


def test_stability_entry_points_are_declared_listed_and_exported():
    import qchem_rs_amd as q
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    declared = set(re.findall(r"\b(qc_[a-z0-9_]+)\s*\(", header))
    L = q.lib()
    for name in NEW:
        assert name in declared and name in q.hf.EXPORTS and hasattr(L, name), name
    assert "} qc_stability;" in header
    for name in ("stabilize", "StabilityOutput", "StabilizeOutput"):
        assert hasattr(q, name)
    assert ctypes.sizeof(q.hf._Stability) == 4 * 4 + 8 + 16 * 8 + 4 * 4 + 2 * 8


def test_argument_errors_answer_on_the_host():
    import qchem_rs_amd as q
    L = q.lib()
    s = q.System(h2(3.0))
    vp = ctypes.c_void_p
    INV = q.hf.QC_ERR_INVALID
    io = q.hf._Stability(kind=0, nroots=1)
    x = np.zeros(4)
    D = np.zeros((s.n, s.n))
    p = lambda a: a.ctypes.data_as(vp)
    assert L.qc_scf_stability(None, ctypes.byref(io), None) == INV
    assert L.qc_scf_stability_dim(None, 0) == INV
    assert L.qc_scf_rotated_density(None, 0, p(x), 0.1, p(D), p(D), None) == INV
    out = vp()
    assert L.qc_scf_begin_rhf_from(s.handle, None, ctypes.byref(out)) == INV and not out
    assert L.qc_scf_begin_rhf_from(None, p(D), ctypes.byref(out)) == INV
    assert L.qc_scf_begin_rhf_from(s.handle, p(D), None) == INV
    assert L.qc_scf_begin_uhf_from(s.handle, 1, 1, None, p(D), ctypes.byref(out)) == INV
    assert L.qc_scf_begin_uhf_from(s.handle, 1, 1, p(D), None, ctypes.byref(out)) == INV and not out
    with pytest.raises(q.QcError):
        q.ScfStepper(s, density=np.zeros((3, 3)))                         # wrong shape: refused before the library is called
    import torch
    if not torch.cuda.is_available():
        assert L.qc_scf_begin_rhf_from(s.handle, p(D), ctypes.byref(out)) == q.hf.QC_ERR_NO_DEVICE
    s.close()


@pytest.mark.parametrize("sub", ["rhf", "uhf"])
def test_cli_parses_stability_and_follow(sub):
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    a = cli.parse_args([sub, "-b", B, "-m", M])
    assert a.stability is False and a.follow is False
    a = cli.parse_args([sub, "-b", B, "-m", M, "--stability"])
    assert a.stability is True and a.follow is False
    a = cli.parse_args([sub, "-b", B, "-m", M, "--follow", "--json"])
    assert a.follow is True and a.json is True
