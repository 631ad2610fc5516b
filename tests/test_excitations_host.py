"""Host tests of the excited-state reference (tests/excitations_reference.py) and of the parts of the new interface that need no device.

The reference is checked before anything trusts it, on numpy RHF states (plain Roothaan iteration on the oracle's integrals, max|dD| <= 1e-11)
of H2 at 1.4 bohr / 6-31G, water/STO-3G, water_crawford/STO-3G and water/cc-pVDZ:

  1. A + B of both kinds equals stability_reference.hessian_rhf (another arrangement of the same integrals).  Bound 1e-12: sums of four
     integrals of magnitude <= 5 in f64; measured <= 3.6e-15.
  2. The CIS matrix built from antisymmetrised spin-orbital integrals has the singlet spectrum once and the triplet spectrum three times.
     Bound 1e-11 (eigenvalues of symmetric matrices of norm <= 25 by LAPACK: a few hundred ulps); measured 9e-16 (H2) to 1.6e-13 (water/cc-pVDZ).
  3. The TDHF sum over all states, 2 sum_k mu_k mu_k^T / w_k, equals the static polarizability of dipole_reference.polarizability_rhf, which a
     finite-field test pins (tests/test_dipole_host.py).  Bound 1e-10 (a non-symmetric eigenproblem against a linear solve); measured
     2.7e-15 (H2), 5.9e-14 (water/STO-3G), 7.5e-13 (water/cc-pVDZ).
  4. Pinned excitation energies and oscillator strengths, produced by an independent script: reproduced to 1e-8.
  5. The C surface without a device: symbols, struct size, null arguments, and the command-line flags."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_system
import dipole_reference as D
import excitations_reference as X
import stability_reference as R
from test_dipole_host import _h2, _numpy_rhf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = {"h2@1.4/6-31G": _h2, "water/STO-3G": lambda: load_system("water", "STO-3G"),
           "water_crawford/STO-3G": lambda: load_system("water_crawford", "STO-3G"), "water/cc-pVDZ": lambda: load_system("water", "cc-pVDZ")}

PINNED = {
    "water_crawford/STO-3G": {("cis", 0): [0.3564617754, 0.4160717500, 0.5056282996], ("cis", 1): [0.2872555165, 0.3444250081, 0.3659890067],
                              ("tdhf", 0): [0.3547782699, 0.4153175060, 0.5001011523], ("tdhf", 1): [0.2851637340, 0.2997434579, 0.3526266685]},
    "h2@1.4/6-31G": {("cis", 0): [0.5600084646, 1.0574655460, 1.6112568775], ("tdhf", 0): [0.5516115504, 1.0517986861, 1.6023528533]},
}
PINNED_F = {"water_crawford/STO-3G": {"cis": [2.3412740e-3, 0.0, 6.4926270e-2, 1.5467354e-2]}, "h2@1.4/6-31G": {"cis": [0.77060040], "tdhf": [0.65129083]}}


@pytest.fixture(scope="module")
def states():
    """per system: I, C, eps, nocc, dipole matrices, r, and per kind (P, M) - computed once"""
    from oracle.oracle import Oracle
    out = {}
    for name, make in SYSTEMS.items():
        m = make()
        o = Oracle(m)
        S, H0, I = o.overlap(), o.kinetic() + o.nuclear(), o.eri()
        nocc = int(np.sum(m.atomic_numbers())) // 2
        _, C, eps = _numpy_rhf(S, H0, I, nocc)
        _, Mdip = D.overlap_and_dipole(m)
        out[name] = dict(I=I, C=C, eps=eps, nocc=nocc, Mdip=Mdip, r=X.rhs(C, nocc, Mdip), PM=[X.matrices_rhf(I, C, eps, nocc, k) for k in (0, 1)])
    return out


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_a_plus_b_is_the_stability_hessian(states, name):
    c = states[name]
    for kind in (0, 1):
        P, M = c["PM"][kind]
        H = R.hessian_rhf(c["I"], c["C"], c["eps"], c["nocc"], kind)
        err = float(np.abs(P - H).max())
        print(name, "kind", kind, "|A + B - hessian_rhf|", err, "asymmetry", float(np.abs(P - P.T).max()), float(np.abs(M - M.T).max()))
        assert err <= 1e-12
        assert np.abs(P - P.T).max() <= 1e-12 and np.abs(M - M.T).max() <= 1e-12
    assert np.array_equal(c["PM"][0][1], c["PM"][1][1])                 # A - B is the same matrix for both kinds


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_spin_orbital_cis_has_the_singlets_once_and_the_triplets_three_times(states, name):
    c = states[name]
    ws, wt = X.cis(*c["PM"][0])[0], X.cis(*c["PM"][1])[0]
    A = X.spin_orbital_cis(c["I"], c["C"], c["eps"], c["nocc"])
    assert np.abs(A - A.T).max() <= 1e-12
    got, want = np.linalg.eigvalsh(A), np.sort(np.concatenate([ws, wt, wt, wt]))
    err = float(np.abs(got - want).max())
    print(name, "dim", A.shape[0], "max |spectrum difference|", err)
    assert got.shape == want.shape and err <= 1e-11


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_tdhf_sum_over_states_is_the_static_polarizability(states, name):
    c = states[name]
    P, M = c["PM"][0]
    w, Rv, Lv = X.tdhf(P, M)
    assert float(np.abs(np.einsum("ki,ki->k", Lv, Rv) - 1.0).max()) <= 1e-10
    res = max(float(np.abs(P @ Rv.T - Lv.T * w).max()), float(np.abs(M @ Lv.T - Rv.T * w).max()))
    mu = X.transition_dipoles(c["r"], Rv)
    sos = 2.0 * np.einsum("kp,kq,k->pq", mu, mu, 1.0 / w)
    alpha, _, _ = D.polarizability_rhf(c["I"], c["C"], c["eps"], c["nocc"], c["Mdip"])
    err = float(np.abs(sos - alpha).max())
    # Thomas-Reiche-Kuhn in a finite basis holds only approximately: print it, assert nothing on it
    print(name, "|sum over states - alpha|", err, "residuals", res, "sum f", float(X.oscillator_strengths(w, mu).sum()), "alpha_zz", alpha[2, 2])
    assert res <= 1e-10 and err <= 1e-10
    # TDHF lies below CIS root by root (both kinds where A + B is positive definite)
    assert np.all(w <= X.cis(P, M)[0] + 1e-12)


@pytest.mark.parametrize("name", list(PINNED))
def test_pinned_values(states, name):
    c = states[name]
    for (method, kind), want in PINNED[name].items():
        P, M = c["PM"][kind]
        w = X.cis(P, M)[0] if method == "cis" else X.tdhf(P, M)[0]
        err = float(np.abs(w[:len(want)] - np.array(want)).max())
        print(name, method, "kind", kind, w[:len(want)].tolist(), "err", err)
        assert err <= 1e-8
    P, M = c["PM"][0]
    for method, want in PINNED_F[name].items():
        if method == "cis":
            w, V = X.cis(P, M)
        else:
            w, V, _ = X.tdhf(P, M)
        f = X.oscillator_strengths(w, X.transition_dipoles(c["r"], V))
        err = float(np.abs(f[:len(want)] - np.array(want)).max())
        print(name, method, "f", f[:len(want)].tolist(), "err", err)
        assert err <= 1e-8


# ---- the C surface without a device

def test_new_symbols_exist_and_reject_null_pointers():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    for name in ("qc_scf_excitations", "qc_scf_excitation_matrices"):
        assert hasattr(L, name) and name in q.hf.EXPORTS and ("int %s(" % name) in header
    assert "} qc_excitations;" in header
    assert hasattr(q, "ExcitationsOutput") and hasattr(q.ScfStepper, "excitations") and hasattr(q.ScfStepper, "excitation_matrices")
    io = q.hf._Excitations(method=1, kind=0, nroots=3)
    assert ctypes.sizeof(io) == 16 + 8 + 64 + 64 + 64 + 192 + 16 + 32
    assert L.qc_scf_excitations(None, ctypes.byref(io), None) == INV
    assert L.qc_scf_excitations(None, None, None) == INV
    buf = np.zeros(9)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.qc_scf_excitation_matrices(None, 0, p, p) == INV and L.qc_scf_excitation_matrices(None, 2, None, None) == INV


def test_cli_flags_parse_on_rhf_and_are_rejected_on_uhf(capsys):
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    b, m = os.path.join(ROOT, "data", "basis", "STO-3G.json"), os.path.join(ROOT, "data", "mol", "water.json")
    a = cli.parse_args(["rhf", "-b", b, "-m", m])
    assert (a.cis, a.tdhf, a.triplets) == (0, 0, False)
    a = cli.parse_args(["rhf", "-b", b, "-m", m, "--cis", "3", "--tdhf", "2", "--triplets"])
    assert (a.cis, a.tdhf, a.triplets) == (3, 2, True)
    for bad in (["--cis", "9"], ["--tdhf", "-1"], ["--triplets"], ["--cis", "2", "--follow"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["rhf", "-b", b, "-m", m] + bad)
        capsys.readouterr()
    for flag in (["--cis", "3"], ["--tdhf", "3"], ["--triplets"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["uhf", "-b", b, "-m", m] + flag)
        assert "unrecognized arguments" in capsys.readouterr().err


def test_cli_prints_one_line_per_state_with_a_stubbed_driver(monkeypatch, capsys):
    import json
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli, hf
    b, m = os.path.join(ROOT, "data", "basis", "STO-3G.json"), os.path.join(ROOT, "data", "mol", "water.json")
    out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11)
    seen = []

    class State:
        def excitations(self, method, kind, nroots):
            seen.append((method, kind, nroots))
            e = np.array([0.25, 0.5, 1.0])[:nroots]
            return hf.ExcitationsOutput(method, kind, e, np.zeros(nroots), np.array([0.125, 0.0, 0.5])[:nroots] * (1 - kind), np.zeros((nroots, 3)), True, False,
                                        nroots, 2, 12, 3.0, 1.0, 1.0, 1.0)

    monkeypatch.setattr(hf, "_stepped", lambda system, cfg, uhf, after: (out, after(State())))
    assert cli.main(["rhf", "-b", b, "-m", m, "--cis", "3", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[5:8] == ["cis singlet state 1: 0.25000000 Eh = 6.802847 eV, f = 0.12500000", "cis singlet state 2: 0.50000000 Eh = 13.605693 eV, f = 0.00000000",
                          "cis singlet state 3: 1.00000000 Eh = 27.211386 eV, f = 0.50000000"]
    doc = json.loads(lines[-1])
    assert len(doc["excitations"]) == 1 and doc["excitations"][0]["energies"] == [0.25, 0.5, 1.0]
    assert doc["excitations"][0]["kind"] == "singlets" and doc["excitations"][0]["method"] == "cis"
    assert cli.main(["rhf", "-b", b, "-m", m, "--tdhf", "2", "--triplets"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[5:] == ["tdhf triplet state 1: 0.25000000 Eh = 6.802847 eV", "tdhf triplet state 2: 0.50000000 Eh = 13.605693 eV"]
    assert seen == [("cis", 0, 3), ("tdhf", 1, 2)]
    # both flags: a list of two; a refused reference is reported and ends the command with status 1
    refused = hf.ExcitationsOutput("tdhf", 1, np.zeros(2), np.zeros(2), np.zeros(2), np.zeros((2, 3)), False, True, 0, 0, 4, 1.0, 0.5, 0.3, 0.2)
    good = State.excitations
    State.excitations = lambda self, method, kind, nroots: refused if method == "tdhf" else good(self, method, kind, nroots)
    assert cli.main(["rhf", "-b", b, "-m", m, "--cis", "1", "--tdhf", "2", "--triplets", "--json"]) == cli.EXCITATIONS_FAILED == 1
    cap = capsys.readouterr()
    doc = json.loads(cap.out.splitlines()[-1])
    assert [e["method"] for e in doc["excitations"]] == ["cis", "tdhf"] and doc["excitations"][1]["reference_unstable"] is True
    assert "the reference is unstable" in cap.err and not any(l.startswith("tdhf") for l in cap.out.splitlines())
