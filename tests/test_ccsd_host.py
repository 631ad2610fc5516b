"""Host tests of the CCSD feature: the spin-orbital numpy reference of tests/ccsd_reference.py against pinned numbers, the map from its
amplitudes onto the closed-shell layout the GPU test compares in, H2 against full CI, and what of qc_scf_ccsd and `rhf --ccsd` needs no
device.

The pinned numbers are those of a plain denominator iteration (no DIIS) to max |dt| <= 1e-11 from the oracle's ERI tensor and a numpy
RHF converged to max |dD| <= 1e-11.  water_crawford/STO-3G agrees with the published -0.049149636120 and -0.070680088376 for this
geometry to 6e-10.  Measured here: every pinned energy is reproduced to <= 5e-13, the closed-shell energy expression equals the
spin-orbital one to <= 2e-17, and H2 CCSD equals the full-CI correlation energy to 9e-13."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import ROOT, load_system
import ccsd_reference as R
from test_dipole_host import _h2, _numpy_rhf

# name, n_frozen, E(MP2), E(CCSD), iterations, T1 diagnostic, max |t2|
PINNED = [("h2@1.4/6-31G", 0, -0.017390457635, -0.024936326683, 24, 0.00574, 0.0772),
          ("water_crawford/STO-3G", 0, -0.049149636689, -0.070680088811, 37, 0.00991, 0.1002),
          ("water_crawford/STO-3G", 1, -0.049060281438, -0.070616816874, 37, 0.01108, 0.1002),
          ("water/6-31G", 0, -0.104729670606, -0.110689391318, 29, 0.00790, 0.0531),
          ("water/6-31G", 1, -0.103568040891, -0.109658040800, 29, 0.00880, 0.0531)]
_cache = {}


def _scf(name):
    if name not in _cache:
        from oracle.oracle import Oracle
        m = _h2() if name.startswith("h2") else load_system(*name.split("/"))
        o = Oracle(m)
        S, H, I = o.overlap(), o.kinetic() + o.nuclear(), o.eri()
        nocc = int(np.sum(m.atomic_numbers())) // 2
        e, C, eps = _numpy_rhf(S, H, I, nocc)
        _cache[name] = (H, I, C, eps, nocc, e)
    return _cache[name]


def _reference(name, nf):
    if (name, nf) not in _cache:
        _, I, C, eps, nocc, _ = _scf(name)
        _cache[(name, nf)] = R.ccsd(I, C, eps, nocc, nf, tol=1e-11)
    return _cache[(name, nf)]


@pytest.mark.parametrize("name,nf,e_mp2,e_ccsd,its,t1d,t2max", PINNED)
def test_reference_reproduces_the_pinned_energies(name, nf, e_mp2, e_ccsd, its, t1d, t2max):
    r = _reference(name, nf)
    d = R.diagnostics(r)
    print(name, nf, "E(MP2) %.12f E(CCSD) %.12f" % (r.e_mp2, r.e_ccsd), "differences", r.e_mp2 - e_mp2, r.e_ccsd - e_ccsd, "iterations", r.iterations, d)
    assert r.converged and r.iterations == its
    assert abs(r.e_mp2 - e_mp2) <= 1e-9 and abs(r.e_ccsd - e_ccsd) <= 1e-9
    assert abs(d[0] - t1d) <= 5e-6 and abs(d[2] - t2max) <= 5e-5                    # (the digits the table gives)


@pytest.mark.parametrize("name,nf", [(p[0], p[1]) for p in PINNED])
def test_closed_shell_projection_of_the_reference(name, nf):
    """The alpha-beta-alpha-beta block of T2 has t_ij^ab = t_ji^ba, the same-spin block is its antisymmetrised image, and the closed-shell
    energy expression over the projected amplitudes equals the spin-orbital energy."""
    r = _reference(name, nf)
    t1, t2 = R.closed_shell(r)
    o, v = r.o, r.v
    assert t1.shape == (o, v) and t2.shape == (o, o, v, v)
    assert np.abs(t2 - t2.transpose(1, 0, 3, 2)).max() <= 1e-14
    assert np.abs(r.t1[o:, v:] - t1).max() <= 1e-14 and np.abs(r.t1[:o, v:]).max() == 0.0
    assert np.abs(r.t2[:o, :o, :v, :v] - (t2 - t2.transpose(0, 1, 3, 2))).max() <= 1e-13
    e = R.closed_shell_energy(r)
    print(name, nf, "closed-shell - spin-orbital energy", e - r.e_ccsd)
    assert abs(e - r.e_ccsd) <= 1e-12


def test_h2_ccsd_is_full_ci():
    """Two electrons: CCSD is exact.  Full CI here: the two-electron Hamiltonian over the products phi_p(1) phi_q(2) of the four MOs,
    H[pq, rs] = h_pr d_qs + d_pr h_qs + (pr|qs), restricted to the symmetric (singlet) combinations and diagonalised."""
    H, I, C, eps, nocc, e_rhf = _scf("h2@1.4/6-31G")
    r = _reference("h2@1.4/6-31G", 0)
    n = C.shape[0]
    h = C.T @ H @ C
    mo = R.mo_integrals(I, C, 0, n)
    eye = np.eye(n)
    H2 = (np.einsum("pr,qs->pqrs", h, eye) + np.einsum("pr,qs->pqrs", eye, h) + mo.transpose(0, 2, 1, 3)).reshape(n * n, n * n)
    basis = []
    for p in range(n):
        for q in range(p, n):
            x = np.zeros((n, n))
            x[p, q] += 1.0
            x[q, p] += 1.0
            basis.append(x.ravel() / np.linalg.norm(x))
    U = np.array(basis).T                                                           # 16 x 10, orthonormal
    e_fci = np.linalg.eigvalsh(U.T @ H2 @ U)[0]
    assert abs((2.0 * h[0, 0] + mo[0, 0, 0, 0]) - e_rhf) <= 1e-10                    # (the determinant's energy in the same integrals)
    print("H2: E(FCI) - E(RHF) = %.12f, E(CCSD) = %.12f, difference %.2e" % (e_fci - e_rhf, r.e_ccsd, e_fci - e_rhf - r.e_ccsd))
    assert abs((e_fci - e_rhf) - r.e_ccsd) <= 1e-9


# ---- the C ABI and the command line without a device

def test_abi_surface():
    import qchem_rs_amd as q
    L = q.lib()
    # header: 4 int32, tol, 2 + 4 doubles, 4 int32, 4 doubles
    assert ctypes.sizeof(q.hf._Ccsd) == 4 * 4 + 8 + 6 * 8 + 4 * 4 + 4 * 8 == 120
    assert q.hf._Ccsd.tol.offset == 16 and q.hf._Ccsd.e_mp2.offset == 24 and q.hf._Ccsd.iterations.offset == 72 and q.hf._Ccsd.ms_total.offset == 88
    with open(os.path.join(ROOT, "include", "qchem_hip.h")) as f:
        header = f.read()
    body = header[header.index("int32_t n_frozen, max_iterations, diis_size, reserved0;"):header.index("} qc_ccsd;")]
    assert [w.strip(" ;,") for w in body.split() if w.strip(" ;,") in ("int32_t", "double")] == ["int32_t", "double", "double", "double", "int32_t", "double"]
    for name in ("qc_scf_ccsd", "qc_debug_gemm"):
        assert hasattr(L, name) and name in q.hf.EXPORTS
    io = q.hf._Ccsd()
    assert L.qc_scf_ccsd(None, ctypes.byref(io), None, None) == q.hf.QC_ERR_INVALID
    assert L.qc_scf_ccsd(None, None, None, None) == q.hf.QC_ERR_INVALID
    A = np.zeros((2, 2))
    p = A.ctypes.data_as(ctypes.c_void_p)
    for bad in ((2, 2, 2, 2), (1, 0, 2, 2), (1, 2, 0, 2), (1, 2, 2, 0)):
        assert L.qc_debug_gemm(bad[0], bad[1], bad[2], bad[3], 1.0, p, p, 0.0, p, 0, None) == q.hf.QC_ERR_INVALID
    assert L.qc_debug_gemm(1, 2, 2, 2, 1.0, None, p, 0.0, p, 0, None) == q.hf.QC_ERR_INVALID


def test_command_line_flag_is_rhf_only(capsys):
    from qchem_rs_amd import cli
    args = cli.parse_args(["rhf", "-b", "b", "-m", "m", "--ccsd", "--frozen-core", "1"])
    assert args.ccsd and args.frozen_core == 1 and not args.mp2
    assert not cli.parse_args(["rhf", "-b", "b", "-m", "m"]).ccsd
    for argv in (["uhf", "-b", "b", "-m", "m", "--ccsd"], ["rhf", "-b", "b", "-m", "m", "--ccsd", "--follow"],
                 ["rhf", "-b", "b", "-m", "m", "--ccsd", "--solvent", "78.4"], ["rhf", "-b", "b", "-m", "m", "--frozen-core", "1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
    assert "unrecognized arguments: --ccsd" in capsys.readouterr().err


def test_cli_prints_the_ccsd_lines_with_a_stubbed_driver(monkeypatch, capsys):
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli, hf
    b, m = os.path.join(ROOT, "data", "basis", "STO-3G.json"), os.path.join(ROOT, "data", "mol", "water.json")
    out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11)
    seen = []

    class State:
        converged = True

        def ccsd(self, n_frozen):
            seen.append(n_frozen)
            return hf.CcsdOutput(-0.03125, -0.0625, 0.015625, 0.02, 0.1, 1e-9, 12, self.converged, n_frozen, 4.0, 1.0, 2.0, 1.0)

        def mp2(self, n_frozen):
            return hf.Mp2Output(-0.02, -0.01125, -0.03125, 1.0, 1.0, 1.0, n_frozen)

    monkeypatch.setattr(hf, "_stepped", lambda system, cfg, uhf, after: (out, after(State())))
    assert cli.main(["rhf", "-b", b, "-m", m, "--ccsd", "--frozen-core", "1", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    e_hf = out.total_energy()
    assert lines[5:10] == ["ccsd first-iteration (mp2) correlation energy: -0.0312500000", "ccsd correlation energy: -0.0625000000",
                           "ccsd total energy: %.10f" % (e_hf - 0.0625), "ccsd t1 diagnostic: 0.015625", "ccsd converged after 12 iterations"]
    doc = json.loads(lines[-1])
    assert doc["ccsd"]["e_ccsd"] == -0.0625 and doc["ccsd"]["e_mp2"] == -0.03125 and doc["ccsd"]["e_total"] == e_hf - 0.0625
    assert doc["ccsd"]["iterations"] == 12 and doc["ccsd"]["converged"] is True and doc["ccsd"]["n_frozen"] == 1 and doc["ccsd"]["t1_diagnostic"] == 0.015625
    assert set(doc["ccsd"]["timings_ms"]) == {"total", "tensor", "transform", "solve"} and "mp2" not in doc
    # with --mp2 the MP2 lines come first; amplitudes that do not converge end the command with the SCF's status
    State.converged = False
    assert cli.main(["rhf", "-b", b, "-m", m, "--ccsd", "--mp2"]) == 101
    cap = capsys.readouterr()
    lines = cap.out.splitlines()
    assert lines[5].startswith("mp2 correlation energy: ") and lines[6].startswith("mp2 total energy: ") and lines[7].startswith("ccsd first-iteration (mp2) ")
    assert sum(l.startswith("mp2 correlation energy: ") for l in lines) == 1
    assert lines[11] == "ccsd did not converge after 12 iterations" and "ccsd did not converge" in cap.err
    assert seen == [1, 0]
