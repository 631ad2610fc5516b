"""Host tests of the dipole matrices (qc_dipole_matrices) against the numpy reference of tests/dipole_reference.py, the self-checks of
that reference, and the argument checks of the new entry points that need no device.

Systems: synthetic_systems.tetra(True, 2), tetra(False, 1), deep() and water/cc-pVTZ - every pair of s..f shells, pure and Cartesian, no
centre on an axis, and 169 > 64 primitive pairs in one shell pair (deep).

Measured on the CPU (max |difference| over the matrix; M with origin 0 and with origin (0.3, -0.2, 0.5)):
  system          n   |S_ref - S_oracle|  |M_host - M_ref|  max|M_ref|  |M_host(O) - M_ref(O)|  |M(O) - (M(0) - O S)|
  tetra-pure-2    64  8.9e-16             1.3e-15           1.90        9.4e-16                 6.7e-16
  tetra-cart-1    80  1.1e-15             2.2e-15           1.90        2.3e-15                 6.7e-16
  deep            18  4.4e-16             1.3e-15           1.10        6.7e-16                 1.3e-15
  water/cc-pVTZ   58  8.9e-16             5.6e-16           1.21        5.6e-16                 2.8e-16
Tolerance of the M checks: 10 x the largest |S_ref - S_oracle| of the four systems (1.1e-14 as measured), never more than 1e-10, times
max(1, max|M_ref|).  The S check itself: 1e-13 - unit-norm functions, sums of at most 169 primitive-pair terms of magnitude <= 1 in f64
(169 x 2.2e-16 = 4e-14), two different recurrences.

Finite-field self-check of the polarizability reference (test_reference_polarizability_is_the_second_derivative_of_the_energy): measured
|alpha_fd - alpha_ref| = 9.3e-6 (H2/6-31G, zz) and <= 9.8e-7 (water/STO-3G) against the bound 1e-4 derived there."""
import ctypes

import numpy as np
import pytest

from conftest import data, load_system
import dipole_reference as D
import stability_reference as R
import synthetic_systems as Y

ORIGIN = np.array([0.3, -0.2, 0.5])
SYSTEMS = {"tetra-pure-2": lambda: Y.tetra(True, 2)[0], "tetra-cart-1": lambda: Y.tetra(False, 1)[0], "deep": lambda: Y.deep()[0],
           "water/cc-pVTZ": lambda: load_system("water", "cc-pVTZ")}
S_BOUND = 1e-13


@pytest.fixture(scope="module")
def computed():
    """per system: reference S and M (origin 0 and ORIGIN), oracle S, host M (both origins), host S - computed once"""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    out = {}
    for name, make in SYSTEMS.items():
        m = make()
        S, M = D.overlap_and_dipole(m)
        _, MO = D.overlap_and_dipole(m, ORIGIN)
        s = q.System(m)
        out[name] = dict(S=S, M=M, MO=MO, S_oracle=Oracle(m).overlap(), S_host=s.overlap(), M_host=s.dipole_matrices(), MO_host=s.dipole_matrices(ORIGIN),
                         M_none=s.dipole_matrices(None))
        s.close()
    for c in out.values():
        c["dS"] = float(np.abs(c["S"] - c["S_oracle"]).max())
    worst = max(c["dS"] for c in out.values())
    for c in out.values():
        c["tol"] = min(10.0 * worst, 1e-10) * max(1.0, float(np.abs(c["M"]).max()))
    return out


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_reference_overlap_reproduces_the_oracle(computed, name):
    c = computed[name]
    print(name, "|S_ref - S_oracle|", c["dS"])
    assert c["S"].shape == c["S_oracle"].shape and c["dS"] <= S_BOUND


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_dipole_matrices_match_the_reference(computed, name):
    c = computed[name]
    d0, dO = float(np.abs(c["M_host"] - c["M"]).max()), float(np.abs(c["MO_host"] - c["MO"]).max())
    print(name, "tol", c["tol"], "|M_host - M_ref|", d0, "with origin", dO, "max|M_ref|", float(np.abs(c["M"]).max()))
    assert c["dS"] <= S_BOUND                                            # (the reference is trusted only where its S is right)
    assert d0 <= c["tol"] and dO <= c["tol"]
    assert np.array_equal(c["M_none"], c["M_host"])                     # a null origin is (0, 0, 0)


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_dipole_matrices_are_exactly_symmetric_and_shift_with_the_origin(computed, name):
    c = computed[name]
    for M in (c["M_host"], c["MO_host"]):
        assert np.array_equal(M, M.transpose(0, 2, 1))
    shift = max(float(np.abs(c["MO_host"][k] - (c["M_host"][k] - ORIGIN[k] * c["S_host"])).max()) for k in range(3))
    print(name, "|M(O) - (M(0) - O S)|", shift, "tol", c["tol"])
    assert shift <= c["tol"]


# ---- the polarizability reference against a finite field

FIELD = 1e-3
# alpha = -d2E/dF2.  Central difference: -(E(F) + E(-F) - 2 E(0)) / F^2 = alpha + gamma F^2 / 12 + O(F^4) with gamma the second
# hyperpolarizability, far below 1e3 a.u. in these small bases -> truncation <= 1e3 x 1e-6 / 12 = 8.3e-5.  The SCF below stops at
# max|dD| <= 1e-11; the energy is stationary, so its error is that squared and what remains is rounding of |E| <= 76 Eh:
# dE <= 1e-12 per energy, four energies' worth over F^2 -> 4e-12 / 1e-6 = 4e-6.  Sum, rounded up: 1e-4.
FD_BOUND = 1e-4


def _numpy_rhf(S, H, I, nocc):
    """plain Roothaan iteration to max|dD| <= 1e-11: (energy without nuclear repulsion, C, eps)"""
    C, eps = R.orbitals(H, S)
    Dm = 2.0 * C[:, :nocc] @ C[:, :nocc].T
    for _ in range(2000):
        F = R.fock_rhf(I, H, Dm)
        C, eps = R.orbitals(F, S)
        Dn = 2.0 * C[:, :nocc] @ C[:, :nocc].T
        done = np.abs(Dn - Dm).max() <= 1e-11
        Dm = Dn
        if done:
            break
    else:
        raise AssertionError("numpy RHF did not converge")
    F = R.fock_rhf(I, H, Dm)
    return 0.5 * float(np.sum(Dm * (H + F))), C, eps


def _h2():
    import qchem_rs_amd as q
    b = q.BasisSet.load(data("basis", "6-31G.json"))
    return q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, 1.4])], b)


@pytest.mark.parametrize("name", ["h2@1.4/6-31G", "water/STO-3G"])
def test_reference_polarizability_is_the_second_derivative_of_the_energy(name):
    """Pins the factor 4 and the signs of polarizability_rhf without a GPU: numpy RHF from the oracle's integrals and the reference's
    dipole matrices under the fields +-F along each axis (an electron in a field F along k: h = h0 + F M_k)."""
    from oracle.oracle import Oracle
    m = _h2() if name.startswith("h2") else load_system("water", "STO-3G")
    o = Oracle(m)
    S, H0, I = o.overlap(), o.kinetic() + o.nuclear(), o.eri()
    S_ref, M = D.overlap_and_dipole(m)
    assert np.abs(S_ref - S).max() <= S_BOUND
    nocc = int(np.sum(m.atomic_numbers())) // 2
    e0, C, eps = _numpy_rhf(S, H0, I, nocc)
    alpha, Hess, r = D.polarizability_rhf(I, C, eps, nocc, M)
    assert np.linalg.eigvalsh(Hess)[0] > 0
    for k in range(3):
        ep, em = _numpy_rhf(S, H0 + FIELD * M[k], I, nocc)[0], _numpy_rhf(S, H0 - FIELD * M[k], I, nocc)[0]
        fd = -(ep + em - 2.0 * e0) / FIELD ** 2
        print(name, "xyz"[k], "finite field", fd, "4 r (A+B)^-1 r", alpha[k, k], "difference", fd - alpha[k, k])
        assert abs(fd - alpha[k, k]) <= FD_BOUND
    assert alpha[2, 2] > 0.1                                             # (a factor or a sign wrong would not hide behind a zero)
    unc = D.uncoupled_rhf(C, eps, nocc, M)
    assert np.all(np.diag(unc) >= 0) and np.abs(alpha - alpha.T).max() <= 1e-12


# ---- the C ABI without a device

def test_new_symbols_exist_and_reject_null_pointers():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    for name in ("qc_dipole_matrices", "qc_dipole_matrices_gpu", "qc_scf_dipole", "qc_scf_polarizability"):
        assert hasattr(L, name) and name in q.hf.EXPORTS
    mu = (ctypes.c_double * 3)()
    io = q.hf._Polarizability()
    assert ctypes.sizeof(io) == 8 + 8 + 72 + 24 + 8 + 16 + 16
    assert L.qc_scf_dipole(None, None, mu, None) == INV
    assert L.qc_scf_polarizability(None, ctypes.byref(io), None) == INV
    assert L.qc_scf_polarizability(None, None, None) == INV
    s = q.System(_h2())
    buf = np.zeros(3 * s.n * s.n)
    out = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.qc_dipole_matrices(None, None, out) == INV
    assert L.qc_dipole_matrices(s.handle, None, None) == INV
    assert L.qc_dipole_matrices_gpu(None, None, out) == INV and L.qc_dipole_matrices_gpu(s.handle, None, None) == INV
    s.close()
