"""GPU tests of the static polarizability by coupled-perturbed HF (qc_scf_polarizability).

The state is converged to 1e-10 without Schwarz screening; the reference is dense: (A + B) built in numpy (tests/stability_reference.py)
from the stored ERI tensor (qc_eri_full) and the state's own C and orbital energies, the right-hand sides from the dipole matrices of the
numpy reference (tests/dipole_reference.py), numpy.linalg.solve, and the factors 4 (RHF) and 2 (UHF).

Bound, with tol = 1e-7 the residual asked of the solver: alpha_pq - alpha_ref,pq = c r^p . H^-1 rho^q with rho^q the residual, so
  |alpha_pq - alpha_ref,pq| <= c |r^p| tol / lambda_min(H_ref) + 1e-9 max|alpha_ref|
(the second term: rounding of the f64 reference and of the fixed-point Fock builds).  lambda_min > 0 is asserted first.

Measured on an MI355X (max |alpha - alpha_ref| / smallest bound / lambda_min / rounds / builds):
  h2@1.4 6-31G RHF           4.4e-15  6.5e-9   0.632   2   2     water/cc-pVDZ RHF          2.7e-15  1.0e-6   0.429   9  26
  water/cc-pVDZ UHF (5, 5)   4.9e-15  8.3e-7   0.376  10  27     benzene/6-31G RHF          6.1e-11  8.5e-5   0.0099 17  43
  oxygen/cc-pVDZ (9, 7) min  2.5e-14  1.6e-5   0.0229 13  33     UHF against RHF water      1.0e-10
  water/STO-3G RHF (dim 10)  2.2e-15  1.2e-8   0.736   4   9
  h_atom/6-311++G** (1, 0)   2.2e-16  3.4e-7   0.381   1   3   (begun from its self-consistent density, see begun_converged)
  chloroform/6-31G** RHF     1.1e-13  5.9e-6   0.187  14  39     the same to 1e-9           1.1e-13  9.7e-8   0.187  16  46
chloroform/6-31G** has dim = 29 x 48 = 1392 > 1024, the length of one trip of the expand kernel's loops (error / bound: 1.9e-8 at tol 1e-7,
1.2e-6 at 1e-9; |H U - r| / (10 tol): 0.033 and 0.084)."""
import ctypes

import numpy as np
import pytest

from conftest import load_system
import dipole_reference as D
import synthetic_systems as Y
from test_stability_gpu import _mol, converged, h2

pytestmark = pytest.mark.gpu

TOL = 1e-7


def reference(s, st, m, uhf, nocc):
    """(alpha_ref, H_ref, r, c) of a converged state"""
    I = s.eri()
    _, M = D.overlap_and_dipole(m)
    if uhf:
        a, H, r = D.polarizability_uhf(I, st.coefficients(0), st.orbital_energies(0), nocc[0], st.coefficients(1), st.orbital_energies(1), nocc[1], M)
        return a, H, r, 2.0
    a, H, r = D.polarizability_rhf(I, st.coefficients(0), st.orbital_energies(0), nocc[0], M)
    return a, H, r, 4.0


def bound(H, r, c, alpha_ref, tol=TOL):
    lam = float(np.linalg.eigvalsh(H)[0])
    assert lam > 0, "the case is unsuitable: (A + B) is not positive definite (lambda_min %g)" % lam
    rn = np.linalg.norm(r, axis=1)
    return c * rn[:, None] * tol / lam + 1e-9 * float(np.abs(alpha_ref).max()), lam


def check(name, s, st, m, uhf, nocc, tol=TOL, ref=None):
    """ref: the value of reference() of a call before, for a second solve on the same state"""
    p = st.polarizability(tol=tol, response=True)
    a_ref, H, r, c = ref or reference(s, st, m, uhf, nocc)
    B, lam = bound(H, r, c, a_ref, tol)
    err = np.abs(p.alpha - a_ref)
    resid = [float(np.linalg.norm(H @ p.response[q] - r[q])) for q in range(3)]
    print(name, "uhf" if uhf else "rhf", "alpha", p.alpha.tolist(), "ref", a_ref.tolist(), "max err", float(err.max()), "bound", B.tolist(), "lambda_min", lam,
          "residuals", p.residuals, "|H U - r|", resid, "asymmetry", p.asymmetry, "iterations", p.iterations, "builds", p.builds, "ms", p.ms_total, p.ms_builds)
    assert p.converged and np.all(p.residuals <= tol)
    assert np.all(err <= B)
    assert p.asymmetry <= float(B.max())
    assert np.array_equal(p.alpha, p.alpha.T) and abs(p.isotropic - np.trace(p.alpha) / 3.0) <= 1e-15 * abs(p.isotropic)
    assert p.response.shape == (3, H.shape[0]) and max(resid) <= 10 * tol
    return p, a_ref, B


def test_h2_has_two_exactly_zero_right_hand_sides():
    s, st, _ = converged("h2@1.4")
    try:
        assert st.stability_dim(0) == 3
        p, a_ref, _ = check("h2@1.4", s, st, h2(1.4), False, (1, 1))
        assert p.alpha[0, 0] == 0.0 and p.alpha[1, 1] == 0.0 and np.count_nonzero(p.alpha) == 1 and p.alpha[2, 2] > 1.0
        assert 1 <= p.builds <= 2 and np.all(np.isfinite(p.alpha)) and np.all(np.isfinite(p.response))
        assert np.all(p.response[:2] == 0.0) and p.residuals[0] == 0.0 and p.residuals[1] == 0.0
    finally:
        st.close(); s.close()


def test_water_rhf_and_the_same_state_as_uhf():
    out = {}
    for uhf in (False, True):
        s, st, _ = converged("water/cc-pVDZ", uhf, 5 if uhf else 0, 5 if uhf else 0)
        try:
            out[uhf] = check("water/cc-pVDZ", s, st, load_system("water", "cc-pVDZ"), uhf, (5, 5))
        finally:
            st.close(); s.close()
    (pr, _, Br), (pu, _, Bu) = out[False], out[True]
    print("uhf - rhf", np.abs(pu.alpha - pr.alpha).max())
    assert np.all(np.abs(pu.alpha - pr.alpha) <= Br + Bu)             # the UHF vector (r, r) of a closed-shell state: the RHF tensor


def test_a_space_that_fits_the_subspace_is_never_collapsed():
    """water/STO-3G, dim = 5 x 2 = 10 <= 40: the basis grows until it spans the space at the latest - never more builds than dimensions."""
    s, st, _ = converged("water/STO-3G")
    try:
        assert st.stability_dim(0) == 10
        p, _, _ = check("water/STO-3G", s, st, load_system("water", "STO-3G"), False, (5, 5))
        assert p.builds <= 10
    finally:
        st.close(); s.close()


def begun_converged(m, na, nb, Da, Db):
    """(System, ScfStepper) of a UHF state begun from densities that are already self-consistent: its first pass must report a density
    change below 1e-10.  For states with an empty beta block, which the plain loop cannot reach: from its second pass on the DIIS
    system of a spin without electrons is singular ("DIIS failed", as in the reference); the first pass (window shorter than the
    minimum length) does not extrapolate."""
    import qchem_rs_amd as q
    s = q.System(m)
    s.set_schwarz(0.0)
    st = q.ScfStepper(s, uhf=True, n_alpha=na, n_beta=nb, density=(Da, Db))
    _, rms = st.iterate()
    print("first pass from the self-consistent density: rms", rms)
    assert rms / 2.0 < 1e-10
    return s, st


def test_hydrogen_atom_with_an_empty_beta_block():
    """One electron: (J - K)[D_alpha] annihilates the occupied orbital, so the lowest eigenvector c of the core Hamiltonian is the
    self-consistent UHF orbital and D_alpha = c c^T, D_beta = 0 (numpy, from the library's own S, T, V)."""
    import scipy.linalg as sl
    import qchem_rs_amd as q
    m = load_system("h_atom", "6-311++G_st_st")
    h = q.System(m)
    _, Cm = sl.eigh(h.kinetic() + h.nuclear(), h.overlap())
    h.close()
    Da = np.outer(Cm[:, 0], Cm[:, 0])
    s, st = begun_converged(m, 1, 0, Da, np.zeros_like(Da))
    try:
        assert st.stability_dim(0) == s.n - 1
        check("h_atom/6-311++G**", s, st, m, True, (1, 0))
    finally:
        st.close(); s.close()


def test_a_state_without_any_occupied_virtual_pair():
    """H2/STO-3G with both electrons in the alpha orbitals: every alpha orbital occupied (D_alpha = S^-1), no beta electron, dim = 0."""
    import qchem_rs_amd as q
    from conftest import data
    b = q.BasisSet.load(data("basis", "STO-3G.json"))
    m = q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, 1.4])], b)
    h = q.System(m)
    Da = np.linalg.inv(h.overlap())
    h.close()
    s, st = begun_converged(m, 2, 0, Da, np.zeros_like(Da))
    try:
        assert st.stability_dim(0) == 0
        p = st.polarizability(response=True)
        assert p.converged and p.builds == 0 and p.iterations == 0 and not p.alpha.any() and p.response.shape == (3, 0)
        assert np.linalg.norm(st.dipole(np.array([0.0, 0.0, 0.7]))) <= 1e-10
    finally:
        st.close(); s.close()


def test_benzene_needs_more_vectors_than_the_subspace_holds_at_once():
    s, st, _ = converged("benzene/6-31G")
    try:
        assert st.stability_dim(0) == 21 * 45 > 40
        p, _, _ = check("benzene/6-31G", s, st, load_system("benzene", "6-31G"), False, (21, 21))
        assert p.builds > 40                                             # (more vectors than the subspace holds: the collapse has run)
    finally:
        st.close(); s.close()


def test_chloroform_has_vectors_longer_than_one_stride_of_the_expand_kernel():
    """dim = 29 x 48 = 1392 > 1024: the second trip of every loop of the one-workgroup expand kernel, with three right-hand sides.  At tol 1e-7
    the solver is done after 13 rounds and 39 builds, one vector short of a full subspace, so the collapse does not run; the same state solved to
    1e-9 (the same bound with that tol) needs more than 40 builds, and the collapse runs on vectors of 1392."""
    name = "chloroform/6-31G_st_st"
    s, st, _ = converged(name)
    try:
        assert (s.n, st.stability_dim(0)) == (77, 1392) and Y.TILE_SYSTEMS[name] == (77, 29, 48)
        m = _mol(name)
        ref = reference(s, st, m, False, (29, 29))
        check(name, s, st, m, False, (29, 29), ref=ref)
        p, _, _ = check(name + " to 1e-9", s, st, m, False, (29, 29), tol=1e-9, ref=ref)
        assert p.builds > 40                                             # (more vectors than the subspace holds: the collapse has run)
    finally:
        st.close(); s.close()


def test_oxygen_triplet_at_its_minimum():
    import qchem_rs_amd as q
    m = load_system("oxygen", "cc-pVDZ")
    s = q.System(m)
    s.set_schwarz(0.0)
    res = q.stabilize(s, q.HartreeFockConfig(2000, 1e-10), 9, 7)
    assert res is not None and res.stable and res.history[-1][1] > 0.0
    st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7, density=res.density)
    try:
        for _ in range(2000):
            _, rms = st.iterate()
            if rms / 2.0 < 1e-10:
                break
        else:
            raise AssertionError("oxygen did not converge again from its own density")
        check("oxygen/cc-pVDZ (9, 7), followed to the minimum", s, st, m, True, (9, 7))
    finally:
        st.close(); s.close()


@pytest.mark.parametrize("name,uhf,na,nb", [("water/cc-pVDZ", False, 0, 0), ("oxygen/cc-pVDZ", True, 9, 7)])
def test_a_call_is_bitwise_reproducible(name, uhf, na, nb):
    runs = []
    for handle in range(2):
        s, st, _ = converged(name, uhf, na, nb, eps=1e-8, schwarz0=False)
        for _ in range(2 - handle):
            p = st.polarizability(tol=TOL, response=True)
            runs.append((p.alpha, p.response, p.residuals, p.iterations, p.builds))
        st.close(); s.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1]) and np.array_equal(runs[0][2], other[2])
        assert runs[0][3:] == other[3:]


@pytest.mark.parametrize("name,uhf,na,nb,passes", [("water/cc-pVTZ", False, 0, 0, 6), ("oxygen/cc-pVDZ", True, 9, 7, 12)])
def test_the_state_is_left_exactly_as_it_was(name, uhf, na, nb, passes):
    """Two identical states on fresh handles; dipole and polarizability on one of them; one more pass on both: energy, rms and density bit
    for bit equal.  The stability eigenvalues before and after the two calls are identical too."""
    import qchem_rs_amd as q
    out = []
    for touch in (False, True):
        s = q.System(_mol(name))
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        for _ in range(passes):
            st.iterate()
        if touch:
            before = st.stability(kind=0, nroots=2, tol=1e-5)
            st.dipole()
            st.polarizability(tol=1e-5)
            after = st.stability(kind=0, nroots=2, tol=1e-5)
            assert np.array_equal(before.eigenvalues, after.eigenvalues) and before.builds == after.builds
        e, rms = st.iterate()
        out.append((e, rms, [st.density(k) for k in range(2 if uhf else 1)]))
        st.close(); s.close()
    (e0, r0, D0), (e1, r1, D1) = out
    print(name, e0, e1, r0, r1)
    assert e0 == e1 and r0 == r1
    for a, b in zip(D0, D1):
        assert np.array_equal(a, b)


def test_argument_errors_on_a_live_state():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    s = q.System(h2(1.4))
    st = q.ScfStepper(s)
    io = q.hf._Polarizability()
    assert L.qc_scf_polarizability(st._st, ctypes.byref(io), None) == INV                 # before the first pass
    st.iterate()
    assert L.qc_scf_polarizability(st._st, None, None) == INV
    for kw in (dict(tol=-1.0), dict(tol=float("nan")), dict(max_iterations=-1)):
        io = q.hf._Polarizability(**kw)
        assert L.qc_scf_polarizability(st._st, ctypes.byref(io), None) == INV, kw
    io = q.hf._Polarizability(max_iterations=1, tol=1e-30)                                # cannot be reached: outputs are filled all the same
    assert L.qc_scf_polarizability(st._st, ctypes.byref(io), None) == q.hf.QC_NOT_CONVERGED and io.builds == 1 and io.iterations == 1
    assert io.alpha[8] > 1.0 and io.alpha[0] == 0.0
    st.close()
    s.set_shard(0, 2)
    st = q.ScfStepper(s)
    st.iterate()
    io = q.hf._Polarizability()
    assert L.qc_scf_polarizability(st._st, ctypes.byref(io), None) == q.hf.QC_ERR_UNSUPPORTED
    st.close(); s.close()
