"""GPU tests of the stability analysis (qc_scf_stability), the rotation along an eigenvector (qc_scf_rotated_density), the restart entry
points (qc_scf_begin_*_from) and the following driver (hf.stabilize, `--stability` / `--follow`).

The eigenvalues are checked against a dense Hessian built in numpy (tests/stability_reference.py) from the GPU state's own orbitals and
orbital energies and the stored ERI tensor (qc_eri_full) - another code path than the direct build and the Davidson iteration under test.
Tolerance: |lambda - lambda_ref| <= 2 tol with tol = 1e-7 the residual asked of the solver (Rayleigh-Ritz: |lambda - theta| <= |r|; the
factor 2 covers rounding in the f64 reference); vectors: |H_ref x - lambda x| <= 10 tol, orthonormal to 1e-10.

chloroform/6-31G** (n = 77, o = 29, v = 48) has dim = 1392 > 1024: every loop of the one-workgroup expand kernel (residual, preconditioner,
two Gram-Schmidt passes, normalisation) makes a second trip, and the dot-product and linear-combination kernels run more than one
workgroup's worth of a row past element 1024.  The largest dimension before it was 945 (benzene/6-31G).

Measured on an MI355X (2 roots, tol 1e-7; rounds / builds / max |lambda - lambda_ref| and its ratio to 2 tol / max |H_ref x - lambda x| over 10 tol):
  chloroform/6-31G** singlet   18 / 37 / 1.1e-14, 5e-8 / 0.043          chloroform/6-31G** triplet   22 / 40 / 2.3e-14, 1e-7 / 0.055"""
import json

import numpy as np
import pytest

from conftest import data, load_system
import stability_reference as R
import synthetic_systems as Y

pytestmark = pytest.mark.gpu

TOL = 1e-7
E_H2_R3_RHF = -0.981670914            # total RHF energy of H2/6-31G at R = 3.0 bohr (tests/golden/stability_golden.json)


def h2(R_bohr):
    import qchem_rs_amd as q
    b = q.BasisSet.load(data("basis", "6-31G.json"))
    return q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, float(R_bohr)])], b)


def _mol(name):
    if name.startswith("h2@"):
        return h2(float(name[3:]))
    mol, basis = name.split("/")
    if basis in Y.EDITED_BASES:
        return Y.load_system(name)
    return load_system(mol, basis)


def converged(name, uhf=False, na=0, nb=0, eps=1e-10, schwarz0=True, max_passes=1500):
    """(System, ScfStepper, electronic energy) converged to eps; the caller closes both."""
    import qchem_rs_amd as q
    s = q.System(_mol(name))
    if schwarz0:
        s.set_schwarz(0.0)
    st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
    for _ in range(max_passes):
        e, rms = st.iterate()
        if (rms / 2.0 if uhf else rms) < eps:
            return s, st, e
    raise AssertionError("%s did not converge" % name)


def dense_hessian(s, st, uhf, kind, nocc):
    I = s.eri()
    if uhf:
        return R.hessian_uhf(I, st.coefficients(0), st.orbital_energies(0), nocc[0], st.coefficients(1), st.orbital_energies(1), nocc[1])
    return R.hessian_rhf(I, st.coefficients(0), st.orbital_energies(0), nocc[0], kind)


CASES = [("h2@1.4", False, 0, 1, (1, 1)), ("h2@1.4", False, 1, 1, (1, 1)), ("h2@3.0", False, 0, 1, (1, 1)), ("h2@3.0", False, 1, 1, (1, 1)),
         ("water/cc-pVDZ", False, 0, 3, (5, 5)), ("water/cc-pVDZ", False, 1, 3, (5, 5)), ("ethylene/6-31G", False, 1, 1, (8, 8)),
         ("oxygen/cc-pVDZ", True, 0, 4, (9, 7)), ("benzene/6-31G", False, 0, 2, (21, 21)), ("benzene/6-31G", False, 1, 2, (21, 21)),
         ("chloroform/6-31G_st_st", False, 0, 2, (29, 29)), ("chloroform/6-31G_st_st", False, 1, 2, (29, 29))]


@pytest.mark.parametrize("name,uhf,kind,nroots,nocc", CASES, ids=["%s-k%d" % (c[0], c[2]) for c in CASES])
def test_eigenvalues_and_vectors_match_the_dense_hessian(name, uhf, kind, nroots, nocc):
    s, st, _ = converged(name, uhf, nocc[0] if uhf else 0, nocc[1] if uhf else 0)
    try:
        r = st.stability(kind=kind, nroots=nroots, tol=TOL, vectors=True)
        H = dense_hessian(s, st, uhf, kind, nocc)
        w = np.linalg.eigvalsh(H)
        X = r.vectors
        res = [float(np.linalg.norm(H @ X[k] - r.eigenvalues[k] * X[k])) for k in range(nroots)]
        orth = float(np.abs(X @ X.T - np.eye(nroots)).max())
        print(name, "kind", kind, "gpu", r.eigenvalues, "ref", w[:nroots], "iterations", r.iterations, "builds", r.builds, "residuals", r.residuals,
              "|H x - l x|", res, "orth", orth, "ms", r.ms_total, r.ms_builds, "max |l - l_ref|", float(np.abs(r.eigenvalues - w[:nroots]).max()))
        if name in Y.TILE_SYSTEMS:
            n, o, v = Y.TILE_SYSTEMS[name]
            assert (s.n, nocc[0], X.shape[1]) == (n, o, o * v)
        assert r.converged and X.shape == (nroots, st.stability_dim(kind)) == (nroots, H.shape[0])
        assert np.abs(r.eigenvalues - w[:nroots]).max() <= 2 * TOL
        assert np.all(np.diff(r.eigenvalues) >= 0) and np.all(r.residuals <= TOL)
        assert max(res) <= 10 * TOL and orth <= 1e-10
    finally:
        st.close(); s.close()


def test_signs_of_the_lowest_roots():
    got = {}
    for name, uhf, kind, nroots, nocc in (("h2@1.4", False, 1, 1, (1, 1)), ("h2@1.4", False, 0, 1, (1, 1)), ("h2@3.0", False, 1, 1, (1, 1)),
                                          ("ethylene/6-31G", False, 1, 1, (8, 8)), ("oxygen/cc-pVDZ", True, 0, 5, (9, 7))):
        s, st, _ = converged(name, uhf, nocc[0] if uhf else 0, nocc[1] if uhf else 0)
        got[(name, kind)] = st.stability(kind=kind, nroots=nroots, tol=TOL).eigenvalues
        st.close(); s.close()
    print(got)
    assert got[("h2@1.4", 1)][0] > 0 and got[("h2@1.4", 0)][0] > 0
    assert got[("h2@3.0", 1)][0] < 0 and got[("ethylene/6-31G", 1)][0] < 0 and got[("oxygen/cc-pVDZ", 0)][0] < 0
    assert int((got[("oxygen/cc-pVDZ", 0)] < -1e-5).sum()) == 3


@pytest.mark.parametrize("name,uhf,na,nb,passes", [("water/cc-pVTZ", False, 0, 0, 6), ("oxygen/cc-pVDZ", True, 9, 7, 12)])
def test_the_state_is_left_exactly_as_it_was(name, uhf, na, nb, passes):
    """Two identical states on fresh handles, `passes` passes each; stability (every kind) and a rotation on one of them; one more pass on
    both: energy, rms and density bit for bit equal."""
    import qchem_rs_amd as q
    out = []
    for touch in (False, True):
        s = q.System(_mol(name))
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        for _ in range(passes):
            st.iterate()
        if touch:
            for kind in ((0,) if uhf else (0, 1)):
                r = st.stability(kind=kind, nroots=2, tol=1e-5, vectors=True)
                st.rotated_density(r.vectors[0], 0.2, kind=kind)
            st.rotated_density(r.vectors[0], 0.0, kind=kind)
        e, rms = st.iterate()
        out.append((e, rms, [st.density(k) for k in range(2 if uhf else 1)]))
        st.close(); s.close()
    (e0, r0, D0), (e1, r1, D1) = out
    print(name, e0, e1, r0, r1)
    assert e0 == e1 and r0 == r1
    for a, b in zip(D0, D1):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,uhf,na,nb,kind,nroots", [("water/cc-pVDZ", False, 0, 0, 1, 3), ("oxygen/cc-pVDZ", True, 9, 7, 0, 4)])
def test_a_call_is_bitwise_reproducible(name, uhf, na, nb, kind, nroots):
    runs = []
    for handle in range(2):
        s, st, _ = converged(name, uhf, na, nb, eps=1e-8, schwarz0=False)
        for _ in range(2 - handle):
            r = st.stability(kind=kind, nroots=nroots, tol=TOL, vectors=True)
            runs.append((r.eigenvalues, r.vectors, r.iterations, r.builds))
        st.close(); s.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1]) and runs[0][2:] == other[2:]


def test_rotation_is_orthogonal_and_its_energy_is_the_determinants():
    s, st, e0 = converged("h2@3.0")
    try:
        S, H = st.matrix("S"), st.matrix("H")
        r = st.stability(kind=1, nroots=1, tol=TOL, vectors=True)
        lam, x = r.eigenvalues[0], r.vectors[0]
        for kind, xk in ((1, x), (0, st.stability(kind=0, nroots=1, tol=TOL, vectors=True).vectors[0])):
            Da, Db, e = st.rotated_density(xk, 0.3, kind=kind)
            for D in (Da, Db):
                assert np.abs(D @ S @ D - D).max() <= 1e-12 and abs(np.trace(D @ S) - 1.0) <= 1e-12
            assert (np.abs(Da - Db).max() > 1e-3) == (kind == 1)
            Ga, Gb = s.fock_uhf(Da, Db)
            e_np = 0.5 * (np.sum(Da * (2 * H + Ga)) + np.sum(Db * (2 * H + Gb)))
            print("kind", kind, "E(0.3)", e, "numpy", e_np)
            assert abs(e - e_np) <= 1e-11
        # second order: E(theta) - E(0) = c theta^2 lambda, c = 2 for an RHF vector
        assert R.ROTATION_C["rhf"] == 2.0
        for theta in (0.01, 0.02):
            _, _, e = st.rotated_density(x, theta, kind=1)
            ratio = (e - e0) / (R.ROTATION_C["rhf"] * theta ** 2 * lam)
            print("theta", theta, "dE", e - e0, "ratio", ratio)
            assert abs(ratio - 1.0) <= 0.05
        # the library's own choice of angle goes downhill
        _, _, e = st.rotated_density(x, 0.0, kind=1)
        assert e < e0 - 1e-6
    finally:
        st.close(); s.close()


def test_rotation_of_a_uhf_state_keeps_both_occupations():
    s, st, e0 = converged("oxygen/cc-pVDZ", True, 9, 7, eps=1e-8)
    try:
        S = st.matrix("S")
        r = st.stability(kind=0, nroots=1, tol=1e-6, vectors=True)
        Da, Db, e = st.rotated_density(r.vectors[0], 0.3)
        assert np.abs(Da @ S @ Da - Da).max() <= 1e-12 and np.abs(Db @ S @ Db - Db).max() <= 1e-12
        assert abs(np.trace(Da @ S) - 9.0) <= 1e-11 and abs(np.trace(Db @ S) - 7.0) <= 1e-11
        assert e < e0
    finally:
        st.close(); s.close()


def test_restart_entry_points_reproduce_a_converged_state():
    """A state begun from the densities of a state converged to 1e-11 gives that state's energy on its first pass, to 1e-10."""
    import ctypes
    import qchem_rs_amd as q
    for uhf in (True, False):
        s, st, e = converged("water/cc-pVDZ", uhf, eps=1e-11, schwarz0=False)
        Ds = [st.density(k) for k in range(2 if uhf else 1)]
        st.close()
        st2 = q.ScfStepper(s, uhf=uhf, density=tuple(Ds) if uhf else Ds[0])
        e2, rms2 = st2.iterate()
        print("uhf" if uhf else "rhf", e, e2, rms2)
        assert abs(e2 - e) <= 1e-10
        st2.close()
        out = ctypes.c_void_p()
        assert q.lib().qc_scf_begin_uhf_from(s.handle, 5, 5, None, None, ctypes.byref(out)) == q.hf.QC_ERR_INVALID
        assert q.lib().qc_scf_begin_rhf_from(s.handle, None, ctypes.byref(out)) == q.hf.QC_ERR_INVALID and not out
        s.close()


def test_argument_errors_on_a_live_state():
    import ctypes
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    s = q.System(h2(1.4))
    st = q.ScfStepper(s, uhf=True)
    io = q.hf._Stability(kind=0, nroots=1)
    assert L.qc_scf_stability(st._st, ctypes.byref(io), None) == INV                   # before the first pass
    st.iterate()
    assert L.qc_scf_stability(st._st, None, None) == INV
    for kind, nroots in ((1, 1), (-1, 1), (0, 0), (0, 9), (0, 7)):                      # kind 1 on a UHF state; ranges; nroots > dim = 6
        io = q.hf._Stability(kind=kind, nroots=nroots)
        assert L.qc_scf_stability(st._st, ctypes.byref(io), None) == INV, (kind, nroots)
    assert L.qc_scf_stability_dim(st._st, 0) == 6 and L.qc_scf_stability_dim(st._st, 1) == INV
    io = q.hf._Stability(kind=0, nroots=1, max_iterations=1, tol=1e-30)               # cannot be reached: outputs are filled all the same
    assert L.qc_scf_stability(st._st, ctypes.byref(io), None) == q.hf.QC_NOT_CONVERGED and io.builds > 0 and io.iterations == 1
    st.close()
    s.set_shard(0, 2)
    st = q.ScfStepper(s)
    st.iterate()
    io = q.hf._Stability(kind=0, nroots=1)
    assert L.qc_scf_stability(st._st, ctypes.byref(io), None) == q.hf.QC_ERR_UNSUPPORTED
    st.close(); s.close()


def test_following_h2_reaches_the_stable_uhf_determinant():
    import qchem_rs_amd as q
    res = q.stabilize(h2(3.0), q.HartreeFockConfig(500, 1e-9))
    print(res.history, res.output.total_energy(), res.spin_square)
    assert res is not None and res.stable and isinstance(res.output, q.UnrestrictedHartreeFockOutput)
    assert abs(res.history[0][0] + res.output.nuclear_repulsion - E_H2_R3_RHF) < 1e-6 and res.history[0][1] < -0.1
    assert res.output.total_energy() < E_H2_R3_RHF - 1e-6 and res.spin_square > 1e-3


def test_following_o2_goes_downhill_every_cycle():
    """O2 triplet/cc-pVDZ from the symmetric saddle: every cycle lowers the energy by more than 1e-6 and the end lies below the saddle.
    (Whether the end state is stable within 8 cycles, its energy and <S^2>: measured)"""
    import qchem_rs_amd as q
    res = q.stabilize(load_system("oxygen", "cc-pVDZ"), q.HartreeFockConfig(2000, 1e-8), 9, 7)
    assert res is not None
    print(res.history, res.stable, res.output.total_energy(), res.spin_square)
    e = [h[0] for h in res.history]
    assert len(e) >= 2 and res.history[0][1] < -1e-5
    assert all(b < a - 1e-6 for a, b in zip(e, e[1:])) and e[-1] < e[0] - 1e-6


def test_cli_reports_the_instability_and_is_unchanged_without_the_flags(tmp_path, capsys):
    from qchem_rs_amd import cli
    M = tmp_path / "h2_r3.json"
    M.write_text(json.dumps([{"element": "1", "position": [0.0, 0.0, 0.0]}, {"element": "1", "position": [0.0, 0.0, 3.0]}]))
    B = data("basis", "6-31G.json")
    assert cli.main(["rhf", "-b", B, "-m", str(M), "--epsilon", "1e-10"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert len(plain) == 5 and plain[1:4] == ["electronic energy: -1.315", "nuclear repulsion energy: 0.333", "hartree fock energy: -0.982"]
    assert cli.main(["rhf", "-b", B, "-m", str(M), "--epsilon", "1e-10", "--stability", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[1:5] == plain[1:5]                                     # (line 0 carries the wall time)
    assert lines[5].startswith("stability triplet: lowest eigenvalue -0.1422") and lines[6].startswith("stability singlet: lowest eigenvalue 0.4571")
    assert lines[7] == "wave function: unstable"
    doc = json.loads(lines[8])["stability"]
    assert doc["stable"] is False and abs(doc["eigenvalues"]["triplet"] + 0.14224799) < 1e-5 and abs(doc["eigenvalues"]["singlet"] - 0.45719193) < 1e-5
    assert cli.main(["rhf", "-b", B, "-m", str(M), "--epsilon", "1e-10", "--follow"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("cycle 0: electronic energy -1.31500") and lines[-1] == "wave function: stable"
