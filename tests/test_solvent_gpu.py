"""GPU tests of the conductor-like continuum: the device SPD inverse (qc_chol.hip), the cavity matrix and K, the response
at a fixed density, the solvated SCF (RHF and UHF, the one-workgroup path and the generic one, one-shot and stepped), reproducibility bit
for bit, the calls a solvated state refuses, properties of the solvated density, and the command line.  The reference is
tests/solvent_reference.py (numpy, scipy's erf, the oracle's integrals, the host entry qc_potential_matrix).

Bounds.  Inverse: max |A Ainv - I| <= 8 n u cond_2(A), u = 2^-53 (numpy's own inverse meets a tenth of it: test_solvent_host.py).
S: 1e-13 relative per element (device erf against scipy's: a few ulp).  K: max |S K + f I| <= 8 M u cond_2(S).  Response: q within
1e-9 max |q_ref| (cond_2(S) < 2000 times the 1e-12 of the potentials, rounded up), V_R within 1e-9 (1 + max |V_ref|), the two energies
within 1e-9 Eh, the central difference of G_pol against tr(Delta V_R) within 1e-9 (G_pol is exactly quadratic in D).  SCF at
epsilon = 1e-10, dielectric constant 78.39: total energy and both halves of G_pol within 1e-8 (the bar of smoke()), q within
1e-7 max |q_ref|."""
import ctypes
import json

import numpy as np
import pytest

from conftest import data, load_system
import solvent_reference as SR
import synthetic_systems as Y

pytestmark = pytest.mark.gpu

EPS = 78.39
CONV = 1e-10
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def handle():
    import qchem_rs_amd as q
    return cached("handle", lambda: q.System(load_system("water", "STO-3G")))


# ---------------------------------------------------------------------------------------------------------------- the SPD inverse

@pytest.mark.parametrize("n", SR.INVERSE_SIZES)
def test_spd_inverse_meets_the_bar_is_symmetric_and_repeats_bit_for_bit(n):
    s = handle()
    for k in SR.INVERSE_DECADES:
        A = SR.spd_matrix(n, k)
        w = np.linalg.eigvalsh(A)
        Ainv = s.spd_inverse(A)
        err = float(np.abs(A @ Ainv - np.eye(n)).max())
        print("n", n, "k", k, "max |A Ainv - I|", err, "bar", SR.inverse_bar(n, w[-1] / w[0]))
        assert np.all(np.isfinite(Ainv)) and err <= SR.inverse_bar(n, w[-1] / w[0])
        assert np.array_equal(Ainv, Ainv.T)
        assert np.array_equal(Ainv, s.spd_inverse(A))


def test_spd_inverse_refuses_indefinite_and_nan_matrices():
    import qchem_rs_amd as q
    s = handle()
    fn = q.lib().qc_spd_inverse
    for n in (3, 70, 130):
        A = SR.spd_matrix(n, 1)
        w, U = np.linalg.eigh(A)
        w[n // 2] = -0.5
        B = (U * w) @ U.T
        B = 0.5 * (B + B.T)
        out = np.zeros((n, n))
        assert fn(s.handle, n, B.ctypes.data, out.ctypes.data) == q.hf.QC_ERR_INVALID
        Cn = A.copy()
        Cn[n - 1, 0] = Cn[0, n - 1] = float("nan")
        assert fn(s.handle, n, Cn.ctypes.data, out.ctypes.data) == q.hf.QC_ERR_INVALID
        Z = np.zeros((n, n))
        assert fn(s.handle, n, Z.ctypes.data, out.ctypes.data) == q.hf.QC_ERR_INVALID
        assert np.array_equal(s.spd_inverse(A), s.spd_inverse(A))            # the handle works on afterwards


# ---------------------------------------------------------------------------------------------------------------- S and K

@pytest.mark.parametrize("mol,density", [("water", 1.0), ("water", 2.0), ("water", 5.0), ("chloroform", 5.0)])
def test_cavity_matrix_and_its_inverse(mol, density):
    import qchem_rs_amd as q
    m = load_system(mol, "STO-3G")
    s = q.System(m)
    s.set_solvent(EPS, density=density)
    P, a, _ = SR.surface(m.atomic_numbers(), m.coordinates(), 1.2, density)
    Sr = SR.s_matrix(P, a)
    M = len(a)
    assert s.solvent_points() == M == {("water", 1.0): 43, ("water", 2.0): 85, ("water", 5.0): 216, ("chloroform", 5.0): 537}[(mol, density)]
    Sg, K = s.solvent_matrix(inverse=True)
    rel = float((np.abs(Sg - Sr) / np.abs(Sr)).max())
    w = np.linalg.eigvalsh(Sr)
    f = SR.factor(EPS)
    res = float(np.abs(Sr @ K + f * np.eye(M)).max())
    print(mol, density, "M", M, "max relative |dS|", rel, "max |S K + f I|", res, "bar", SR.inverse_bar(M, w[-1] / w[0]), "set-up ms", s.solvent_timings()[0])
    assert rel <= 1e-13 and np.array_equal(Sg, Sg.T)
    assert res <= SR.inverse_bar(M, w[-1] / w[0]) and np.array_equal(K, K.T)
    S2, K2 = s.solvent_matrix(inverse=True)
    assert np.array_equal(Sg, S2) and np.array_equal(K, K2)
    h = q.System(m)                                                          # a fresh handle gives the same bits
    h.set_solvent(EPS, density=density)
    S3, K3 = h.solvent_matrix(inverse=True)
    assert np.array_equal(Sg, S3) and np.array_equal(K, K3)
    h.close(); s.close()


# ---------------------------------------------------------------------------------------------------------------- the response

def vacuum_density(s):
    import qchem_rs_amd as q
    st = q.ScfStepper(s)
    try:
        for _ in range(100):
            _, rms = st.iterate()
            if rms < CONV:
                return st.density(0)
    finally:
        st.close()
    raise AssertionError("the vacuum SCF did not converge")


def response_case(basis):
    """water in `basis`, cavity at 1 point per Angstrom^2 (M = 43): handle, reference K, v_nuc, A - computed once"""
    def make():
        import qchem_rs_amd as q
        m = load_system("water", basis)
        s = q.System(m)
        s.set_solvent(EPS, density=1.0)
        P, a, _ = SR.surface(m.atomic_numbers(), m.coordinates(), 1.2, 1.0)
        K = SR.k_matrix(SR.s_matrix(P, a), EPS)
        return dict(m=m, s=s, K=K, vn=SR.v_nuc(m.atomic_numbers(), m.coordinates(), P), A=SR.potential_tensor(s, P))
    return cached(("response", basis), make)


@pytest.mark.parametrize("basis", ["STO-3G", "6-31G_st_st", "cc-pVTZ"])
def test_response_at_a_random_and_at_the_vacuum_density(basis):
    c = response_case(basis)
    s, n = c["s"], c["s"].n
    if basis == "cc-pVTZ":
        assert int(c["m"].shell_L.max()) == 3                                # f functions
    s.set_solvent(None)
    Dv = vacuum_density(s)
    s.set_solvent(EPS, density=1.0)
    for name, D in (("random", Y.rand_sym(n, 7)), ("vacuum", Dv)):
        q, V, (en, ee) = s.solvent_response(D)
        qr, Vr, enr, eer = SR.response(c["K"], c["vn"], c["A"], D)
        dq, dV = float(np.abs(q - qr).max()), float(np.abs(V - Vr).max())
        print(basis, name, "max |dq|", dq, "of max |q|", float(np.abs(qr).max()), "max |dV_R|", dV, "of", float(np.abs(Vr).max()), "dE", en - enr, ee - eer)
        assert dq <= 1e-9 * np.abs(qr).max() and dV <= 1e-9 * (1.0 + np.abs(Vr).max()) and np.array_equal(V, V.T)
        assert abs(en - enr) <= 1e-9 and abs(ee - eer) <= 1e-9
        # dG_pol/dD = V_R: G_pol is exactly quadratic in D, so the central difference has no truncation error
        Delta, h = Y.rand_sym(n, 8, scale=0.01), 1.0
        gp = sum(s.solvent_response(D + h * Delta)[2])
        gm = sum(s.solvent_response(D - h * Delta)[2])
        fd, an = (gp - gm) / (2.0 * h), float(np.sum(Delta * V))
        print(basis, name, "central difference", fd, "tr(Delta V_R)", an, "difference", fd - an)
        assert abs(fd - an) <= 1e-9
        q2, V2, e2 = s.solvent_response(D)                                   # bit for bit, on this handle and on a fresh one
        assert np.array_equal(q, q2) and np.array_equal(V, V2) and e2 == (en, ee)
        import qchem_rs_amd as qq
        h = qq.System(c["m"])
        h.set_solvent(EPS, density=1.0)
        q3, V3, e3 = h.solvent_response(D)
        h.close()
        assert np.array_equal(q, q3) and np.array_equal(V, V3) and e3 == (en, ee)
    ms = s.solvent_timings()
    assert ms.shape == (4,) and np.all(ms >= 0.0) and ms[0] > 0.0


# ---------------------------------------------------------------------------------------------------------------- the SCF

def reference_scf(mol, basis, density, nocc, x=0.0, solvated=True):
    def make():
        import qchem_rs_amd as q
        from oracle.oracle import Oracle
        m = load_system(mol, basis)
        o = Oracle(m)
        S, H, I = o.overlap(), o.kinetic() + o.nuclear(), o.eri()
        if not solvated:
            r = SR.scf(S, H, I, nocc)
        else:
            s = q.System(m)
            P, a, _ = SR.surface(m.atomic_numbers(), m.coordinates(), 1.2, density)
            K = SR.k_matrix(SR.s_matrix(P, a), EPS, x)
            r = SR.scf(S, H, I, nocc, K, SR.v_nuc(m.atomic_numbers(), m.coordinates(), P), SR.potential_tensor(s, P))
            s.close()
        r["total"] = r["electronic"] + o.nuclear_repulsion() + r["e_nuc"]
        return r
    return cached(("ref", mol, basis, density, nocc, x, solvated), make)


def stepped(s, uhf=False, n_alpha=0, n_beta=0, density=None, max_passes=200, same_rule=False):
    """the stepped API to CONV: per-pass energies, the final SolventOutput (None in vacuum), orbital energies, densities.  The stopping rule
    is the drivers' (rms < epsilon for RHF, rms / 2 < epsilon for UHF: uhf.rs:139); same_rule: rms < epsilon for UHF too, so that a UHF run
    is converged as far as the RHF run it is compared with (a pass's energy is first order in its last density change)"""
    import qchem_rs_amd as q
    st = q.ScfStepper(s, uhf=uhf, n_alpha=n_alpha, n_beta=n_beta, density=density)
    try:
        es = []
        for _ in range(max_passes):
            e, rms = st.iterate()
            es.append(e)
            if (rms / 2.0 if uhf and not same_rule else rms) < CONV:
                sv = st.solvent(charges=True)
                return dict(es=np.array(es), sv=sv, w=[st.orbital_energies(k) for k in range(2 if uhf else 1)],
                            D=[st.density(k) for k in range(2 if uhf else 1)], total=e + s.nuclear_repulsion() + (sv.nuclear if sv else 0.0))
    finally:
        st.close()
    raise AssertionError("the SCF did not converge")


SCF_CASES = {
    "water/STO-3G rhf": ("water", "STO-3G", 5.0, 5, 0.0),
    "water/6-31G** rhf": ("water", "6-31G_st_st", 2.0, 5, 0.0),
    "ethylene/6-311++G** rhf": ("ethylene", "6-311++G_st_st", 1.0, 8, 0.0),
    "water+/6-31G** uhf": ("water", "6-31G_st_st", 2.0, (5, 4), 0.0),
    "water/STO-3G rhf cosmo": ("water", "STO-3G", 1.0, 5, 0.5),
}


@pytest.mark.parametrize("name", list(SCF_CASES))
def test_converged_scf_matches_the_reference_loop(name):
    import qchem_rs_amd as q
    mol, basis, density, nocc, x = SCF_CASES[name]
    ref = reference_scf(mol, basis, density, nocc, x)
    s = q.System(load_system(mol, basis))
    s.set_solvent(EPS, density=density, x=x)
    uhf = not np.isscalar(nocc)
    if name.startswith("ethylene"):
        assert s.n == 72 and s.solvent_points() == 84                       # above QC_SMALL_MAXN: the generic launch sequence
    else:
        assert s.n <= 64
    r = stepped(s, uhf=uhf, n_alpha=nocc[0] if uhf else 0, n_beta=nocc[1] if uhf else 0)
    sv = r["sv"]
    dq = float(np.abs(sv.charges - ref["q"]).max())
    print(name, "passes", len(r["es"]), "dE_total", r["total"] - ref["total"], "d(1/2 q.v_nuc)", sv.nuclear - ref["e_nuc"], "d(1/2 q.v_elec)", sv.electronic - ref["e_elec"],
          "max |dq|", dq, "of", float(np.abs(ref["q"]).max()), "sum q", sv.total_charge, "G_pol", sv.polarization_energy())
    assert abs(r["total"] - ref["total"]) <= 1e-8
    assert abs(sv.nuclear - ref["e_nuc"]) <= 1e-8 and abs(sv.electronic - ref["e_elec"]) <= 1e-8
    assert dq <= 1e-7 * np.abs(ref["q"]).max() and sv.npoints == len(ref["q"])
    assert abs(sv.total_charge - float(np.sum(sv.charges))) <= 1e-12
    # the one-shot driver and the stepped API agree bit for bit; so do a second run and a fresh handle
    cfg = q.HartreeFockConfig(200, CONV, *(nocc if uhf else (0, 0)))
    one = (q.unrestricted_hartree_fock if uhf else q.restricted_hartree_fock)(s, cfg)
    assert one is not None and one.electronic_energy == r["es"][-1] and one.iterations == len(r["es"]) - 1
    assert one.solvent_nuclear_energy == sv.nuclear and one.total_energy() == r["total"]
    last = s.solvent_last()
    assert (last.nuclear, last.electronic, last.total_charge, last.npoints) == (sv.nuclear, sv.electronic, sv.total_charge, sv.npoints)
    assert np.array_equal(np.asarray(one.orbital_energies_alpha if uhf else one.orbital_energies), r["w"][0])
    h = q.System(load_system(mol, basis))
    h.set_solvent(EPS, density=density, x=x)
    r2 = stepped(h, uhf=uhf, n_alpha=nocc[0] if uhf else 0, n_beta=nocc[1] if uhf else 0)
    assert np.array_equal(r["es"], r2["es"]) and np.array_equal(sv.charges, r2["sv"].charges) and all(np.array_equal(a, b) for a, b in zip(r["w"], r2["w"]))
    assert all(np.array_equal(a, b) for a, b in zip(r["D"], r2["D"]))
    h.close(); s.close()


def test_uhf_of_a_closed_shell_equals_rhf_and_a_run_from_a_density_ends_in_the_same_state():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "6-31G_st_st"))
    s.set_solvent(EPS, density=2.0)
    r = stepped(s)
    u = stepped(s, uhf=True, n_alpha=5, n_beta=5, same_rule=True)
    print("UHF(5,5) - RHF: dE", u["total"] - r["total"], "dG_pol", u["sv"].polarization_energy() - r["sv"].polarization_energy())
    assert abs(u["total"] - r["total"]) <= 1e-9 and abs(u["sv"].polarization_energy() - r["sv"].polarization_energy()) <= 1e-9
    assert np.abs(u["sv"].charges - r["sv"].charges).max() <= 1e-9
    f = stepped(s, density=r["D"][0])                                        # qc_scf_begin_rhf_from at the converged density: stays there
    assert abs(f["total"] - r["total"]) <= 1e-9 and len(f["es"]) <= 3
    fu = stepped(s, uhf=True, n_alpha=5, n_beta=5, density=(u["D"][0], u["D"][1]), same_rule=True)
    assert abs(fu["total"] - r["total"]) <= 1e-9
    s.close()


def test_variational_order_and_removal_of_the_solvent():
    import qchem_rs_amd as q
    m = load_system("water", "6-31G_st_st")
    s = q.System(m)
    s.set_solvent(EPS, density=2.0)
    solv = stepped(s)
    s.set_solvent(None)
    vac = stepped(s)
    assert vac["sv"] is None
    s.set_solvent(EPS, density=2.0)
    g_vac = sum(s.solvent_response(vac["D"][0])[2])                           # G_pol at the vacuum density
    print("E_vac", vac["total"], "G_pol(D_vac)", g_vac, "E_solvated", solv["total"], "G_pol", solv["sv"].polarization_energy())
    assert vac["total"] + g_vac >= solv["total"] - 1e-9
    assert solv["sv"].polarization_energy() < 1e-9 and g_vac < 1e-9 and solv["total"] < vac["total"]
    # after the removal a run is the vacuum run of a fresh handle, bit for bit
    s.set_solvent(None)
    again = stepped(s)
    h = q.System(m)
    fresh = stepped(h)
    assert np.array_equal(again["es"], fresh["es"]) and np.array_equal(again["w"][0], fresh["w"][0]) and np.array_equal(vac["es"], fresh["es"])
    h.close(); s.close()


def test_solvated_states_refuse_what_lacks_the_solvent_terms_and_keep_their_cavity():
    import qchem_rs_amd as q
    UNS = q.hf.QC_ERR_UNSUPPORTED
    L = q.lib()
    s = q.System(load_system("water", "STO-3G"))
    s.set_solvent(EPS, density=1.0)
    for uhf in (False, True):
        st = q.ScfStepper(s, uhf=uhf, n_alpha=5 if uhf else 0, n_beta=5 if uhf else 0)
        e0 = st.solvent()
        assert e0 is not None and e0.npoints == 43                           # the reaction field of the guess
        st.iterate(); st.iterate()
        n = s.n
        buf = np.zeros(max(3 * n * n, 4096))
        b = buf.ctypes.data
        assert L.qc_scf_gradient(st._st, buf[:9].copy()) == UNS
        stab = q.hf._Stability(); stab.kind = 0; stab.nroots = 1
        assert L.qc_scf_stability(st._st, ctypes.byref(stab), None) == UNS
        assert L.qc_scf_rotated_density(st._st, 0, b, 0.1, b, b, None) == UNS
        pol = q.hf._Polarizability()
        assert L.qc_scf_polarizability(st._st, ctypes.byref(pol), None) == UNS
        exc = q.hf._Excitations(); exc.nroots = 1
        assert L.qc_scf_excitations(st._st, ctypes.byref(exc), None) == UNS
        assert L.qc_scf_excitation_matrices(st._st, 0, b, b) == UNS
        # the state keeps its cavity when the handle's changes, and the vacuum H is what qc_scf_matrix reports
        s.set_solvent(None)
        e1, _ = st.iterate()
        assert st.solvent().npoints == 43
        assert np.abs(st.matrix("H") - (s.kinetic() + s.nuclear())).max() <= 1e-12
        mp2 = st.mp2()                                                       # correlation on the solvated orbitals: runs
        assert mp2.e_corr < 0.0
        s.set_solvent(EPS, density=1.0)
        st.close()
    s.close()


def test_properties_of_a_solvated_state_are_those_of_its_density():
    import qchem_rs_amd as q
    m = load_system("water", "6-31G_st_st")
    s = q.System(m)
    s.set_solvent(EPS, density=2.0)
    st = q.ScfStepper(s)
    for _ in range(200):
        _, rms = st.iterate()
        if rms < CONV:
            break
    D = st.density(0)
    P = np.array([[0.0, 0.0, 3.0], [1.5, -2.0, 0.5], [-2.5, 1.0, -1.0]])
    mu = st.dipole()
    # (a handle has no dipole call of its own: its entry points are the dipole matrices, here by the kernel qc_scf_dipole itself uses)
    Mk = s.dipole_matrices(gpu=True)
    mu_ref = np.array([sum(a.ordinal * a.position[k] for a in m.atoms) - np.sum(D * Mk[k]) for k in range(3)])
    v_state, v_handle = st.esp_on_points(P), s.esp_on_points(D, P)
    print("dipole", mu, "max |d mu|", np.abs(mu - mu_ref).max(), "max |dV|", np.abs(v_state - v_handle).max())
    assert np.abs(mu - mu_ref).max() <= 1e-10 and np.array_equal(v_state, v_handle)
    # the solvated dipole is larger than the vacuum one (the continuum polarises the molecule)
    st.close()
    s.set_solvent(None)
    sv = q.ScfStepper(s)
    for _ in range(200):
        _, rms = sv.iterate()
        if rms < CONV:
            break
    assert np.linalg.norm(mu) > np.linalg.norm(sv.dipole())
    sv.close(); s.close()


def test_command_line_numbers_are_the_api_numbers(capsys):
    import qchem_rs_amd as q
    from qchem_rs_amd import cli
    B, Mf = data("basis", "STO-3G.json"), data("mol", "water.json")
    s = q.System(load_system("water", "STO-3G"))
    s.set_solvent(EPS, model="cosmo", density=2.0)
    for sub, run in (("rhf", q.restricted_hartree_fock), ("uhf", q.unrestricted_hartree_fock)):
        out = run(s, q.HartreeFockConfig(100, 1e-8))
        sv = s.solvent_last()
        assert cli.main([sub, "-b", B, "-m", Mf, "--epsilon", "1e-8", "--solvent", str(EPS), "--solvent-model", "cosmo", "--solvent-density", "2", "--json"]) == 0
        lines = capsys.readouterr().out.splitlines()
        doc = json.loads(lines[-1])
        assert lines[0] == "solvent: cosmo, epsilon %s, surface elements: 85" % cli.fmt_f(EPS)
        assert doc["total_energy"] == out.total_energy() and doc["electronic_energy"] == out.electronic_energy
        assert doc["solvent"] == {"model": "cosmo", "epsilon": EPS, "points": 85, "nuclear_energy": sv.nuclear, "electronic_energy": sv.electronic,
                                  "polarization_energy": sv.nuclear + sv.electronic, "total_charge": sv.total_charge}
        assert "solvent surface charge: " + cli.fmt_f(sv.total_charge) in lines
    s.close()
