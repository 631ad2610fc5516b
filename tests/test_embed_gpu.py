"""GPU tests of the point-charge embedding (qc_embed.hip): the embedding matrix, the field on points, the embedded SCF, the gradient
terms and the SCF gradients with charges, reproducibility bit for bit, errors on a live state.

Systems of the matrix and field tests: the five of test_points_gpu.ALL, 300 charges each (embed_reference.charge_set: one full tile of 256
and a masked remainder; a charge 1e-7 bohr off a nucleus, midpoints, two far ones, five charges exactly 0) and the 300 points of
points_reference.sample_points for the field.  Bounds, per element / point: V_pc 1e-12 (1 + sum_c |q_c| |A_ab(R_c)|) against the host
entry and against -sum_c q_c qc_potential_matrix(R_c); e_elec 1e-12 (1 + sum_ab |D_ab| |B_ab|) against tr(D B_host) - E = -grad V with
v_elec = -tr(D A) gives e_elec = +tr(D B) for B = dA/dr; gradient terms 1e-9 max(1, |fd|) against five-point stencils (h = 1e-3) of the
oracle on the ghost system (the Hermite sums behind V_pc and the atoms' gradient in both orientations, lane = record and lane = charge:
QC_PC_ORIENT); SCF gradients 1e-7 against stencils of the oracle's converged UHF(5, 5) energy minus the charge-charge energy.
The oracle's energy of a stencil point is that of its FINAL densities, evaluated with its own integrals: the energy a pass reports is
first order in the last density change, and the stencil's 1.5 / h amplifies that past the bound (as in test_gradient_gpu).

Measured on an MI355X (largest ratio of the error to its bound, or the error itself):
  system          V_pc vs host  V_pc vs -sum q A  tr(D V_pc) identity (relative)  e_elec vs tr(D B_host)
  tetra-pure-2    1.1e-3        5.4e-4            1.0e-14                         5.0e-4
  tetra-cart-1    2.9e-4        7.7e-4            1.6e-15                         4.2e-4
  deep            3.3e-4        3.9e-4            4.4e-15                         1.1e-3
  water/cc-pVTZ   1.4e-3        2.0e-3            8.3e-16                         2.4e-4
  far             6.0e-4        6.4e-4            1.5e-15                         2.5e-4
Embedded SCF against the oracle minus E_cc: STO-3G 2.6e-12 (RHF), 0 (UHF); 6-31G** 9.7e-10, 3.0e-12 (bound 1e-8).  Scaled charges,
E against 1/2 sum D (2H' + G): 3.8e-12, 3.3e-10.  SCF gradients against the energy stencils: at most 6.4e-11 (STO-3G) and 7.9e-11
(6-31G**) over the six coordinates (bound 1e-7); net force 1.4e-15, torque 4.1e-12 and 3.8e-11.  V_pc with the Hermite sums forced
to lane = record / lane = charge: at most 2.0e-3 / 1.5e-3 of the bound (water/cc-pVTZ).  The whole file takes 12 s.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_system
import embed_reference as ER
import points_reference as PR
import synthetic_systems as Y
from test_points_gpu import ALL

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """per system, computed once and left unchanged: charges, points, density, host references and what the GPU gave"""
    if name not in _CASES:
        import qchem_rs_amd as q
        m = ALL[name]()
        k = list(ALL).index(name)
        s = q.System(m)
        C, qc = ER.charge_set(m, 500 + k)
        P = PR.sample_points(m, 300 + k, boys_switch=(name == "far"))
        D = Y.rand_sym(s.n, 60 + k)
        s.set_point_charges(C, qc)
        c = dict(m=m, s=s, C=C, q=qc, P=P, D=D, V_host=s.point_charge_matrix())
        ref, scale = np.zeros((s.n, s.n)), np.zeros((s.n, s.n))
        for r, x in zip(C, qc):
            A = s.potential_matrix(r)
            ref -= x * A
            scale += abs(x) * np.abs(A)
        c["V_ref"], c["V_bound"] = ref, 1e-12 * (1.0 + scale)
        c["V"] = s.point_charge_matrix(gpu=True)
        # both orientations of the Hermite sums (QC_PC_ORIENT, read by a handle at its first embedding call): at 300 charges the
        # library itself takes lane = charge
        for orient in ("record", "charge"):
            os.environ["QC_PC_ORIENT"] = orient
            try:
                h = q.System(m)
                h.set_point_charges(C, qc)
                c["V_" + orient] = h.point_charge_matrix(gpu=True)
                h.close()
            finally:
                del os.environ["QC_PC_ORIENT"]
        c["E"], c["ee"], c["en"] = s.field_on_points(D, P, parts=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", list(ALL))
def test_matrix_matches_the_host_entry_the_potential_sum_and_the_potential_on_points(name):
    c = case(name)
    assert len(c["q"]) == 300 and np.sum(c["q"] == 0.0) == 5
    r_host = float((np.abs(c["V"] - c["V_host"]) / c["V_bound"]).max())
    r_sum = float((np.abs(c["V"] - c["V_ref"]) / c["V_bound"]).max())
    print(name, "V_pc: largest error / bound vs the host entry", r_host, "vs -sum q A", r_sum)
    assert np.all(np.isfinite(c["V"])) and r_host <= 1.0 and r_sum <= 1.0
    assert np.array_equal(c["V"], c["V"].T)
    for orient in ("record", "charge"):
        Vo = c["V_" + orient]
        r_o = max(float((np.abs(Vo - c["V_host"]) / c["V_bound"]).max()), float((np.abs(Vo - c["V_ref"]) / c["V_bound"]).max()))
        print(name, "V_pc, lane =", orient, ": largest error / bound", r_o)
        assert r_o <= 1.0 and np.array_equal(Vo, Vo.T)
    assert np.array_equal(c["V"], c["V_charge"])
    want = float(np.sum(c["q"] * c["s"].esp_on_points(c["D"], c["C"], parts=True)[1]))
    got = float(np.sum(c["D"] * c["V"]))
    print(name, "tr(D V_pc)", got, "sum q v_elec", want, "relative", abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * abs(want)
    ms = c["s"].point_charge_timings()
    assert ms.shape == (4,) and np.all(ms >= 0.0)


@pytest.mark.parametrize("name", list(ALL))
def test_field_matches_the_host_field_matrix_and_numpy(name):
    c = case(name)
    s, D, P, m = c["s"], c["D"], c["P"], c["m"]
    ref, scale = np.zeros((len(P), 3)), np.zeros((len(P), 3))
    for i, r in enumerate(P):
        B = s.field_matrix(r)
        ref[i] = np.einsum("kab,ab->k", B, D)
        scale[i] = np.einsum("kab,ab->k", np.abs(B), np.abs(D))
    ratio = float((np.abs(c["ee"] - ref) / (1e-12 * (1.0 + scale))).max())
    print(name, "e_elec: largest error / bound vs tr(D B_host)", ratio)
    assert np.all(np.isfinite(c["ee"])) and ratio <= 1.0
    nat = len(m.atoms)
    Z, R = np.asarray(m.atomic_numbers(), float), m.coordinates()
    d = P[nat:, None, :] - R[None, :, :]
    en = (Z[None, :, None] * d / np.linalg.norm(d, axis=2)[:, :, None] ** 3).sum(axis=1)
    assert not np.any(np.isfinite(c["en"][:nat]).all(axis=1))            # a point on a nucleus: not finite
    assert np.all(np.isfinite(c["en"][nat:])) and np.abs(c["en"][nat:] - en).max() <= 1e-13 * np.abs(en).max()
    assert np.array_equal(c["E"][nat:], c["en"][nat:] + c["ee"][nat:])
    # the value of a point depends neither on its company nor on the order
    assert np.array_equal(s.field_on_points(D, P[5:12], parts=True)[1], c["ee"][5:12])
    assert np.array_equal(s.field_on_points(D, P[::-1], parts=True)[1][::-1], c["ee"])
    # up to 4096 points the record list is spread over workgroups and the tiles' sums are added in a second pass (all calls above);
    # larger batches walk the list in one workgroup per 256 points: the same bits
    assert np.array_equal(s.field_on_points(D, np.tile(P, (14, 1)), parts=True)[1], np.tile(c["ee"], (14, 1)))
    # The field batches and splits by the potential's rule (test_points_gpu): QC_POINTS_SPLIT=0 forces the walk, QC_POINTS_BATCH=64 forces
    # five batches, each transposed from component-major to point-major on its own (the switches are read by a handle at its first point
    # call): the same bits every way.
    import qchem_rs_amd as q
    for env in ({}, {"QC_POINTS_SPLIT": "0"}, {"QC_POINTS_BATCH": "64"}, {"QC_POINTS_BATCH": "64", "QC_POINTS_SPLIT": "0"},
                {"QC_POINTS_BATCH": "256", "QC_POINTS_SPLIT": "100"}):
        os.environ.update(env)
        try:
            h = q.System(m)
            got = h.field_on_points(D, P, parts=True)[1]
            h.close()
        finally:
            for key in env:
                del os.environ[key]
        assert np.array_equal(got, c["ee"]), env


def _four(s, D, C):
    """matrix, field at the charges, the charges' gradient terms, the atoms' gradient terms with charges"""
    W = Y.rand_sym(s.n, 5)
    t = s.gradient(D, W)
    return s.point_charge_matrix(gpu=True), s.field_on_points(D, C, parts=True)[1], s.point_charge_gradient(D), np.array([t[0], t[1]])


@pytest.mark.parametrize("orient", ["auto", "record", "charge"])
@pytest.mark.parametrize("name", ["tetra-pure-2", "water/cc-pVTZ"])
def test_results_are_reproducible_and_do_not_depend_on_the_charge_batches(name, orient):
    import qchem_rs_amd as q
    c = case(name)
    fixed = {} if orient == "auto" else {"QC_PC_ORIENT": orient}
    got = {}
    for batch in ({}, {"QC_PC_BATCH": "256"}, {"QC_PC_BATCH": "512"}):
        env = dict(fixed, **batch)
        os.environ.update(env)
        try:
            h = q.System(c["m"])
            h.set_point_charges(c["C"], c["q"])
            got[tuple(batch.items())] = _four(h, c["D"], c["C"])
            h.close()
        finally:
            for key in env:
                del os.environ[key]
    base = got[()]
    assert np.array_equal(base[0], c["V"] if orient == "auto" else c["V_" + orient])
    if orient == "auto":
        again = _four(c["s"], c["D"], c["C"])                           # the handle of the other tests, a second call
        assert all(np.array_equal(again[k], base[k]) for k in range(4))
    for key, val in got.items():
        for k in range(4):
            assert np.array_equal(val[k], base[k]), (key, k)
    # the charges' gradient is -q E_elec at the charges, and its nuclear part is numpy's
    assert np.array_equal(base[2][1], -c["q"][:, None] * base[1])


def _converge(s, uhf, eps=1e-10, max_passes=400):
    import qchem_rs_amd as q
    st = q.ScfStepper(s, uhf=uhf, n_alpha=5 if uhf else 0, n_beta=5 if uhf else 0)
    for _ in range(max_passes):
        e, rms = st.iterate()
        if (rms / 2.0 if uhf else rms) < eps:
            return st, e
    raise AssertionError("the embedded SCF did not converge")


def _oracle_final_energy(g):
    """total energy of the oracle's converged UHF(5, 5) on system g, evaluated from its final densities with its own integrals"""
    from oracle.oracle import Oracle
    o = Oracle(g)
    r = o.uhf(200, 1e-10, 5, 5)
    assert r["status"] == 0
    Da, Db = r["density_alpha"], r["density_beta"]
    H, I = o.kinetic() + o.nuclear(), o.eri()
    Dt = Da + Db
    J = np.einsum("mnls,ls->mn", I, Dt)
    Ka, Kb = np.einsum("mlns,ls->mn", I, Da), np.einsum("mlns,ls->mn", I, Db)
    return float(np.sum(Dt * H) + 0.5 * np.sum(Dt * J) - 0.5 * np.sum(Da * Ka) - 0.5 * np.sum(Db * Kb)) + r["nuclear_repulsion"], r


@pytest.mark.parametrize("basis", ["STO-3G", "6-31G_st_st"])
@pytest.mark.parametrize("uhf", [False, True], ids=["rhf", "uhf"])
def test_embedded_scf_matches_the_oracle_on_the_ghost_system(basis, uhf):
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = load_system("water", basis)
    s = q.System(m)
    early = q.ScfStepper(s, uhf=uhf, n_alpha=5 if uhf else 0, n_beta=5 if uhf else 0)      # begun before the charges are set
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    T, V, Vpc = s.one_electron_gpu(1), s.one_electron_gpu(2), s.point_charge_matrix(gpu=True)
    st, e = _converge(s, uhf)
    assert np.array_equal(st.matrix("H"), (T + V) + Vpc) and st.point_charge_count() == 3
    assert s.n_electrons() == 10 and s.nuclear_repulsion() == q.System(m).nuclear_repulsion()
    R, Z = m.coordinates(), np.asarray(m.atomic_numbers(), float)
    enq = ER.e_nq(R, Z, ER.THREE_POS, ER.THREE_Q)
    assert abs(st.embedding_nuclear_energy() - enq) <= 1e-13 * abs(enq) and st.embedding_nuclear_energy() == s.point_charge_nuclear_energy()
    ref = Oracle(ER.embedded_ghost(m, ER.THREE_POS, ER.THREE_Q)).uhf(200, 1e-10, 5, 5)
    assert ref["status"] == 0
    total = e + s.nuclear_repulsion() + st.embedding_nuclear_energy()
    want = ref["total_energy"] - ER.e_cc(ER.THREE_POS, ER.THREE_Q)
    print(basis, "uhf" if uhf else "rhf", "E", total, "oracle - E_cc", want, "dE", total - want)
    assert abs(total - want) < 1e-8
    # the drivers report the same energy, E_nq in its own field
    cfg = q.HartreeFockConfig(200, 1e-10, 5 if uhf else 0, 5 if uhf else 0)
    out = (q.unrestricted_hartree_fock if uhf else q.restricted_hartree_fock)(s, cfg)
    assert out is not None and out.embedding_nuclear_energy == s.point_charge_nuclear_energy() and out.nuclear_repulsion == s.nuclear_repulsion()
    assert abs(out.total_energy() - want) < 1e-8
    # MP2 reads the C and orbital energies of the embedded state
    nocc = (5, 5) if uhf else 5
    Cs = np.array([st.coefficients(k) for k in range(2)]) if uhf else st.coefficients(0)
    es = np.array([st.orbital_energies(k) for k in range(2)]) if uhf else st.orbital_energies(0)
    assert abs(st.mp2().e_corr - s.mp2(Cs, es, nocc).e_corr) <= 1e-12
    st.close()
    # the state begun before the charges were set is the vacuum state, pass for pass
    clean = q.System(m)
    twin = q.ScfStepper(clean, uhf=uhf, n_alpha=5 if uhf else 0, n_beta=5 if uhf else 0)
    assert early.point_charge_count() == 0 and early.embedding_nuclear_energy() == 0.0
    assert np.array_equal(early.matrix("H"), twin.matrix("H")) and np.array_equal(early.matrix("H"), T + V)
    for _ in range(3):
        assert early.iterate() == twin.iterate()
    for x in (early, twin):
        x.close()
    clean.close(); s.close()


@pytest.mark.parametrize("basis", ["STO-3G", "6-31G_st_st"])
def test_scaled_charges_energy_is_the_energy_of_the_embedded_hamiltonian(basis):
    import qchem_rs_amd as q
    m = load_system("water", basis)
    s = q.System(m)
    s.set_schwarz(0.0)
    s.set_point_charges(ER.THREE_POS, 0.37 * ER.THREE_Q)
    st, e = _converge(s, False)
    D = st.density(0)
    Hp = s.kinetic() + s.nuclear() + s.point_charge_matrix()
    want = 0.5 * float(np.sum(D * (2.0 * Hp + s.fock_rhf(D))))
    print(basis, "E_el", e, "1/2 sum D (2H' + G)", want, "dE", e - want)
    assert abs(e - want) < 1e-8
    st.close(); s.close()


def _cart_vtz(tmp_path):
    import json
    from conftest import data
    import qchem_rs_amd as q
    b = json.load(open(data("basis", "cc-pVTZ.json")))
    for el in b["elements"].values():
        for sh in el["electron_shells"]:
            if sh["angular_momentum"][0] >= 2:
                sh["function_type"] = "gto_cartesian"
    f = tmp_path / "cc-pVTZ-cart.json"
    f.write_text(json.dumps(b))
    return q.MolecularSystem.load(data("mol", "water.json"), q.BasisSet.load(str(f)))


@pytest.mark.parametrize("orient", ["record", "charge"])
@pytest.mark.parametrize("basis", ["STO-3G", "6-31G_st_st", "cc-pVTZ", "cc-pVTZ-cart"])
def test_gradient_terms_match_oracle_stencils_on_the_ghost_system(basis, orient, tmp_path, monkeypatch):
    import qchem_rs_amd as q
    m = _cart_vtz(tmp_path) if basis == "cc-pVTZ-cart" else load_system("water", basis)
    monkeypatch.setenv("QC_PC_ORIENT", orient)          # (read at the handle's first embedding call: both orientations up to order 7)
    s = q.System(m)
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    few = basis.startswith("cc-pVTZ")
    for nspin in (1, 2):
        Da, Db, W = Y.rand_sym(s.n, 21), Y.rand_sym(s.n, 22), Y.rand_sym(s.n, 23)
        Pt = Da if nspin == 1 else Da + Db
        t = s.gradient(Da, W) if nspin == 1 else s.gradient(Da, W, Db=Db)
        tc = s.point_charge_gradient(Da) if nspin == 1 else s.point_charge_gradient(Da, Db)
        gcc = ER.e_cc_gradient(ER.THREE_POS, ER.THREE_Q)
        atoms = [(0, 2), (1, 0), (2, 1)] if few or nspin == 2 else [(a, k) for a in range(3) for k in range(3)]
        for a, k in atoms:
            fd = ER.ghost_term_stencil(m, ER.THREE_POS, ER.THREE_Q, Pt, "atom_shift", a, k)
            for j in range(2):
                assert abs(t[j][a, k] - fd[j]) <= 1e-9 * max(1.0, abs(fd[j])), (basis, nspin, "atom", a, k, j, t[j][a, k], fd[j])
        for c, k in [(0, 0), (1, 2), (2, 1)]:
            fd = ER.ghost_term_stencil(m, ER.THREE_POS, ER.THREE_Q, Pt, "charge_shift", c, k)
            fd[0] -= gcc[c, k]
            for j in range(2):
                assert abs(tc[j][c, k] - fd[j]) <= 1e-9 * max(1.0, abs(fd[j])), (basis, nspin, "charge", c, k, j, tc[j][c, k], fd[j])
    s.close()


@pytest.mark.parametrize("basis,uhf", [("STO-3G", False), ("6-31G_st_st", True)], ids=["sto3g-rhf", "631gss-uhf"])
def test_scf_gradients_match_oracle_energy_stencils(basis, uhf):
    import qchem_rs_amd as q
    m = load_system("water", basis)
    s = q.System(m)
    s.set_schwarz(0.0)
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    st, _ = _converge(s, uhf)
    before = [st.density(k) for k in range(2 if uhf else 1)], st.matrix("H")
    g, gc = st.gradient(), st.point_charge_gradient()
    E = st.field_on_points(ER.THREE_POS)
    assert np.abs(gc + ER.THREE_Q[:, None] * E).max() <= 1e-13 * np.abs(gc).max()
    assert np.array_equal(g, st.gradient()) and np.array_equal(gc, st.point_charge_gradient())
    h = Y.H
    ecc = lambda pos: ER.e_cc(pos, ER.THREE_Q)
    for which, idx, k, an in [("atom_shift", 0, 2, g[0, 2]), ("atom_shift", 1, 0, g[1, 0]), ("atom_shift", 2, 1, g[2, 1]),
                              ("charge_shift", 0, 0, gc[0, 0]), ("charge_shift", 1, 2, gc[1, 2]), ("charge_shift", 2, 1, gc[2, 1])]:
        f = {}
        for j in (-2, -1, 1, 2):
            pos = ER.THREE_POS.copy()
            if which == "charge_shift":
                pos[idx, k] += j * h
            f[j] = _oracle_final_energy(ER.embedded_ghost(m, ER.THREE_POS, ER.THREE_Q, **{which: (idx, k, j * h)}))[0] - ecc(pos)
        fd = (f[-2] - 8 * f[-1] + 8 * f[1] - f[2]) / (12 * h)
        print(basis, which, idx, k, "analytic", an, "stencil", fd, "difference", an - fd)
        assert abs(an - fd) <= 1e-7, (which, idx, k, an, fd)
    # translation and rotation of molecule + charges together leave the energy alone
    R = m.coordinates()
    assert np.abs(g.sum(axis=0) + gc.sum(axis=0)).max() <= 1e-10
    torque = np.cross(R, g).sum(axis=0) + np.cross(ER.THREE_POS, gc).sum(axis=0)
    print(basis, "net force", g.sum(axis=0) + gc.sum(axis=0), "torque", torque)
    assert np.abs(torque).max() <= 1e-9
    # the state is left exactly as it was
    after = [st.density(k) for k in range(2 if uhf else 1)], st.matrix("H")
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    twin_s = q.System(m)
    twin_s.set_schwarz(0.0)
    twin_s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    twin, _ = _converge(twin_s, uhf)
    assert st.iterate() == twin.iterate()
    st.close(); twin.close(); s.close(); twin_s.close()


def _f(name, *argtypes):
    import qchem_rs_amd as q
    return ctypes.CFUNCTYPE(ctypes.c_int, *argtypes)((name, q.lib()))


def test_errors_on_a_live_state():
    import qchem_rs_amd as q
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    INV, UNS, OK = q.hf.QC_ERR_INVALID, q.hf.QC_ERR_UNSUPPORTED, q.hf.QC_OK
    fld = _f("qc_scf_field_on_points", vp, i64, vp, vp, vp)
    pcg = _f("qc_scf_point_charge_gradient", vp, vp)
    s = q.System(load_system("water", "STO-3G"))
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    st = q.ScfStepper(s)
    h = st._st
    P, out = np.zeros((4, 3)) + 0.3, np.full(64, 7.0)
    p, o = P.ctypes.data, out.ctypes.data
    assert fld(h, -1, p, o, None) == INV and fld(h, 4, None, o, None) == INV and fld(h, 4, p, None, None) == INV and pcg(h, None) == INV
    assert fld(h, 0, p, o, o) == OK and np.all(out == 7.0)              # refused and empty calls write nothing
    assert fld(h, 4, p, o, None) == OK and pcg(h, o) == OK              # the densities exist from the start
    s.set_point_charges()                                               # the state keeps the set it began with
    assert st.point_charge_count() == 3 and s.point_charge_count() == 0 and st.point_charge_gradient().shape == (3, 3)
    st.close(); s.close()
    s = q.System(load_system("water", "STO-3G"))
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    s.set_shard(0, 2)
    st = q.ScfStepper(s)                                                # a sharded handle builds V_pc whole
    st.iterate()
    h = st._st
    assert np.array_equal(st.matrix("H"), (s.one_electron_gpu(1) + s.one_electron_gpu(2)) + s.point_charge_matrix(gpu=True))
    assert fld(h, 4, p, o, None) == UNS and pcg(h, o) == UNS and fld(h, -1, p, o, None) == INV
    D = np.zeros((s.n, s.n))
    assert _f("qc_field_on_points", vp, vp, i64, vp, vp, vp)(s.handle, D.ctypes.data, 4, p, o, None) == UNS
    assert _f("qc_point_charge_gradient", vp, ctypes.c_int, vp, vp)(s.handle, 1, D.ctypes.data, o) == UNS
    assert _f("qc_gradient", vp, ctypes.c_int, vp, vp, vp)(s.handle, 1, D.ctypes.data, D.ctypes.data, o) == UNS
    assert _f("qc_scf_gradient", vp, vp)(h, o) == UNS
    st.close(); s.close()
