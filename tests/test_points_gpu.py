"""GPU tests of the values on points: basis functions, density, orbitals and electrostatic potential (qc_points.hip) against numpy, the
library's host potential matrix and the oracle; batching and independence bit for bit; the SCF-state entry points; errors; the CLI's cube.

Systems: the four of test_dipole_host.SYSTEMS (n = 64, 80, 18, 58) and synthetic_systems.far(2.0) (n = 32) for the Boys switch.  300 points
each (points_reference.sample_points: one full 256-lane workgroup and a masked remainder; the nuclei, a point 1e-7 bohr off one, midpoints,
two far points, and for far() three points on both sides of QC_BOYS_XMAX for the same-centre pairs).  D = rand_sym(n, seed).

Bounds, per point: phi 1e-13 max(1, max|phi|); rho 1e-12 (1 + sum_ab |D_ab| |phi_a phi_b|); v_elec 1e-12 (1 + sum_ab |D_ab| |A_ab|) against
-tr(D qc_potential_matrix) on all points and against the oracle route on the first 40; v_nuc 1e-13 relative, +inf on the nuclei;
sum_A Z_A v_elec(R_A) = tr(D V_gpu) to 1e-11 |tr(D V)|.

Measured on an MI355X (largest ratio of the error to its bound):
  system          phi vs host  phi vs numpy  rho      v_elec vs host  v_elec vs oracle  trace identity (relative)
  tetra-pure-2    1.5e-3       1.5e-3        1.6e-3   2.1e-4          1.6e-4            1.1e-15
  tetra-cart-1    3.3e-3       2.2e-3        9.2e-4   1.7e-4          1.3e-4            3.5e-14
  deep            6.5e-5       1.4e-3        8.1e-4   3.4e-4          2.3e-4            8.7e-16
  water/cc-pVTZ   9.3e-5       1.5e-3        2.6e-4   1.3e-4          1.1e-4            6.9e-16
  far             1.7e-3       1.4e-3        1.7e-4   1.5e-4          1.6e-4            1.7e-15
SCF states: rho against sum_i n_i psi_i^2 at 6.6e-4 (water/cc-pVDZ RHF) and 3.8e-4 (O2/cc-pVDZ UHF) of the rho bound.  No case comes near
its bound; the whole file takes 3.3 s.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import data, load_system
import points_reference as PR
import synthetic_systems as Y
from test_dipole_host import SYSTEMS
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu

ALL = dict(SYSTEMS)
ALL["far"] = lambda: Y.far(2.0)[0]
NREF = 40
_CASES = {}


def case(name):
    """per system, computed once and left unchanged: points, density, the references and what the GPU gave for them"""
    if name not in _CASES:
        import qchem_rs_amd as q
        m = ALL[name]()
        k = list(ALL).index(name)
        s = q.System(m)
        P = PR.sample_points(m, 300 + k, boys_switch=(name == "far"))
        D = Y.rand_sym(s.n, 40 + k)
        c = dict(m=m, s=s, P=P, D=D, phi_ref=PR.phi(m, P), phi_host=s.basis_on_points(P))
        ve_ref, ve_scale = np.zeros(len(P)), np.zeros(len(P))
        for i, r in enumerate(P):
            A = s.potential_matrix(r)
            ve_ref[i], ve_scale[i] = -np.sum(D * A), np.sum(np.abs(D) * np.abs(A))
        c["ve_ref"], c["ve_bound"] = ve_ref, 1e-12 * (1.0 + ve_scale)
        c["ve_oracle"] = np.array([-np.sum(D * PR.potential_matrix_oracle(m, r)) for r in P[:NREF]])
        c["phi"] = s.orbitals_on_points(np.eye(s.n), P).T
        c["rho"] = s.density_on_points(D, P)
        c["V"], c["ve"], c["vn"] = s.esp_on_points(D, P, parts=True)
        _CASES[name] = c
    return _CASES[name]


@pytest.mark.parametrize("name", list(ALL))
def test_basis_values_match_the_host_entry_and_numpy(name):
    c = case(name)
    bound = 1e-13 * max(1.0, float(np.abs(c["phi_ref"]).max()))
    e_host, e_ref = float(np.abs(c["phi"] - c["phi_host"]).max()), float(np.abs(c["phi"] - c["phi_ref"]).max())
    print(name, "phi: vs host", e_host / bound, "vs numpy", e_ref / bound, "of the bound", bound)
    assert c["phi"].shape == c["phi_ref"].shape == (PR.NPOINTS, c["s"].n)
    assert e_host <= bound and e_ref <= bound


@pytest.mark.parametrize("name", list(ALL))
def test_density_matches_numpy(name):
    c = case(name)
    ref = np.einsum("ka,ab,kb->k", c["phi_ref"], c["D"], c["phi_ref"])
    bound = 1e-12 * (1.0 + np.einsum("ka,ab,kb->k", np.abs(c["phi_ref"]), np.abs(c["D"]), np.abs(c["phi_ref"])))
    ratio = float((np.abs(c["rho"] - ref) / bound).max())
    print(name, "rho: largest error / bound", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("name", list(ALL))
def test_potential_matches_the_host_matrix_the_oracle_and_numpy(name):
    c = case(name)
    r_host = float((np.abs(c["ve"] - c["ve_ref"]) / c["ve_bound"]).max())
    r_orc = float((np.abs(c["ve"][:NREF] - c["ve_oracle"]) / c["ve_bound"][:NREF]).max())
    print(name, "v_elec: largest error / bound vs -tr(D A_host)", r_host, "vs the oracle route", r_orc)
    assert np.all(np.isfinite(c["ve"]))
    assert r_host <= 1.0 and r_orc <= 1.0
    vn = PR.nuclear_potential(c["m"], c["P"])
    nat = len(c["m"].atoms)
    assert np.all(np.isposinf(c["vn"][:nat])) and np.all(np.isposinf(vn[:nat])) and np.all(np.isposinf(c["V"][:nat]))
    assert np.all(np.isfinite(c["vn"][nat:])) and np.abs(c["vn"][nat:] - vn[nat:]).max() <= 1e-13 * np.abs(vn[nat:]).max()
    assert np.array_equal(c["V"][nat:], c["vn"][nat:] + c["ve"][nat:])


@pytest.mark.parametrize("name", list(ALL))
def test_potential_at_the_nuclei_gives_the_nuclear_attraction_trace(name):
    c = case(name)
    Z = np.asarray(c["m"].atomic_numbers(), float)
    want = float(np.sum(c["D"] * c["s"].one_electron_gpu(2)))
    got = float(np.sum(Z * c["ve"][:len(Z)]))
    print(name, "tr(D V)", want, "sum_A Z_A v_elec(R_A)", got, "relative", abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * abs(want)


def _three(s, D, P):
    return s.density_on_points(D, P), s.esp_on_points(D, P, parts=True)[1], s.orbitals_on_points(np.eye(s.n), P)


@pytest.mark.parametrize("name", list(ALL))
def test_results_do_not_depend_on_batching_order_or_company(name):
    import qchem_rs_amd as q
    c = case(name)
    s, D, P = c["s"], c["D"], c["P"]
    base = (c["rho"], c["ve"], c["phi"].T)
    again = _three(s, D, P)                                             # a second call
    a, b = _three(s, D, P[:299]), _three(s, D, P[299:])
    rev = _three(s, D, P[::-1])
    for k in range(3):
        assert np.array_equal(again[k], base[k])
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=-1), base[k])
        assert np.array_equal(rev[k][..., ::-1], base[k])
    for npts in (1, 7, 64):
        few = _three(s, D, P[5:5 + npts])
        for k in range(3):
            assert np.array_equal(few[k], base[k][..., 5:5 + npts]), (npts, k)
    # The potential of a batch of at most 4096 points spreads the tiles of the record list over workgroups and adds their sums in a
    # second pass (all calls above); larger batches walk the list in one workgroup per 256 points.  QC_POINTS_SPLIT=0 forces the walk,
    # QC_POINTS_BATCH=64 forces five batches (the switches are read by a handle at its first point call): the same bits every way.
    got = {}
    for env in ({}, {"QC_POINTS_SPLIT": "0"}, {"QC_POINTS_BATCH": "64"}, {"QC_POINTS_BATCH": "64", "QC_POINTS_SPLIT": "0"},
                {"QC_POINTS_BATCH": "256", "QC_POINTS_SPLIT": "100"}):
        os.environ.update(env)
        try:
            h = q.System(c["m"])
            got[tuple(env.items())] = _three(h, D, P)
            if env.get("QC_POINTS_SPLIT") == "0":
                got[tuple(env.items()) + ("few",)] = tuple(x[..., :7] for x in _three(h, D, P[:7]))
            h.close()
        finally:
            for key in env:
                del os.environ[key]
    for key, val in got.items():
        for k in range(3):
            assert np.array_equal(val[k], base[k][..., :val[k].shape[-1]]), (key, k)


SCF = {"rhf": ("water/cc-pVDZ", False, 0, 0, 1e-10), "uhf": ("oxygen/cc-pVDZ", True, 9, 7, 1e-8)}


@pytest.mark.parametrize("kind", list(SCF))
def test_scf_state_calls_match_the_host_pointer_calls_and_leave_the_state_alone(kind):
    name, uhf, na, nb, eps = SCF[kind]
    s, st, _ = converged(name, uhf, na, nb, eps=eps)
    s2, twin, _ = converged(name, uhf, na, nb, eps=eps)
    try:
        m = s.mol
        P = PR.sample_points(m, 77)
        nat, n = len(m.atoms), s.n
        Ds = [st.density(k) for k in range(2 if uhf else 1)]
        Cs = [st.coefficients(k) for k in range(2 if uhf else 1)]
        Dt = Ds[0] + Ds[1] if uhf else Ds[0]
        rel = lambda x, y: float(np.abs(x - y).max()) <= 1e-13 * float(np.abs(y).max())
        rho = st.density_on_points(P)
        assert rel(rho, s.density_on_points(Dt, P))
        V, ve, vn = st.esp_on_points(P, parts=True)
        V2, ve2, vn2 = s.esp_on_points(Dt, P, parts=True)
        assert rel(ve, ve2) and np.all(np.isposinf(V[:nat])) and rel(V[nat:], V2[nat:]) and np.all(np.isfinite(ve))
        occ = [(0, na, 1.0), (1, nb, 1.0)] if uhf else [(0, int(np.sum(m.atomic_numbers())) // 2, 2.0)]
        total, scale = np.zeros(len(P)), np.zeros(len(P))
        phi = PR.phi(m, P)
        for spin, nocc, weight in occ:
            psi = st.orbitals_on_points(P, list(range(nocc)), spin=spin)
            assert psi.shape == (nocc, len(P)) and rel(psi, s.orbitals_on_points(Cs[spin][:, :nocc], P))
            total += weight * (psi ** 2).sum(axis=0)
        scale = np.einsum("ka,ab,kb->k", np.abs(phi), np.abs(Dt), np.abs(phi))
        ratio = float((np.abs(rho - total) / (1e-12 * (1.0 + scale))).max())
        print(kind, "rho vs sum n_i psi_i^2: largest error / bound", ratio)
        assert ratio <= 1.0
        # scattered indices come out in the order asked for
        pick = st.orbitals_on_points(P[:9], [3, 0, 1, 2], spin=0)
        assert np.array_equal(pick, st.orbitals_on_points(P[:9], list(range(4)), spin=0)[[3, 0, 1, 2]])
        spin_rho = st.density_on_points(P, spin=True)
        if uhf:
            ra, rb = s.density_on_points(Ds[0], P), s.density_on_points(Ds[1], P)
            assert rel(rho, ra + rb) and float(np.abs(spin_rho - (ra - rb)).max()) <= 1e-13 * float(np.abs(ra + rb).max())
            assert abs(spin_rho).max() > 1e-3
        else:
            assert np.array_equal(spin_rho, np.zeros(len(P)))
        # the next pass is the one a state without point calls makes
        e1, r1 = st.iterate()
        e2, r2 = twin.iterate()
        assert (e1, r1) == (e2, r2)
        for k in range(2 if uhf else 1):
            assert np.array_equal(st.density(k), twin.density(k))
    finally:
        st.close(); twin.close(); s.close(); s2.close()


def _f(name, *argtypes):
    import qchem_rs_amd as q
    return ctypes.CFUNCTYPE(ctypes.c_int, *argtypes)((name, q.lib()))


def test_errors_on_a_live_state():
    import qchem_rs_amd as q
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    INV, UNS, OK = q.hf.QC_ERR_INVALID, q.hf.QC_ERR_UNSUPPORTED, q.hf.QC_OK
    dens = _f("qc_scf_density_on_points", vp, ci, i64, vp, vp)
    esp = _f("qc_scf_esp_on_points", vp, i64, vp, vp, vp)
    orb = _f("qc_scf_orbitals_on_points", vp, ci, ci, ci, i64, vp, vp)
    s = q.System(load_system("water", "STO-3G"))
    st = q.ScfStepper(s)
    n, h = s.n, st._st
    P, out = np.zeros((4, 3)) + 0.3, np.full(4 * n, 7.0)
    p, o = P.ctypes.data, out.ctypes.data
    assert orb(h, 0, 0, 1, 4, p, o) == INV                              # no orbitals before the first pass ...
    assert dens(h, 0, 4, p, o) == OK and esp(h, 4, p, o, None) == OK    # ... but the densities exist from the start
    st.iterate()
    assert orb(h, 0, 0, 1, 4, p, o) == OK
    out[:] = 7.0
    for which in (-1, 2):
        assert dens(h, which, 4, p, o) == INV
    assert dens(h, 0, -1, p, o) == INV and dens(h, 0, 4, None, o) == INV and dens(h, 0, 4, p, None) == INV
    assert esp(h, -1, p, o, None) == INV and esp(h, 4, None, o, None) == INV and esp(h, 4, p, None, None) == INV
    for spin, first, count in ((1, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, 0), (0, 0, n + 1), (0, n, 1), (0, n - 1, 2)):
        assert orb(h, spin, first, count, 4, p, o) == INV, (spin, first, count)
    assert orb(h, 0, 0, 1, -1, p, o) == INV and orb(h, 0, 0, 1, 4, None, o) == INV and orb(h, 0, 0, 1, 4, p, None) == INV
    assert dens(h, 0, 0, p, o) == OK and esp(h, 0, p, o, o) == OK and orb(h, 0, 0, n, 0, p, o) == OK
    assert np.all(out == 7.0)                                           # refused and empty calls write nothing
    st.close(); s.close()
    s = q.System(load_system("water", "STO-3G"))
    s.set_shard(0, 2)
    st = q.ScfStepper(s)
    st.iterate()
    h = st._st
    assert dens(h, 0, 4, p, o) == UNS and esp(h, 4, p, o, None) == UNS and orb(h, 0, 0, 1, 4, p, o) == UNS
    assert dens(h, 2, 4, p, o) == INV                                   # a bad argument is reported first
    D = np.zeros((n, n))
    assert _f("qc_density_on_points", vp, vp, i64, vp, vp)(s.handle, D.ctypes.data, 4, p, o) == UNS
    st.close(); s.close()


def _read_cube(path):
    lines = open(path).read().splitlines()
    nat = int(lines[2].split()[0])
    origin = [float(x) for x in lines[2].split()[1:]]
    shape = [int(lines[3 + k].split()[0]) for k in range(3)]
    vecs = [[float(x) for x in lines[3 + k].split()[1:]] for k in range(3)]
    atoms = [[float(x) for x in l.split()] for l in lines[6:6 + nat]]
    body = lines[6 + nat:]
    return origin, shape, vecs, atoms, np.array(" ".join(body).split(), float), body


def test_cli_writes_cube_files(tmp_path, capsys):
    from qchem_rs_amd import cli, hf
    import qchem_rs_amd as q
    B, M = data("basis", "STO-3G.json"), data("mol", "hydrogen.json")
    path = str(tmp_path / "rho.cube")
    common = ["--cube-spacing", "0.2", "--cube-margin", "4.0", "--json"]
    assert cli.main(["rhf", "-b", B, "-m", M, "--cube", "density", "--cube-file", path] + common) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[4].startswith("orbital energies: ") and len(lines) == 6             # nothing but the JSON object is added
    doc = json.loads(lines[5])["cube"]
    origin, shape, vecs, atoms, val, body = _read_cube(path)
    assert shape == [41, 41, 48] == doc["shape"] and origin == [-4.0, -4.0, -4.0] == doc["origin"]
    assert vecs == [[0.2, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 0.2]] and doc["spacing"] == 0.2 and doc["what"] == "density" and doc["file"] == path
    assert atoms == [[1.0, 1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0, 1.4]]
    assert len(body) == 41 * 41 * 8 and len(val) == 41 * 41 * 48
    m = q.MolecularSystem.load(M, q.BasisSet.load(B))
    pts = cli.cube_grid(m, 0.2, 4.0)[2]
    _, rho = hf._stepped(m, hf.HartreeFockConfig(100, 1e-6), False, lambda st: st.density_on_points(pts))
    assert np.all(np.abs(val - rho) <= 1e-5 * np.abs(rho) + 1e-12)
    print("integral", doc["integral"], "min", doc["min"], "max", doc["max"])
    assert abs(doc["integral"] - 2.0) <= 2e-3 and abs(doc["integral"] - rho.sum() * 0.2 ** 3) <= 1e-12
    assert doc["min"] == rho.min() and doc["max"] == rho.max()
    for what in ("esp", "homo"):
        path = str(tmp_path / (what + ".cube"))
        assert cli.main(["rhf", "-b", B, "-m", M, "--cube", what, "--cube-file", path] + common) == 0
        capsys.readouterr()
        val = _read_cube(path)[4]
        assert len(val) == 41 * 41 * 48 and np.all(np.isfinite(val))
        if what == "homo":                                               # the bonding orbital: one sign, normalised
            assert abs(abs(val.sum()) - np.abs(val).sum()) <= 1e-3 * np.abs(val).sum() and abs((val ** 2).sum() * 0.2 ** 3 - 1.0) <= 2e-3
        else:
            assert val.max() > 1.0                                       # near a nucleus its potential wins
