"""Host tests of the Cartesian multipole matrices (qc_multipole_matrices), the Merz-Kollman grid (qc_esp_fit_points) and the charge fit
(qc_esp_fit_solve) against the numpy references of tests/multipole_reference.py, and the argument checks of the new entry points
that need no device.

Matrices: the four systems of tests/test_dipole_host.py (every pair of s..f shells, pure and Cartesian, 169 > 64 primitive pairs in one
shell pair), orders 0..4, origin 0 and ORIGIN.  Tolerance as in that file: 10 x the worst |S_ref - S_oracle| of the four systems, at
most 1e-10, times max(1, max|M_ref|) of the component's order.

Measured on the CPU (tolerance base 1.1e-14; per system the largest |M_host - M_ref| / tolerance over orders and origins, and max|M_ref|
at order 4): tetra-pure-2 0.087 (24.7), tetra-cart-1 0.12 (49.7), deep 0.076 (18.9), water/cc-pVTZ 0.060 (28.3); translation identity at
most 0.092 of the tolerance (deep).

Grid: water 344 points, H2 254, O2 424, ethylene 546, benzene 660, chloroform 728; the closest candidate to an exclusion boundary is
2.4e-5 bohr away (benzene; 1.1e-5 with the custom configuration).  Fit: charges recovered to at most 0.065 (O2) of the bound
100 x 2.2e-16 x cond(A^T A) x max(1, max|q|) - |q - q0| from 2.2e-14 (H2, cond 112) to 3.7e-11 (benzene, cond 1.8e5); rms <= 7.3e-14."""
import ctypes
from math import comb

import numpy as np
import pytest

from conftest import load_system
import dipole_reference as D
import multipole_reference as MR
from test_dipole_host import ORIGIN, SYSTEMS

ORDER = 4
MOLECULES = {"water": "6-31G", "hydrogen": "6-31G", "oxygen": "6-31G", "ethylene": "6-31G", "benzene": "6-31G", "chloroform": "6-31G_st_st"}
NPTS = {"water": 344, "hydrogen": 254, "oxygen": 424, "ethylene": 546, "benzene": 660, "chloroform": 728}


@pytest.fixture(scope="module")
def computed():
    """per system: reference matrices of order 4 (origin 0 and ORIGIN), the host's at every order, host S and dipole matrices - once"""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    out = {}
    for name, make in SYSTEMS.items():
        m = make()
        s = q.System(m)
        out[name] = dict(ref=MR.multipole_matrices(m, ORDER), refO=MR.multipole_matrices(m, ORDER, ORIGIN), dS=float(np.abs(D.overlap_and_dipole(m)[0] - Oracle(m).overlap()).max()),
                         host=[s.multipole_matrices(k) for k in range(ORDER + 1)], hostO=[s.multipole_matrices(k, ORIGIN) for k in range(ORDER + 1)],
                         S_host=s.overlap(), dip=s.dipole_matrices(), dipO=s.dipole_matrices(ORIGIN), none=s.multipole_matrices(2, None))
        s.close()
    base = min(10.0 * max(c["dS"] for c in out.values()), 1e-10)
    for c in out.values():
        c["base"] = base
    return out


def _tols(c, ref):
    """per component: base x max(1, max|M_ref| of the component's order)"""
    t = np.zeros(len(ref))
    for sl in MR.order_slices(ORDER):
        t[sl] = c["base"] * max(1.0, float(np.abs(ref[sl]).max()))
    return t


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_multipole_matrices_match_the_reference(computed, name):
    c = computed[name]
    assert c["dS"] <= 1e-13                                             # (the reference's shells are trusted only where their S is right)
    worst = 0.0
    for ref, host in ((c["ref"], c["host"]), (c["refO"], c["hostO"])):
        tol = _tols(c, ref)
        for k in range(ORDER + 1):
            cnt = len(MR.components(k))
            assert host[k].shape == (cnt,) + ref.shape[1:]
            d = np.abs(host[k] - ref[:cnt]).max(axis=(1, 2))
            worst = max(worst, float((d / tol[:cnt]).max()))
            assert np.all(d <= tol[:cnt]), (name, k, d / tol[:cnt])
    print(name, "base", c["base"], "largest |M_host - M_ref| / tol", worst, "max|M_ref| order 4", float(np.abs(c["ref"][20:]).max()))
    assert np.array_equal(c["none"], c["host"][2])                      # a null origin is (0, 0, 0)


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_components_zero_to_three_are_the_overlap_and_the_dipole_matrices(computed, name):
    c = computed[name]
    for host, dip, ref in ((c["host"][ORDER], c["dip"], c["ref"]), (c["hostO"][ORDER], c["dipO"], c["refO"])):
        tol = _tols(c, ref)
        assert np.abs(host[0] - c["S_host"]).max() <= tol[0]
        for k in range(3):
            assert np.abs(host[1 + k] - dip[k]).max() <= tol[1 + k]


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_every_matrix_is_exactly_symmetric_and_lower_orders_are_leading_parts(computed, name):
    c = computed[name]
    for host in (c["host"], c["hostO"]):
        assert np.array_equal(host[ORDER], host[ORDER].transpose(0, 2, 1))
        for k in range(ORDER):
            assert np.array_equal(host[k], host[ORDER][:len(host[k])])


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_matrices_shift_with_the_origin_by_the_binomial_identity(computed, name):
    c = computed[name]
    comps = MR.components(ORDER)
    idx = {e: k for k, e in enumerate(comps)}
    M0, MO, tol = c["host"][ORDER], c["hostO"][ORDER], _tols(c, c["refO"])
    worst = 0.0
    for k, (i, j, l) in enumerate(comps):
        acc = np.zeros_like(M0[0])
        for r in range(i + 1):
            for s in range(j + 1):
                for t in range(l + 1):
                    acc += (comb(i, r) * comb(j, s) * comb(l, t) * (-ORIGIN[0]) ** (i - r) * (-ORIGIN[1]) ** (j - s) * (-ORIGIN[2]) ** (l - t)) * M0[idx[(r, s, t)]]
        d = float(np.abs(MO[k] - acc).max())
        worst = max(worst, d / tol[k])
        assert d <= tol[k], (name, comps[k], d, tol[k])
    print(name, "translation identity, largest ratio to the tolerance", worst)


def test_multipole_count_and_argument_errors():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    assert [L.qc_multipole_count(k) for k in range(-1, 6)] == [-1, 1, 4, 10, 20, 35, -1]
    assert [len(q.hf.multipole_components(k)) for k in range(5)] == [1, 4, 10, 20, 35]
    assert q.hf.multipole_components(2)[4:] == [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2)]
    assert ctypes.sizeof(q.hf._Multipoles) == 8 + 24 + 3 * 35 * 8 + 48 and ctypes.sizeof(q.hf._EspFit) == 8 + 64 + 8 + 8 + 24 + 24 + 16
    s = q.System(load_system("hydrogen", "STO-3G"))
    try:
        out = np.zeros(35 * s.n * s.n).ctypes.data_as(ctypes.c_void_p)
        for fn in (L.qc_multipole_matrices, L.qc_multipole_matrices_gpu):
            assert fn(None, 2, None, out) == INV and fn(s.handle, 2, None, None) == INV
            assert fn(s.handle, -1, None, out) == INV and fn(s.handle, 5, None, out) == INV
        with pytest.raises(q.QcError):
            s.multipole_matrices(5)
        io = q.hf._Multipoles(order=2)
        assert L.qc_scf_multipoles(None, ctypes.byref(io)) == INV
        q2 = np.zeros(2).ctypes.data_as(ctypes.c_void_p)
        assert L.qc_scf_populations(None, 0, q2, None, None, None) == INV
        Dm = np.eye(s.n).ctypes.data_as(ctypes.c_void_p)
        assert L.qc_populations(None, 0, 1, Dm, q2, None, None, None) == INV and L.qc_populations(s.handle, 0, 1, None, q2, None, None, None) == INV
        assert L.qc_populations(s.handle, 0, 1, Dm, None, None, None, None) == INV
        assert L.qc_populations(s.handle, 2, 1, Dm, q2, None, None, None) == INV and L.qc_populations(s.handle, -1, 1, Dm, q2, None, None, None) == INV
        assert L.qc_populations(s.handle, 0, 0, Dm, q2, None, None, None) == INV and L.qc_populations(s.handle, 0, 3, Dm, q2, None, None, None) == INV
        fit = q.hf._EspFit()
        assert L.qc_scf_esp_charges(None, ctypes.byref(fit), 0, None, q2, None) == INV
    finally:
        s.close()


def test_gpu_calls_fail_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    try:
        assert not q.device_ready()
        with pytest.raises(q.QcError, match="no CPU fallback"):
            s.multipole_matrices(2, gpu=True)
        with pytest.raises(q.QcError, match="no CPU fallback"):
            s.populations(np.eye(s.n))
        with pytest.raises(q.QcError, match="no CPU fallback"):
            s.populations(np.eye(s.n), "lowdin", bond_orders=True)
    finally:
        s.close()


# ---- the grid

@pytest.fixture(scope="module")
def grids():
    import qchem_rs_amd as q
    out = {}
    for mol, basis in MOLECULES.items():
        m = load_system(mol, basis)
        s = q.System(m)
        ref, margin = MR.esp_grid(m, with_margin=True)
        out[mol] = dict(m=m, ref=ref, margin=margin, lib=s.esp_fit_points(), again=s.esp_fit_points(),
                        custom=s.esp_fit_points(scales=[2.2, 1.5], density=0.5), custom_ref=MR.esp_grid(m, (2.2, 1.5), 0.5, with_margin=True))
        s.close()
    return out


@pytest.mark.parametrize("mol", list(MOLECULES))
def test_grid_equals_the_numpy_restatement(grids, mol):
    g = grids[mol]
    print(mol, "points", len(g["ref"]), "closest candidate to an exclusion boundary", g["margin"], "custom", len(g["custom_ref"][0]), g["custom_ref"][1])
    assert g["margin"] >= 1e-9 and g["custom_ref"][1] >= 1e-9            # (on the reference alone: no candidate sits on a boundary)
    assert len(g["ref"]) == NPTS[mol]
    assert g["lib"].shape == g["ref"].shape and np.abs(g["lib"] - g["ref"]).max() <= 1e-12
    assert g["lib"].tobytes() == g["again"].tobytes()
    assert g["custom"].shape == g["custom_ref"][0].shape and np.abs(g["custom"] - g["custom_ref"][0]).max() <= 1e-12
    assert len(g["custom"]) != len(g["lib"])


@pytest.mark.parametrize("mol", list(MOLECULES))
def test_every_point_lies_on_its_sphere_and_outside_the_others(grids, mol):
    g = grids[mol]
    xyz, r = np.asarray(g["m"].coordinates(), float).reshape(-1, 3), MR.radii_bohr(g["m"])
    P = g["lib"]
    d = np.linalg.norm(P[:, None, :] - xyz[None, :, :], axis=2)          # (npts, natoms)
    # the shells come in the order of the scales, so the scale of a point is that of the block it sits in
    start = 0
    for f in MR.DEFAULT_SCALES:
        cnt = len(MR.esp_grid(g["m"], (f,)))
        blk = d[start:start + cnt] / (f * r)[None, :]
        assert np.all(np.abs(blk - 1.0).min(axis=1) * (f * r).max() <= 1e-12)      # on its own sphere
        assert np.all(blk >= 1.0 - 1e-12)                                           # and outside every other
        start += cnt
    assert start == len(P)


def test_grid_capacity_protocol_and_bad_configurations():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    s = q.System(load_system("water", "6-31G"))
    try:
        k = ctypes.c_int64(-7)
        assert L.qc_esp_fit_points(s.handle, None, 0, None, ctypes.byref(k)) == INV and k.value == 344
        buf = np.full((344, 3), np.nan)
        k2 = ctypes.c_int64()
        assert L.qc_esp_fit_points(s.handle, None, 343, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(k2)) == INV and k2.value == 344
        assert np.all(np.isnan(buf))                                     # (nothing is written into a buffer that is too small)
        assert L.qc_esp_fit_points(s.handle, None, 344, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(k2)) == 0 and k2.value == 344
        assert np.array_equal(buf, s.esp_fit_points())
        assert L.qc_esp_fit_points(None, None, 0, None, ctypes.byref(k)) == INV and L.qc_esp_fit_points(s.handle, None, 0, None, None) == INV
        assert L.qc_esp_fit_points(s.handle, None, 344, None, ctypes.byref(k)) == INV
        for bad in (dict(nscales=9), dict(nscales=-1), dict(density=-1.0), dict(density=float("nan"))):
            assert L.qc_esp_fit_points(s.handle, ctypes.byref(q.hf._EspFit(**bad)), 0, None, ctypes.byref(k)) == INV
        cfg = q.hf._EspFit(nscales=1)
        cfg.scales[0] = -1.4
        assert L.qc_esp_fit_points(s.handle, ctypes.byref(cfg), 0, None, ctypes.byref(k)) == INV
    finally:
        s.close()


# ---- the fit

@pytest.mark.parametrize("mol", list(MOLECULES))
def test_fit_recovers_charges_placed_on_the_atoms(grids, mol):
    import qchem_rs_amd as q
    g = grids[mol]
    m, P = g["m"], g["ref"]
    na = len(m.atoms)
    rng = np.random.default_rng(7 + na)
    total = 1.0 if mol == "water" else 0.0
    q0 = rng.uniform(-1.0, 1.0, na)
    q0 += (total - q0.sum()) / na
    A = MR.design_matrix(m, P)
    v = A @ q0
    cond = float(np.linalg.cond(A.T @ A))
    bound = 100.0 * 2.2e-16 * cond * max(1.0, float(np.abs(q0).max()))
    s = q.System(m)
    try:
        r = s.esp_fit_solve(P, v, total)
        ref = MR.kkt_fit(m, P, v, total)
        err = float(np.abs(r.charges - q0).max())
        print(mol, "cond", cond, "bound", bound, "|q - q0|", err, "ratio", err / bound, "numpy", float(np.abs(ref[0] - q0).max()), "rms", r.rms, "sum", r.charges.sum())
        assert err <= bound
        assert r.rms <= 1e-12 and abs(r.charges.sum() - total) <= 1e-13 and r.total_charge == total
        assert np.abs(r.dipole - r.charges @ np.asarray(m.coordinates(), float).reshape(-1, 3)).max() <= 1e-13
        assert r.charges.tobytes() == s.esp_fit_solve(P, v, total).charges.tobytes()
    finally:
        s.close()


def test_fit_rejects_bad_input():
    import qchem_rs_amd as q
    L, INV = q.lib(), q.hf.QC_ERR_INVALID
    m = load_system("water", "6-31G")
    s = q.System(m)
    try:
        P = s.esp_fit_points()
        v = MR.design_matrix(m, P) @ np.array([-0.8, 0.4, 0.4])
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        io, qq = q.hf._EspFit(), np.zeros(3)
        ok = lambda P_, v_, n=None: L.qc_esp_fit_solve(s.handle, len(P_) if n is None else n, p(P_), p(v_), 0.0, ctypes.byref(io), p(qq))
        assert ok(P, v) == 0
        assert ok(P, v, 2) == INV                                        # fewer points than atoms
        vb = v.copy(); vb[5] = np.inf
        assert ok(P, vb) == INV
        vb[5] = np.nan
        assert ok(P, vb) == INV
        Pb = P.copy(); Pb[3] = np.asarray(m.coordinates(), float).reshape(-1, 3)[1]
        assert ok(Pb, v) == INV                                          # a point on a nucleus
        same = np.ascontiguousarray(np.tile(P[:1], (10, 1)))
        assert ok(same, v[:10].copy()) == INV                            # ten copies of one point: a singular system
        assert L.qc_esp_fit_solve(None, len(P), p(P), p(v), 0.0, ctypes.byref(io), p(qq)) == INV
        assert L.qc_esp_fit_solve(s.handle, len(P), None, p(v), 0.0, ctypes.byref(io), p(qq)) == INV
        assert L.qc_esp_fit_solve(s.handle, len(P), p(P), None, 0.0, ctypes.byref(io), p(qq)) == INV
        assert L.qc_esp_fit_solve(s.handle, len(P), p(P), p(v), 0.0, None, p(qq)) == INV
        assert L.qc_esp_fit_solve(s.handle, len(P), p(P), p(v), 0.0, ctypes.byref(io), None) == INV
        assert L.qc_esp_fit_solve(s.handle, len(P), p(P), p(v), float("nan"), ctypes.byref(io), p(qq)) == INV
    finally:
        s.close()
