"""GPU tests of the multipole kernel (qc_multipole_matrices_gpu) and of the total moments of an SCF state (qc_scf_multipoles); also
the checks that span the three property groups of DESIGN.md 3.12: the state is left untouched, and the errors on a live state.

Matrices: GPU against host on the four systems of tests/test_dipole_host.py, orders 0..4, origin 0 and ORIGIN, to
1e-12 max(1, max|M|) per order - the margin of the dipole kernel test; exactly symmetric; two calls give equal bits.
Moments: every component against sum Z R^c - sum P . M_ref formed in numpy from the state's density and the reference matrices
(tests/multipole_reference.py), to 1e-12 (1 + sum_A Z_A |R_A^c| + sum_ab |P_ab| |M_c,ab|): f64 sums of that magnitude.

Measured on an MI355X (largest ratio of the error to its bound): |M_gpu - M_host| 5.7e-4 (tetra-pure-2), 3.3e-4 (tetra-cart-1), 7.4e-4
(deep), 4.1e-4 (water/cc-pVTZ); moments against the numpy trace 1.2e-4 (water), 2.6e-4 (O2), 1.0e-4 (H2O+)."""
import ctypes

import numpy as np
import pytest

from conftest import load_system
import multipole_reference as MR
from test_dipole_host import ORIGIN, SYSTEMS
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu

ORDER = 4
STATES = {"water": ("water/cc-pVDZ", False, 0, 0, 0), "oxygen": ("oxygen/cc-pVDZ", True, 9, 7, 0), "water+": ("water/cc-pVDZ", True, 5, 4, 1)}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_gpu_multipole_matrices_match_the_host(name):
    import qchem_rs_amd as q
    s = q.System(SYSTEMS[name]())
    try:
        worst = 0.0
        for origin in (None, ORIGIN):
            for k in range(ORDER + 1):
                Mh, Mg = s.multipole_matrices(k, origin), s.multipole_matrices(k, origin, gpu=True)
                for sl in MR.order_slices(k):
                    scale = max(1.0, float(np.abs(Mh[sl]).max()))
                    d = float(np.abs(Mg[sl] - Mh[sl]).max())
                    worst = max(worst, d / (1e-12 * scale))
                    assert d <= 1e-12 * scale, (name, k, sl, d, scale)
                assert np.array_equal(Mg, Mg.transpose(0, 2, 1))
                assert Mg.tobytes() == s.multipole_matrices(k, origin, gpu=True).tobytes()
        print(name, "largest |M_gpu - M_host| / (1e-12 scale)", worst)
    finally:
        s.close()


@pytest.mark.parametrize("kind", list(STATES))
def test_scf_multipoles_are_the_traces_with_the_reference_matrices(kind):
    name, uhf, na, nb, charge = STATES[kind]
    s, st, _ = converged(name, uhf, na, nb, eps=1e-8, schwarz0=False)
    try:
        m = load_system(*name.split("/"))
        P = st.density(0) + (st.density(1) if uhf else 0.0)
        worst = 0.0
        for origin in (None, ORIGIN):
            O = np.zeros(3) if origin is None else origin
            M = MR.multipole_matrices(m, ORDER, O)
            nuc = MR.nuclear_moments(m, ORDER, O)
            ref = nuc - np.array([np.sum(P * M[c]) for c in range(len(M))])
            bound = 1e-12 * (1.0 + MR.nuclear_moments_abs(m, ORDER, O) + np.array([np.sum(np.abs(P) * np.abs(M[c])) for c in range(len(M))]))
            r = st.multipoles(ORDER, origin)
            worst = max(worst, float((np.abs(r.total - ref) / bound).max()))
            assert np.all(np.abs(r.total - ref) <= bound), (kind, np.abs(r.total - ref) / bound)
            assert np.all(np.abs(r.nuclear - nuc) <= bound) and np.array_equal(r.total, r.nuclear + r.electronic)
            assert abs(r.total[0] - charge) <= bound[0]
            assert np.abs(r.total[1:4] - st.dipole(origin)).max() <= 1e-10
            qt = r.quadrupole_traceless
            scale = float(bound[4:10].max())
            assert abs(np.trace(qt)) <= 3.0 * scale and np.array_equal(qt, qt.T)
            assert np.abs(qt[np.triu_indices(3)] - MR.traceless_quadrupole(ref[4:10])).max() <= 3.0 * scale
            # lower orders: the leading components, and equal bits twice
            r2 = st.multipoles(2, origin)
            assert np.array_equal(r2.total, r.total[:10]) and np.array_equal(r2.quadrupole_traceless, qt)
            assert st.multipoles(ORDER, origin).total.tobytes() == r.total.tobytes()
            assert np.array_equal(st.multipoles(1, origin).quadrupole_traceless, np.zeros((3, 3)))
        if charge == 0:      # a neutral molecule: the first moments do not depend on the origin
            assert np.abs(st.multipoles(1, ORIGIN).total[1:4] - st.multipoles(1).total[1:4]).max() <= 1e-10
        print(kind, "largest |moment - reference| / bound", worst, "total", st.multipoles(2).total)
    finally:
        st.close(); s.close()


@pytest.mark.parametrize("kind", ["water", "oxygen"])
def test_property_calls_leave_the_state_alone(kind):
    name, uhf, na, nb, _ = STATES[kind]
    s, st, _ = converged(name, uhf, na, nb, eps=1e-8)
    s2, twin, _ = converged(name, uhf, na, nb, eps=1e-8)
    try:
        before = st.stability(nroots=2, tol=1e-6).eigenvalues
        st.multipoles(ORDER, ORIGIN)
        for scheme in ("mulliken", "lowdin"):
            st.populations(scheme, bond_orders=True)
        st.esp_charges()
        after = st.stability(nroots=2, tol=1e-6).eigenvalues
        assert np.array_equal(before, after)
        twin.stability(nroots=2, tol=1e-6); twin.stability(nroots=2, tol=1e-6)
        e1, r1 = st.iterate()
        e2, r2 = twin.iterate()
        assert (e1, r1) == (e2, r2)
        for k in range(2 if uhf else 1):
            assert np.array_equal(st.density(k), twin.density(k))
    finally:
        st.close(); twin.close(); s.close(); s2.close()


def test_errors_on_a_live_state():
    import qchem_rs_amd as q
    L = q.lib()
    INV, UNS, OK = q.hf.QC_ERR_INVALID, q.hf.QC_ERR_UNSUPPORTED, q.hf.QC_OK
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = q.System(load_system("water", "STO-3G"))
    st = q.ScfStepper(s)
    h, n = st._st, s.n
    qq, sp, orb, bo = np.zeros(3), np.zeros(3), np.zeros(n), np.zeros(9)
    io = q.hf._Multipoles(order=2)
    assert L.qc_scf_multipoles(h, ctypes.byref(io)) == OK and abs(io.total[0]) < 1e-10      # available from qc_scf_begin_* on
    assert L.qc_scf_populations(h, 0, p(qq), p(sp), p(orb), p(bo)) == OK and abs(qq.sum()) < 1e-10
    st.iterate()
    assert L.qc_scf_multipoles(h, None) == INV
    for order in (-1, 5):
        assert L.qc_scf_multipoles(h, ctypes.byref(q.hf._Multipoles(order=order))) == INV
    assert L.qc_scf_populations(h, 0, None, p(sp), p(orb), p(bo)) == INV
    for scheme in (-1, 2):
        assert L.qc_scf_populations(h, scheme, p(qq), None, None, None) == INV
    assert L.qc_scf_populations(h, 1, p(qq), None, None, None) == OK
    D = st.density(0)
    for nspin in (0, 3):
        assert L.qc_populations(s.handle, 0, nspin, p(D), p(qq), None, None, None) == INV
    fit = q.hf._EspFit()
    P = s.esp_fit_points()
    v = np.zeros(len(P))
    assert L.qc_scf_esp_charges(h, None, len(P), p(P), p(qq), p(v)) == INV
    assert L.qc_scf_esp_charges(h, ctypes.byref(fit), len(P), p(P), None, p(v)) == INV
    assert L.qc_scf_esp_charges(h, ctypes.byref(fit), 2, p(P), p(qq), p(v)) == INV           # npts < natoms
    assert L.qc_scf_esp_charges(h, ctypes.byref(fit), -1, p(P), p(qq), p(v)) == INV
    assert L.qc_scf_esp_charges(h, ctypes.byref(q.hf._EspFit(nscales=9)), 0, None, p(qq), None) == INV
    assert L.qc_scf_esp_charges(h, ctypes.byref(fit), 0, None, p(qq), None) == OK and fit.npts == len(P)
    st.close(); s.close()
    s = q.System(load_system("water", "STO-3G"))
    s.set_shard(0, 2)
    st = q.ScfStepper(s)
    st.iterate()
    h = st._st
    assert L.qc_scf_multipoles(h, ctypes.byref(io)) == UNS and L.qc_scf_populations(h, 0, p(qq), None, None, None) == UNS
    assert L.qc_scf_esp_charges(h, ctypes.byref(fit), 0, None, p(qq), None) == UNS
    assert L.qc_scf_multipoles(h, ctypes.byref(q.hf._Multipoles(order=7))) == INV           # a bad argument is reported first
    assert L.qc_populations(s.handle, 0, 1, p(D), p(qq), None, None, None) == UNS
    M = np.zeros((4, n, n))
    assert L.qc_multipole_matrices_gpu(s.handle, 1, None, p(M)) == UNS
    st.close(); s.close()
