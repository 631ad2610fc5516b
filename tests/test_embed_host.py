"""Host tests (no device) of the point-charge embedding: the charge set on the handle, E_nq, the host embedding matrix
(qc_point_charge_matrix) against the oracle and against the host potential matrix, the field matrix (qc_field_matrix) against a
five-point stencil of the potential matrix, argument errors, the bindings.

Measured on the CPU (largest ratio of the error to its bound):
  V_pc vs the oracle's ghost-system difference, water, three charges   STO-3G 5.4e-3, 6-31G** 2.2e-3 (bound 1e-12 (1 + sum |q| |A|))
  V_pc vs -sum q A_host, 40 real charges                               tetra-pure-2 3.5e-4, tetra-cart-1 2.6e-4, deep 1.6e-4, water/cc-pVTZ 4.0e-4
  field matrix vs the stencil (h = 1e-3, 8 points >= 1 bohr from every nucleus, none left out; bound 1e-9 max(1, |fd|))
                                                                       tetra-pure-2 6.5e-3, tetra-cart-1 5.4e-3, deep 4.7e-4, water/cc-pVTZ 5.9e-3
The last row is the stencil's own error as much as the matrix's: the analytic matrix is exact to rounding, the five-point formula carries
h^4 / 30 times the fifth derivative and the rounding of four matrices divided by 12 h.  Largest ratio: 6.5e-3 of the bound.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_system
import embed_reference as ER
import points_reference as PR
from test_dipole_host import SYSTEMS

NEW = ("qc_set_point_charges", "qc_point_charge_count", "qc_point_charge_nuclear_energy", "qc_scf_point_charge_count",
       "qc_scf_point_charge_nuclear_energy", "qc_point_charge_matrix", "qc_point_charge_matrix_gpu", "qc_field_matrix", "qc_field_on_points",
       "qc_scf_field_on_points", "qc_point_charge_gradient", "qc_scf_point_charge_gradient", "qc_point_charge_timings")


def test_exports_and_bindings():
    import qchem_rs_amd as q
    for name in NEW:
        assert name in q.hf.EXPORTS and hasattr(q.lib(), name), name
    for cls, names in ((q.System, ("set_point_charges", "point_charge_count", "point_charge_nuclear_energy", "point_charge_matrix", "field_matrix",
                                   "field_on_points", "point_charge_gradient", "point_charge_timings")),
                       (q.ScfStepper, ("field_on_points", "point_charge_gradient", "embedding_nuclear_energy", "point_charge_count"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    for cls in (q.hf.RestrictedHartreeFockOutput, q.hf.UnrestrictedHartreeFockOutput):
        args = ([0.0], [0.0]) if cls is q.hf.UnrestrictedHartreeFockOutput else ([0.0],)
        out = cls(*args, -2.0, 0.5, 3)
        assert out.embedding_nuclear_energy == 0.0 and out.total_energy() == -1.5
        out.embedding_nuclear_energy = 0.25
        assert out.total_energy() == -1.25


@pytest.mark.parametrize("basis", ["STO-3G", "6-31G_st_st"])
def test_host_matrix_matches_the_oracle_ghost_system_difference(basis):
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = load_system("water", basis)
    s = q.System(m)
    s.set_point_charges(ER.THREE_POS, ER.THREE_Q)
    V = s.point_charge_matrix()
    ref = Oracle(ER.embedded_ghost(m, ER.THREE_POS, ER.THREE_Q)).nuclear() - Oracle(m).nuclear()
    scale = sum(abs(c) * np.abs(s.potential_matrix(r)) for r, c in zip(ER.THREE_POS, ER.THREE_Q))
    ratio = float((np.abs(V - ref) / (1e-12 * (1.0 + scale))).max())
    print(basis, "V_pc vs the oracle: largest error / bound", ratio)
    assert np.array_equal(V, V.T) and ratio <= 1.0
    s.close()


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_matrix_matches_the_potential_matrix_sum(name):
    import qchem_rs_amd as q
    m = SYSTEMS[name]()
    s = q.System(m)
    rng = np.random.default_rng(11)
    P = m.coordinates().mean(axis=0) + 2.5 * rng.standard_normal((40, 3))
    c = rng.standard_normal(40)
    c[7] = 0.0
    s.set_point_charges(P, c)
    V = s.point_charge_matrix()
    ref, scale = np.zeros_like(V), np.zeros_like(V)
    for r, qc in zip(P, c):
        A = s.potential_matrix(r)
        ref -= qc * A
        scale += abs(qc) * np.abs(A)
    ratio = float((np.abs(V - ref) / (1e-12 * (1.0 + scale))).max())
    print(name, "V_pc vs -sum q A: largest error / bound", ratio)
    assert np.array_equal(V, V.T) and ratio <= 1.0
    s.set_point_charges()
    assert s.point_charge_count() == 0 and np.array_equal(s.point_charge_matrix(), np.zeros_like(V))
    s.close()


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_field_matrix_matches_a_stencil_of_the_potential_matrix(name):
    import qchem_rs_amd as q
    m = SYSTEMS[name]()
    s = q.System(m)
    h, worst = 1e-3, 0.0
    for r in ER.field_points(m, 5, 8):
        assert np.linalg.norm(m.coordinates() - r, axis=1).min() >= 1.0
        B = s.field_matrix(r)
        assert B.shape == (3, s.n, s.n)
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            A = {j: s.potential_matrix(r + j * e) for j in (-2, -1, 1, 2)}
            fd = (A[-2] - 8 * A[-1] + 8 * A[1] - A[2]) / (12 * h)
            worst = max(worst, float((np.abs(B[k] - fd) / (1e-9 * np.maximum(1.0, np.abs(fd)))).max()))
            assert np.array_equal(B[k], B[k].T)
    print(name, "field matrix vs the stencil: largest error / bound", worst)
    assert worst <= 1.0
    s.close()


def test_count_energy_and_argument_errors():
    import qchem_rs_amd as q
    m = load_system("water", "STO-3G")
    s = q.System(m)
    L = q.lib()
    INV, OK = q.hf.QC_ERR_INVALID, q.hf.QC_OK
    assert s.point_charge_count() == 0 and s.point_charge_nuclear_energy() == 0.0
    rng = np.random.default_rng(3)
    P, c = 3.0 * rng.standard_normal((17, 3)), rng.standard_normal(17)
    s.set_point_charges(P, c)
    R, Z = m.coordinates(), np.asarray(m.atomic_numbers(), float)
    want = ER.e_nq(R, Z, P, c)
    assert s.point_charge_count() == 17 and abs(s.point_charge_nuclear_energy() - want) <= 1e-13 * abs(want)
    assert s.n_electrons() == 10                                          # the charges are not atoms
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    setpc = ctypes.CFUNCTYPE(ctypes.c_int, vp, i64, vp, vp)(("qc_set_point_charges", L))
    h, p, qq = s.handle, P.ctypes.data, c.ctypes.data
    assert setpc(None, 17, p, qq) == INV and setpc(h, -1, p, qq) == INV and setpc(h, 17, None, qq) == INV and setpc(h, 17, p, None) == INV
    for bad in (np.nan, np.inf, -np.inf):
        P2, c2 = P.copy(), c.copy()
        P2[4, 1] = bad
        assert setpc(h, 17, P2.ctypes.data, qq) == INV
        c2[9] = bad
        assert setpc(h, 17, p, c2.ctypes.data) == INV
    P2 = P.copy()
    P2[16] = R[2]                                                       # a charge on an atom
    assert setpc(h, 17, P2.ctypes.data, qq) == INV
    assert s.point_charge_count() == 17 and abs(s.point_charge_nuclear_energy() - want) <= 1e-13 * abs(want)   # refused sets change nothing
    with pytest.raises(q.hf.QcError):
        s.set_point_charges(P, c[:5])
    out = np.zeros((3, s.n, s.n))
    fm = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, vp)(("qc_field_matrix", L))
    assert fm(None, p, out.ctypes.data) == INV and fm(h, None, out.ctypes.data) == INV and fm(h, p, None) == INV
    pm = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp)(("qc_point_charge_matrix", L))
    assert pm(None, out.ctypes.data) == INV and pm(h, None) == INV and pm(h, out.ctypes.data) == OK
    tm = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp)(("qc_point_charge_timings", L))
    assert tm(None, out.ctypes.data) == INV and tm(h, None) == INV
    assert np.array_equal(s.point_charge_timings(), np.zeros(4))
    assert setpc(h, 0, None, None) == OK and s.point_charge_count() == 0   # npc == 0 removes the set
    assert L.qc_point_charge_count(None) == INV
    s.close()


def test_gpu_entries_check_arguments_before_the_device():
    import qchem_rs_amd as q
    m = load_system("water", "STO-3G")
    s = q.System(m)
    L = q.lib()
    INV = q.hf.QC_ERR_INVALID
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    n = s.n
    D, P, out = np.zeros((2, n, n)), np.zeros((4, 3)) + 0.3, np.zeros(64)
    d, p, o = D.ctypes.data, P.ctypes.data, out.ctypes.data
    fld = ctypes.CFUNCTYPE(ci, vp, vp, i64, vp, vp, vp)(("qc_field_on_points", L))
    assert fld(None, d, 4, p, o, None) == INV and fld(s.handle, None, 4, p, o, None) == INV and fld(s.handle, d, 4, None, o, None) == INV
    assert fld(s.handle, d, 4, p, None, None) == INV and fld(s.handle, d, -1, p, o, None) == INV
    assert fld(s.handle, d, 0, p, o, None) == q.hf.QC_OK                  # an empty call: nothing launched, no device needed
    pg = ctypes.CFUNCTYPE(ci, vp, ci, vp, vp)(("qc_point_charge_gradient", L))
    assert pg(None, 1, d, o) == INV and pg(s.handle, 0, d, o) == INV and pg(s.handle, 3, d, o) == INV and pg(s.handle, 1, None, o) == INV
    assert pg(s.handle, 1, d, None) == INV
    assert pg(s.handle, 1, d, o) == q.hf.QC_OK and np.all(out == 0.0)     # no charges: nothing to do
    sf = ctypes.CFUNCTYPE(ci, vp, i64, vp, vp, vp)(("qc_scf_field_on_points", L))
    sg = ctypes.CFUNCTYPE(ci, vp, vp)(("qc_scf_point_charge_gradient", L))
    assert sf(None, 4, p, o, None) == INV and sg(None, o) == INV
    assert ctypes.CFUNCTYPE(ci, vp, vp)(("qc_point_charge_matrix_gpu", L))(None, o) == INV
    s.close()
