"""GPU tests of the ESP-fitted charges of an SCF state (qc_scf_esp_charges) on water/cc-pVDZ RHF, H2O+/cc-pVDZ UHF (5, 4) and
ethylene/6-31G RHF: the potential is the V of qc_scf_esp_on_points bit for bit (the library's grid and a caller's 300 points), the
charges are qc_esp_fit_solve of that V bit for bit and match the numpy KKT fit (tests/multipole_reference.py) to
100 x 2.2e-16 x cond(A^T A) x max(1, max|q|); rms, rrms and the dipole of the charges equal their numpy values to 1e-12 x scale.

Measured on an MI355X (|q - q_numpy| over its bound; library grid / own 300 points): water 5.2e-4 / 7.0e-4 (344 points, cond 546 / 279),
H2O+ 2.5e-3 / 0.012, ethylene 7.6e-3 / 7.1e-5 (546 points, cond 9027 / 1924)."""
import numpy as np
import pytest

import multipole_reference as MR
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu

STATES = {"water": ("water/cc-pVDZ", False, 0, 0, 0), "water+": ("water/cc-pVDZ", True, 5, 4, 1), "ethylene": ("ethylene/6-31G", False, 0, 0, 0)}


def _own_points(xyz):
    """300 points, normal with sigma = 3 bohr around the centroid, none closer than 2 bohr to a nucleus"""
    rng = np.random.default_rng(300)
    P = xyz.mean(axis=0) + 3.0 * rng.standard_normal((4000, 3))
    P = P[np.linalg.norm(P[:, None, :] - xyz[None, :, :], axis=2).min(axis=1) >= 2.0]
    assert len(P) >= 300
    return np.ascontiguousarray(P[:300])


@pytest.mark.parametrize("kind", list(STATES))
def test_esp_charges_are_the_fit_of_the_state_potential(kind):
    name, uhf, na, nb, charge = STATES[kind]
    s, st, _ = converged(name, uhf, na, nb, eps=1e-8, schwarz0=False)
    try:
        m = s.mol
        xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
        own = _own_points(xyz)
        for points in (None, own):
            r = st.esp_charges(points)
            P = s.esp_fit_points() if points is None else own
            assert np.array_equal(r.points, P) and len(P) >= 300
            assert r.potential.tobytes() == st.esp_on_points(P).tobytes()
            fit = s.esp_fit_solve(P, r.potential, charge)
            assert r.charges.tobytes() == fit.charges.tobytes() and (r.rms, r.rrms) == (fit.rms, fit.rrms) and np.array_equal(r.dipole, fit.dipole)
            qn, rms, rrms, dip, cond = MR.kkt_fit(m, P, r.potential, charge)
            bound = 100.0 * 2.2e-16 * cond * max(1.0, float(np.abs(qn).max()))
            err = float(np.abs(r.charges - qn).max())
            vmax = float(np.abs(r.potential).max())
            print(kind, "library grid" if points is None else "own points", len(P), "charges", r.charges, "cond", cond, "|q - q_numpy| / bound", err / bound,
                  "rms", r.rms, "rrms", r.rrms, "dipole", r.dipole, "ms", r.ms_total, r.ms_potential)
            assert err <= bound
            assert abs(r.charges.sum() - charge) <= 1e-12 and r.total_charge == charge
            # rms: a root mean square of residuals of size up to vmax, with charges good to `bound`
            assert abs(r.rms - rms) <= 1e-12 * max(1.0, vmax) and abs(r.rrms - rrms) <= 1e-12 * max(1.0, rrms)
            assert np.abs(r.dipole - dip).max() <= 1e-12 * max(1.0, float(np.abs(xyz).max()) * float(np.abs(qn).sum()))
            r2 = st.esp_charges(points)
            assert r2.charges.tobytes() == r.charges.tobytes() and r2.potential.tobytes() == r.potential.tobytes()
        r = st.esp_charges(scales=[1.5, 2.5], density=0.5)
        assert np.array_equal(r.points, s.esp_fit_points([1.5, 2.5], 0.5)) and r.potential.tobytes() == st.esp_on_points(r.points).tobytes()
    finally:
        st.close(); s.close()
