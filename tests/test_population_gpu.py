"""GPU tests of the population analysis (qc_scf_populations, qc_populations): Mulliken charges with Mayer bond orders, Loewdin charges with
Wiberg indices, against the numpy reference of tests/multipole_reference.py built from the library's own S (st.matrix) and densities.

States: water/cc-pVDZ RHF, O2/cc-pVDZ UHF (9, 7), H2O+/cc-pVDZ UHF (5, 4), chloroform/6-31G** RHF (n = 77, not a multiple of the 16-wide
GEMM tile; five atoms with 2 to 19 functions each) and ethylene/6-31G (six atoms), converged to 1e-8.

Bounds: Mulliken and Mayer 1e-12 (1 + sum |P_ab| |S_ab|) - f64 sums of that magnitude; Loewdin and Wiberg
min(1e-8, 1e-13 cond(S) N_electrons) - S^1/2 = S X inherits the conditioning of X = S^-1/2, the reference takes square roots of the
eigenvalues of S directly.  The sum rules (sum q = charge, sum spin = n_alpha - n_beta, sum_B B_AB = 2 N_A for an idempotent determinant, orbital
populations summing to N_A) are held to the same bounds.

Measured on an MI355X (largest ratio to the bound; state call / host-density call / sum rule sum_B B_AB = 2 N_A):
  Mulliken, Mayer   water 5.7e-5 / 5.7e-5 / 0.091   O2 7.2e-5 / 7.2e-5 / 1.6e-3   H2O+ 1.4e-5 / 1.4e-5 / 7.1e-4   chloroform 4.1e-5 / 4.1e-5 / 0.16
                    ethylene 8.5e-5 / 8.5e-5 / 0.030
  Loewdin, Wiberg   water 6.3e-3 / 6.3e-3 / 2.6e-3  O2 1.8e-4 / 0.015 / 6.5e-3    H2O+ 1.5e-5 / 7.2e-3 / 2.3e-3   chloroform 0.012 / 0.012 / 7.3e-3
                    ethylene 3.7e-3 / 3.7e-3 / 1.2e-3
The largest is the Mayer sum rule of chloroform, 0.16 of its bound of 8.6e-11; the Loewdin bounds run from 5.0e-10 (O2) to the cap 1e-8
(chloroform).  The state call and the host-density call agree bit for bit on the closed shells and to 0.015 of the Loewdin bound on
the open shells, whose state built its X with another eigensolver."""
import numpy as np
import pytest

import multipole_reference as MR
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu

STATES = {"water": ("water/cc-pVDZ", False, 5, 5, 0), "oxygen": ("oxygen/cc-pVDZ", True, 9, 7, 0), "water+": ("water/cc-pVDZ", True, 5, 4, 1),
          "chloroform": ("chloroform/6-31G_st_st", False, 29, 29, 0), "ethylene": ("ethylene/6-31G", False, 8, 8, 0)}


@pytest.mark.parametrize("kind", list(STATES))
def test_populations_and_bond_orders_match_the_reference(kind):
    import qchem_rs_amd as q
    name, uhf, na, nb, charge = STATES[kind]
    s, st, _ = converged(name, uhf, na if uhf else 0, nb if uhf else 0, eps=1e-8, schwarz0=False)
    try:
        m = s.mol
        S = st.matrix("S")
        Pa, Pb = (st.density(0), st.density(1)) if uhf else (0.5 * st.density(0), 0.5 * st.density(0))
        nel = na + nb
        fa = MR.function_atoms(m)
        bounds = {"mulliken": 1e-12 * (1.0 + float(np.sum(np.abs(Pa + Pb) * np.abs(S)))),
                  "lowdin": min(1e-8, 1e-13 * float(np.linalg.cond(S)) * nel)}
        for scheme in ("mulliken", "lowdin"):
            b = bounds[scheme]
            qr, sr, orr, br = MR.populations(m, scheme, Pa, Pb, S)
            r = st.populations(scheme, bond_orders=True)
            h = s.populations(st.density(0), scheme, Db=st.density(1) if uhf else None, bond_orders=True)
            errs = {}
            for tag, got in (("state", r), ("host", h)):
                errs[tag] = max(float(np.abs(got.charges - qr).max()), float(np.abs(got.spin - sr).max()), float(np.abs(got.orbital - orr).max()),
                                float(np.abs(got.bond_orders - br).max()))
                assert errs[tag] <= b, (kind, scheme, tag, errs[tag], b)
                assert np.array_equal(got.bond_orders, got.bond_orders.T)
                assert abs(got.charges.sum() - charge) <= b and abs(got.spin.sum() - (na - nb)) <= b
                if not uhf:
                    assert np.array_equal(got.spin, np.zeros(len(m.atoms)))
                N = np.asarray(m.atomic_numbers(), float) - got.charges
                idem = float(np.abs(got.bond_orders.sum(axis=1) - 2.0 * N).max())                       # idempotency of the determinant
                errs[tag + "-idem"] = idem
                assert idem <= b, (kind, scheme, tag, idem, b)
                assert np.abs(np.array([got.orbital[fa == a].sum() for a in range(len(m.atoms))]) - N).max() <= b
            d = max(float(np.abs(h.charges - r.charges).max()), float(np.abs(h.bond_orders - r.bond_orders).max()), float(np.abs(h.orbital - r.orbital).max()))
            assert d <= b
            # equal bits twice, and on a fresh handle
            r2 = st.populations(scheme, bond_orders=True)
            for x, y in ((r.charges, r2.charges), (r.spin, r2.spin), (r.orbital, r2.orbital), (r.bond_orders, r2.bond_orders)):
                assert x.tobytes() == y.tobytes()
            s2 = q.System(m)
            try:
                h2 = s2.populations(st.density(0), scheme, Db=st.density(1) if uhf else None, bond_orders=True)
                for x, y in ((h.charges, h2.charges), (h.spin, h2.spin), (h.orbital, h2.orbital), (h.bond_orders, h2.bond_orders)):
                    assert x.tobytes() == y.tobytes()
            finally:
                s2.close()
            # without the bond orders the charges are the same bits
            assert st.populations(scheme).charges.tobytes() == r.charges.tobytes()
            print(kind, scheme, "n", s.n, "bound", b, "state / bound", errs["state"] / b, "host-density / bound", errs["host"] / b, "state vs host-density / bound", d / b,
                  "sum rule / bound", max(errs["state-idem"], errs["host-idem"]) / b, "charges", r.charges)
    finally:
        st.close(); s.close()
