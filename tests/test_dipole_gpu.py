"""GPU tests of the dipole kernel (qc_dipole_matrices_gpu) and of the dipole moment of an SCF state (qc_scf_dipole).

Matrices: against the host routine to 1e-12 max(1, max|M|) - the margin of the S/T/V host-versus-oracle test - on the four systems of
tests/test_dipole_host.py (every pair of s..f shells, pure and Cartesian, no centre on an axis, 169 primitive pairs in one shell pair),
and with a non-zero origin against the numpy reference (tests/dipole_reference.py).  Moments: against Z.R - tr(P M_ref) formed in numpy
from qc_scf_density, to 1e-10.

Measured on an MI355X: |M_gpu - M_host| 8.9e-16 (tetra-pure-2), 4.4e-16 (tetra-cart-1), 6.7e-16 (deep), 3.3e-16 (water/cc-pVTZ);
|M_gpu(O) - M_ref(O)| 9.6e-16, 2.3e-15, 4.4e-16, 5.6e-16; moments against the numpy trace: 1e-15 (water, |mu| = 0.924 e bohr) and 2e-15 (O2)."""
import numpy as np
import pytest

from conftest import load_system
import dipole_reference as D
from test_dipole_host import ORIGIN, SYSTEMS
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_gpu_dipole_matrices_match_the_host_and_the_reference(name):
    import qchem_rs_amd as q
    m = SYSTEMS[name]()
    s = q.System(m)
    try:
        Mh, Mg = s.dipole_matrices(), s.dipole_matrices(gpu=True)
        scale = max(1.0, float(np.abs(Mh).max()))
        d = float(np.abs(Mg - Mh).max())
        _, Mref = D.overlap_and_dipole(m, ORIGIN)
        MgO = s.dipole_matrices(ORIGIN, gpu=True)
        dO = float(np.abs(MgO - Mref).max())
        print(name, "|M_gpu - M_host|", d, "|M_gpu(O) - M_ref(O)|", dO, "scale", scale)
        assert d <= 1e-12 * scale and dO <= 1e-12 * max(1.0, float(np.abs(Mref).max()))
        assert np.array_equal(Mg, Mg.transpose(0, 2, 1)) and np.array_equal(MgO, MgO.transpose(0, 2, 1))
        assert np.array_equal(Mg, s.dipole_matrices(gpu=True))
    finally:
        s.close()


@pytest.mark.parametrize("name,uhf,na,nb", [("water/cc-pVDZ", False, 0, 0), ("oxygen/cc-pVDZ", True, 9, 7)])
def test_scf_dipole_is_the_trace_with_the_reference_matrices(name, uhf, na, nb):
    s, st, _ = converged(name, uhf, na, nb, eps=1e-8, schwarz0=False)
    try:
        m = load_system(*name.split("/"))
        P = st.density(0) + (st.density(1) if uhf else 0.0)
        for origin in (None, ORIGIN):
            O = np.zeros(3) if origin is None else origin
            _, M = D.overlap_and_dipole(m, O)
            ref_nuc = D.nuclear_dipole(m, O)
            ref = ref_nuc - np.array([np.sum(P * M[k]) for k in range(3)])
            mu, nuc = st.dipole(origin, nuclear=True)
            print(name, "origin", O, "mu", mu, "reference", ref, "nuclear", nuc)
            assert np.abs(mu - ref).max() <= 1e-10 and np.abs(nuc - ref_nuc).max() <= 1e-12
            assert np.array_equal(mu, st.dipole(origin))                 # two calls: the same bits
        # a neutral molecule: the moment does not depend on the origin
        assert np.abs(st.dipole(ORIGIN) - st.dipole()).max() <= 1e-10
    finally:
        st.close(); s.close()


def test_h2_has_no_dipole_moment():
    s, st, _ = converged("h2@1.4", eps=1e-10)
    try:
        for origin in (None, ORIGIN):
            mu = st.dipole(origin)
            print("h2", origin, mu)
            assert np.linalg.norm(mu) <= 1e-10
    finally:
        st.close(); s.close()
