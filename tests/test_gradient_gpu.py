"""Analytic nuclear gradients on the GPU (qc_gradient / qc_scf_gradient): each term against a central finite difference of the
oracle's CPU integrals at fixed densities, the total against finite differences of converged GPU SCF energies, the invariants
(translation, rotation, closed-shell UHF = RHF, screening), reproducibility, an untouched state, and the CLI end to end."""
import json
import numpy as np
import pytest

from conftest import data
from synthetic_systems import H, check_terms as _check_terms, displaced as _displaced, rand_sym as _rand_sym

pytestmark = pytest.mark.gpu


def _load(mol, basis, basis_path=None):
    import qchem_rs_amd as q
    b = q.BasisSet.load(basis_path or data("basis", basis + ".json"))
    return q.MolecularSystem.load(data("mol", mol + ".json"), b)


def _cart_basis(tmp_path):
    b = json.load(open(data("basis", "cc-pVTZ.json")))
    for el in b["elements"].values():
        for sh in el["electron_shells"]:
            if sh["angular_momentum"][0] >= 2:
                sh["function_type"] = "gto_cartesian"
    f = tmp_path / "cc-pVTZ-cart.json"
    f.write_text(json.dumps(b))
    return str(f)


def _converged(s, uhf=False, na=0, nb=0, eps=1e-10, maxit=1000):
    import qchem_rs_amd as q
    st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
    for _ in range(maxit + 1):
        e, rms = st.iterate()
        if (rms / 2.0 if uhf else rms) < eps:
            return st, e
    st.close()
    raise AssertionError("SCF did not converge")


def _rhf_pw(st):
    """P (qc_fock_rhf convention) and W of an RHF state, from its coefficients and orbital energies"""
    n = st.system.n
    nocc = st.system.n_electrons() // 2
    Cm, e = st.coefficients(0), st.orbital_energies(0)
    Co = Cm[:, :nocc]
    return st.density(0), 2.0 * (Co * e[:nocc]) @ Co.T


SYSTEMS = [("STO-3G", None, "all"), ("6-31G_st_st", None, "all"), ("cc-pVDZ", None, "all"), ("cc-pVTZ", None, "few"), ("cc-pVTZ", "cart", "few")]


@pytest.mark.parametrize("basis,variant,which", SYSTEMS, ids=["sto3g", "631gss", "ccpvdz", "ccpvtz", "ccpvtz-cart"])
def test_terms_match_oracle_finite_differences(basis, variant, which, tmp_path):
    import qchem_rs_amd as q
    m = _load("water", basis, _cart_basis(tmp_path) if variant else None)
    s = q.System(m)
    s.set_schwarz(0.0)
    coords = [(a, k) for a in range(3) for k in range(3)] if which == "all" else [(0, 2), (1, 0), (2, 1)]
    # SCF densities: P and the energy-weighted W of a converged RHF state
    st, _ = _converged(s)
    P, W = _rhf_pw(st)
    st.close()
    _check_terms(s, m, coords, P, 0.5 * P, 0.5 * P, W, 1)
    # one random symmetric UHF pair (Da != Db) with a random W
    Da, Db, Wr = _rand_sym(s.n, 1), _rand_sym(s.n, 2), _rand_sym(s.n, 3)
    _check_terms(s, m, coords[:3], Da + Db, Da, Db, Wr, 2)


def _energy(m, uhf=False, na=0, nb=0, eps=1e-10, variational=False):
    import qchem_rs_amd as q
    s = q.System(m)
    s.set_schwarz(0.0)
    st, e = _converged(s, uhf, na, nb, eps)
    if variational:          # energy of the final density (not the stale-G energy the pass reports)
        H = s.kinetic() + s.nuclear()
        if uhf:
            Da, Db = st.density(0), st.density(1)
            Ga, Gb = s.fock_uhf(Da, Db)
            e = 0.5 * np.sum(Da * (2 * H + Ga)) + 0.5 * np.sum(Db * (2 * H + Gb))
        else:
            D = st.density(0)
            e = 0.5 * np.sum(D * (2 * H + s.fock_rhf(D)))
    st.close()
    return e + s.nuclear_repulsion()


def _analytic(m, uhf=False, na=0, nb=0, eps=1e-10):
    import qchem_rs_amd as q
    s = q.System(m)
    s.set_schwarz(0.0)
    st, _ = _converged(s, uhf, na, nb, eps)
    g = st.gradient()
    st.close()
    return g


# UHF: the H2O+ doublet (n_alpha = 5, n_beta = 4) in 6-31G**, converged to epsilon = 1e-10 like the RHF cases (the reference's DIIS(2, 8)
# takes 80-200 passes on it, hence the pass cap of 1000).  Every coordinate but one: with the hydrogen atom 1 moved along z by -2h or +h
# the run does not reach 1e-10 in 1000 passes (smallest rms/2 seen: 3.1e-10 and 1.2e-10), so (1, z) is left out.  The energies are
# those of the final densities: the one a pass reports is built with the previous pass's G, first order in the last density change,
# and the stencil's 1.5 / h amplifies that to a few 1e-7 Eh/bohr.
@pytest.mark.parametrize("mol,basis,uhf", [("water", "cc-pVDZ", False), ("water", "cc-pVTZ", False), ("water", "6-31G_st_st", True)],
                         ids=["rhf-dz", "rhf-tz", "uhf-h2o-cation"])
def test_scf_gradient_matches_energy_finite_differences(mol, basis, uhf):
    m = _load(mol, basis)
    na, nb = (5, 4) if uhf else (0, 0)
    g = _analytic(m, uhf, na, nb)
    coords = [(0, 2), (1, 0), (1, 2), (2, 1)] if basis == "cc-pVTZ" else [(a, k) for a in range(3) for k in range(3)]
    if uhf:
        coords.remove((1, 2))
    for atom, axis in coords:
        e = {k: _energy(_displaced(m, atom, axis, k * H), uhf, na, nb, variational=True) for k in (-2, -1, 1, 2)}
        fd = (e[-2] - 8 * e[-1] + 8 * e[1] - e[2]) / (12 * H)
        assert abs(g[atom, axis] - fd) <= 1e-7, (atom, axis, g[atom, axis], fd)


def test_benzene_scf_gradient_matches_energy_finite_differences():
    m = _load("benzene", "cc-pVDZ")
    g = _analytic(m, eps=1e-8)
    for atom, axis in [(0, 0), (1, 1), (7, 2)]:
        e = {k: _energy(_displaced(m, atom, axis, k * H), eps=1e-8, variational=True) for k in (-2, -1, 1, 2)}
        fd = (e[-2] - 8 * e[-1] + 8 * e[1] - e[2]) / (12 * H)
        assert abs(g[atom, axis] - fd) <= 1e-6, (atom, axis, g[atom, axis], fd)


def test_invariants():
    import qchem_rs_amd as q
    m = _load("water", "cc-pVDZ")
    s = q.System(m)
    st, _ = _converged(s)
    g = st.gradient()
    st.close()
    R = m.coordinates().reshape(-1, 3)
    assert np.abs(g.sum(axis=0)).max() <= 1e-10
    assert np.abs(np.cross(R, g).sum(axis=0)).max() <= 1e-9
    # closed-shell UHF equals RHF
    stu, _ = _converged(s, True, 5, 5)
    gu = stu.gradient()
    stu.close()
    assert np.abs(gu - g).max() <= 1e-10
    # default screening against none
    s0 = q.System(m)
    s0.set_schwarz(0.0)
    st0, _ = _converged(s0)
    g0 = st0.gradient()
    st0.close()
    assert np.abs(g0 - g).max() <= 1e-9


def test_reproducible_and_state_untouched():
    import qchem_rs_amd as q
    m = _load("water", "cc-pVDZ")
    s = q.System(m)
    st, _ = _converged(s, eps=1e-6)
    g1, g2 = st.gradient(), st.gradient()
    assert np.array_equal(g1, g2)
    # the P used is qc_scf_density's: the fixed-density form from that P and the same W gives the same numbers
    P, W = _rhf_pw(st)
    t = s.gradient(P, W)
    assert np.abs(sum(t) - g1).max() <= 1e-12
    # a state that computed a gradient continues bit for bit like one that did not
    s2 = q.System(m)
    st2, _ = _converged(s2, eps=1e-6)
    assert np.array_equal(st2.gradient(), g1)                 # fresh handle: bitwise identical
    a = [st.iterate() for _ in range(2)]
    s3 = q.System(m)
    st3, _ = _converged(s3, eps=1e-6)
    b = [st3.iterate() for _ in range(2)]
    assert a == b and np.array_equal(st.density(0), st3.density(0))
    # fixed-density calls repeat bitwise too
    t2 = s.gradient(P, W)
    assert all(np.array_equal(x, y) for x, y in zip(t, t2))
    for x in (st, st2, st3):
        x.close()


def test_errors_on_device():
    import ctypes as C
    import qchem_rs_amd as q
    from qchem_rs_amd.hf import QC_ERR_INVALID, QC_ERR_UNSUPPORTED
    m = _load("water", "STO-3G")
    s = q.System(m)
    st = q.ScfStepper(s)
    g = np.zeros((3, 3))
    assert q.lib().qc_scf_gradient(st._st, g) == QC_ERR_INVALID
    st.close()
    # a sharded handle: both entry points
    s2 = q.System(m)
    st2, _ = _converged(s2, eps=1e-6)
    s2.set_shard(0, 2)
    assert q.lib().qc_scf_gradient(st2._st, g) == QC_ERR_UNSUPPORTED
    st2.close()
    s.set_shard(0, 2)
    n = s.n
    D, W, t = np.zeros((n, n)), np.zeros((n, n)), np.zeros(4 * 9)
    assert q.lib().qc_gradient(s.handle, 1, D, W, t) == QC_ERR_UNSUPPORTED


@pytest.mark.parametrize("cmd", ["rhf", "uhf"])
def test_cli_gradient_end_to_end(cmd, capsys):
    import qchem_rs_amd as q
    from qchem_rs_amd import cli
    args = [cmd, "-b", data("basis", "cc-pVDZ.json"), "-m", data("mol", "water.json"), "--epsilon", "1e-10"]
    assert cli.main(args) == 0
    plain = capsys.readouterr().out.splitlines()
    assert cli.main(args + ["--gradient"]) == 0
    withg = capsys.readouterr().out.splitlines()
    # the reference's lines are unchanged (the first one carries the wall time), then one line per atom
    assert withg[0].split(" and ")[0] == plain[0].split(" and ")[0] and withg[1:len(plain)] == plain[1:]
    rows = withg[len(plain):]
    m = _load("water", "cc-pVDZ")
    assert len(rows) == 3 and rows[0].split()[:2] == ["0", str(m.atoms[0].ordinal)]
    assert cli.main(args + ["--gradient", "--json"]) == 0
    g = np.array(json.loads(capsys.readouterr().out.strip().splitlines()[-1])["gradient"])
    s = q.System(m)
    st, _ = _converged(s, uhf=cmd == "uhf")
    assert np.abs(g - st.gradient()).max() <= 1e-12
    st.close()
