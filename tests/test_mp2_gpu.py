"""MP2 on the GPU (qc_mp2 / qc_scf_mp2 / qc_scf_coefficients) against a numpy restatement of the definitions on the oracle's ERI tensor:
the kernels alone on synthetic orbitals, RHF and UHF states, Crawford's published water MP2, the coefficients themselves, bitwise
reproducibility, a state left untouched, and the CLI end to end."""
import ctypes
import json

import numpy as np
import pytest

from conftest import data, load_system

pytestmark = pytest.mark.gpu

TOL = 1e-10


# ---- numpy checker: quarter transforms by tensordot, sums exactly as defined in include/qchem_hip.h ----------------------------------
def _ovov(I, Ci, Ca, Cj, Cb):
    T = np.tensordot(Ci, I, axes=(0, 0))          # (i, nu, la, si)
    T = np.tensordot(T, Ca, axes=(1, 0))          # (i, la, si, a)
    T = np.tensordot(T, Cj, axes=(1, 0))          # (i, si, a, j)
    T = np.tensordot(T, Cb, axes=(1, 0))          # (i, a, j, b)
    return T


def _den(eo1, ev1, eo2, ev2):
    return eo1[:, None, None, None] - ev1[None, :, None, None] + eo2[None, None, :, None] - ev2[None, None, None, :]


def ref_rmp2(I, C, eps, nocc, nf=0):
    o, v = C[:, nf:nocc], C[:, nocc:]
    W = _ovov(I, o, v, o, v)
    D = _den(eps[nf:nocc], eps[nocc:], eps[nf:nocc], eps[nocc:])
    Wx = W.transpose(0, 3, 2, 1)                  # (ib|ja)
    return float((W * W / D).sum()), float((W * (W - Wx) / D).sum())


def ref_ump2(I, Ca, Cb, ea, eb, na, nb, nf=0):
    """(e_os, e_ss alpha-alpha half, e_ss beta-beta half)"""
    def ss(C, e, no):
        if no - nf == 0 or no == C.shape[0]:
            return 0.0
        W = _ovov(I, C[:, nf:no], C[:, no:], C[:, nf:no], C[:, no:])
        return 0.5 * float((W * (W - W.transpose(0, 3, 2, 1)) / _den(e[nf:no], e[no:], e[nf:no], e[no:])).sum())
    e_os = 0.0
    if na > nf and nb > nf and na < Ca.shape[0] and nb < Cb.shape[0]:
        W = _ovov(I, Ca[:, nf:na], Ca[:, na:], Cb[:, nf:nb], Cb[:, nb:])
        e_os = float((W * W / _den(ea[nf:na], ea[na:], eb[nf:nb], eb[nb:])).sum())
    return e_os, ss(Ca, ea, na), ss(Cb, eb, nb)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _sys(mol, basis):
    import qchem_rs_amd as q
    return q.System(load_system(mol, basis))


def _oracle_eri(mol, basis):
    key = (mol, basis)
    if key not in _CACHE:
        import os
        from oracle.oracle import Oracle
        _CACHE.clear()                                # (before the next tensor exists: one at a time, 7.3 GB at n = 174)
        _CACHE[key] = Oracle(load_system(mol, basis)).eri_strided_mt(0, 1, min(16, len(os.sched_getaffinity(0))))[0]
    return _CACHE[key]


def _synthetic(n, nocc_list, seed):
    rng = np.random.default_rng(seed)
    Cs, es = [], []
    for no in nocc_list:
        Cs.append(np.linalg.qr(rng.standard_normal((n, n)))[0])
        es.append(np.r_[np.sort(rng.uniform(-3.0, -0.4, no)), np.sort(rng.uniform(0.1, 4.0, n - no))])
    return Cs, es


def _converge(st, eps, uhf=False, max_it=600):
    for _ in range(max_it):
        e, rms = st.iterate()
        if (rms / 2.0 if uhf else rms) < eps:
            return e
    raise AssertionError("SCF did not converge")


# ---- 1. kernels alone ---------------------------------------------------------------------------------------------------------------
CASES = [("STO-3G", 5, 0), ("STO-3G", 1, 0), ("STO-3G", 6, 0), ("STO-3G", 5, 1),
         ("6-31G_st_st", 5, 0), ("6-31G_st_st", 24, 0), ("6-31G_st_st", 5, 2), ("6-31G_st_st", 1, 0),
         ("cc-pVTZ", 5, 0), ("cc-pVTZ", 57, 3), ("cc-pVTZ", 1, 0), ("cc-pVTZ", 5, 1)]


@pytest.mark.parametrize("basis,nocc,nf", CASES)
def test_kernels_rhf_synthetic_orbitals(basis, nocc, nf):
    s = _sys("water", basis)
    I = _oracle_eri("water", basis)
    (C,), (e,) = _synthetic(s.n, [nocc], seed=nocc + 7 * nf)
    got = s.mp2(C, e, nocc, nf)
    e_os, e_ss = ref_rmp2(I, C, e, nocc, nf)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - e_ss) <= TOL, (got, e_os, e_ss)
    assert got.e_corr == got.e_os + got.e_ss and got.n_frozen == nf


UCASES = [("STO-3G", 5, 4, 0), ("STO-3G", 6, 1, 1), ("STO-3G", 3, 0, 0), ("6-31G_st_st", 5, 4, 1), ("6-31G_st_st", 24, 1, 0),
          ("cc-pVTZ", 6, 4, 0), ("cc-pVTZ", 57, 2, 2), ("cc-pVTZ", 1, 1, 0)]


@pytest.mark.parametrize("basis,na,nb,nf", UCASES)
def test_kernels_uhf_synthetic_orbitals(basis, na, nb, nf):
    s = _sys("water", basis)
    I = _oracle_eri("water", basis)
    (Ca, Cb), (ea, eb) = _synthetic(s.n, [na, nb], seed=na + 3 * nb + 11 * nf)
    got = s.mp2(np.stack([Ca, Cb]), np.stack([ea, eb]), [na, nb], nf)
    e_os, aa, bb = ref_ump2(I, Ca, Cb, ea, eb, na, nb, nf)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - (aa + bb)) <= TOL, (got, e_os, aa, bb)


# Above n = 64, against the oracle's tensor.  chloroform/6-31G** (n = 77, odd): every GEMM's B rows unaligned (the non-VEC loads);
# ethylene/cc-pVTZ (n = 116): the tensor of the VALU f-ket route; benzene/6-311++G** (n = 174): two 128-wide N tiles in steps 3 (N = n)
# and 4 (N = v >= 141) with their masked edges, the batched (b, nt) tiles of step 3, o = 16 / 17 on the edge of the second MFMA row band,
# o = 33 with a one-row second M tile, and both B alignments of step 4 (B = C + nocc: even and odd nocc).
BIG = [("chloroform", "6-31G_st_st", 77, (29,), 0), ("chloroform", "6-31G_st_st", 77, (29,), 5), ("chloroform", "6-31G_st_st", 77, (30, 28), 0),
       ("ethylene", "cc-pVTZ", 116, (8,), 2), ("ethylene", "cc-pVTZ", 116, (9, 7), 0),
       ("benzene", "6-311++G_st_st", 174, (16,), 0), ("benzene", "6-311++G_st_st", 174, (17,), 0),
       ("benzene", "6-311++G_st_st", 174, (21,), 6), ("benzene", "6-311++G_st_st", 174, (33,), 0),
       ("benzene", "6-311++G_st_st", 174, (22, 21), 0), ("benzene", "6-311++G_st_st", 174, (17, 16), 6)]


@pytest.mark.parametrize("mol,basis,n,nocc,nf", BIG)
def test_kernels_synthetic_orbitals_above_n64(mol, basis, n, nocc, nf):
    s = _sys(mol, basis)
    assert s.n == n
    if n == 174:
        assert n > 128 and n - max(nocc) > 128                    # two N tiles in steps 3 and 4
    I = _oracle_eri(mol, basis)
    Cs, es = _synthetic(n, nocc, seed=sum(nocc) + 13 * nf + n)
    if len(nocc) == 1:
        got = s.mp2(Cs[0], es[0], nocc[0], nf)
        e_os, e_ss = ref_rmp2(I, Cs[0], es[0], nocc[0], nf)
    else:
        got = s.mp2(np.stack(Cs), np.stack(es), list(nocc), nf)
        e_os, aa, bb = ref_ump2(I, Cs[0], Cs[1], es[0], es[1], nocc[0], nocc[1], nf)
        e_ss = aa + bb
    s.close()
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - e_ss) <= TOL, (got, e_os, e_ss)


def test_mp2_n174_is_bitwise_reproducible():
    s = _sys("benzene", "6-311++G_st_st")
    (C,), (e,) = _synthetic(s.n, [17], seed=3)
    m1, m2 = s.mp2(C, e, 17, 6), s.mp2(C, e, 17, 6)
    s.close()
    assert (m1.e_os, m1.e_ss, m1.e_corr) == (m2.e_os, m2.e_ss, m2.e_corr)


# ---- 2. RHF states ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol,basis,nf", [("water", "STO-3G", 0), ("water", "6-31G_st_st", 0), ("water", "cc-pVDZ", 0),
                                          ("water", "cc-pVTZ", 0), ("water", "cc-pVTZ", 1), ("ethylene", "cc-pVDZ", 0)])
def test_rhf_state_mp2_matches_numpy(mol, basis, nf):
    import qchem_rs_amd as q
    s = _sys(mol, basis)
    st = q.ScfStepper(s)
    _converge(st, 1e-10)
    got = st.mp2(nf)
    e_os, e_ss = ref_rmp2(_oracle_eri(mol, basis), st.coefficients(), st.orbital_energies(), s.n_electrons() // 2, nf)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - e_ss) <= TOL, (got, e_os, e_ss)
    st.close()


def test_rhf_state_mp2_benzene_ccpvdz_beyond_one_workgroup():
    import qchem_rs_amd as q
    s = _sys("benzene", "cc-pVDZ")
    assert s.n == 114
    st = q.ScfStepper(s)
    _converge(st, 1e-8)
    got = st.mp2(6)
    C, e = st.coefficients(), st.orbital_energies()
    st.close()
    e_os, e_ss = ref_rmp2(_oracle_eri("benzene", "cc-pVDZ"), C, e, 21, 6)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - e_ss) <= TOL, (got, e_os, e_ss)


def test_rhf_state_mp2_ethylene_ccpvtz():
    """A converged RHF state at n = 116 (f functions), two frozen core orbitals, against numpy on its own orbitals and the oracle's tensor."""
    import qchem_rs_amd as q
    s = _sys("ethylene", "cc-pVTZ")
    assert s.n == 116
    st = q.ScfStepper(s)
    _converge(st, 1e-8)
    got = st.mp2(2)
    C, e = st.coefficients(), st.orbital_energies()
    st.close()
    e_os, e_ss = ref_rmp2(_oracle_eri("ethylene", "cc-pVTZ"), C, e, s.n_electrons() // 2, 2)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - e_ss) <= TOL, (got, e_os, e_ss)


def test_uhf_state_mp2_triplet_ethylene_ccpvtz():
    """Triplet ethylene (n_alpha = 9, n_beta = 7) at n = 116 after 12 passes - not converged (see test_open_shell_passes_above_n64_match_oracle),
    but its orbitals are those of a pass, and both spins' highest occupied orbital lies below the lowest virtual one (qc_mp2_validate;
    gaps of 0.31 and 0.37 Eh) - against numpy on that state's coefficients and orbital energies."""
    import qchem_rs_amd as q
    s = _sys("ethylene", "cc-pVTZ")
    st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
    for _ in range(12):
        st.iterate()
    got = st.mp2()
    Ca, Cb, ea, eb = st.coefficients(0), st.coefficients(1), st.orbital_energies(0), st.orbital_energies(1)
    st.close()
    e_os, aa, bb = ref_ump2(_oracle_eri("ethylene", "cc-pVTZ"), Ca, Cb, ea, eb, 9, 7)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - (aa + bb)) <= TOL, (got, e_os, aa, bb)


# ---- 3. known answer ----------------------------------------------------------------------------------------------------------------
def test_crawford_water_sto3g_mp2():
    """T.D. Crawford's programming project #4: E_MP2 = -0.049149636120, E_total = -74.991229564312 Eh (all electrons)."""
    import qchem_rs_amd as q
    res = q.restricted_mp2(load_system("water_crawford", "STO-3G"), q.HartreeFockConfig(100, 1e-10))
    assert res is not None
    hf_out, mp2 = res
    assert abs(mp2.e_corr - (-0.049149636120)) < 1e-7
    assert abs(hf_out.total_energy() + mp2.e_corr - (-74.991229564312)) < 1e-7


# ---- 4. coefficients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol,basis,uhf,na,nb", [("water", "6-31G_st_st", False, 0, 0), ("benzene", "6-31G", False, 0, 0),
                                                 ("water", "6-31G_st_st", True, 5, 4)])
def test_coefficients_are_the_states_orbitals(mol, basis, uhf, na, nb):
    import qchem_rs_amd as q
    s = _sys(mol, basis)
    st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
    _converge(st, 1e-10 if not uhf else 1e-9, uhf)
    S = st.matrix("S")
    nocc = [na, nb] if uhf else [s.n_electrons() // 2]
    for spin, no in enumerate(nocc):
        C = st.coefficients(spin)
        O = np.abs(C.T @ S @ C - np.eye(s.n))
        # (above n = 64 the orbitals carry the stopping tolerance of that path's eigensolver: measured on benzene/6-31G, 2.5e-10 between
        # occupied and virtual orbitals, 2e-8 among the highest virtuals)
        assert O[:no, :].max() < (1e-10 if s.n <= 64 else 1e-9)      # the occupied orbitals: orthonormal, orthogonal to every virtual
        assert O.max() < (1e-10 if s.n <= 64 else 1e-7)
        D = (1.0 if uhf else 2.0) * C[:, :no] @ C[:, :no].T
        assert np.abs(D - st.density(spin)).max() < 1e-12
        w = st.orbital_energies(spin)
        assert np.all(np.diff(w) >= 0)
    st.close()


# ---- 5. UHF -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mol,basis,na,nb,eps", [("water", "6-31G_st_st", 5, 4, 1e-10), ("oxygen", "cc-pVDZ", 9, 7, 1e-10)])
def test_uhf_state_mp2_matches_numpy(mol, basis, na, nb, eps):
    import qchem_rs_amd as q
    s = _sys(mol, basis)
    st = q.ScfStepper(s, uhf=True, n_alpha=na, n_beta=nb)
    _converge(st, eps, True, max_it=1000)
    got = st.mp2()
    e_os, aa, bb = ref_ump2(_oracle_eri(mol, basis), st.coefficients(0), st.coefficients(1), st.orbital_energies(0),
                            st.orbital_energies(1), na, nb)
    assert abs(got.e_os - e_os) <= TOL and abs(got.e_ss - (aa + bb)) <= TOL, (got, e_os, aa, bb)
    st.close()


def test_closed_shell_uhf_equals_rhf():
    import qchem_rs_amd as q
    s = _sys("water", "6-31G_st_st")
    r = q.ScfStepper(s)
    _converge(r, 1e-10)
    rm = r.mp2()
    r.close()
    u = q.ScfStepper(s, uhf=True)
    _converge(u, 1e-10, True)
    um = u.mp2()
    assert abs(um.e_os - rm.e_os) <= TOL and abs(um.e_ss - rm.e_ss) <= TOL, (um, rm)
    # the same-spin halves: each spin alone (the other one empty)
    C = np.stack([u.coefficients(0), u.coefficients(1)])
    e = np.stack([u.orbital_energies(0), u.orbital_energies(1)])
    u.close()
    aa = s.mp2(C, e, [5, 0]).e_ss
    bb = s.mp2(C, e, [0, 5]).e_ss
    assert abs(aa - bb) <= TOL and abs(aa + bb - rm.e_ss) <= TOL, (aa, bb, rm.e_ss)


# ---- 6. reproducible, non-intrusive, single GPU -------------------------------------------------------------------------------------
def test_mp2_is_bitwise_reproducible_and_leaves_the_state_alone():
    import qchem_rs_amd as q
    s1, s2 = _sys("water", "cc-pVDZ"), _sys("water", "cc-pVDZ")
    a, b = q.ScfStepper(s1), q.ScfStepper(s2)
    for _ in range(5):
        assert a.iterate() == b.iterate()
    m1, m2 = a.mp2(), a.mp2()
    assert (m1.e_os, m1.e_ss, m1.e_corr) == (m2.e_os, m2.e_ss, m2.e_corr)
    for _ in range(3):
        assert a.iterate() == b.iterate()
    a.close(); b.close()


def test_mp2_on_a_sharded_handle_is_unsupported():
    import qchem_rs_amd as q
    s = _sys("water", "STO-3G")
    q.lib().qc_set_shard(s.handle, 0, 2)
    C = np.linalg.qr(np.random.default_rng(0).standard_normal((s.n, s.n)))[0]
    e = np.r_[np.linspace(-2, -1, 5), np.linspace(1, 2, 2)]
    with pytest.raises(q.QcError, match="unsupported"):
        s.mp2(C, e, 5)


def test_scf_mp2_before_the_first_pass_is_invalid():
    import qchem_rs_amd as q
    s = _sys("water", "STO-3G")
    st = q.ScfStepper(s)
    o = q.hf._Mp2Output()
    assert q.lib().qc_scf_mp2(st._st, 0, ctypes.byref(o)) == q.hf.QC_ERR_INVALID
    st.iterate()
    assert q.lib().qc_scf_mp2(st._st, 0, ctypes.byref(o)) == q.hf.QC_OK
    st.close()


# ---- 7. CLI end to end --------------------------------------------------------------------------------------------------------------
def test_cli_rhf_mp2_end_to_end(capsys):
    from qchem_rs_amd import cli
    B, M = data("basis", "STO-3G.json"), data("mol", "water_crawford.json")
    assert cli.main(["rhf", "-b", B, "-m", M, "--epsilon", "1e-10"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert cli.main(["rhf", "-b", B, "-m", M, "--epsilon", "1e-10", "--mp2"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].rsplit(" and ", 1)[0] == plain[0].rsplit(" and ", 1)[0]      # iterations; the elapsed time differs
    assert lines[1:len(plain)] == plain[1:]
    assert lines[len(plain):] == ["mp2 correlation energy: -0.049", "mp2 total energy: -74.991"]


def test_cli_uhf_mp2_triplet_json(capsys):
    from qchem_rs_amd import cli
    B, M = data("basis", "cc-pVDZ.json"), data("mol", "oxygen.json")
    assert cli.main(["uhf", "-b", B, "-m", M, "-s", "3", "--mp2", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert any(l.startswith("<S^2>: ") for l in lines)
    assert lines[-3].startswith("mp2 correlation energy: ") and lines[-2].startswith("mp2 total energy: ")
    doc = json.loads(lines[-1])
    m = doc["mp2"]
    assert m["e_corr"] < 0 and m["e_os"] < 0 and m["n_frozen"] == 0
    assert m["e_corr"] == m["e_os"] + m["e_ss"] and abs(m["e_total"] - (doc["total_energy"] + m["e_corr"])) < 1e-12
    assert set(m["timings_ms"]) == {"tensor", "transform", "energy"}
