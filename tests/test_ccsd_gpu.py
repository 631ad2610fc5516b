"""GPU tests of the closed-shell CCSD (qc_scf_ccsd) and of the split-k GEMM (qc_gemm_splitk through qc_debug_gemm) against the
spin-orbital numpy reference of tests/ccsd_reference.py, built from qc_eri_full and the state's own C and orbital energies.

Cases (n, o, v), each the smallest that reaches what it names:
  h2@1.4/6-31G            4,  1,  3   one occupied pair; every tile partial; o^2 = 1 row through split-k
  water_crawford/STO-3G   7,  5,  2   odd n; v = 2; the published number
  water/6-31G            13,  5,  8   frozen core 0 and 1
  water/cc-pVDZ          24,  5, 19   v^2 = 361: k and n of the ladder not multiples of 16 or 4; several k slices
  benzene/STO-3G         36, 21, 15   o > 16: a second row of MFMA tiles; o^2 = 441 rows
  water/cc-pVTZ-cut      38,  5, 33   v one past a 32-tile of the permute kernel; v^2 = 1089
States are converged to 1e-10 without Schwarz screening; both sides iterate to tol = 1e-10 on max |t_new - t_old|, and the iteration
counts compared are those.  The reference has no DIIS and converges linearly, at a rate of 0.8 on benzene/STO-3G (92 passes): stopped
at a change of tol it would still be 4 tol from its fixed point.  It therefore goes on until its own estimate of that distance,
change rho / (1 - rho), is below tol / 10 (ccsd_reference.ccsd, polish), which keeps the factor 2 below honest.  A reference is computed
once per module.

Bars.  u = 2^-53.  dI = 8 n u Emax bounds the rounding of any MO integral of the quarter chain (Emax the largest element of
the four-index transform of |I| with |C|).  One element of a residual is the bare integral plus at most 16 contractions, each a sum over
at most N^2 products of one integral with amplitudes of magnitude <= tmax, so the integrals' rounding moves it by at most
W dI, W = 1 + 16 N^2 tmax, and an amplitude by W dI / gap with gap the smallest denominator.  An iteration stopped at a change <= tol is
within tol rho / (1 - rho) <= tol of its fixed point for a contraction rate rho <= 1/2, on either side; the same factor 1 / (1 - rho) <= 2
carries the integral term:
  amplitudes   |t - t_ref| <= min(1e-8, 2 tol + 2 W dI / gap): the rounding term is a worst case over signs and grows with Emax, which
               the diffuse virtual orbitals of the larger bases drive up (dI = 6e-7 on water/cc-pVTZ-cut); it is cut off at 1e-8, the
               scale of the energy's cap and of the bar on max |t1| and max |t2|
  energy       |E - E_ref| <= min(1e-8, sum|L| (2 tol + 2 W dI / gap) + 3 dI sum|tau|),  L = 2 (ia|jb) - (ib|ja)
  diagnostics  1e-8; e_mp2 against qc_scf_mp2 1e-12; the published CCSD energy of water_crawford/STO-3G 1e-8
  split-k      |C - C_numpy| <= 4 k u (|alpha| |A| |B| + |beta| |C0|) elementwise, and bitwise equal from call to call
  DIIS         the library (DIIS of 8) needs no more iterations than the DIIS-free reference to the same tol

Measured on the MI355X (tol = 1e-10; iterations: library with DIIS of 8 / reference without, to the same tol):
  case                    E - E_ref   max|dt1|  max|dt2|  e_mp2 - qc_scf_mp2  iterations  amplitude bar  energy bar
  h2@1.4/6-31G            -6.2e-12    8.0e-12   4.2e-11   0                   15 / 22     2.2e-10        1.1e-10
  water_crawford/STO-3G   -5.3e-12    4.3e-11   6.5e-11   0                   13 / 33     2.0e-10        3.1e-10
  water/6-31G              1.3e-13    2.1e-11   1.6e-11   0                   13 / 26     7.2e-9         1e-8
  water/6-31G, 1 frozen   -6.6e-13    2.1e-11   1.6e-11   0                   13 / 26     6.2e-9         1e-8
  water/cc-pVDZ           -3.2e-12    3.8e-11   2.9e-11   0                   13 / 27     1e-8           1e-8
  benzene/STO-3G          -2.8e-13    5.0e-11   1.1e-10   -1.1e-16            23 / 92     1e-8           1e-8
  water/cc-pVTZ-cut       -8.6e-13    3.5e-11   1.1e-11   2.8e-17             14 / 26     1e-8           1e-8
Every amplitude difference is below 2 tol = 2e-10 and every energy difference below 7e-12 Eh.  E(CCSD) - published = -4.4e-10 on
water_crawford/STO-3G; the diagnostics agree to 4.3e-11; split-k: worst error / bound 0.13 (k = 9), 4.4e-4 at k = 1089."""
import ctypes
import json

import numpy as np
import pytest

from conftest import data
import ccsd_reference as R
import synthetic_systems as Y
from test_stability_gpu import converged

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TOL = 1e-10
E_PUBLISHED = -0.070680088376       # water_crawford/STO-3G, CCSD correlation energy
CASES = [("h2@1.4", 0, (4, 1, 3)), ("water_crawford/STO-3G", 0, (7, 5, 2)), ("water/6-31G", 0, (13, 5, 8)), ("water/6-31G", 1, (13, 4, 8)),
         ("water/cc-pVDZ", 0, (24, 5, 19)), ("benzene/STO-3G", 0, (36, 21, 15)), ("water/cc-pVTZ-cut", 0, (38, 5, 33))]
_cache = {}


class Case:
    """a converged state with the library's CCSD and the reference's, both to TOL; closed after use by the module's finaliser"""

    def __init__(self, name, nf):
        self.s, self.st, _ = converged(name)
        self.n, self.nocc = self.s.n, self.s.n_electrons() // 2
        self.I, self.C, self.eps = self.s.eri(), self.st.coefficients(), self.st.orbital_energies()
        self.mp2 = self.st.mp2(nf)
        self.gpu = self.st.ccsd(n_frozen=nf, tol=TOL, amplitudes=True)
        self.ref = R.ccsd(self.I, self.C, self.eps, self.nocc, nf, tol=TOL, polish=True)

    def close(self):
        self.st.close()
        self.s.close()


def case(name, nf):
    if (name, nf) not in _cache:
        _cache[(name, nf)] = Case(name, nf)
    return _cache[(name, nf)]


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _cache.values():
        c.close()
    _cache.clear()


def integral_bound(c, nf):
    """8 n u Emax over the active MOs"""
    Ca = np.abs(c.C[:, nf:])
    E = np.abs(c.I)
    for _ in range(4):
        E = np.tensordot(E, Ca, axes=(0, 0))                     # (contracts the first index, appends the MO index: four times = all four)
    return 8.0 * c.n * U * float(E.max())


@pytest.mark.parametrize("name,nf,shape", CASES)
def test_ccsd_matches_the_reference(name, nf, shape):
    c = case(name, nf)
    g, r = c.gpu, c.ref
    o, v = r.o, r.v
    assert (c.n, o, v) == shape and g.converged and r.converged and g.n_frozen == nf
    t1, t2 = R.closed_shell(r)
    d = R.diagnostics(r)
    ovov = r.mo[:o, o:, :o, o:]
    L = 2.0 * ovov - ovov.transpose(0, 3, 2, 1)
    tau = t2 + np.einsum("ia,jb->ijab", t1, t1)
    gap = 2.0 * float(c.eps[c.nocc] - c.eps[c.nocc - 1])
    dI = integral_bound(c, nf)
    W = 1.0 + 16.0 * (o + v) ** 2 * max(d[1], d[2])
    bar_t = min(2.0 * TOL + 2.0 * W * dI / gap, 1e-8)
    bar_e = min(1e-8, float(np.abs(L).sum()) * bar_t + 3.0 * dI * float(np.abs(tau).sum()))
    e1, e2 = float(np.abs(g.t1 - t1).max()), float(np.abs(g.t2 - t2).max())
    print(name, nf, "E(CCSD) %.12f reference %.12f difference %.2e (bar %.2e)" % (g.e_ccsd, r.e_ccsd, g.e_ccsd - r.e_ccsd, bar_e),
          "max|dt1| %.2e max|dt2| %.2e (bar %.2e, dI %.2e, W %.0f)" % (e1, e2, bar_t, dI, W), "e_mp2 - qc_scf_mp2 %.2e" % (g.e_mp2 - c.mp2.e_corr),
          "iterations", g.iterations, "reference", r.iterations, "polished to", r.total_iterations, "diagnostics", g.t1_diagnostic - d[0], g.t1_max - d[1], g.t2_max - d[2],
          "ms", g.ms_tensor, g.ms_transform, g.ms_solve)
    assert abs(g.e_mp2 - c.mp2.e_corr) <= 1e-12
    assert abs(g.e_ccsd - r.e_ccsd) <= bar_e
    assert e1 <= bar_t and e2 <= bar_t
    assert np.array_equal(g.t2, g.t2.transpose(1, 0, 3, 2)) or np.abs(g.t2 - g.t2.transpose(1, 0, 3, 2)).max() <= bar_t
    assert abs(g.t1_diagnostic - d[0]) <= 1e-8 and abs(g.t1_max - d[1]) <= 1e-8 and abs(g.t2_max - d[2]) <= 1e-8
    assert g.residual <= TOL and 1 <= g.iterations <= r.iterations                      # DIIS must not cost iterations


def test_published_value_of_water_crawford():
    g = case("water_crawford/STO-3G", 0).gpu
    print("E(CCSD) - published", g.e_ccsd - E_PUBLISHED)
    assert abs(g.e_ccsd - E_PUBLISHED) <= 1e-8


@pytest.mark.parametrize("m", [1, 25, 441])
def test_gemm_splitk_alone(m):
    """n and k off every tile and slice size: k = 9 is shorter than one slice, k = 361 and 1089 end in a partial slice and a partial
    MFMA step; alpha and beta both at work."""
    from qchem_rs_amd import hf
    rng = np.random.default_rng(100 + m)
    for n in (9, 361):
        for k in (9, 361, 1089):
            A, B, C0 = rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
            for alpha, beta in ((1.0, 0.0), (0.7, -0.3)):
                got = hf.debug_gemm(A, B, C0, alpha, beta, splitk=True)
                ref = alpha * (A @ B) + beta * C0
                bound = 4.0 * k * U * (abs(alpha) * (np.abs(A) @ np.abs(B)) + abs(beta) * np.abs(C0))
                print("split-k", m, n, k, alpha, beta, "worst error / bound", float((np.abs(got - ref) / bound).max()))
                assert np.all(np.abs(got - ref) <= bound)
                assert np.array_equal(got, hf.debug_gemm(A, B, C0, alpha, beta, splitk=True))


def test_a_call_is_bitwise_reproducible():
    a = case("water/cc-pVDZ", 0)
    again = a.st.ccsd(tol=TOL, amplitudes=True)
    s, st, _ = converged("water/cc-pVDZ")
    try:
        fresh = st.ccsd(tol=TOL, amplitudes=True)
    finally:
        st.close()
        s.close()
    for other in (again, fresh):
        assert other.e_ccsd == a.gpu.e_ccsd and other.e_mp2 == a.gpu.e_mp2 and other.iterations == a.gpu.iterations
        assert np.array_equal(other.t1, a.gpu.t1) and np.array_equal(other.t2, a.gpu.t2)


def test_the_state_is_left_exactly_as_it_was():
    """Two identical states on fresh handles, three passes each (n = 38: the fused path); MP2, CCSD and MP2 again on one of them; one more pass on
    both: energy, rms and density bit for bit equal, and the two MP2 calls give identical energies."""
    import qchem_rs_amd as q
    m = Y.load_system("water/cc-pVTZ-cut")
    runs = []
    for with_ccsd in (False, True):
        s = q.System(m)
        st = q.ScfStepper(s)
        try:
            for _ in range(3):
                st.iterate()
            if with_ccsd:
                before = st.mp2()
                r = st.ccsd(max_iterations=3)
                after = st.mp2()
                assert (before.e_os, before.e_ss, before.e_corr) == (after.e_os, after.e_ss, after.e_corr) and r.iterations == 3
            e, rms = st.iterate()
            runs.append((e, rms, st.density()))
        finally:
            st.close()
            s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


def test_argument_errors_on_a_live_state():
    import qchem_rs_amd as q
    from conftest import load_system
    L, INV, UNS = q.lib(), q.hf.QC_ERR_INVALID, q.hf.QC_ERR_UNSUPPORTED
    call = lambda st, **kw: L.qc_scf_ccsd(st._st, ctypes.byref(q.hf._Ccsd(**kw)), None, None)
    m = load_system("water", "STO-3G")
    s = q.System(m)
    st = q.ScfStepper(s)
    try:
        assert call(st) == INV                                                          # before the first pass
        for _ in range(12):
            st.iterate()
        assert L.qc_scf_ccsd(st._st, None, None, None) == INV
        for kw in (dict(n_frozen=-1), dict(n_frozen=5), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iterations=-1), dict(diis_size=-1), dict(diis_size=13)):
            assert call(st, **kw) == INV, kw
        io = q.hf._Ccsd(max_iterations=1, tol=1e-30)
        assert L.qc_scf_ccsd(st._st, ctypes.byref(io), None, None) == q.hf.QC_NOT_CONVERGED
        assert io.iterations == 1 and io.converged == 0 and io.e_ccsd < io.e_mp2 < 0.0
        assert all(np.isfinite(x) for x in (io.e_mp2, io.e_ccsd, io.t1_diagnostic, io.t1_max, io.t2_max, io.residual)) and io.residual > 0.0
        assert call(st, n_frozen=4, diis_size=1, max_iterations=2) in (q.hf.QC_OK, q.hf.QC_NOT_CONVERGED)   # one active occupied orbital, no DIIS
        st.close()
        st = q.ScfStepper(s, uhf=True, n_alpha=5, n_beta=5)
        st.iterate()
        assert call(st) == UNS
        st.close()
        s.set_shard(0, 2)
        st = q.ScfStepper(s)
        st.iterate()
        assert call(st) == UNS
    finally:
        st.close()
        s.close()
    s = q.System(m)
    s.set_solvent(78.4, density=1.0)
    st = q.ScfStepper(s)
    try:
        st.iterate()
        assert call(st) == UNS
    finally:
        st.close()
        s.close()


def test_cli_prints_the_published_energy(capsys):
    from qchem_rs_amd import cli
    assert cli.main(["rhf", "-b", data("basis", "STO-3G.json"), "-m", data("mol", "water_crawford.json"), "--epsilon", "1e-10", "--ccsd", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    doc = json.loads(lines[-1])
    assert abs(doc["ccsd"]["e_ccsd"] - E_PUBLISHED) <= 1e-8 and doc["ccsd"]["converged"] is True
    assert any(l.startswith("ccsd correlation energy: -0.07068008") for l in lines) and any(l.startswith("ccsd converged after ") for l in lines)
