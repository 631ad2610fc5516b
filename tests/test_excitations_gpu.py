"""GPU tests of the CIS / TDHF excited states (qc_scf_excitations) and of the explicit A + B and A - B matrices (qc_scf_excitation_matrices).

Every state is converged to 1e-10 without Schwarz screening.  The reference (tests/excitations_reference.py, proved on the CPU by
tests/test_excitations_host.py) is built in numpy from the stored ERI tensor (qc_eri_full), the state's own C and orbital energies, and
the dipole matrices of tests/dipole_reference.py.

  case              n   o   v   d    what it reaches
  h2@1.4/6-31G      4   1   3   3    one M tile, nroots = dim, the full spectrum
  water/STO-3G      7   5   2   10   odd n (the 8-byte GEMM variant), v = 2
  water/6-31G       13  5   8   40   d = subspace size: the first round is exact, no collapse
  water/cc-pVDZ     24  5   19  95   d > 40: the collapse; 8 roots
  ethylene/6-31G    26  8   18  144  triplet A + B has a negative root: an unstable reference
  benzene/STO-3G    36  21  15  315  o > 16 (second row of MFMA tiles), near-degenerate CIS singlets, a negative CIS triplet root

Past one 32 x 32 tile of (a, b) in the assembly kernel (grid: pairs i >= j, ceil(v / 32), ceil(v / 32)) and past the first trip of the
1024-thread loops of the one-workgroup subspace kernels (synthetic_systems.TILE_SYSTEMS; n, o and v are asserted before anything else, and
tests/test_excitations_host.py proves on the CPU that A + B and A - B of all six are positive definite for both kinds, so TDHF must run):

  water/6-311++G**                 36  5   31  155   one tile, one column short of full
  water/6-311++G**, O d Cartesian  37  5   32  160   exactly one full tile; odd n
  water/cc-pVTZ, cut               38  5   33  165   a second tile one wide: the skipped tile of the diagonal blocks, the exchange tile read from
                                                     another tile, the mirror store and the a < v, b < v guards at their tightest
                                                     (cut: no O f, no H d, two of the three contractions of the O p shell)
  water/cc-pVTZ                    58  5   53  265   f functions, a partial second tile of 21
  ethylene/6-311++G**              72  8   64  512   n > 64; two full tiles each way; the lowest triplet root of A + B is 0.0139, w_1(TDHF triplet) = 0.062
  chloroform/6-31G**               77  29  48  1392  d > 1024 in every subspace kernel; o > 16; n > 64; 435 occupied pairs x 2 x 2 tiles

(In the case names a basis goes by the name of its file: 6-311++G_st_st, 6-31G_st_st; +cart-d and -cut are the two edited ones.)  The (ij|ab) chain
reaches these through the matrices alone: qc_quarter_second with M = o, qc_quarter_third with M = v > 32 on a batch of o^2, qc_quarter_last
with o^2 v rows.  From d = 512 on the TDHF reference is excitations_reference.tdhf_sym.

Bounds.
  matrices     |M - M_ref| <= 8 n u E + 1e-14 elementwise, u = 2.2e-16, E the four-index transform of |I| with |C_occ|, |C_virt| combined with
               the coefficients of the formula (4 E_iajb + E_ibja + E_ijab for singlet A + B, ...): the forward error of four chained
               length-n dot products, twice for the two summation orders; 1e-14 for the diagonal.  Both matrices exactly symmetric.
  CIS          |w_k - w_ref,k| <= residuals[k] + 1e-9 max|w_ref| (Rayleigh-Ritz plus the rounding of the matrices); |A_ref x - w x| <= 10 tol;
               orthonormal to 1e-10.
  TDHF         |P R - w L|, |M L - w R| <= 10 tol with the reference matrices; |L . R - 1| <= 1e-10;
               |w^2 - w_ref^2| <= |M^1/2 W_R + w M^-1/2 W_L| / |M^-1/2 R| + 1e-9 max w_ref^2, from M P R - w^2 R = M W_R + w W_L symmetrised
               with M^-1/2 (u = M^-1/2 R is an approximate eigenvector of the symmetric M^1/2 P M^1/2);
               w_TDHF <= w_CIS,ref root by root, as it stands (the measured distances are 1e-4 Eh and more).
  f            from the returned vectors: f and |mu| to 1e-10.  Against the reference's own TDHF states: see
               test_tdhf_oscillator_strengths_match_the_states_of_the_reference.  Against the reference's own CIS states: with g the distance of w_ref,k to the
               rest of the reference spectrum, |x - x_ref| <= 2 rho / g (sin of the angle <= rho / g), so per component
               |mu - mu_ref| <= sqrt 2 |r^q| 2 rho / g =: dm, and |f - f_ref| <= 2/3 (|dw| |mu_ref|^2 + w (2 |mu_ref| |dm| + |dm|^2)) + 1e-9.

Measured on an MI355X (tol 1e-7, 8 roots or d):
  case             max|P - P_ref|  max|M - M_ref|  worst |.| / bound   CIS s / t rounds (products)   TDHF s rounds (products)   max|w_CIS - w_ref|
  h2@1.4           9.0e-16         6.7e-16         0.006               1 (3) / 1 (3)                 1 (12)                     6.7e-16
  water/STO-3G     3.6e-15         9.4e-16         0.018               1 (10) / 1 (10)               1 (40)                     3.9e-15
  water/6-31G      5.6e-15         3.6e-15         0.043               1 (40) / 1 (40)               1 (160)                    5.1e-15
  water/cc-pVDZ    1.4e-13         3.7e-14         0.020               9 (67) / 19 (82)              23 (521)                   3.0e-14
  ethylene/6-31G   1.7e-14         1.5e-14         0.026               9 (71) / 11 (80)              21 (497)                   4.5e-14
  benzene/STO-3G   4.2e-14         3.0e-14         0.011               33 (102) / 12 (85)            43 (587)                   2.4e-14
  case                    max|P - P_ref|  max|M - M_ref|  worst |.| / bound   CIS s / t rounds (products)   TDHF s / t rounds (products)   max|w_CIS - w_ref|
  water/6-311++G**        1.1e-13         4.9e-14         0.038               31 (107) / 49 (141)           57 (1114) / 68 (1067)          4.5e-14
  water/6-311++G** cart   5.9e-14         3.5e-14         0.037               37 (114) / 49 (133)           62 (1037) / 70 (1118)          9.3e-14
  water/cc-pVTZ, cut      1.4e-12         4.1e-13         0.016               12 (78) / 12 (80)             28 (560) / 26 (536)            2.7e-14
  water/cc-pVTZ           2.3e-12         1.0e-12         0.010               11 (80) / 14 (91)             31 (747) / 33 (684)            2.8e-14
  ethylene/6-311++G**     2.9e-13         2.2e-13         0.027               17 (101) / 19 (122)           42 (996) / 36 (752)            2.3e-14
  chloroform/6-31G**      8.4e-14         2.6e-14         0.049               16 (108) / 19 (118)           35 (774) / 31 (725)            3.4e-14
Every solver converges within its default cap of 100 rounds on the six; the diffuse functions of 6-311++G** cost TDHF on water 57 to 70 of them.
On these six: eigvalsh(A + B)[0] against qc_scf_stability <= 4.5e-14 (ethylene, chloroform); TDHF |w^2 - w_ref^2| <= 1.6e-12 (chloroform)
against a-posteriori bounds of 1.8e-8 .. 3.7e-7; |L . R - 1| <= 6.0e-15; w_1 of the ethylene triplets 0.0618.
The first table: eigvalsh(A + B)[0] against qc_scf_stability: <= 9.4e-15.  TDHF |w^2 - w_ref^2| <= 8e-14 against a-posteriori bounds of 2e-8 .. 3e-7;
|L . R - 1| <= 4e-15.  H2: 2 sum mu_z^2 / w = 6.495195553902852 against alpha_zz = 6.495195553902849 (bound 6.6e-7)."""
import ctypes
import json
import os

import numpy as np
import pytest

import dipole_reference as D
import excitations_reference as X
import synthetic_systems as Y
from test_stability_gpu import _mol, converged

pytestmark = pytest.mark.gpu

TOL = 1e-7
U = 2.2e-16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"h2@1.4": ("h2@1.4/6-31G", 4, 1), "water/STO-3G": ("water/STO-3G", 7, 5), "water/6-31G": ("water/6-31G", 13, 5),
         "water/cc-pVDZ": ("water/cc-pVDZ", 24, 5), "ethylene/6-31G": ("ethylene/6-31G", 26, 8), "benzene/STO-3G": ("benzene/STO-3G", 36, 21)}
SMALL = list(CASES)                                  # v <= 19: one partial tile of the assembly kernel, d <= 315
TILES = list(Y.TILE_SYSTEMS)                         # v = 31 .. 64 and d = 1392: see the module docstring
CASES.update({name: (name, n, o) for name, (n, o, _) in Y.TILE_SYSTEMS.items()})
NAMES = SMALL + TILES
BIG = "chloroform/6-31G_st_st"
SYM_FROM = 512                                       # from this dimension on the TDHF reference is excitations_reference.tdhf_sym
_cache = {}


class Case:
    """a converged state with its reference, built once per module"""

    def __init__(self, name):
        self.name, (_, self.n, self.nocc) = name, CASES[name]
        m = _mol(name)
        self.s, self.st, _ = converged(name)
        # n, o and v before anything else: an edited basis that changed nothing, or another molecule, fails here
        assert self.s.n == self.n and int(np.sum(m.atomic_numbers())) // 2 == self.nocc
        if name in Y.TILE_SYSTEMS:
            assert (self.s.n, self.nocc, self.s.n - self.nocc) == Y.TILE_SYSTEMS[name]
        self.I, self.C, self.eps = self.s.eri(), self.st.coefficients(0), self.st.orbital_energies(0)
        self.d = self.nocc * (self.n - self.nocc)
        assert self.st.stability_dim(0) == self.d                        # (the library's own count of occupied orbitals)
        self.PM = [X.matrices_rhf(self.I, self.C, self.eps, self.nocc, k) for k in (0, 1)]
        _, Mdip = D.overlap_and_dipole(m)
        self.r = X.rhs(self.C, self.nocc, Mdip)
        self._cis, self._tdhf, self._pow = {}, {}, {}

    def cis_ref(self, kind):
        if kind not in self._cis:
            self._cis[kind] = X.cis(*self.PM[kind])
        return self._cis[kind]

    def tdhf_ref(self, kind):
        """(w, R, L) of the reference, ascending: numpy.linalg.eig below d = 512, the symmetric form from there on"""
        if kind not in self._tdhf:
            self._tdhf[kind] = (X.tdhf_sym if self.d >= SYM_FROM else X.tdhf)(*self.PM[kind])
        return self._tdhf[kind]

    def m_power(self, p):
        """(A - B)^p, the same matrix for both kinds"""
        if p not in self._pow:
            self._pow[p] = _sym_power(self.PM[0][1], p)
        return self._pow[p]


@pytest.fixture(scope="module", autouse=True)
def _close_states():
    yield
    for c in _cache.values():
        c.st.close(); c.s.close()
    _cache.clear()


def case(name):
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


# ---- 1. the matrices

XT = 32          # tile of qc_exc_assemble_kernel


def _where(err, bound, o, v):
    """the element with the worst err / bound by the coordinates of the assembly kernel: occupied block (i, j) and tile of (a, b)"""
    if bound is None:
        bound = np.zeros_like(err)                   # (an asymmetry: every nonzero difference is beyond its bound)
    e = int(np.argmax(err / bound if bound.any() else err))
    row, col = divmod(e, o * v)
    (i, a), (j, b) = divmod(row, v), divmod(col, v)
    bad = err > bound
    tiles = sorted({(int(x) // XT, int(y) // XT) for x, y in zip(np.nonzero(bad)[0] % v, np.nonzero(bad)[1] % v)})
    return ("worst element [%d, %d]: block (i, j) = (%d, %d), (a, b) = (%d, %d) in tile (%d, %d) of %d x %d; error %.3e, bound %.3e; %d elements beyond their "
            "bound, in the tiles %s" % (row, col, i, j, a, b, a // XT, b // XT, XT, XT, err[row, col], bound[row, col], int(bad.sum()), tiles[:16]))

@pytest.mark.parametrize("name", NAMES)
def test_matrices_are_exactly_symmetric_and_match_the_reference(name):
    """Measured maxima: the tables in the module docstring (at most 4.9 % of the bound).  A failure names the occupied block (i, j) and the
    32 x 32 tile of (a, b) of the worst element and lists the tiles that hold elements beyond their bound."""
    c = case(name)
    o, v, n = c.nocc, c.n - c.nocc, c.n
    Co, Cv, aI = np.abs(c.C[:, :o]), np.abs(c.C[:, o:]), np.abs(c.I)
    import stability_reference as R
    E1 = R._mo(aI, Co, Cv, Co, Cv)
    Ex = E1.transpose(0, 3, 2, 1).reshape(c.d, c.d)
    Eg = R._mo(aI, Co, Co, Cv, Cv).transpose(0, 2, 1, 3).reshape(c.d, c.d)
    E1 = E1.reshape(c.d, c.d)
    for kind in (0, 1):
        P, M = c.st.excitation_matrices(kind)
        Pr, Mr = c.PM[kind]
        bP = 8 * n * U * ((4.0 if kind == 0 else 0.0) * E1 + Ex + Eg) + 1e-14
        bM = 8 * n * U * (Ex + Eg) + 1e-14
        eP, eM = np.abs(P - Pr), np.abs(M - Mr)
        print(name, "kind", kind, "max|P - P_ref|", float(eP.max()), "max|M - M_ref|", float(eM.max()), "worst ratio to the bound", float((eP / bP).max()),
              float((eM / bM).max()), "smallest bound", float(bP.min()), float(bM.min()))
        assert P.shape == (c.d, c.d) and M.shape == (c.d, c.d)
        assert np.array_equal(P, P.T), "A + B is not symmetric: " + _where(np.abs(P - P.T), None, o, v)
        assert np.array_equal(M, M.T), "A - B is not symmetric: " + _where(np.abs(M - M.T), None, o, v)
        assert np.all(eP <= bP), "A + B: " + _where(eP, bP, o, v)
        assert np.all(eM <= bM), "A - B: " + _where(eM, bM, o, v)


# ---- 2. against the direct-build operator of the stability analysis

@pytest.mark.parametrize("name", ["water/cc-pVDZ", "ethylene/6-31G", "ethylene/6-311++G_st_st", BIG])
def test_a_plus_b_is_the_operator_of_the_stability_analysis(name):
    c = case(name)
    for kind in (0, 1):
        P, _ = c.st.excitation_matrices(kind)
        lo = float(np.linalg.eigvalsh(P)[0])
        direct = float(c.st.stability(kind=kind, tol=TOL).eigenvalues[0])
        print(name, "kind", kind, "eigvalsh(A + B)[0]", lo, "stability", direct, "difference", lo - direct)
        assert abs(lo - direct) <= 2e-7


# ---- 3. CIS

@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_cis(name, kind):
    c = case(name)
    nroots = min(8, c.d)
    r = c.st.excitations("cis", kind=kind, nroots=nroots, tol=TOL, vectors=True)
    w_ref, _ = c.cis_ref(kind)
    A = 0.5 * (c.PM[kind][0] + c.PM[kind][1])
    Xv = r.vectors
    res = [float(np.linalg.norm(A @ Xv[k] - r.energies[k] * Xv[k])) for k in range(nroots)]
    orth = float(np.abs(Xv @ Xv.T - np.eye(nroots)).max())
    err = np.abs(r.energies - w_ref[:nroots])
    print(name, "kind", kind, "cis", r.energies.tolist(), "ref", w_ref[:nroots].tolist(), "max err", float(err.max()), "residuals", r.residuals.tolist(),
          "|A_ref x - w x|", res, "orth", orth, "iterations", r.iterations, "products", r.products, "ms", r.ms_total, r.ms_tensor, r.ms_transform, r.ms_solve)
    assert r.converged and r.nconverged == nroots and np.all(r.residuals <= TOL) and not r.reference_unstable
    assert np.all(err <= r.residuals + 1e-9 * np.abs(w_ref).max())
    assert np.all(np.diff(r.energies) >= 0)
    assert Xv.shape == (nroots, c.d) and orth <= 1e-10
    assert max(res) <= 10 * TOL
    if kind == 1:
        assert np.all(r.oscillator == 0.0) and np.all(r.transition_dipole == 0.0)
    if name == "benzene/STO-3G" and kind == 1:
        assert r.energies[0] < -0.01 and abs(r.energies[0] - w_ref[0]) <= r.residuals[0] + 1e-9 * np.abs(w_ref).max()      # a negative root is a result
    if name == "water/6-31G":
        assert c.d == 40 and r.iterations == 1
    if name == "water/cc-pVDZ":
        assert r.products > 40                                               # more vectors than the subspace holds: the collapse has run
    if name == "h2@1.4":
        assert nroots == c.d == 3


# ---- 4. TDHF

TDHF_CASES = [(n, 0) for n in NAMES] + [(n, 1) for n in ["h2@1.4", "water/STO-3G", "water/6-31G", "water/cc-pVDZ"] + TILES]


def _sym_power(M, p):
    s, V = np.linalg.eigh(M)
    assert s[0] > 0
    return (V * s ** p) @ V.T


@pytest.mark.parametrize("name,kind", TDHF_CASES, ids=["%s-k%d" % t for t in TDHF_CASES])
def test_tdhf(name, kind):
    c = case(name)
    nroots = min(8, c.d)
    r = c.st.excitations("tdhf", kind=kind, nroots=nroots, tol=TOL, vectors=True)
    P, M = c.PM[kind]
    w_ref = c.tdhf_ref(kind)[0]
    w_cis = c.cis_ref(kind)[0]
    assert not r.reference_unstable, "TDHF refused a reference whose A + B and A - B are positive definite"
    Rv, Lv, w = r.vectors[0], r.vectors[1], r.energies
    WR = [P @ Rv[k] - w[k] * Lv[k] for k in range(nroots)]
    WL = [M @ Lv[k] - w[k] * Rv[k] for k in range(nroots)]
    Mh, Mih = c.m_power(0.5), c.m_power(-0.5)
    apost = np.array([np.linalg.norm(Mh @ WR[k] + w[k] * (Mih @ WL[k])) / np.linalg.norm(Mih @ Rv[k]) for k in range(nroots)])
    lr = np.abs(np.einsum("ki,ki->k", Lv, Rv) - 1.0)
    err2 = np.abs(w ** 2 - w_ref[:nroots] ** 2)
    print(name, "kind", kind, "tdhf", w.tolist(), "ref", w_ref[:nroots].tolist(), "|w^2 - w_ref^2|", err2.tolist(), "a-posteriori", apost.tolist(),
          "residuals", r.residuals.tolist(), "|W_R|", [float(np.linalg.norm(x)) for x in WR], "|W_L|", [float(np.linalg.norm(x)) for x in WL],
          "|L.R - 1|", float(lr.max()), "iterations", r.iterations, "products", r.products, "ms", r.ms_total, r.ms_solve)
    assert r.converged and r.nconverged == nroots and not r.reference_unstable and np.all(r.residuals <= TOL)
    assert r.vectors.shape == (2, nroots, c.d)
    assert max(np.linalg.norm(x) for x in WR) <= 10 * TOL and max(np.linalg.norm(x) for x in WL) <= 10 * TOL
    assert lr.max() <= 1e-10
    assert np.all(err2 <= apost + 1e-9 * (w_ref ** 2).max())
    assert np.all(np.diff(w) >= 0) and np.all(w <= w_cis[:nroots])
    if kind == 1:
        assert np.all(r.oscillator == 0.0) and np.all(r.transition_dipole == 0.0)


@pytest.mark.parametrize("name", ["ethylene/6-31G", "benzene/STO-3G"])
def test_tdhf_refuses_a_triplet_unstable_reference(name):
    import qchem_rs_amd as q
    c = case(name)
    lam = float(np.linalg.eigvalsh(c.PM[1][0])[0])
    io = q.hf._Excitations(method=1, kind=1, nroots=2, tol=TOL)
    rc = q.lib().qc_scf_excitations(c.st._st, ctypes.byref(io), None)
    print(name, "lambda_min of the triplet A + B (reference)", lam, "status", rc, "reference_unstable", io.reference_unstable, "products", io.products)
    assert lam < 0
    assert rc == q.hf.QC_NOT_CONVERGED and io.reference_unstable == 1 and io.nconverged == 0
    r = c.st.excitations("tdhf", kind=1, nroots=2, tol=TOL, vectors=True)
    assert r.reference_unstable and not r.converged and not r.vectors.any()


# ---- 5. oscillator strengths

@pytest.mark.parametrize("name", NAMES)
def test_oscillator_strengths_belong_to_the_returned_vectors(name):
    c = case(name)
    nroots = min(8, c.d)
    for method in ("cis", "tdhf"):
        r = c.st.excitations(method, kind=0, nroots=nroots, tol=TOL, vectors=True)
        V = r.vectors if method == "cis" else r.vectors[0]
        mu = X.transition_dipoles(c.r, V)
        f = X.oscillator_strengths(r.energies, mu)
        dmu = float(np.abs(np.linalg.norm(r.transition_dipole, axis=1) - np.linalg.norm(mu, axis=1)).max())
        print(name, method, "f", r.oscillator.tolist(), "max |f - f(vectors)|", float(np.abs(r.oscillator - f).max()), "max ||mu| - |mu(vectors)||", dmu,
              "max |mu - mu(vectors)|", float(np.abs(r.transition_dipole - mu).max()))
        assert r.converged
        assert np.abs(r.oscillator - f).max() <= 1e-10 and dmu <= 1e-10


@pytest.mark.parametrize("name", [n for n in NAMES if n != "benzene/STO-3G"])
def test_cis_oscillator_strengths_match_the_states_of_the_reference(name):
    """benzene is left to the energies: its CIS singlets come in pairs 6e-7 Eh apart, where a vector of its own means nothing."""
    c = case(name)
    nroots = min(8, c.d)
    r = c.st.excitations("cis", kind=0, nroots=nroots, tol=TOL)
    w_ref, X_ref = c.cis_ref(0)
    mu_ref = X.transition_dipoles(c.r, X_ref)
    f_ref = X.oscillator_strengths(w_ref, mu_ref)
    rn = np.linalg.norm(c.r, axis=1)
    for k in range(nroots):
        gap = float(np.abs(np.delete(w_ref, k) - w_ref[k]).min()) if c.d > 1 else 1.0
        dw = r.residuals[k] + 1e-9 * np.abs(w_ref).max()
        dm = float(np.linalg.norm(np.sqrt(2.0) * rn * 2.0 * r.residuals[k] / gap))
        m = float(np.linalg.norm(mu_ref[k]))
        b = 2.0 / 3.0 * (dw * m * m + abs(w_ref[k]) * (2.0 * m * dm + dm * dm)) + 1e-9
        print(name, "state", k, "f", r.oscillator[k], "f_ref", f_ref[k], "difference", abs(r.oscillator[k] - f_ref[k]), "bound", b, "gap", gap)
        assert abs(r.oscillator[k] - f_ref[k]) <= b


@pytest.mark.parametrize("name", [n for n in NAMES if n != "benzene/STO-3G"])
def test_tdhf_oscillator_strengths_match_the_states_of_the_reference(name):
    """The bound, in the metric in which the problem is symmetric.  K = M^1/2 P M^1/2 has the eigenpairs (w_ref^2, u_ref), |u_ref| = 1, and
    R_ref = c_ref M^1/2 u_ref with c_ref = w_ref^-1/2 (from R^T P R = w).  The returned R gives u = M^-1/2 R / c, c = |M^-1/2 R|, whose
    residual K u - w^2 u is the a-posteriori quantity rho' of test_tdhf.  With b2 = rho' + 1e-9 max w_ref^2 the bound on |w^2 - w_ref^2| and g2 the
    distance of w_ref,k^2 to the rest of the reference spectrum:
      |u - u_ref| <= sqrt 2 sin(angle) <= sqrt 2 rho' / (g2 - b2) =: du          (Davis-Kahan; the Ritz value is within b2 of w_ref^2)
      dw = b2 / w_ref >= |w - w_ref|
      c^2 = R^T M^-1 R = (L.R - R^T M^-1 W_L) / w  (from M L = w R + W_L), so |c^2 - 1/w| <= (1e-10 + |M^-1 R| |W_L|) / w and
      |c - c_ref| <= (|c^2 - 1/w| + dw / (w w_ref)) / c_ref =: dc                (c + c_ref >= c_ref)
      |mu_q - mu_ref,q| <= sqrt 2 |M^1/2 r^q| ((c_ref + dc) du + dc),  dm its norm over q
      |f - f_ref| <= 2/3 (dw (|mu_ref| + dm)^2 + w_ref (2 |mu_ref| dm + dm^2)) + 1e-9
    benzene is left to the energies, as for CIS.  H2: the pinned f of the first singlet (0.65129083 TDHF, 0.77060040 CIS; a state converged
    to 1e-10 and eight printed digits: 1e-7).
    Measured on an MI355X: |f - f_ref| <= 1.1e-9 (ethylene, f = 0.2775) against bounds of 1.4e-9 .. 5.1e-5; ||mu| - |mu_ref|| <= 1.5e-8
    against dm of 9e-6 .. 1.6e-4."""
    c = case(name)
    nroots = min(8, c.d)
    r = c.st.excitations("tdhf", kind=0, nroots=nroots, tol=TOL, vectors=True)
    P, M = c.PM[0]
    w_ref, R_ref, _ = c.tdhf_ref(0)
    mu_ref = X.transition_dipoles(c.r, R_ref)
    f_ref = X.oscillator_strengths(w_ref, mu_ref)
    Mh, Mih, Mi = c.m_power(0.5), c.m_power(-0.5), np.linalg.inv(M)
    rq = np.linalg.norm(c.r @ Mh, axis=1)                                    # |M^1/2 r^q|
    assert r.converged
    for k in range(nroots):
        Rk, Lk, w = r.vectors[0][k], r.vectors[1][k], r.energies[k]
        WR, WL = P @ Rk - w * Lk, M @ Lk - w * Rk
        rho = float(np.linalg.norm(Mh @ WR + w * (Mih @ WL)) / np.linalg.norm(Mih @ Rk))
        b2 = rho + 1e-9 * float((w_ref ** 2).max())
        g2 = float(np.abs(np.delete(w_ref, k) ** 2 - w_ref[k] ** 2).min()) if c.d > 1 else 1.0
        assert abs(float(Lk @ Rk) - 1.0) <= 1e-10 and g2 > 2.0 * b2, "the case is unsuitable: state %d is not separated from the spectrum" % k
        du = np.sqrt(2.0) * rho / (g2 - b2)
        dw = b2 / w_ref[k]
        wl = w_ref[k] - dw                                                  # (a lower bound of the returned w)
        c_ref = w_ref[k] ** -0.5
        dc = ((1e-10 + float(np.linalg.norm(Mi @ Rk) * np.linalg.norm(WL))) / wl + dw / (wl * w_ref[k])) / c_ref
        dm = float(np.linalg.norm(np.sqrt(2.0) * rq * ((c_ref + dc) * du + dc)))
        m = float(np.linalg.norm(mu_ref[k]))
        b = 2.0 / 3.0 * (dw * (m + dm) ** 2 + w_ref[k] * (2.0 * m * dm + dm * dm)) + 1e-9
        got_m = float(np.linalg.norm(r.transition_dipole[k]))
        print(name, "state", k, "f", r.oscillator[k], "f_ref", f_ref[k], "difference", abs(r.oscillator[k] - f_ref[k]), "bound", b, "||mu| - |mu_ref||", abs(got_m - m),
              "dm", dm, "rho'", rho, "g2", g2, "dc", dc)
        assert abs(r.oscillator[k] - f_ref[k]) <= b and abs(got_m - m) <= dm + 1e-9
    if name == "h2@1.4":
        cis = c.st.excitations("cis", kind=0, nroots=1, tol=TOL)
        print("h2 pinned f: tdhf", r.oscillator[0], "cis", cis.oscillator[0])
        assert abs(r.oscillator[0] - 0.65129083) <= 1e-7 and abs(cis.oscillator[0] - 0.77060040) <= 1e-7


def test_h2_tdhf_sum_over_states_is_the_static_polarizability():
    c = case("h2@1.4")
    r = c.st.excitations("tdhf", kind=0, nroots=3, tol=TOL)
    p = c.st.polarizability(tol=TOL)
    sos = 2.0 * float((r.transition_dipole[:, 2] ** 2 / r.energies).sum())
    lam = float(np.linalg.eigvalsh(c.PM[0][0])[0])
    b = 4.0 * float(np.linalg.norm(c.r[2])) * TOL / lam + 1e-9 * abs(p.alpha[2, 2])
    print("h2 sum over states", sos, "alpha_zz (CPHF)", p.alpha[2, 2], "difference", abs(sos - p.alpha[2, 2]), "bound", b)
    assert r.converged and p.converged and lam > 0
    assert abs(sos - p.alpha[2, 2]) <= b


# ---- 6. determinism, and the state is left as it was

def _reproducible(name, method):
    runs = []
    for handle in range(2):
        s, st, _ = converged(name)
        for _ in range(2 - handle):
            r = st.excitations(method, kind=0, nroots=4, tol=TOL, vectors=True)
            runs.append((r.energies, r.residuals, r.vectors, r.oscillator, r.transition_dipole, (r.iterations, r.products, r.nconverged)))
        st.close(); s.close()
    for other in runs[1:]:
        for a, b in zip(runs[0][:5], other[:5]):
            assert np.array_equal(a, b)
        assert runs[0][5] == other[5]
    return runs[0]


@pytest.mark.parametrize("method", ["cis", "tdhf"])
def test_a_call_is_bitwise_reproducible(method):
    _reproducible("water/cc-pVDZ", method)


@pytest.mark.parametrize("method", ["cis", "tdhf"])
def test_a_call_is_bitwise_reproducible_past_dimension_1024(method):
    """chloroform/6-31G**, d = 1392: the fixed-order sums of the one-workgroup kernels over two trips of 1024, 435 occupied pairs x 2 x 2 tiles."""
    energies, residuals = _reproducible(BIG, method)[:2]
    assert np.all(energies > 0.1) and np.all(residuals <= TOL)           # (two runs that both failed alike would be equal too)


def _left_as_it_was(name):
    import qchem_rs_amd as q
    out = []
    for touch in (False, True):
        s = q.System(_mol(name))
        st = q.ScfStepper(s)
        for _ in range(6):
            st.iterate()
        if touch:
            before = st.mp2()
            st.excitations("cis", kind=0, nroots=2, tol=1e-5)
            st.excitations("tdhf", kind=1, nroots=2, tol=1e-5)
            st.excitation_matrices(1)
            after = st.mp2()
            assert (before.e_os, before.e_ss, before.e_corr) == (after.e_os, after.e_ss, after.e_corr)
        e, rms = st.iterate()
        out.append((e, rms, st.density(0)))
        st.close(); s.close()
    (e0, r0, D0), (e1, r1, D1) = out
    print(name, e0, e1, r0, r1)
    assert e0 == e1 and r0 == r1 and np.array_equal(D0, D1)


def test_the_state_is_left_exactly_as_it_was():
    """Two identical states of water/cc-pVTZ (n = 58, the fused path) after 6 passes; excitations and matrices on one of them; one more
    pass on both: energy, rms and density bit for bit equal.  MP2 before and after the calls is identical too."""
    _left_as_it_was("water/cc-pVTZ")


def test_the_state_is_left_exactly_as_it_was_past_dimension_1024():
    """The same on chloroform/6-31G** (n = 77, the generic path; d = 1392)."""
    _left_as_it_was(BIG)


# ---- 7. errors on a live state

def test_argument_errors_on_a_live_state():
    import qchem_rs_amd as q
    from test_stability_gpu import h2
    L, INV, UNS = q.lib(), q.hf.QC_ERR_INVALID, q.hf.QC_ERR_UNSUPPORTED
    s = q.System(h2(1.4))
    st = q.ScfStepper(s)
    io = q.hf._Excitations(nroots=1)
    buf = np.zeros(9)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.qc_scf_excitations(st._st, ctypes.byref(io), None) == INV                     # before the first pass
    assert L.qc_scf_excitation_matrices(st._st, 0, p, p) == INV
    st.iterate()
    assert L.qc_scf_excitations(st._st, None, None) == INV
    for kw in (dict(nroots=0), dict(nroots=9), dict(nroots=4), dict(nroots=1, method=2), dict(nroots=1, method=-1), dict(nroots=1, kind=2),
               dict(nroots=1, tol=-1.0), dict(nroots=1, tol=float("nan")), dict(nroots=1, max_iterations=-1)):
        io = q.hf._Excitations(**kw)
        assert L.qc_scf_excitations(st._st, ctypes.byref(io), None) == INV, kw
    assert L.qc_scf_excitation_matrices(st._st, 2, p, p) == INV
    for method in (0, 1):
        io = q.hf._Excitations(method=method, nroots=2, max_iterations=1, tol=1e-30)      # cannot be reached: outputs are filled all the same
        assert L.qc_scf_excitations(st._st, ctypes.byref(io), None) == q.hf.QC_NOT_CONVERGED
        assert io.iterations == 1 and np.all(np.isfinite(io.energies[:2])) and io.energies[0] > 0.1 and np.all(np.isfinite(io.residuals[:2]))
        assert np.all(np.isfinite(io.oscillator[:2])) and np.all(np.isfinite(io.transition_dipole[:6]))
    st.close()
    st = q.ScfStepper(s, uhf=True, n_alpha=1, n_beta=1)
    st.iterate()
    io = q.hf._Excitations(nroots=1)
    assert L.qc_scf_excitations(st._st, ctypes.byref(io), None) == UNS
    assert L.qc_scf_excitation_matrices(st._st, 0, p, p) == UNS
    st.close()
    s.set_shard(0, 2)
    st = q.ScfStepper(s)
    st.iterate()
    io = q.hf._Excitations(nroots=1)
    assert L.qc_scf_excitations(st._st, ctypes.byref(io), None) == UNS
    assert L.qc_scf_excitation_matrices(st._st, 0, p, p) == UNS
    st.close(); s.close()


# ---- 8. the command line

PINNED = {("--cis", False): [0.3564617754, 0.4160717500, 0.5056282996], ("--tdhf", True): [0.2851637340, 0.2997434579, 0.3526266685]}


@pytest.mark.parametrize("flag,triplets", list(PINNED))
def test_cli_prints_the_pinned_states(capsys, flag, triplets):
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    b, m = os.path.join(ROOT, "data", "basis", "STO-3G.json"), os.path.join(ROOT, "data", "mol", "water_crawford.json")
    argv = ["rhf", "-b", b, "-m", m, "--epsilon", "1e-10", flag, "3", "--json"] + (["--triplets"] if triplets else [])
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    doc = json.loads(lines[-1])["excitations"]
    assert isinstance(doc, list) and len(doc) == 1
    doc = doc[0]
    word = "%s %s state" % (flag[2:], "triplet" if triplets else "singlet")
    states = [l for l in lines if l.startswith(word)]
    print(states, doc["energies"])
    assert len(states) == 3 and len(doc["energies"]) == 3 and doc["converged"] is True
    assert np.abs(np.array(doc["energies"]) - np.array(PINNED[(flag, triplets)])).max() <= 1e-7
    for k, l in enumerate(states):
        assert abs(float(l.split(": ")[1].split()[0]) - PINNED[(flag, triplets)][k]) <= 1e-7
        assert ("f = " in l) == (not triplets)
