"""GPU tests on systems in general position (tests/synthetic_systems.py) against the CPU oracle.  Every shipped molecule with f
functions lies in a coordinate plane or on an axis, so for Hermite orders 9..12 one component of P - Q has always been exactly zero and
every R_tuv with an odd index along it was multiplied by 0; the gradient has only seen planar molecules; no ket pair had more than 100
primitive pairs; and no d / f quartet met a Boys argument beyond the table with a prefactor left.  Here:

  tetra   four centres, no shared coordinate, s..f on each: every (LAB, LCD) class with four distinct centres, at n = 64 (pure, the
          one-workgroup limit) and n = 80 (Cartesian, generic launches)                              [gap: quartets at general position]
  deep    169 primitive pairs in the same-centre ss and ps kets: bra-major lists of plain pair indices       [gap: K > 127 ket pairs]
  far     single-primitive s..f shells on two centres at T = 40 (last table rows of qc_boys, above the 38 switch of qc_md_boys) and
          T = 59 (beyond QC_BOYS_XMAX)                                                       [gap: high-order Boys beyond the table]
  and gradient terms of tetra, deep and far at T = 40 against the oracle's five-point stencil      [gap: gradient off a plane]

Tolerances are those of test_gpu_parity.py and test_gradient_gpu.py: 1e-10 on integrals and Fock matrices (times the scale of G),
1e-11 times the scale on one-electron matrices, 1e-9 on gradient terms.  The oracle's tensors are computed once per module."""
import numpy as np
import pytest

import synthetic_systems as syn
from synthetic_systems import BOYS_SERIES_SWITCH, BOYS_XMAX, BUILDERS
from test_gpu_parity import TOL_INT, _column_classes, _pp_bm_unit, _valu_fket_quartets

pytestmark = pytest.mark.gpu

TENSOR_SYSTEMS = ["tetra-pure-2", "tetra-cart-2", "deep", "far-40", "far-59"]


@pytest.fixture(scope="module")
def refs():
    """name -> (MolecularSystem, Oracle, oracle tensor), each built on first use and kept unchanged for the module"""
    from oracle.oracle import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            m = BUILDERS[name]()[0]
            o = Oracle(m)
            I = syn.oracle_tensor(o)
            I.setflags(write=False)
            cache[name] = (m, o, I)
        return cache[name]
    yield get
    cache.clear()


def _worst_class(o, E):
    """the shell-quartet class - four L values, number of distinct centres - with the largest element of |E|, walking the oracle's shell table"""
    tab, atom = o.shell_table(), o.system.shell_atom
    ns = len(tab)
    sl = [slice(t[0], t[0] + t[1]) for t in tab]
    per_ab = np.array([[np.abs(E[sl[a], sl[b]]).max(axis=(0, 1)) for b in range(ns)] for a in range(ns)])      # (ns, ns, n, n)
    worst = {}
    for a in range(ns):
        for b in range(ns):
            for c in range(ns):
                for d in range(ns):
                    key = (tab[a][2], tab[b][2], tab[c][2], tab[d][2], len({int(atom[x]) for x in (a, b, c, d)}))
                    worst[key] = max(worst.get(key, 0.0), float(per_ab[a, b][sl[c], sl[d]].max()))
    key = max(worst, key=worst.get)
    return "worst class (%s%s|%s%s) on %d distinct centres: %.3e" % (tuple("spdf"[l] for l in key[:4]) + (key[4], worst[key]))


def _check_tensor(o, I_gpu, I_ref, what):
    E = I_gpu - I_ref
    err = float(np.abs(E).max())
    print("%s: max |ERI - oracle| = %.3e (tolerance %.0e)" % (what, err, TOL_INT))
    assert err < TOL_INT, "%s: %s" % (what, _worst_class(o, E))


def _check_fock(s, o, I, what, seeds=(0, 1)):
    """fock_rhf for two seeds and fock_uhf (Da != Db) against the oracle's dense contraction; G symmetric and repeatable bit for bit"""
    worst = 0.0
    for seed in seeds:
        D = syn.rand_sym(s.n, seed, 1.0)
        G_ref = o.g_rhf(D, I)
        G = s.fock_rhf(D)
        scale = max(1.0, np.abs(G_ref).max())
        err = float(np.abs(G - G_ref).max())
        worst = max(worst, err / scale)
        assert err < TOL_INT * scale, (what, "rhf", seed, err, scale)
        assert np.array_equal(G, G.T), (what, "rhf", seed)
        assert np.array_equal(s.fock_rhf(D), G), (what, "rhf", seed)
    Da, Db = syn.rand_sym(s.n, 3, 1.0), syn.rand_sym(s.n, 4, 1.0)
    Ga, Gb = s.fock_uhf(Da, Db)
    for X, R, spin in ((Ga, o.g_uhf(Da, Db, I), "alpha"), (Gb, o.g_uhf(Db, Da, I), "beta")):
        scale = max(1.0, np.abs(R).max())
        err = float(np.abs(X - R).max())
        worst = max(worst, err / scale)
        assert err < TOL_INT * scale, (what, "uhf", spin, err, scale)
        assert np.array_equal(X, X.T), (what, "uhf", spin)
    Ga2, Gb2 = s.fock_uhf(Da, Db)
    assert np.array_equal(Ga2, Ga) and np.array_equal(Gb2, Gb), what
    print("%s: max |G - oracle| / scale = %.3e (tolerance %.0e)" % (what, worst, TOL_INT))


def _far_sides(name, m):
    if name.startswith("far"):
        T = syn.far_boys_argument(m)
        assert (BOYS_SERIES_SWITCH < T < BOYS_XMAX) if name == "far-40" else (T > BOYS_XMAX), (name, T)


@pytest.mark.parametrize("name", TENSOR_SYSTEMS)
def test_eri_tensor_matches_oracle_at_general_position(name, refs):
    """qc_eri_full element by element.  tetra: every class up to (ff|ff) on four distinct centres, R tables of orders 9..12 with no
    vanishing component of P - Q (the generated tables, the MFMA column kernels); deep: K = 169 kets; far: d / f quartets at
    T = 40 and T = 59.  A failure names the worst class."""
    import qchem_rs_amd as q
    m, o, I = refs(name)
    _far_sides(name, m)
    s = q.System(m)
    I_gpu = s.eri()
    _check_tensor(o, I_gpu, I, name)
    assert np.array_equal(s.eri(), I_gpu)
    s.close()


@pytest.mark.parametrize("name", TENSOR_SYSTEMS)
def test_fock_builds_match_dense_contraction_at_general_position(name, refs):
    """The direct build (default screening): RHF for two seeds and UHF against the dense contraction of the oracle's tensor, G == G^T
    and a repeated build bit for bit.  deep: the bra-major kernels took quartets, and their ss / ps kets hold 169 primitive pairs -
    more than a packed list entry can say, so those lists are plain pair indices; also with screening off."""
    import qchem_rs_amd as q
    m, o, I = refs(name)
    _far_sides(name, m)
    s = q.System(m)
    _check_fock(s, o, I, name)
    if name == "deep":
        assert syn.same_centre_ket_primitives(m) == 169 > 127
        bm = s.unit_quartets()[14:]
        assert all(q.hf.unit_name(u).startswith("qc_fock_bm_kernel") for u in range(14, q.hf.PROFILE_UNITS))
        print("deep: quartets per bra-major unit", bm.tolist())
        assert bm.max() > 0, "deep reaches no bra-major kernel: the plain-entry lists were bypassed"
        s0 = q.System(m)
        s0.set_schwarz(0.0)
        _check_fock(s0, o, I, "deep, screening off", seeds=(0,))
        assert s0.unit_quartets()[14:].sum() >= bm.sum() > 0
        s0.close()
    s.close()


@pytest.mark.parametrize("route", ["valu-fket", "pp-bm-to-column"])
def test_route_switches_on_tetra(route, refs, monkeypatch):
    """The two route switches of test_eri_tensor_routes_on_small_systems and test_fock_f_basis_valu_route_on_small_systems on tetra
    (pure, two primitives): QC_MFMA4_MAX = 0 (every d.d / f.p-ket list of a d.p ... f.f bra in the 32-lane VALU form) and
    QC_BM_PP_MIN = 1 (the p.p-ket bra-major class, which tensor mode hands to the column kernels) - tensor and Fock builds."""
    import qchem_rs_amd as q
    m, o, I = refs("tetra-pure-2")
    var = "QC_MFMA4_MAX" if route == "valu-fket" else "QC_BM_PP_MIN"
    if route == "valu-fket":
        s_def = q.System(m)
        nq_def = sum(_valu_fket_quartets(_column_classes(s_def, s_def.n)))
        s_def.close()
    monkeypatch.setenv(var, "0" if route == "valu-fket" else "1")
    s = q.System(m)
    monkeypatch.delenv(var)
    if route == "valu-fket":
        nq = sum(_valu_fket_quartets(_column_classes(s, s.n)))
        assert nq > 0 and nq > nq_def, (nq, nq_def)
    else:
        s.fock_rhf(syn.rand_sym(s.n, 0, 1.0))
        assert s.unit_quartets()[_pp_bm_unit(q)] > 0
    I_gpu = s.eri()
    _check_tensor(o, I_gpu, I, "tetra-pure-2, " + route)
    assert np.array_equal(s.eri(), I_gpu)
    _check_fock(s, o, I, "tetra-pure-2, " + route)
    s.close()


@pytest.mark.parametrize("name", list(BUILDERS))
def test_one_electron_matrices_at_general_position(name):
    """S, T and V of qc_one_electron.hip on every builder: f.f pairs off every axis, 13-primitive shells (exponents up to 1750),
    and nuclear attraction at Boys arguments on both sides of the 38 switch of qc_md_boys."""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = BUILDERS[name]()[0]
    _far_sides(name, m)
    s, o = q.System(m), Oracle(m)
    for which, ref in ((0, o.overlap()), (1, o.kinetic()), (2, o.nuclear())):
        M = s.one_electron_gpu(which)
        assert np.abs(M - ref).max() < 1e-11 * max(1.0, np.abs(ref).max()), (name, which)
        assert np.abs(M - M.T).max() == 0.0, (name, which)
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Gradient terms.  The reference is the oracle's five-point stencil at h = 1e-3.  Its own error was measured on the CPU as the
# difference to the stencil at h = 2e-3 (whose truncation error is 16 times larger), per term, RHF and UHF pair, for the densities below:
#   tetra-pure-1  (0,y) 2.9e-11  (1,z) 7.8e-11  (2,x) 3.3e-11  (3,x) 4.9e-11     (rejected: (0,z) 1.7e-10)
#   tetra-cart-1  (0,y) 7.3e-11  (1,z) 3.3e-11  (2,x) 2.0e-11  (3,x) 6.0e-11     (rejected: (0,x) 1.2e-10)
#   deep          all nine coordinates, largest 4.3e-11 at (1,x)
#   far-40        all six coordinates below 7e-13
# all within the 1e-10 the 1e-9 bar of the term test needs.

GRAD_COORDS = {"tetra-pure-1": [(0, 1), (1, 2), (2, 0), (3, 0)], "tetra-cart-1": [(0, 1), (1, 2), (2, 0), (3, 0)],
               "deep-atom0": [(0, 0), (0, 1), (0, 2)], "deep-atom1": [(1, 0), (1, 1), (1, 2)], "deep-atom2": [(2, 0), (2, 1), (2, 2)],
               "far-40": [(1, 1)]}


def _densities(n):
    """an RHF-convention pair (P, W) and a UHF set (Da != Db, W), symmetric and random"""
    P, W = syn.rand_sym(n, 11), syn.rand_sym(n, 12)
    Da, Db, Wu = syn.rand_sym(n, 13), syn.rand_sym(n, 14), syn.rand_sym(n, 15)
    return (P, W), (Da, Db, Wu)


@pytest.mark.parametrize("case", list(GRAD_COORDS))
def test_gradient_terms_match_oracle_finite_differences_off_every_plane(case):
    """The four terms of qc_gradient at fixed random densities against the stencil: quartets on four distinct centres (centre D by
    translational invariance from three computed ones), every y derivative alive, f shells pure and Cartesian; deep with its
    169-primitive pairs on all nine coordinates (one case per atom); far at T = 40, where qc_md_boys runs its asymptotic branch at orders up to 13."""
    import qchem_rs_amd as q
    name = case.split("-atom")[0]
    m = BUILDERS[name]()[0]
    _far_sides(name, m)
    s = q.System(m)
    s.set_schwarz(0.0)
    coords = GRAD_COORDS[case]
    if name.startswith("tetra"):             # one coordinate per atom, every axis among them
        assert {a for a, _ in coords} == set(range(len(m.atoms))) and {k for _, k in coords} == {0, 1, 2}
    (P, W), (Da, Db, Wu) = _densities(s.n)
    syn.check_terms(s, m, coords, P, 0.5 * P, 0.5 * P, W, 1)
    syn.check_terms(s, m, coords, Da + Db, Da, Db, Wu, 2)
    s.close()


def _cartesian_rotation(m, R):
    """U with phi_i(R^T r) = sum_j U[i, j] phi'_j(r) for the all-Cartesian shells of m (phi') of the copy rotated by R): a Cartesian
    shell spans every monomial of its degree, so a rotation mixes functions inside a shell only.  Each function is normalised on its own,
    N(a, b, c) ~ 1 / sqrt((2a-1)!! (2b-1)!! (2c-1)!!).  No integral enters."""
    from itertools import product
    from math import factorial, prod
    assert not np.any(m.shell_pure)
    dfact = lambda k: prod(range(k, 0, -2)) if k > 0 else 1
    carts = lambda L: [(lx, ly, L - lx - ly) for lx in range(L, -1, -1) for ly in range(L - lx, -1, -1)]
    blocks = []
    for L in m.shell_L:
        cl = carts(int(L))
        norm = np.array([1.0 / np.sqrt(dfact(2 * a - 1) * dfact(2 * b - 1) * dfact(2 * c - 1)) for a, b, c in cl])
        M = np.zeros((len(cl), len(cl)))
        for i, mono in enumerate(cl):
            # prod_k ((R^T r)_k)^(mono_k), (R^T r)_k = sum_l R[l, k] r_l: choose for each of the L factors which r_l it contributes
            axes = [k for k in range(3) for _ in range(mono[k])]
            for choice in product(range(3), repeat=len(axes)):
                e = [0, 0, 0]
                c = 1.0
                for k, l in zip(axes, choice):
                    e[l] += 1
                    c *= R[l, k]
                M[i, cl.index(tuple(e))] += c
        blocks.append(norm[:, None] * M / norm[None, :])
    n = sum(len(b) for b in blocks)
    U, pos = np.zeros((n, n)), 0
    for b in blocks:
        U[pos:pos + len(b), pos:pos + len(b)] = b
        pos += len(b)
    return U


def _plane_rotation(th, i, j):
    M = np.eye(3)
    M[i, i] = M[j, j] = np.cos(th)
    M[i, j], M[j, i] = -np.sin(th), np.sin(th)
    return M


def test_gradient_invariants_at_general_position():
    """tetra (Cartesian, one primitive): each of the four terms sums to zero over the atoms (1e-11), and the terms of a rigidly rotated
    and shifted copy are the rotated terms (1e-10).  The densities of the copy are pulled back shell by shell with the monomial
    representation of the rotation - no oracle, no SCF - and that pull-back is itself checked on the GPU's overlap matrices."""
    import qchem_rs_amd as q
    m = BUILDERS["tetra-cart-1"]()[0]
    s = q.System(m)
    s.set_schwarz(0.0)
    (P, W), (Da, Db, Wu) = _densities(s.n)
    t = np.array(s.gradient(P, W))
    tu = np.array(s.gradient(Da, Wu, Db=Db))
    for terms in (t, tu):
        assert np.abs(terms).max() > 1e-3
        assert np.abs(terms.sum(axis=1)).max() <= 1e-11, np.abs(terms.sum(axis=1)).max(axis=1)
    R = _plane_rotation(0.7, 0, 1) @ _plane_rotation(-1.1, 1, 2) @ _plane_rotation(0.4, 0, 2)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.abs(R).min() > 0.05          # skew: no axis kept, no zero entry
    m2 = syn.rotated(m, R, shift=(0.3, -1.1, 2.0))
    s2 = q.System(m2)
    s2.set_schwarz(0.0)
    U = _cartesian_rotation(m, R)
    S, S2 = s.one_electron_gpu(0), s2.one_electron_gpu(0)
    assert np.abs(U @ S2 @ U.T - S).max() < 1e-12                                     # <phi_i o R^T | phi_j o R^T> = S_ij
    back = lambda D: U.T @ D @ U
    t2 = np.array(s2.gradient(back(P), back(W)))
    tu2 = np.array(s2.gradient(back(Da), back(Wu), Db=back(Db)))
    for x, y in ((t, t2), (tu, tu2)):
        assert np.abs(y - x @ R.T).max() <= 1e-10, np.abs(y - x @ R.T).max(axis=(1, 2))
    s.close(); s2.close()
