"""Synthetic systems in general position, built from raw shell arrays (no basis file), and the finite-difference machinery of the
gradient term tests.  Every molecule the shipped data gives f functions lies in a coordinate plane or on an axis; these do not.

  tetra(pure, nprim)  four centres, no three collinear, no shared coordinate; one s, p, d and f shell on each.  n = 64 (pure d and f:
                      exactly the limit of the one-workgroup SCF path) or 80 (Cartesian: the generic launch path); every (LAB, LCD)
                      class occurs with four distinct centres.
  deep()              three centres; 13-primitive s and p shells, so the same-centre ss and ps pairs keep 169 > 127 primitive pairs and
                      the bra-major work lists carry plain pair indices instead of packed (pair | first | length) entries.
  far(R)              two centres R apart along a skew direction, single-primitive s..f shells of exponent 1.2: the Boys argument of
                      a same-centre bra against a same-centre ket is T = 1.2 R^2.

  spread()            five centres strung out over 19 bohr along the skew direction (off the line by up to 1.1 bohr), contracted s and p
                      shells on each, two pure d shells and a pure f shell: n = 37, Schwarz factors from 1e-41 to 1.4, so that screening
                      bites at every threshold and the far pairs fall under the primitive cut-off and are not stored at all.

Each builder returns (MolecularSystem, atoms); displaced() gives the same shells with one atom moved.  All are deterministic.

TILE_SYSTEMS are molecules of the shipped data, two of them in an edited basis, chosen by their counts of occupied and virtual orbitals
(o, v): the excited-state assembly kernel works on 32 x 32 tiles of virtual pairs and the reduced-space kernels stride over a vector
1024 elements at a time.  load_system() loads one of them, or any mol/basis pair of the shipped data."""
import json
import os
import tempfile

import numpy as np

import qchem_rs_amd as q

TETRA_XYZ = [(0.0, 0.0, 0.0), (1.9, 0.3, -0.4), (-0.5, 1.7, 0.6), (0.4, -0.7, 1.8)]
DEEP_XYZ = [(0.0, 0.0, 0.0), (0.9, 0.5, -0.7), (-0.6, 1.1, 0.8)]
FAR_DIRECTION = (4.1, -3.9, 4.2)
FAR_EXPONENT = 1.2
DEEP_NPRIM = 13


def _system(xyz, shells):
    """shells: (atom, L, pure, exponents, coefficients) in order; every atom is a hydrogen (Z = 1)"""
    atoms = [q.Atom(1, [float(x) for x in r]) for r in xyz]
    m = q.MolecularSystem(atoms,
                          np.asarray([s[0] for s in shells], np.int32), np.asarray([s[1] for s in shells], np.int32),
                          np.asarray([1 if (s[2] and s[1] >= 2) else 0 for s in shells], np.int32),
                          np.asarray([len(s[3]) for s in shells], np.int32),
                          np.asarray([e for s in shells for e in s[3]], np.float64),
                          np.asarray([c for s in shells for c in s[4]], np.float64))
    return m, atoms


def tetra(pure, nprim):
    rng = np.random.default_rng(20240 + nprim)
    shells = []
    for atom in range(4):
        for L in range(4):
            exps = [[0.9, 1.1, 1.3, 1.0][L] * (1 + 0.13 * atom) * 3.1 ** k for k in range(nprim)]
            shells.append((atom, L, pure, exps, (0.3 + rng.uniform(0, 1, nprim)).tolist()))
    return _system(TETRA_XYZ, shells)


def deep():
    rng = np.random.default_rng(1313)
    long = lambda: ([0.08 * 2.3 ** k for k in range(DEEP_NPRIM)], (0.3 + rng.uniform(0, 1, DEEP_NPRIM)).tolist())
    one = ([0.7], [1.0])
    shells = [(0, 0, True) + long(), (0, 1, True) + long(),
              (1, 0, True) + long(), (1, 1, True) + one,
              (2, 1, True) + long(), (2, 0, True) + one, (2, 2, False) + one]          # (the d shell is Cartesian: n = 18)
    return _system(DEEP_XYZ, shells)


SPREAD_ALONG = (0.0, 2.6, 6.5, 12.0, 19.0)          # bohr along FAR_DIRECTION ...
SPREAD_ACROSS = (0.0, 0.4, -0.7, 1.1, 0.3)          # ... and along (1, 2, -0.5)


def spread():
    u = np.asarray(FAR_DIRECTION) / np.linalg.norm(FAR_DIRECTION)
    v = np.asarray((1.0, 2.0, -0.5)) / np.linalg.norm((1.0, 2.0, -0.5))
    xyz = [tuple(a * u + b * v) for a, b in zip(SPREAD_ALONG, SPREAD_ACROSS)]
    shells = []
    for a in range(5):
        shells.append((a, 0, True, [18.0 * (1 + 0.1 * a), 2.7, 0.45], [0.4, 0.7, 0.5]))
        shells.append((a, 1, True, [3.3 * (1 + 0.07 * a), 0.55], [0.6, 0.8]))
    shells += [(1, 2, True, [0.9], [1.0]), (3, 2, True, [0.7], [1.0]), (2, 3, True, [1.1], [1.0])]
    return _system(xyz, shells)


def far_distance(T):
    """the separation at which same-centre bra and ket pairs (alpha = 1.2) meet at the Boys argument T"""
    return float(np.sqrt(T / FAR_EXPONENT))


def far(R):
    u = np.asarray(FAR_DIRECTION) / np.linalg.norm(FAR_DIRECTION)
    shells = [(atom, L, True, [FAR_EXPONENT], [1.0]) for atom in range(2) for L in range(4)]
    return _system([(0.0, 0.0, 0.0), tuple(u * R)], shells)


def far_boys_argument(m):
    """T = alpha |P - Q|^2 of the (A A | B B) primitive quartets of a far() system, from its exponents and coordinates"""
    a = float(m.exponents[0])
    assert np.all(m.exponents == a)
    p = qq = 2 * a
    R = m.coordinates()
    return p * qq / (p + qq) * float(np.sum((R[0] - R[1]) ** 2))


T_LOW, T_HIGH = 40.0, 59.0           # Boys arguments of the two far() systems of the tests
BOYS_SERIES_SWITCH = 38.0            # qc_md_boys (qc_md.h): asymptotic form from here on
BOYS_XMAX = 41.9                     # QC_BOYS_XMAX (qc_internal.h): end of the table of qc_boys<L>

BUILDERS = {"tetra-pure-1": lambda: tetra(True, 1), "tetra-cart-1": lambda: tetra(False, 1),
            "tetra-pure-2": lambda: tetra(True, 2), "tetra-cart-2": lambda: tetra(False, 2),
            "deep": deep, "spread": spread, "far-40": lambda: far(far_distance(T_LOW)), "far-59": lambda: far(far_distance(T_HIGH))}
SIZES = {"tetra-pure-1": (64, 9316), "tetra-cart-1": (80, 9316), "tetra-pure-2": (64, 9316), "tetra-cart-2": (80, 9316),
         "deep": (18, 406), "spread": (37, 4186), "far-40": (32, 666), "far-59": (32, 666)}          # (n, unique shell quartets)


# ---------------------------------------------------------------------------------------------------------------------------------
# Molecules by orbital counts (the excited states, the stability analysis and CPHF past one tile and past dimension 1024).

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")


def _edit_cartesian_o_d(b):
    """6-311++G**: the d shell of oxygen as six Cartesian functions (n + 1)"""
    d = [sh for sh in b["elements"]["8"]["electron_shells"] if sh["angular_momentum"] == [2]]
    assert len(d) == 1 and d[0]["function_type"] == "gto_spherical"
    d[0]["function_type"] = "gto_cartesian"


def _edit_cut_vtz(b):
    """cc-pVTZ without the f shell of oxygen, without the d shell of hydrogen and with two of the three contractions of the oxygen p shell"""
    O, H = b["elements"]["8"]["electron_shells"], b["elements"]["1"]["electron_shells"]
    assert [sh["angular_momentum"] for sh in O] == [[0], [1], [2], [2], [3]] and [sh["angular_momentum"] for sh in H] == [[0], [1], [2]]
    assert len(O[1]["coefficients"]) == 3
    del O[1]["coefficients"][2]
    del O[4]
    del H[2]


EDITED_BASES = {"6-311++G_st_st+cart-d": ("6-311++G_st_st", _edit_cartesian_o_d), "cc-pVTZ-cut": ("cc-pVTZ", _edit_cut_vtz)}

# name -> (n, o, v); d = o v.  What each reaches: tests/test_excitations_gpu.py
TILE_SYSTEMS = {"water/6-311++G_st_st": (36, 5, 31), "water/6-311++G_st_st+cart-d": (37, 5, 32), "water/cc-pVTZ-cut": (38, 5, 33),
                "water/cc-pVTZ": (58, 5, 53), "ethylene/6-311++G_st_st": (72, 8, 64), "chloroform/6-31G_st_st": (77, 29, 48)}


def load_system(name):
    """MolecularSystem of "mol/basis": a basis file of data/basis, or one of EDITED_BASES written to a temporary directory from its file"""
    mol, basis = name.split("/")
    mol = os.path.join(DATA, "mol", mol + ".json")
    if basis not in EDITED_BASES:
        return q.MolecularSystem.load(mol, q.BasisSet.load(os.path.join(DATA, "basis", basis + ".json")))
    parent, edit = EDITED_BASES[basis]
    with open(os.path.join(DATA, "basis", parent + ".json")) as f:
        b = json.load(f)
    edit(b)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, basis + ".json")
        with open(path, "w") as f:
            json.dump(b, f)
        return q.MolecularSystem.load(mol, q.BasisSet.load(path))


def orbital_counts(m):
    """(n, o, v) of the closed-shell determinant of a MolecularSystem"""
    from oracle.oracle import Oracle
    n, o = Oracle(m).n, int(np.sum(m.atomic_numbers())) // 2
    return n, o, n - o


def displaced(m, atom, axis, d):
    """the shells of m with one atom moved by d along one axis"""
    atoms = [q.Atom(a.ordinal, list(a.position)) for a in m.atoms]
    atoms[atom].position[axis] += d
    return q.MolecularSystem(atoms, m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim, m.exponents, m.coefficients)


def rotated(m, R, shift=(0.0, 0.0, 0.0)):
    atoms = [q.Atom(a.ordinal, (R @ np.asarray(a.position) + np.asarray(shift)).tolist()) for a in m.atoms]
    return q.MolecularSystem(atoms, m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim, m.exponents, m.coefficients)


def same_centre_ket_primitives(m):
    """most primitive pairs of an ss or ps shell pair on one centre (nothing of such a pair is below the primitive cutoff: its
    Gaussian-product factor is exp(-mu 0) = 1) - the pairs the bra-major kernels take as kets"""
    return max(int(m.shell_nprim[a] * m.shell_nprim[b]) for a in range(m.n_shells) for b in range(a + 1)
               if m.shell_atom[a] == m.shell_atom[b] and m.shell_L[a] + m.shell_L[b] <= 1)


def skew_signs(n, k):
    """the k-th +-1 vector under which tests/golden/skew_quartets_golden.json sums a whole ERI block"""
    return np.random.default_rng(7000 + k).integers(0, 2, n) * 2.0 - 1.0


def n_unique_quartets(m):
    npair = m.n_shells * (m.n_shells + 1) // 2
    return npair * (npair + 1) // 2


def oracle_threads():
    return min(16, len(os.sched_getaffinity(0)))


def oracle_tensor(o):
    """the oracle's dense tensor on up to 16 threads (bit for bit the serial one: test_openmp_baseline_equals_the_serial_tensor)"""
    I, _ = o.eri_strided_mt(0, 1, oracle_threads())
    return I


def rand_sym(n, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) * scale
    return 0.5 * (A + A.T)


# ---------------------------------------------------------------------------------------------------------------------------------
# Gradient terms against a five-point stencil of the oracle's integrals at fixed densities (shared with test_gradient_gpu.py).

H = 1e-3


_INTEGRALS = {}          # geometry -> (Vnn, T + V, S, tensor) of small systems: the RHF and the UHF check of a test visit the same geometries


def _oracle_integrals(m):
    from oracle.oracle import Oracle
    key = tuple(np.asarray(a).tobytes() for a in (m.coordinates(), m.atomic_numbers(), m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim,
                                                   m.exponents, m.coefficients))
    if key not in _INTEGRALS:
        o = Oracle(m)
        val = (o.nuclear_repulsion(), o.kinetic() + o.nuclear(), o.overlap(), oracle_tensor(o))
        if val[3].nbytes > 8 << 20:          # (a tensor of n > 32 is not kept)
            return val
        if len(_INTEGRALS) >= 64:
            _INTEGRALS.pop(next(iter(_INTEGRALS)))
        _INTEGRALS[key] = val
    return _INTEGRALS[key]


def term_energies(m, Pt, Pa, Pb, W, mask=None):
    """[Vnn, core, overlap, two-electron] of fixed AO densities, from the oracle's integrals at geometry m.  mask (n, n, n, n), if
    given, multiplies the tensor: the two-electron energy over the kept integrals alone (a screened build's energy)"""
    vnn, h, S, I = _oracle_integrals(m)
    if mask is not None:
        I = I * mask
    e2 = 0.5 * (np.einsum("mnls,mn,ls->", I, Pt, Pt, optimize=True) - np.einsum("mnls,ml,ns->", I, Pa, Pa, optimize=True)
                - np.einsum("mnls,ml,ns->", I, Pb, Pb, optimize=True))
    return np.array([vnn, np.sum(Pt * h), -np.sum(W * S), e2])


def fd_terms(m, coord, Pt, Pa, Pb, W, h=H, mask=None):
    """five-point stencil of term_energies along one coordinate; the mask, if any, is the same at every displaced geometry (the
    derivative of the energy over a FIXED set of kept quartets - what a gradient over screened work lists computes)"""
    atom, axis = coord
    f = {k: term_energies(displaced(m, atom, axis, k * h), Pt, Pa, Pb, W, mask) for k in (-2, -1, 1, 2)}
    return (f[-2] - 8 * f[-1] + 8 * f[1] - f[2]) / (12 * h)


def check_terms(s, m, coords, Pt, Pa, Pb, W, nspin):
    if nspin == 1:
        t = np.array(s.gradient(Pt, W))
    else:
        t = np.array(s.gradient(Pa, W, Db=Pb))
    for c in coords:
        fd = fd_terms(m, c, Pt, Pa, Pb, W)
        for k in range(4):
            an = t[k][c[0], c[1]]
            assert abs(an - fd[k]) <= 1e-9 * max(1.0, abs(fd[k])), (c, k, an, fd[k])
