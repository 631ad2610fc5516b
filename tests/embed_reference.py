"""References of the point-charge embedding tests, independent of the library's code.

  THREE                          the three integer charges of the oracle checks: (+1, -1, +2) at (3, .5, .2), (-1, 3, 1), (.3, -2.8, -2) bohr
  embedded_ghost(m, pos, Z)      the molecule plus shell-less atoms of integer Z at pos (the construction of points_reference.ghost_system
                                 with the molecule's own nuclei kept): the oracle's nuclear() is then V + V_pc, its nuclear_repulsion()
                                 Vnn + E_nq + E_cc, its SCF the embedded SCF
  e_nq, e_cc, e_cc_gradient      numpy: sum_A sum_c Z_A q_c / |R_A - R_c|; the charge-charge energy and its derivative by the charges
  charge_set(m, seed)            the 300 real charges of the GPU tests: points_reference.sample_points without the nuclei, filled up with
                                 normal points; q normal, five of them exactly 0
  field_points(m, seed, k)       k points at least 1 bohr from every nucleus
  ghost_term_stencil(...)        five-point stencils (h = 1e-3) of the oracle's Vnn and tr(P (T + V)) on the ghost system along an atom's or
                                 a charge's coordinate
"""
import numpy as np

import points_reference as PR
from synthetic_systems import H

THREE_Q = np.array([1.0, -1.0, 2.0])
THREE_POS = np.array([[3.0, 0.5, 0.2], [-1.0, 3.0, 1.0], [0.3, -2.8, -2.0]])


def embedded_ghost(m, pos, Z, atom_shift=None, charge_shift=None):
    """atom_shift / charge_shift: (index, axis, d) moves one atom / one charge"""
    import qchem_rs_amd as q
    atoms = [q.Atom(a.ordinal, list(a.position)) for a in m.atoms]
    if atom_shift is not None:
        atoms[atom_shift[0]].position[atom_shift[1]] += atom_shift[2]
    P = np.array(pos, float)
    if charge_shift is not None:
        P[charge_shift[0], charge_shift[1]] += charge_shift[2]
    atoms += [q.Atom(int(z), [float(x) for x in r]) for z, r in zip(Z, P)]
    return q.MolecularSystem(atoms, m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim, m.exponents, m.coefficients)


def e_nq(R, Z, pos, q):
    return float(sum(Z[a] * q[c] / np.linalg.norm(R[a] - pos[c]) for a in range(len(Z)) for c in range(len(q))))


def e_cc(pos, q):
    return float(sum(q[c] * q[d] / np.linalg.norm(pos[c] - pos[d]) for c in range(len(q)) for d in range(c)))


def e_cc_gradient(pos, q):
    g = np.zeros((len(q), 3))
    for c in range(len(q)):
        for d in range(len(q)):
            if c != d:
                r = pos[c] - pos[d]
                g[c] -= q[c] * q[d] * r / np.linalg.norm(r) ** 3
    return g


def charge_set(m, seed):
    nat = len(m.atoms)
    P = PR.sample_points(m, seed)[nat:]
    rng = np.random.default_rng(9000 + seed)
    P = np.concatenate([P, m.coordinates().mean(axis=0) + 2.0 * rng.standard_normal((PR.NPOINTS - len(P), 3))])
    q = rng.standard_normal(len(P))
    q[[3, 17, 255, 256, 299]] = 0.0
    return np.ascontiguousarray(P), q


def field_points(m, seed, k):
    R = m.coordinates()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < k:
        p = R.mean(axis=0) + 2.0 * rng.standard_normal(3)
        if np.linalg.norm(R - p, axis=1).min() >= 1.0:
            out.append(p)
    return np.array(out)


def ghost_terms(m, pos, Z, Pt, **shift):
    """[Vnn, tr(Pt (T + V))] of the ghost system"""
    from oracle.oracle import Oracle
    o = Oracle(embedded_ghost(m, pos, Z, **shift))
    return np.array([o.nuclear_repulsion(), float(np.sum(Pt * (o.kinetic() + o.nuclear())))])


def ghost_term_stencil(m, pos, Z, Pt, which, index, axis, h=H):
    """which: "atom_shift" or "charge_shift" """
    f = {k: ghost_terms(m, pos, Z, Pt, **{which: (index, axis, k * h)}) for k in (-2, -1, 1, 2)}
    return (f[-2] - 8 * f[-1] + 8 * f[1] - f[2]) / (12 * h)
