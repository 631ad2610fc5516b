"""numpy / oracle references of the values on points, independent of the library's code.

  phi(m, points)                 basis functions on points from dipole_reference.shells_of(m): contracted radial part x Cartesian
                                 monomials x the shell's transform T (normalisation of the oracle, see dipole_reference.py)
  potential_matrix_oracle(m, r)  A_ab = (a| 1/|r' - r| |b) from the ORACLE's nuclear-attraction matrix: the same shells on atoms whose
                                 atomic numbers are all 0, plus one shell-less atom with Z = 1 at r, give V = -A.  (It agrees with the
                                 difference route V(without the extra atom) - V(with it) to 1.2e-15 on tetra(True, 2).)  5-45 ms a point.
  sample_points(m, seed)           the 300 deterministic points of the GPU tests
  nuclear_potential(m, points)   sum_A Z_A / |r - R_A|, +inf on a nucleus
"""
import numpy as np

import dipole_reference as DR
import synthetic_systems as Y


def phi(m, points):
    """(npts, n)"""
    P = np.asarray(points, float).reshape(-1, 3)
    cols = []
    for s in DR.shells_of(m):
        d = P - s.A
        radial = (s.c[None, :] * np.exp(-s.e[None, :] * (d ** 2).sum(axis=1)[:, None])).sum(axis=1)
        mono = np.stack([d[:, 0] ** lx * d[:, 1] ** ly * d[:, 2] ** lz for lx, ly, lz in s.comps], axis=1)      # (0.0 ** 0 == 1.0 in numpy)
        cols.append((mono * radial[:, None]) @ s.T.T)
    return np.concatenate(cols, axis=1)


def ghost_system(m, r):
    """the shells of m on atoms of atomic number 0, and one more atom without shells, Z = 1, at r"""
    import qchem_rs_amd as q
    atoms = [q.Atom(0, list(a.position)) for a in m.atoms] + [q.Atom(1, [float(x) for x in r])]
    return q.MolecularSystem(atoms, m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim, m.exponents, m.coefficients)


def potential_matrix_oracle(m, r):
    from oracle.oracle import Oracle
    return -Oracle(ghost_system(m, r)).nuclear()


def nuclear_potential(m, points):
    P = np.asarray(points, float).reshape(-1, 3)
    Z, R = np.asarray(m.atomic_numbers(), float), m.coordinates()
    with np.errstate(divide="ignore"):
        return (Z[None, :] / np.sqrt(((P[:, None, :] - R[None, :, :]) ** 2).sum(axis=2))).sum(axis=1)


NPOINTS = 300


def sample_points(m, seed, boys_switch=False):
    """every nucleus; one point 1e-7 bohr off the first; the midpoints of all nucleus pairs; two points 30 and 200 bohr out along
    FAR_DIRECTION; (boys_switch: three points at distances d from centre 0 with 2.4 d^2 = 41.85, 41.90, 41.95 - both sides of QC_BOYS_XMAX
    for the same-centre pairs of far()); the rest normal with sigma = 2 bohr around the centroid.  300 in all."""
    R = m.coordinates()
    u = np.asarray(Y.FAR_DIRECTION) / np.linalg.norm(Y.FAR_DIRECTION)
    pts = [r.copy() for r in R]
    pts.append(R[0] + np.array([1e-7, 0.0, 0.0]))
    pts += [0.5 * (R[i] + R[j]) for i in range(len(R)) for j in range(i)]
    c = R.mean(axis=0)
    pts += [c + 30.0 * u, c + 200.0 * u]
    if boys_switch:
        v = np.array([0.3, 0.5, -0.8]) / np.linalg.norm([0.3, 0.5, -0.8])
        pts += [R[0] + np.sqrt(x / (2.0 * Y.FAR_EXPONENT)) * v for x in (41.85, 41.90, 41.95)]
    rng = np.random.default_rng(seed)
    pts += list(c + 2.0 * rng.standard_normal((NPOINTS - len(pts), 3)))
    return np.ascontiguousarray(pts, float)
