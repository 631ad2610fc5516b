"""numpy references of the Cartesian multipole matrices, the population analysis and the ESP charge fit, independent of the library.

Multipole matrices: the Obara-Saika overlap tables of tests/dipole_reference.py with the ket raised, through the binomial expansion about
the ket centre B,
  (x - O)^m = sum_k C(m, k) (x - B)^k (B - O)^(m-k)   ->   <i| (x - O)^m |j> = sum_k C(m, k) (B - O)^(m-k) S_i(j+k),
so a moment integral is a sum of overlaps with the ket raised by k <= 4.  No Hermite moments: the library's recurrence and these
binomials share nothing.  Shells, normalisation and transforms are those of dipole_reference (which proves itself on the overlap).

Populations and bond orders from (P_alpha, P_beta, S) with numpy.linalg.eigh for S^1/2; the Merz-Kollman grid rule restated; the
constrained least-squares fit through its KKT system with numpy.linalg.solve."""
from math import comb

import numpy as np

import dipole_reference as D

BOHR_ANGSTROM = 0.529177210903
VDW_ANGSTROM = {1: 1.20, 2: 1.40, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 10: 1.54, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 18: 1.88}
DEFAULT_SCALES = (1.4, 1.6, 1.8, 2.0)


def components(order):
    """(i, j, k) by i + j + k ascending, then i descending, then j descending"""
    return [(i, j, l - i - j) for l in range(order + 1) for i in range(l, -1, -1) for j in range(l - i, -1, -1)]


def order_slices(order):
    off = [l * (l + 1) * (l + 2) // 6 for l in range(order + 2)]
    return [slice(off[l], off[l + 1]) for l in range(order + 1)]


def multipole_matrices(m, order, origin=(0.0, 0.0, 0.0)):
    """(count, n, n): <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b> for every component of components(order)"""
    sh = D.shells_of(m)
    off = np.concatenate([[0], np.cumsum([s.nfunc for s in sh])])
    n, comps = int(off[-1]), np.array(components(order))
    O = np.asarray(origin, float)
    out = np.zeros((len(comps), n, n))
    for ia, A in enumerate(sh):
        ca = np.array(A.comps)
        for ib, B in enumerate(sh):
            cb = np.array(B.comps)
            cc = A.c[:, None] * B.c[None, :]
            G = []                                                      # per axis: [i, j, m, prim a, prim b]
            for k in range(3):
                tb = D.os_tables(A.L, B.L + order, A.e[:, None], B.e[None, :], A.A[k], B.A[k])
                g = np.zeros((A.L + 1, B.L + 1, order + 1) + cc.shape)
                for i in range(A.L + 1):
                    for j in range(B.L + 1):
                        for p in range(order + 1):
                            g[i, j, p] = sum(comb(p, r) * (B.A[k] - O[k]) ** (p - r) * tb[i][j + r] for r in range(p + 1))
                G.append(g)
            blk = np.ones((len(ca), len(cb), len(comps)) + cc.shape)
            for k in range(3):
                blk = blk * G[k][ca[:, k][:, None, None], cb[:, k][None, :, None], comps[:, k][None, None, :]]
            cm = np.einsum("xycpq,pq->cxy", blk, cc)
            out[:, off[ia]:off[ia + 1], off[ib]:off[ib + 1]] = np.einsum("fx,cxy,gy->cfg", A.T, cm, B.T)
    return out


def nuclear_moments(m, order, origin=(0.0, 0.0, 0.0)):
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3) - np.asarray(origin, float)
    Z = np.asarray(m.atomic_numbers(), float)
    return np.array([np.sum(Z * xyz[:, 0] ** i * xyz[:, 1] ** j * xyz[:, 2] ** k) for i, j, k in components(order)])


def nuclear_moments_abs(m, order, origin=(0.0, 0.0, 0.0)):
    """sum_A Z_A |R_A^c|: the magnitude of the terms of the nuclear sum"""
    xyz = np.abs(np.asarray(m.coordinates(), float).reshape(-1, 3) - np.asarray(origin, float))
    Z = np.asarray(m.atomic_numbers(), float)
    return np.array([np.sum(Z * xyz[:, 0] ** i * xyz[:, 1] ** j * xyz[:, 2] ** k) for i, j, k in components(order)])


def traceless_quadrupole(second):
    """xx xy xz yy yz zz of (3 Q_ab - delta_ab tr Q) / 2 from the six second moments in that order"""
    q = np.asarray(second, float)
    t = q[0] + q[3] + q[5]
    return 0.5 * (3.0 * q - t * np.array([1.0, 0, 0, 1.0, 0, 1.0]))


def function_atoms(m):
    """atom of every basis function"""
    out = []
    for s in range(m.n_shells):
        L = int(m.shell_L[s])
        out += [int(m.shell_atom[s])] * ((2 * L + 1) if (m.shell_pure[s] and L >= 2) else (L + 1) * (L + 2) // 2)
    return np.array(out)


def populations(m, scheme, Pa, Pb, S):
    """(charges, spin, orbital, bond_orders) - scheme "mulliken": A_x = P_x S, Mayer; "lowdin": A_x = S^1/2 P_x S^1/2, Wiberg"""
    fa = function_atoms(m)
    Z = np.asarray(m.atomic_numbers(), float)
    na = len(Z)
    Pt, Ps = Pa + Pb, Pa - Pb
    if scheme == "mulliken":
        At, As = Pt @ S, Ps @ S
    else:
        w, U = np.linalg.eigh(S)
        Sh = (U * np.sqrt(w)) @ U.T
        At, As = Sh @ Pt @ Sh, Sh @ Ps @ Sh
    orb = np.diag(At).copy()
    sel = [fa == a for a in range(na)]
    N = np.array([orb[s].sum() for s in sel])
    spin = np.array([np.diag(As)[s].sum() for s in sel])
    W = At * At.T + As * As.T
    bo = np.array([[W[np.ix_(sel[a], sel[b])].sum() for b in range(na)] for a in range(na)])
    return Z - N, spin, orb, bo


def radii_bohr(m):
    return np.array([VDW_ANGSTROM.get(int(z), 2.00) for z in m.atomic_numbers()]) / BOHR_ANGSTROM


def esp_grid(m, scales=DEFAULT_SCALES, density=None, with_margin=False):
    """the grid rule restated: (points (npts, 3), and with_margin the smallest | distance - exclusion radius | over all candidates)"""
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
    r = radii_bohr(m)
    dens = BOHR_ANGSTROM ** 2 if density is None else density
    pts, margin = [], np.inf
    for f in scales:
        for A in range(len(xyz)):
            R = f * r[A]
            N = int(np.ceil(dens * 4.0 * np.pi * R * R))
            k = np.arange(N)
            z = 1.0 - (2.0 * k + 1.0) / N
            phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
            rho = np.sqrt(1.0 - z * z)
            cand = xyz[A] + R * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
            keep = np.ones(N, bool)
            for B in range(len(xyz)):
                if B == A:
                    continue
                d = np.linalg.norm(cand - xyz[B], axis=1)
                margin = min(margin, float(np.abs(d - f * r[B]).min()))
                keep &= d >= f * r[B]
            pts.append(cand[keep])
    P = np.concatenate(pts) if pts else np.zeros((0, 3))
    return (P, margin) if with_margin else P


def design_matrix(m, points):
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
    return 1.0 / np.linalg.norm(np.asarray(points, float)[:, None, :] - xyz[None, :, :], axis=2)


def kkt_fit(m, points, v, total_charge):
    """(charges, rms, rrms, dipole, cond(A^T A)) of the constrained fit"""
    A = design_matrix(m, points)
    na = A.shape[1]
    K = np.zeros((na + 1, na + 1))
    K[:na, :na] = A.T @ A
    K[:na, na] = K[na, :na] = 1.0
    q = np.linalg.solve(K, np.concatenate([A.T @ v, [total_charge]]))[:na]
    res = v - A @ q
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
    return q, float(np.sqrt(np.mean(res ** 2))), float(np.sqrt(np.sum(res ** 2) / np.sum(v ** 2))), q @ xyz, float(np.linalg.cond(A.T @ A))
