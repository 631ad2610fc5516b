"""numpy reference of the dipole matrices and of the static polarizability, independent of the library's McMurchie-Davidson code.

One-dimensional Obara-Saika overlap tables over Cartesian primitives,
  S_00 = sqrt(pi/p) exp(-mu X_AB^2),  S_(i+1)j = X_PA S_ij + (i S_(i-1)j + j S_i(j-1)) / 2p,  S_i(j+1) = X_PB S_ij + (same),
give, from one and the same set of tables, the overlap S = Sx Sy Sz and the dipole matrices through x = (x - A_x) + A_x:
  <a| x - O_x |b> = S_(a+1)b + (A_x - O_x) S_ab   on the axis of the component, the plain S_ab on the other two.
Normalisation and Cartesian-to-pure transforms follow the conventions of the oracle (oracle/qc_oracle.c): Cartesian components in the
order lx descending then ly descending; contraction coefficients times the norm of the x^L primitive; real solid harmonics m = -l..l
(Helgaker, Jorgensen, Olsen eq. 6.4.47); every function scaled to unit self-overlap.  The reference proves itself on the overlap: its S
must reproduce Oracle(m).overlap() before its M is trusted (tests/test_dipole_host.py).

polarizability_rhf / polarizability_uhf: the dense (A + B) of tests/stability_reference.py, numpy.linalg.solve, and
  alpha_pq = c r^p . (A + B)^-1 r^q,  r^q = C_occ^T M_q C_virt,  c = 4 (RHF, singlet operator) or 2 (UHF, vector [x^alpha; x^beta]).
"""
from math import comb

import numpy as np

import stability_reference as R


def cart_components(L):
    return [(lx, ly, L - lx - ly) for lx in range(L, -1, -1) for ly in range(L - lx, -1, -1)]


def _dfact(n):
    r = 1.0
    while n > 1:
        r *= n
        n -= 2
    return r


def solid_harmonic_rows(l):
    """(2l + 1, ncart) coefficients of the real solid harmonics S_lm, m = -l..l, in the Cartesian monomials (scale fixed later)"""
    comps = cart_components(l)
    T = np.zeros((2 * l + 1, len(comps)))
    for m in range(-l, l + 1):
        am, vm2 = abs(m), (1 if m < 0 else 0)                     # v_m = 0 or 1/2, kept doubled
        for t in range((l - am) // 2 + 1):
            for u in range(t + 1):
                for v2 in range(vm2, am + 1, 2):
                    c = (-1.0) ** (t + (v2 - vm2) // 2) * 0.25 ** t * comb(l, t) * comb(l - t, am + t) * comb(t, u) * comb(am, v2)
                    e = (2 * t + am - 2 * u - v2, 2 * u + v2, l - 2 * t - am)
                    if min(e) >= 0:
                        T[m + l, comps.index(e)] += c
    return T


def os_tables(imax, jmax, a, b, A, B):
    """S[i][j] for i <= imax, j <= jmax on one axis; a, b: exponent arrays that broadcast against each other"""
    p = a + b
    P = (a * A + b * B) / p
    xpa, xpb, h = P - A, P - B, 0.5 / p
    S = [[None] * (jmax + 1) for _ in range(imax + 1)]
    S[0][0] = np.sqrt(np.pi / p) * np.exp(-a * b / p * (A - B) ** 2)
    for i in range(imax):
        S[i + 1][0] = xpa * S[i][0] + (i * h * S[i - 1][0] if i else 0.0)
    for i in range(imax + 1):
        for j in range(jmax):
            S[i][j + 1] = xpb * S[i][j] + (i * h * S[i - 1][j] if i else 0.0) + (j * h * S[i][j - 1] if j else 0.0)
    return S


class _Shell:
    def __init__(self, atom, L, pure, centre, exps, coefs):
        self.L, self.A, self.e = L, np.asarray(centre, float), np.asarray(exps, float)
        self.c = np.asarray(coefs, float) * (2.0 * self.e / np.pi) ** 0.75 * (4.0 * self.e) ** (0.5 * L) / np.sqrt(_dfact(2 * L - 1))
        self.comps = cart_components(L)
        T = solid_harmonic_rows(L) if (pure and L >= 2) else np.eye(len(self.comps))
        # unit self-overlap, from the same one-centre tables
        tb = os_tables(L, L, self.e[:, None], self.e[None, :], 0.0, 0.0)
        cc = self.c[:, None] * self.c[None, :]
        M = np.array([[np.sum(cc * tb[x[0]][y[0]] * tb[x[1]][y[1]] * tb[x[2]][y[2]]) for y in self.comps] for x in self.comps])
        self.T = T / np.sqrt(np.einsum("fx,xy,fy->f", T, M, T))[:, None]
        self.nfunc = T.shape[0]


def shells_of(m):
    """the shells of a MolecularSystem, in its order"""
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
    out, po = [], 0
    for s in range(m.n_shells):
        k = int(m.shell_nprim[s])
        out.append(_Shell(int(m.shell_atom[s]), int(m.shell_L[s]), bool(m.shell_pure[s]), xyz[int(m.shell_atom[s])],
                          m.exponents[po:po + k], m.coefficients[po:po + k]))
        po += k
    return out


def overlap_and_dipole(m, origin=(0.0, 0.0, 0.0)):
    """(S (n, n), M (3, n, n)) of a MolecularSystem, both from one set of 1-D tables per shell pair"""
    sh = shells_of(m)
    off = np.concatenate([[0], np.cumsum([s.nfunc for s in sh])])
    n = int(off[-1])
    S, M = np.zeros((n, n)), np.zeros((3, n, n))
    O = np.asarray(origin, float)
    for ia, A in enumerate(sh):
        for ib, B in enumerate(sh):
            tb = [os_tables(A.L + 1, B.L, A.e[:, None], B.e[None, :], A.A[k], B.A[k]) for k in range(3)]
            cc = A.c[:, None] * B.c[None, :]
            cs = np.zeros((len(A.comps), len(B.comps)))
            cm = np.zeros((3,) + cs.shape)
            for x, ca in enumerate(A.comps):
                for y, cb in enumerate(B.comps):
                    s1 = [tb[k][ca[k]][cb[k]] for k in range(3)]
                    cs[x, y] = np.sum(cc * s1[0] * s1[1] * s1[2])
                    for k in range(3):
                        d1 = list(s1)
                        d1[k] = tb[k][ca[k] + 1][cb[k]] + (A.A[k] - O[k]) * s1[k]
                        cm[k, x, y] = np.sum(cc * d1[0] * d1[1] * d1[2])
            ra, rb = slice(off[ia], off[ia + 1]), slice(off[ib], off[ib + 1])
            S[ra, rb] = A.T @ cs @ B.T.T
            for k in range(3):
                M[k][ra, rb] = A.T @ cm[k] @ B.T.T
    return S, M


def nuclear_dipole(m, origin=(0.0, 0.0, 0.0)):
    xyz = np.asarray(m.coordinates(), float).reshape(-1, 3)
    return (np.asarray(m.atomic_numbers(), float)[:, None] * (xyz - np.asarray(origin, float))).sum(axis=0)


def rhs(C, nocc, M):
    """(3, o * v): r^q = C_occ^T M_q C_virt, laid out [i * v + a]"""
    return np.array([(C[:, :nocc].T @ M[q] @ C[:, nocc:]).reshape(-1) for q in range(3)])


def polarizability_rhf(I, C, eps, nocc, M):
    """(alpha (3, 3), H = singlet (A + B), r (3, dim)) from an ERI tensor, orbitals and dipole matrices"""
    H, r = R.hessian_rhf(I, C, eps, nocc, 0), rhs(C, nocc, M)
    return 4.0 * r @ np.linalg.solve(H, r.T), H, r


def polarizability_uhf(I, Ca, ea, na, Cb, eb, nb, M):
    H, r = R.hessian_uhf(I, Ca, ea, na, Cb, eb, nb), np.concatenate([rhs(Ca, na, M), rhs(Cb, nb, M)], axis=1)
    return 2.0 * r @ np.linalg.solve(H, r.T), H, r


def uncoupled_rhf(C, eps, nocc, M):
    """alpha = 4 sum_ia r_ia r'_ia / (e_a - e_i): the limit without the two-electron response"""
    r = rhs(C, nocc, M)
    d = (eps[None, nocc:] - eps[:nocc, None]).reshape(-1)
    return 4.0 * (r / d) @ r.T
