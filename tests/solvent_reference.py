"""numpy / scipy statement of the conductor-like continuum (C-PCM / COSMO), the reference of test_solvent_host.py and
test_solvent_gpu.py.  Nothing here calls the library's solvent code: the surface, S, K, the response and the SCF loops are restated; the
integrals of the loops come from the oracle, and A(s_i) from the host entry qc_potential_matrix (pinned by test_points_host.py).

  surface   spheres of radius scale * r_vdW, N = ceil(density 4 pi R^2) golden-angle points each, a point kept iff it is outside every
            other sphere (distance to the centre >= radius); order atom, k; area 4 pi R^2 / N
  S         S_ii = zeta_i sqrt(2 / pi), S_ij = erf(zeta_ij r_ij) / r_ij, zeta_i = 1.0694 pi sqrt(2) / sqrt(a_i)
  K         -f S^-1, f = (eps - 1) / (eps + x)
  response  v = v_nuc + v_elec, q = K v, G_pol = 1/2 q.v, V_R = -sum_i q_i A(s_i)
  SCF       F = H + G(D) + V_R(D) with plain DIIS (window 6, on FDS - SDF), to max |dD| <= 1e-10"""
import math

import numpy as np
from scipy.special import erf

BOHR_ANGSTROM = 0.529177210903
VDW_ANGSTROM = {1: 1.20, 2: 1.40, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 10: 1.54, 14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 18: 1.88}
ZETA_C = 1.0694 * math.pi * math.sqrt(2.0)


def factor(eps, x=0.0):
    return (eps - 1.0) / (eps + x)


def sphere_points(R, N):
    k = np.arange(N, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / N
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return R * np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def surface(Z, xyz, scale=1.2, density=5.0, radii=None):
    """(points (M, 3), areas (M,), owners (M,)) - density in points per Angstrom^2, radii (bohr, before scaling) default to the table"""
    Z, xyz = np.asarray(Z), np.asarray(xyz, np.float64).reshape(-1, 3)
    r = np.asarray(radii, np.float64) if radii is not None else np.array([VDW_ANGSTROM.get(int(z), 2.00) / BOHR_ANGSTROM for z in Z])
    R = scale * r
    dens = density * BOHR_ANGSTROM * BOHR_ANGSTROM
    P, a, own = [], [], []
    for A in range(len(Z)):
        N = int(math.ceil(dens * 4.0 * math.pi * R[A] * R[A]))
        pts = xyz[A] + sphere_points(R[A], N)
        keep = np.ones(N, bool)
        for B in range(len(Z)):
            if B != A:
                keep &= np.sqrt(((pts - xyz[B]) ** 2).sum(axis=1)) >= R[B]
        P.append(pts[keep]); a.append(np.full(int(keep.sum()), 4.0 * math.pi * R[A] * R[A] / N)); own.append(np.full(int(keep.sum()), A, np.int32))
    return np.concatenate(P), np.concatenate(a), np.concatenate(own)


def distances(P):
    d = P[:, None, :] - P[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def s_matrix(P, area):
    """the Gaussian-blurred (York-Karplus) cavity matrix"""
    zeta = ZETA_C / np.sqrt(area)
    r = distances(P)
    zij = zeta[:, None] * zeta[None, :] / np.sqrt(zeta[:, None] ** 2 + zeta[None, :] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = erf(zij * r) / r
    S[np.diag_indices(len(P))] = zeta * math.sqrt(2.0 / math.pi)
    return S


def s_matrix_point_charges(P, area):
    """the point-charge form 1 / r_ij with Klamt's diagonal: NOT positive definite on these surfaces (why the erf form is used)"""
    r = distances(P)
    with np.errstate(divide="ignore"):
        S = 1.0 / r
    S[np.diag_indices(len(P))] = 1.0694 * np.sqrt(4.0 * math.pi / area)
    return S


def k_matrix(S, eps, x=0.0):
    K = -factor(eps, x) * np.linalg.inv(S)
    return 0.5 * (K + K.T)


def v_nuc(Z, xyz, P):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return sum(float(z) / np.sqrt(((P - c) ** 2).sum(axis=1)) for z, c in zip(Z, xyz))


def potential_tensor(system, P):
    """A[i] = (a| 1/|r - s_i| |b), (M, n, n), from the host entry qc_potential_matrix"""
    return np.stack([system.potential_matrix(p) for p in P])


def response(K, vn, A, D):
    """(q, V_R, 1/2 q.v_nuc, 1/2 q.v_elec) at the total density D"""
    ve = -np.einsum("iab,ab->i", A, D)
    q = K @ (vn + ve)
    return q, -np.einsum("i,iab->ab", q, A), 0.5 * float(q @ vn), 0.5 * float(q @ ve)


def born(R, N, eps, x=0.0):
    """G_pol of a unit point charge at the centre of one sphere of radius R with N points, and the exact -f / 2R"""
    P = sphere_points(R, N)
    S = s_matrix(P, np.full(N, 4.0 * math.pi * R * R / N))
    v = np.full(N, 1.0 / R)
    q = -factor(eps, x) * np.linalg.solve(S, v)
    return 0.5 * float(q @ v), -factor(eps, x) / (2.0 * R)


class _Diis:
    def __init__(self, size=6):
        self.F, self.e, self.size = [], [], size

    def __call__(self, F, e):
        self.F.append(F); self.e.append(e)
        self.F, self.e = self.F[-self.size:], self.e[-self.size:]
        m = len(self.F)
        if m < 2:
            return F
        B = -np.ones((m + 1, m + 1)); B[m, m] = 0.0
        for i in range(m):
            for j in range(m):
                B[i, j] = float(np.sum(self.e[i] * self.e[j]))
        rhs = np.zeros(m + 1); rhs[m] = -1.0
        c = np.linalg.lstsq(B, rhs, rcond=None)[0][:m]
        return sum(ci * Fi for ci, Fi in zip(c, self.F))


def _orbitals(F, X):
    w, Cp = np.linalg.eigh(X.T @ F @ X)
    return w, X @ Cp


def _x(S):
    w, U = np.linalg.eigh(S)
    return U @ np.diag(w ** -0.5) @ U.T


def scf(S, H, I, nocc, K=None, vn=None, A=None, eps_conv=1e-10, max_iter=200):
    """RHF (nocc an int) or UHF (nocc = (n_alpha, n_beta)) in the continuum (K, vn, A given) or in vacuum, from the core guess.
    Returns a dict: electronic (1/2 tr[D (2H + G + V_R)] per spin convention), e_nuc, e_elec (the halves of G_pol), q, D (total),
    Da, Db, orbital energies."""
    uhf = not np.isscalar(nocc)
    na, nb = (nocc if uhf else (nocc, nocc))
    X = _x(S)
    J = lambda D: np.einsum("ijkl,kl->ij", I, D)
    Kx = lambda D: np.einsum("ikjl,kl->ij", I, D)
    _, C = _orbitals(H, X)
    Da, Db = C[:, :na] @ C[:, :na].T, C[:, :nb] @ C[:, :nb].T
    da, db = _Diis(), _Diis()
    for it in range(max_iter):
        Dt = Da + Db
        VR = response(K, vn, A, Dt)[1] if K is not None else 0.0
        Jt = J(Dt)
        Fa, Fb = H + Jt - Kx(Da) + VR, H + Jt - Kx(Db) + VR
        Fa_x = da(Fa, Fa @ Da @ S - S @ Da @ Fa)
        wa, Ca = _orbitals(Fa_x, X)
        if uhf:
            Fb_x = db(Fb, Fb @ Db @ S - S @ Db @ Fb)
            wb, Cb = _orbitals(Fb_x, X)
        else:
            wb, Cb = wa, Ca
        Na, Nb = Ca[:, :na] @ Ca[:, :na].T, Cb[:, :nb] @ Cb[:, :nb].T
        change = max(float(np.abs(Na - Da).max()), float(np.abs(Nb - Db).max()))
        Da, Db = Na, Nb
        if change <= eps_conv:
            break
    else:
        raise RuntimeError("the reference SCF did not converge")
    Dt = Da + Db
    out = dict(D=Dt, Da=Da, Db=Db, wa=wa, wb=wb, iterations=it, q=None, e_nuc=0.0, e_elec=0.0)
    VR = 0.0
    if K is not None:
        out["q"], VR, out["e_nuc"], out["e_elec"] = response(K, vn, A, Dt)
    Jt = J(Dt)
    Fa, Fb = H + Jt - Kx(Da) + VR, H + Jt - Kx(Db) + VR
    # 1/2 tr[Da (H + Fa)] + 1/2 tr[Db (H + Fb)] = E_HF,el + 1/2 tr(D V_R) = E_HF,el + 1/2 q.v_elec
    out["electronic"] = 0.5 * float(np.sum(Da * (H + Fa)) + np.sum(Db * (H + Fb)))
    return out


# ---- the matrices of the SPD-inverse tests (GPU: qc_spd_inverse; host: numpy.linalg.inv on the same matrices)
INVERSE_SIZES = (1, 2, 63, 64, 65, 128, 129, 200)
INVERSE_DECADES = (1, 3)
UNIT_ROUNDOFF = 2.0 ** -53


def spd_matrix(n, k):
    """Q diag(logspace(0, k, n)) Q^T with Q the orthogonal factor of a seeded Gaussian matrix; exactly symmetric; cond_2 = 10^k (n > 1)"""
    rng = np.random.default_rng(1000 * n + k)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, float(k), n)) @ Q.T
    return 0.5 * (A + A.T)


def inverse_bar(n, cond):
    """the bar of the inverse tests on max |A Ainv - I|"""
    return 8.0 * n * UNIT_ROUNDOFF * cond
