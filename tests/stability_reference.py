"""Dense reference of the stability analysis, in numpy: the real orbital Hessian (A + B) from an ERI tensor, MO coefficients, orbital
energies and occupations.  With (pq|rs) in chemists' notation, i j occupied, a b virtual, rows and columns laid out [i * v + a]:

  same-spin block       delta_ij delta_ab (e_a - e_i) + 2 (ia|jb) - (ib|ja) - (ij|ab)
  opposite-spin block   2 (ia|jb)                       (i a of one spin, j b of the other)
  RHF singlet / triplet same-spin block +/- opposite-spin block (both from the one set of orbitals)
  UHF                   [[same_aa, cross_ab], [cross_ab^T, same_bb]], alpha block first

Second-order energy of a rotation by theta along a unit vector x with eigenvalue lambda:
  E(theta) - E(0) = ROTATION_C * theta^2 * lambda + O(theta^3),  ROTATION_C = 1 for a UHF vector, 2 for an RHF vector (both spins rotate).
"""
import numpy as np

ROTATION_C = {"uhf": 1.0, "rhf": 2.0}


def orbitals(F, S):
    """(C, eps) of F C = S C eps, ascending; columns of C are MOs."""
    s, U = np.linalg.eigh(S)
    X = U @ np.diag(s ** -0.5) @ U.T
    eps, Cp = np.linalg.eigh(X.T @ F @ X)
    return X @ Cp, eps


def coulomb(I, D):
    return np.tensordot(I, D, axes=([2, 3], [0, 1]))


def exchange(I, D):
    return np.tensordot(I, D, axes=([1, 3], [0, 1]))


def fock_rhf(I, H, D):
    """D carries the factor 2."""
    return H + coulomb(I, D) - 0.5 * exchange(I, D)


def fock_uhf(I, H, Da, Db):
    J = coulomb(I, Da + Db)
    return H + J - exchange(I, Da), H + J - exchange(I, Db)


def _mo(I, C1, C2, C3, C4):
    T = np.tensordot(C1, I, axes=(0, 0))
    T = np.tensordot(T, C2, axes=(1, 0))
    T = np.tensordot(T, C3, axes=(1, 0))
    return np.tensordot(T, C4, axes=(1, 0))


def same_spin_block(I, C, eps, nocc):
    Co, Cv = C[:, :nocc], C[:, nocc:]
    o, v = nocc, C.shape[1] - nocc
    ovov = _mo(I, Co, Cv, Co, Cv)                           # (ia|jb)
    oovv = _mo(I, Co, Co, Cv, Cv)                           # (ij|ab)
    A = 2.0 * ovov - ovov.transpose(0, 3, 2, 1) - oovv.transpose(0, 2, 1, 3)
    A = A.reshape(o * v, o * v)
    A[np.diag_indices(o * v)] += (eps[None, nocc:] - eps[:nocc, None]).reshape(-1)
    return A


def cross_block(I, Ca, na, Cb, nb):
    o1, v1, o2, v2 = na, Ca.shape[1] - na, nb, Cb.shape[1] - nb
    return 2.0 * _mo(I, Ca[:, :na], Ca[:, na:], Cb[:, :nb], Cb[:, nb:]).reshape(o1 * v1, o2 * v2)


def hessian_rhf(I, C, eps, nocc, kind):
    """kind 0 singlet, 1 triplet"""
    same, cross = same_spin_block(I, C, eps, nocc), cross_block(I, C, nocc, C, nocc)
    return same + cross if kind == 0 else same - cross


def hessian_uhf(I, Ca, ea, na, Cb, eb, nb):
    X = cross_block(I, Ca, na, Cb, nb)
    return np.block([[same_spin_block(I, Ca, ea, na), X], [X.T, same_spin_block(I, Cb, eb, nb)]])


def rotate(C, nocc, x, theta):
    """Occupied columns of C exp(theta kappa), kappa_ai = x[i * v + a] = -kappa_ia (dense matrix exponential by eigendecomposition of
    the antisymmetric generator)."""
    n = C.shape[1]
    v = n - nocc
    K = np.zeros((n, n))
    K[nocc:, :nocc] = np.asarray(x).reshape(nocc, v).T
    K[:nocc, nocc:] = -np.asarray(x).reshape(nocc, v)
    w, U = np.linalg.eig(theta * K)
    return (C @ (U @ np.diag(np.exp(w)) @ np.linalg.inv(U)).real)[:, :nocc]
