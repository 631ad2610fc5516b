"""Dense reference of the CIS and TDHF excited states of an RHF determinant, in numpy, on top of tests/stability_reference.py (the MO
transformation) and tests/dipole_reference.py (the right-hand sides r^q = C_occ^T M_q C_virt).

With (pq|rs) in chemists' notation, i j occupied, a b virtual, Delta = delta_ij delta_ab (e_a - e_i), rows and columns laid out [i * v + a]:

  singlets  A + B = Delta + 4 (ia|jb) - (ib|ja) - (ij|ab)        triplets  A + B = Delta - (ib|ja) - (ij|ab)
  both      A - B = Delta + (ib|ja) - (ij|ab)                    A = 1/2 [(A + B) + (A - B)]

CIS: A X = w X by numpy.linalg.eigh.  TDHF: (A - B)(A + B) R = w^2 R by numpy.linalg.eig, R = X + Y normalised so that R^T (A + B) R = w,
L = X - Y = (A + B) R / w, hence L . R = X^T X - Y^T Y = 1 (tdhf_sym: the same through the symmetric (A - B)^1/2 (A + B) (A - B)^1/2).  Singlet transition dipoles mu_k = sqrt 2 r . X_k (CIS) or sqrt 2 r . R_k (TDHF),
oscillator strengths f_k = 2/3 w_k |mu_k|^2; triplets have none.

spin_orbital_cis builds the CIS matrix a second time, from antisymmetrised spin-orbital integrals <pq||rs>: A_ia,jb = Delta + <aj||ib>.  Its
spectrum is the singlets once and the triplets three times - the check that pins the factors and signs above (tests/test_excitations_host.py).
"""
import numpy as np

import dipole_reference as D
import stability_reference as R


def matrices_rhf(I, C, eps, nocc, kind):
    """(A + B, A - B) of kind 0 (singlets) or 1 (triplets), (o v, o v) each"""
    Co, Cv = C[:, :nocc], C[:, nocc:]
    o, v = nocc, C.shape[1] - nocc
    ovov = R._mo(I, Co, Cv, Co, Cv)                              # (ia|jb) at [i, a, j, b]
    oovv = R._mo(I, Co, Co, Cv, Cv)                              # (ij|ab) at [i, j, a, b]
    x = ovov.transpose(0, 3, 2, 1).reshape(o * v, o * v)         # (ib|ja) at [i a, j b]
    g = oovv.transpose(0, 2, 1, 3).reshape(o * v, o * v)         # (ij|ab) at [i a, j b]
    delta = np.diag((eps[None, nocc:] - eps[:nocc, None]).reshape(-1))
    P = delta + (4.0 if kind == 0 else 0.0) * ovov.reshape(o * v, o * v) - x - g
    return P, delta + x - g


def cis(P, M):
    """(w ascending, X with the states as rows, |X_k| = 1)"""
    w, X = np.linalg.eigh(0.5 * (P + M))
    return w, X.T


def tdhf(P, M):
    """(w ascending, R, L with the states as rows): M P R = w^2 R, R^T P R = w, L = P R / w.  Both matrices must be positive definite."""
    w2, V = np.linalg.eig(M @ P)
    assert np.abs(w2.imag).max() <= 1e-10 * np.abs(w2).max() and w2.real.min() > 0.0, "A + B or A - B is not positive definite"
    order = np.argsort(w2.real)
    w, V = np.sqrt(w2.real[order]), V.real[:, order]
    Rv = V * np.sqrt(w / np.einsum("ik,ij,jk->k", V, P, V))[None, :]
    return w, Rv.T, (P @ Rv / w[None, :]).T


def tdhf_sym(P, M):
    """tdhf() through the symmetric problem: H = M^1/2 P M^1/2 by numpy.linalg.eigh, H T = w^2 T with |T_k| = 1, R = M^1/2 T w^-1/2 (so that
    R^T P R = T^T H T / w = w), L = P R / w (so that L . R = 1).  Same return value, the signs of the states apart; for the dimensions at which
    a non-symmetric eigensolver is slow and loose (proved against tdhf() in tests/test_excitations_host.py)."""
    s, U = np.linalg.eigh(M)
    assert s[0] > 0.0, "A - B is not positive definite"
    Mh = (U * np.sqrt(s)[None, :]) @ U.T
    H = Mh @ P @ Mh
    w2, T = np.linalg.eigh(0.5 * (H + H.T))
    assert w2[0] > 0.0, "A + B is not positive definite"
    w = np.sqrt(w2)
    Rv = (Mh @ T) / np.sqrt(w)[None, :]
    return w, Rv.T, (P @ Rv / w[None, :]).T


def transition_dipoles(r, vectors):
    """(nstates, 3): sqrt 2 r^q . x_k for r (3, dim) and the states as rows"""
    return np.sqrt(2.0) * vectors @ r.T


def oscillator_strengths(w, mu):
    return 2.0 / 3.0 * w * (mu ** 2).sum(axis=1)


def rhs(C, nocc, Mdip):
    return D.rhs(C, nocc, Mdip)


def spin_orbital_cis(I, C, eps, nocc):
    """The CIS matrix over all 2o x 2v spin-orbital single excitations, Delta + <aj||ib>, from antisymmetrised integrals"""
    n = C.shape[1]
    Cs = np.zeros((2 * n, 2 * n))                                # spin orbitals: alpha block, beta block (AO index doubled likewise)
    Cs[:n, 0::2], Cs[n:, 1::2] = C, C
    es = np.repeat(eps, 2)
    Is = np.zeros((2 * n,) * 4)                                  # (pq|rs) over spin AOs: both pairs carry one spin each
    for s1 in (0, 1):
        for s2 in (0, 1):
            a, b = slice(s1 * n, (s1 + 1) * n), slice(s2 * n, (s2 + 1) * n)
            Is[a, a, b, b] = I
    mo = R._mo(Is, Cs, Cs, Cs, Cs)                               # (pq|rs), chemists'
    phys = mo.transpose(0, 2, 1, 3)                              # <pq|rs> = (pr|qs)
    anti = phys - phys.transpose(0, 1, 3, 2)                     # <pq||rs>
    no = 2 * nocc
    nv = 2 * n - no
    A = anti[no:, :no, :no, no:].transpose(2, 0, 1, 3).reshape(no * nv, no * nv)      # <aj||ib> at [i a, j b]
    return A + np.diag((es[None, no:] - es[:no, None]).reshape(-1))
