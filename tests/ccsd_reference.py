"""Numpy restatement of CCSD in spin orbitals, independent of the closed-shell working equations of qc_ccsd.hip.

The equations are those of Stanton, Gauss, Watts and Bartlett, J. Chem. Phys. 94, 4334 (1991), over antisymmetrised integrals
<pq||rs> = <pq|rs> - <pq|sr>, <pq|rs> = (pr|qs) in chemists' notation, for a canonical closed-shell determinant (f_pq = eps_p delta_pq):

  Fae   = -1/2 sum_m f_me t_m^a + sum_mf t_m^f <ma||fe> - 1/2 sum_mnf tau~_mn^af <mn||ef>
  Fmi   =  1/2 sum_e t_i^e f_me + sum_en t_n^e <mn||ie> + 1/2 sum_nef tau~_in^ef <mn||ef>
  Fme   =  f_me + sum_nf t_n^f <mn||ef>
  Wmnij = <mn||ij> + P(ij) sum_e t_j^e <mn||ie> + 1/4 sum_ef tau_ij^ef <mn||ef>
  Wabef = <ab||ef> - P(ab) sum_m t_m^b <am||ef> + 1/4 sum_mn tau_mn^ab <mn||ef>
  Wmbej = <mb||ej> + sum_f t_j^f <mb||ef> - sum_n t_n^b <mn||ej> - sum_nf (1/2 t_jn^fb + t_j^f t_n^b) <mn||ef>
  D_i^a t_i^a     = f_ia + sum_e t_i^e Fae - sum_m t_m^a Fmi + sum_me t_im^ae Fme - sum_nf t_n^f <na||if>
                    - 1/2 sum_mef t_im^ef <ma||ef> - 1/2 sum_men t_mn^ae <nm||ei>
  D_ij^ab t_ij^ab = <ij||ab> + P(ab) sum_e t_ij^ae (Fbe - 1/2 sum_m t_m^b Fme) - P(ij) sum_m t_im^ab (Fmj + 1/2 sum_e t_j^e Fme)
                    + 1/2 sum_mn tau_mn^ab Wmnij + 1/2 sum_ef tau_ij^ef Wabef
                    + P(ij) P(ab) sum_me (t_im^ae Wmbej - t_i^e t_m^a <mb||ej>) + P(ij) sum_e t_i^e <ab||ej> - P(ab) sum_m t_m^a <mb||ij>
  tau~ = t2 + 1/2 (t1 t1 - t1 t1),  tau = t2 + t1 t1 - t1 t1,  E = sum f_ia t_i^a + 1/4 sum <ij||ab> t_ij^ab + 1/2 sum <ij||ab> t_i^a t_j^b

Spin orbitals are ordered [occupied alpha, occupied beta, virtual alpha, virtual beta] over the active spatial orbitals (the lowest
n_frozen are left out; with canonical orbitals their only trace is in eps).  The iteration is the plain one: t = R / D from t1 = 0 and
t2 = <ij||ab> / D, no DIIS, until max |t_new - t_old| over T1 and T2 is <= tol.

closed_shell() maps the amplitudes onto the closed-shell layout of the library, t1[i, a] = t1(i alpha, a alpha) and
t2[i, j, a, b] = t2(i alpha, j beta, a alpha, b beta)."""
import numpy as np


def _e(spec, *ops):
    return np.einsum(spec, *ops, optimize=True)


def mo_integrals(I, C, first, last):
    """(pq|rs) over the MOs first .. last - 1 from the AO tensor"""
    Ca = C[:, first:last]
    T = np.tensordot(Ca.T, I, axes=(1, 0))
    T = np.tensordot(Ca.T, T, axes=(1, 1)).transpose(1, 0, 2, 3)
    T = np.tensordot(T, Ca, axes=(2, 0)).transpose(0, 1, 3, 2)
    return np.tensordot(T, Ca, axes=(3, 0))


def spin_orbital_integrals(mo, o):
    """<pq||rs> and the map spin orbital -> (spatial orbital, spin) for `o` occupied of N spatial orbitals"""
    N = mo.shape[0]
    spatial = np.concatenate([np.arange(o), np.arange(o), np.arange(o, N), np.arange(o, N)])
    spin = np.concatenate([np.zeros(o, int), np.ones(o, int), np.zeros(N - o, int), np.ones(N - o, int)])
    same = (spin[:, None] == spin[None, :]).astype(float)
    chem = mo[np.ix_(spatial, spatial, spatial, spatial)] * same[:, :, None, None] * same[None, None, :, :]
    phys = chem.transpose(0, 2, 1, 3)                                   # <pq|rs> = (pr|qs)
    return phys - phys.transpose(0, 1, 3, 2), spatial, spin


class Result:
    pass


def ccsd(I, C, eps, nocc, n_frozen=0, tol=1e-10, max_iterations=300, polish=False):
    """Spin-orbital CCSD of the closed-shell determinant of the lowest nocc columns of C.  Returns a Result with e_mp2, e_ccsd,
    iterations, t1 / t2 (spin orbitals), the integrals `g` and o, v (spatial counts of the active space).  iterations counts the passes
    to max |t_new - t_old| <= tol.  polish: the iteration then goes on (total_iterations) until its own estimated distance to the fixed
    point, change rho / (1 - rho), is below tol / 10, so that the returned amplitudes carry no truncation error of their own at the scale
    of tol; the energies and amplitudes returned are those of the last pass either way."""
    n = C.shape[0]
    o, v = nocc - n_frozen, n - nocc
    mo = mo_integrals(I, C, n_frozen, n)
    g, spatial, _ = spin_orbital_integrals(mo, o)
    e = np.asarray(eps)[n_frozen:][spatial]
    O, V = slice(0, 2 * o), slice(2 * o, 2 * (o + v))
    eo, ev = e[O], e[V]
    D1 = eo[:, None] - ev[None, :]
    D2 = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    oovv, ooov, oooo, vvvv, ovvv, ovvo = g[O, O, V, V], g[O, O, O, V], g[O, O, O, O], g[V, V, V, V], g[O, V, V, V], g[O, V, V, O]
    vovv, vvvo, ovoo = g[V, O, V, V], g[V, V, V, O], g[O, V, O, O]
    t1 = np.zeros((2 * o, 2 * v))
    t2 = oovv / D2
    r = Result()
    r.e_mp2 = 0.25 * float(np.sum(oovv * t2))
    r.converged = False
    it, change = 0, None
    for it in range(1, max_iterations + 1):
        tt = _e("ia,jb->ijab", t1, t1)
        tt = tt - tt.transpose(0, 1, 3, 2)
        taut, tau = t2 + 0.5 * tt, t2 + tt
        Fae = _e("mf,mafe->ae", t1, ovvv) - 0.5 * _e("mnaf,mnef->ae", taut, oovv)          # (f_me = 0: canonical orbitals)
        Fmi = _e("ne,mnie->mi", t1, ooov) + 0.5 * _e("inef,mnef->mi", taut, oovv)
        Fme = _e("nf,mnef->me", t1, oovv)
        Wmnij = oooo + 0.25 * _e("ijef,mnef->mnij", tau, oovv)
        x = _e("je,mnie->mnij", t1, ooov)
        Wmnij = Wmnij + x - x.transpose(0, 1, 3, 2)
        Wabef = vvvv + 0.25 * _e("mnab,mnef->abef", tau, oovv)
        x = _e("mb,amef->abef", t1, vovv)
        Wabef = Wabef - x + x.transpose(1, 0, 2, 3)
        Wmbej = ovvo + _e("jf,mbef->mbej", t1, ovvv) - _e("nb,mnej->mbej", t1, g[O, O, V, O])
        Wmbej = Wmbej - _e("jnfb,mnef->mbej", 0.5 * t2 + _e("jf,nb->jnfb", t1, t1), oovv)

        r1 = _e("ie,ae->ia", t1, Fae) - _e("ma,mi->ia", t1, Fmi) + _e("imae,me->ia", t2, Fme) - _e("nf,naif->ia", t1, g[O, V, O, V])
        r1 = r1 - 0.5 * _e("imef,maef->ia", t2, ovvv) - 0.5 * _e("mnae,nmei->ia", t2, g[O, O, V, O])
        Fbe = Fae - 0.5 * _e("mb,me->be", t1, Fme)
        Fmj = Fmi + 0.5 * _e("je,me->mj", t1, Fme)
        r2 = oovv.copy()
        x = _e("ijae,be->ijab", t2, Fbe)
        r2 += x - x.transpose(0, 1, 3, 2)
        x = _e("imab,mj->ijab", t2, Fmj)
        r2 -= x - x.transpose(1, 0, 2, 3)
        r2 += 0.5 * _e("mnab,mnij->ijab", tau, Wmnij) + 0.5 * _e("ijef,abef->ijab", tau, Wabef)
        x = _e("imae,mbej->ijab", t2, Wmbej) - _e("ie,ma,mbej->ijab", t1, t1, ovvo)
        r2 += x - x.transpose(1, 0, 2, 3) - x.transpose(0, 1, 3, 2) + x.transpose(1, 0, 3, 2)
        x = _e("ie,abej->ijab", t1, vvvo)
        r2 += x - x.transpose(1, 0, 2, 3)
        x = _e("ma,mbij->ijab", t1, ovoo)
        r2 -= x - x.transpose(0, 1, 3, 2)
        n1, n2 = r1 / D1, r2 / D2
        prev, change = change, max(float(np.abs(n1 - t1).max()), float(np.abs(n2 - t2).max()))
        t1, t2 = n1, n2
        if not r.converged and change <= tol:
            r.converged, r.iterations, r.residual = True, it, change
            if not polish:
                break
        if r.converged:
            # the plain iteration converges linearly: with the rate rho = change / previous change its distance to the fixed point is
            # change rho / (1 - rho), which at rho > 1/2 exceeds the change it stopped at
            rho = change / prev if prev and prev > 0.0 else 0.0
            if change == 0.0 or (rho < 1.0 and change * rho / (1.0 - rho) <= 0.1 * tol):
                break
    if not r.converged:
        r.iterations, r.residual = it, change
    r.total_iterations = it
    r.e_ccsd = 0.25 * float(np.sum(oovv * t2)) + 0.5 * float(_e("ijab,ia,jb->", oovv, t1, t1))
    r.t1, r.t2, r.g, r.o, r.v, r.mo = t1, t2, g, o, v, mo
    return r


def closed_shell(r):
    """(t1[i, a], t2[i, j, a, b]) of the closed-shell layout: the alpha-alpha block of T1 and the alpha-beta-alpha-beta block of T2"""
    o, v = r.o, r.v
    return r.t1[:o, :v].copy(), r.t2[:o, o:, :v, v:].copy()


def closed_shell_energy(r):
    """sum (2 (ia|jb) - (ib|ja)) (t_ij^ab + t_i^a t_j^b) over the closed-shell amplitudes"""
    t1, t2 = closed_shell(r)
    o = r.o
    ovov = r.mo[:o, o:, :o, o:]
    tau = t2 + _e("ia,jb->ijab", t1, t1)
    return float(_e("iajb,ijab->", 2.0 * ovov - ovov.transpose(0, 3, 2, 1), tau))


def diagnostics(r):
    """(T1 diagnostic sqrt(sum t1^2 / n_active_occ), max |t1|, max |t2|) of the closed-shell amplitudes"""
    t1, t2 = closed_shell(r)
    return float(np.sqrt(np.sum(t1 * t1) / r.o)), float(np.abs(t1).max()), float(np.abs(t2).max())
