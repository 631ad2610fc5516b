#!/usr/bin/env python3
"""Generate tests/golden/*.json with an implementation that is independent of oracle/qc_oracle.c and of the HIP path.

Nothing here is reference code (the reference holds no integral code at all).  It is a deliberately
different restatement of the published formulas, used to pin the C oracle:
  * Boys function through scipy.special.hyp1f1 (the oracle uses a series + recursion),
  * Hermite E coefficients and Coulomb R integrals by memoised *recursion* (the oracle builds tables iteratively),
  * real solid harmonics for d/f/g from explicit textbook polynomials (the oracle uses the general closed formula),
  * per-function normalisation by numerical self-overlap,
  * a numpy SCF loop following SURVEY.md App. A with numpy.linalg.eigh.
Run:  python tools/gen_golden.py      (minutes; pure Python.  `python tools/gen_golden.py skew` writes skew_quartets_golden.json
      alone, `python tools/gen_golden.py schwarz` schwarz_golden.json alone)
"""
import functools
import itertools
import json
import math
import os
import sys

import numpy as np
from scipy.special import hyp1f1

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from qchem_rs_amd import BasisSet, MolecularSystem  # noqa: E402  (loader = plumbing shared with the product)


def boys(n, x):
    return hyp1f1(n + 0.5, n + 1.5, -x) / (2.0 * n + 1.0)


def cart_list(L):
    return [(lx, ly, L - lx - ly) for lx in range(L, -1, -1) for ly in range(L - lx, -1, -1)]


def dfact(n):
    return 1.0 if n < 2 else n * dfact(n - 2)


# explicit real solid harmonics, m = -l..l, as {monomial: coefficient}; scale arbitrary (renormalised below)
SOLID = {
    0: [{(0, 0, 0): 1.0}],
    1: [{(0, 1, 0): 1.0}, {(0, 0, 1): 1.0}, {(1, 0, 0): 1.0}],       # only used if a p shell were flagged pure
    2: [{(1, 1, 0): 1.0},
        {(0, 1, 1): 1.0},
        {(0, 0, 2): 2.0, (2, 0, 0): -1.0, (0, 2, 0): -1.0},
        {(1, 0, 1): 1.0},
        {(2, 0, 0): 1.0, (0, 2, 0): -1.0}],
    3: [{(2, 1, 0): 3.0, (0, 3, 0): -1.0},
        {(1, 1, 1): 1.0},
        {(0, 1, 2): 4.0, (2, 1, 0): -1.0, (0, 3, 0): -1.0},
        {(0, 0, 3): 2.0, (2, 0, 1): -3.0, (0, 2, 1): -3.0},
        {(1, 0, 2): 4.0, (3, 0, 0): -1.0, (1, 2, 0): -1.0},
        {(2, 0, 1): 1.0, (0, 2, 1): -1.0},
        {(3, 0, 0): 1.0, (1, 2, 0): -3.0}],
}


class Shell:
    def __init__(self, A, L, pure, exps, coefs):
        self.A = np.asarray(A, float); self.L = L; self.pure = bool(pure and L >= 2)
        self.exps = list(exps)
        self.carts = cart_list(L)
        self.coefs = [c * (2 * a / math.pi) ** 0.75 * (4 * a) ** (L / 2) / math.sqrt(dfact(2 * L - 1))
                      for a, c in zip(exps, coefs)]
        if self.pure:
            T = np.zeros((2 * L + 1, len(self.carts)))
            for m, poly in enumerate(SOLID[L]):
                for mono, c in poly.items():
                    T[m, self.carts.index(mono)] = c
        else:
            T = np.eye(len(self.carts))
        S = np.zeros((len(self.carts),) * 2)
        for (i, c1), (j, c2) in itertools.product(enumerate(self.carts), repeat=2):
            for a, ca in zip(self.exps, self.coefs):
                for b, cb in zip(self.exps, self.coefs):
                    v = ca * cb
                    for k in range(3):
                        n = c1[k] + c2[k]
                        v *= 0.0 if n % 2 else dfact(n - 1) / (2 * (a + b)) ** (n // 2) * math.sqrt(math.pi / (a + b))
                    S[i, j] += v
        norm = np.sqrt(np.einsum("fi,ij,fj->f", T, S, T))
        self.T = T / norm[:, None]
        self.nfunc = self.T.shape[0]


def E(i, j, t, Q, a, b):
    """Hermite expansion coefficient by plain recursion (Helgaker eq. 9.5.6-9.5.7)."""
    p = a + b
    if t < 0 or t > i + j or i < 0 or j < 0:
        return 0.0
    if i == j == t == 0:
        return math.exp(-a * b / p * Q * Q)
    if j == 0:
        return E(i - 1, j, t - 1, Q, a, b) / (2 * p) - (b / p * Q) * E(i - 1, j, t, Q, a, b) + (t + 1) * E(i - 1, j, t + 1, Q, a, b)
    return E(i, j - 1, t - 1, Q, a, b) / (2 * p) + (a / p * Q) * E(i, j - 1, t, Q, a, b) + (t + 1) * E(i, j - 1, t + 1, Q, a, b)


def make_R(alpha, PC):
    r2 = float(np.dot(PC, PC))

    @functools.lru_cache(maxsize=None)
    def R(t, u, v, n):
        if t < 0 or u < 0 or v < 0:
            return 0.0
        if t == u == v == 0:
            return (-2 * alpha) ** n * boys(n, alpha * r2)
        if t > 0:
            return (t - 1) * R(t - 2, u, v, n + 1) + PC[0] * R(t - 1, u, v, n + 1)
        if u > 0:
            return (u - 1) * R(t, u - 2, v, n + 1) + PC[1] * R(t, u - 1, v, n + 1)
        return (v - 1) * R(t, u, v - 2, n + 1) + PC[2] * R(t, u, v - 1, n + 1)
    return R


def e3(sa, sb, a, b):
    """E arrays per axis: Ex[i][j] -> vector over t."""
    Q = sa.A - sb.A
    out = []
    for k in range(3):
        out.append([[np.array([E(i, j, t, Q[k], a, b) for t in range(sa.L + sb.L + 3)])
                     for j in range(sb.L + 3)] for i in range(sa.L + 1)])
    return out


def one_electron_block(sa, sb, atoms):
    na, nb = len(sa.carts), len(sb.carts)
    S = np.zeros((na, nb)); T = np.zeros((na, nb)); V = np.zeros((na, nb))
    for a, ca in zip(sa.exps, sa.coefs):
        for b, cb in zip(sb.exps, sb.coefs):
            p = a + b
            P = (a * sa.A + b * sb.A) / p
            Ex, Ey, Ez = e3(sa, sb, a, b)
            Rs = [(Z, make_R(p, P - np.asarray(C))) for Z, C in atoms]
            for i, (ax, ay, az) in enumerate(sa.carts):
                for j, (bx, by, bz) in enumerate(sb.carts):
                    s1 = lambda Earr, ii, jj: Earr[ii][jj][0] if jj >= 0 else 0.0
                    sx, sy, sz = s1(Ex, ax, bx), s1(Ey, ay, by), s1(Ez, az, bz)
                    f = ca * cb * (math.pi / p) ** 1.5
                    S[i, j] += f * sx * sy * sz
                    # kinetic by the overlap-shift formula
                    L_b = bx + by + bz
                    t0 = b * (2 * L_b + 3) * sx * sy * sz
                    t1 = -2 * b * b * (s1(Ex, ax, bx + 2) * sy * sz + sx * s1(Ey, ay, by + 2) * sz + sx * sy * s1(Ez, az, bz + 2))
                    t2 = -0.5 * (bx * (bx - 1) * s1(Ex, ax, bx - 2) * sy * sz + by * (by - 1) * sx * s1(Ey, ay, by - 2) * sz
                                 + bz * (bz - 1) * sx * sy * s1(Ez, az, bz - 2))
                    T[i, j] += f * (t0 + t1 + t2)
                    acc = 0.0
                    for Z, R in Rs:
                        for t in range(ax + bx + 1):
                            for u in range(ay + by + 1):
                                for v in range(az + bz + 1):
                                    acc -= Z * Ex[ax][bx][t] * Ey[ay][by][u] * Ez[az][bz][v] * R(t, u, v, 0)
                    V[i, j] += ca * cb * 2 * math.pi / p * acc
    tr = lambda M: sa.T @ M @ sb.T.T
    return tr(S), tr(T), tr(V)


def eri_block(sa, sb, sc, sd):
    na, nb, nc, nd = (len(s.carts) for s in (sa, sb, sc, sd))
    out = np.zeros((na, nb, nc, nd))
    Lab, Lcd = sa.L + sb.L, sc.L + sd.L
    for a, ca in zip(sa.exps, sa.coefs):
        for b, cb in zip(sb.exps, sb.coefs):
            p = a + b; P = (a * sa.A + b * sb.A) / p
            Eab = e3(sa, sb, a, b)
            for c, cc in zip(sc.exps, sc.coefs):
                for d, cd in zip(sd.exps, sd.coefs):
                    q = c + d; Qc = (c * sc.A + d * sd.A) / q
                    Ecd = e3(sc, sd, c, d)
                    alpha = p * q / (p + q)
                    R = make_R(alpha, P - Qc)
                    R6 = np.zeros((Lab + 1,) * 3 + (Lcd + 1,) * 3)
                    for t, u, v in itertools.product(range(Lab + 1), repeat=3):
                        if t + u + v > Lab: continue
                        for tt, uu, vv in itertools.product(range(Lcd + 1), repeat=3):
                            if tt + uu + vv > Lcd: continue
                            R6[t, u, v, tt, uu, vv] = (-1) ** (tt + uu + vv) * R(t + tt, u + uu, v + vv, 0)
                    pref = ca * cb * cc * cd * 2 * math.pi ** 2.5 / (p * q * math.sqrt(p + q))
                    for i, A in enumerate(sa.carts):
                        for j, B in enumerate(sb.carts):
                            bra = np.einsum("t,u,v->tuv", Eab[0][A[0]][B[0]][:Lab + 1], Eab[1][A[1]][B[1]][:Lab + 1],
                                            Eab[2][A[2]][B[2]][:Lab + 1])
                            half = np.einsum("tuv,tuvabc->abc", bra, R6)
                            for k, Cc in enumerate(sc.carts):
                                for l, Dd in enumerate(sd.carts):
                                    ket = np.einsum("t,u,v->tuv", Ecd[0][Cc[0]][Dd[0]][:Lcd + 1], Ecd[1][Cc[1]][Dd[1]][:Lcd + 1],
                                                    Ecd[2][Cc[2]][Dd[2]][:Lcd + 1])
                                    out[i, j, k, l] += pref * float(np.sum(half * ket))
    return np.einsum("ai,bj,ck,dl,ijkl->abcd", sa.T, sb.T, sc.T, sd.T, out)


def build(mol, basis):
    b = BasisSet.load(os.path.join(ROOT, "data/basis", basis + ".json"))
    return build_system(MolecularSystem.load(os.path.join(ROOT, "data/mol", mol + ".json"), b))


def build_system(s):
    shells, off, pos = [], [], 0
    k = 0
    for ia, L, pure, npr in zip(s.shell_atom, s.shell_L, s.shell_pure, s.shell_nprim):
        sh = Shell(s.atoms[ia].position, int(L), int(pure), s.exponents[k:k + npr], s.coefficients[k:k + npr])
        k += npr
        shells.append(sh); off.append(pos); pos += sh.nfunc
    atoms = [(a.ordinal, a.position) for a in s.atoms]
    return s, shells, off, pos, atoms


def full_integrals(mol, basis):
    s, shells, off, n, atoms = build(mol, basis)
    S = np.zeros((n, n)); T = np.zeros((n, n)); V = np.zeros((n, n)); I = np.zeros((n,) * 4)
    for a, sa in enumerate(shells):
        for b, sb in enumerate(shells):
            ss, tt, vv = one_electron_block(sa, sb, atoms)
            sl = (slice(off[a], off[a] + sa.nfunc), slice(off[b], off[b] + sb.nfunc))
            S[sl] = ss; T[sl] = tt; V[sl] = vv
    ns = len(shells)
    for a in range(ns):
        for b in range(a + 1):
            for c in range(a + 1):
                for d in range((b if c == a else c) + 1):
                    blk = eri_block(shells[a], shells[b], shells[c], shells[d])
                    A, B, C, D = (slice(off[x], off[x] + shells[x].nfunc) for x in (a, b, c, d))
                    I[A, B, C, D] = blk
                    I[B, A, C, D] = blk.transpose(1, 0, 2, 3); I[A, B, D, C] = blk.transpose(0, 1, 3, 2)
                    I[B, A, D, C] = blk.transpose(1, 0, 3, 2); I[C, D, A, B] = blk.transpose(2, 3, 0, 1)
                    I[D, C, A, B] = blk.transpose(3, 2, 0, 1); I[C, D, B, A] = blk.transpose(2, 3, 1, 0)
                    I[D, C, B, A] = blk.transpose(3, 2, 1, 0)
    return s, S, T, V, I


def sym_from_upper(f, n):
    M = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            M[i, j] = M[j, i] = f(i, j)
    return M


def rhf(s, S, T, V, I, eps, max_it=100):
    """SURVEY App. A, RHF, with numpy.linalg.eigh as the eigensolver."""
    n = S.shape[0]; nocc = s.n_electrons // 2
    H = T + V
    w, U = np.linalg.eigh(S)
    lam = U.T @ (S @ U)
    X = U @ (np.diag(1.0 / np.sqrt(np.diag(lam))) @ U.T)
    dens = lambda C: sym_from_upper(lambda i, j: 2.0 * float(np.dot(C[i, :nocc], C[j, :nocc])), n)
    Heht = sym_from_upper(lambda i, j: 1.75 * S[i, j] * (H[i, i] + H[j, j]) / 2.0, n)
    _, Cp = np.linalg.eigh(X.T @ (Heht @ X))
    D = dens(X @ Cp)
    T4 = I - 0.5 * I.transpose(0, 2, 1, 3)
    errs, focks = [], []
    for it in range(max_it + 1):
        G = sym_from_upper(lambda i, j: float(np.sum(D * T4[i, j])), n)
        F = H + G
        e = F @ D @ S - S @ D @ F
        errs.insert(0, e); focks.insert(0, F); del errs[6:]; del focks[6:]
        m = len(errs)
        if m >= 4:
            B = np.zeros((m + 1, m + 1)); B[:m, :m] = [[np.sum(a * b) for b in errs] for a in errs]
            B[m, :m] = B[:m, m] = 1.0
            rhs = np.zeros(m + 1); rhs[m] = 1.0
            Qm, Rm = np.linalg.qr(B)                      # Householder QR like diis.rs:50-51
            c = np.linalg.solve(Rm, Qm.T @ rhs) if np.all(np.diag(Rm) != 0.0) else None
            if c is None:
                raise RuntimeError('DIIS failed')
            F = sum(ci * Fi for ci, Fi in zip(c[:m], focks))
        eps_o, Cp = np.linalg.eigh(X.T @ (F @ X))
        Dn = dens(X @ Cp)
        dD = Dn - D; D = D + dD
        Ee = 0.5 * np.trace(D @ (2 * H + G))
        rms = math.sqrt(np.sum(np.diag(dD) ** 2) / n)
        if rms < eps:
            return dict(electronic_energy=Ee, iterations=it, orbital_energies=eps_o.tolist())
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/golden/skew_quartets_golden.json: quartets and pairs in general position (tests/synthetic_systems.py) - shells on four
# distinct centres that share no coordinate, so that no component of P - Q vanishes and every R_tuv of orders 9..12 carries weight -
# and f quartets at a Boys argument beyond the tabulated range.  A Cartesian (ff|ff) block alone has 10^4 elements, so an ERI block is
# stored as a strided sample of at most SKEW_SAMPLE elements (stride coprime to every dimension of the block: the sample walks
# through all index residues) plus SKEW_SIGNS sums of the WHOLE block under seeded +-1 signs: a single wrong element moves every sum by
# its full error, an error pattern e moves a sum by |e|_2 in the mean.  One-electron blocks are stored whole.
SKEW_SAMPLE = 192
SKEW_SIGNS = 4
SKEW_T = 59.0          # the Boys argument of the far() quartets: beyond the tabulated range


def skew_stride(shape):
    n = int(np.prod(shape))
    k = max(1, -(-n // SKEW_SAMPLE))
    while any(math.gcd(k, d) != 1 for d in shape if d > 1) and k > 1:
        k += 1
    return k


def skew_block(shells, quartet):
    from synthetic_systems import skew_signs
    blk = eri_block(*(shells[i] for i in quartet))
    flat = blk.reshape(-1)
    stride = skew_stride(blk.shape)
    return dict(shells=list(map(int, quartet)), L=[shells[i].L for i in quartet], shape=list(blk.shape), stride=stride,
                values=flat[::stride].tolist(), signed_sums=[float(np.dot(skew_signs(flat.size, k), flat)) for k in range(SKEW_SIGNS)])


def main_skew(out_dir):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synthetic_systems as syn
    gold = {"_generator": "tools/gen_golden.py (independent numpy/scipy implementation; NOT reference output)",
            "sample": SKEW_SAMPLE, "signs": SKEW_SIGNS}
    sh = lambda atom, L: 4 * atom + L           # tetra() and far(): one s, p, d, f shell per atom, in that order
    for name, pure in (("tetra-pure", True), ("tetra-cart", False)):
        s, shells, off, n, atoms = build_system(syn.tetra(pure, 1)[0])
        quartets = [(sh(0, 3), sh(1, 3), sh(2, 3), sh(3, 3)), (sh(0, 3), sh(1, 2), sh(2, 3), sh(3, 3)),
                    (sh(0, 3), sh(1, 1), sh(2, 2), sh(3, 3)), (sh(0, 2), sh(1, 2), sh(2, 2), sh(3, 2)),
                    (sh(0, 3), sh(1, 0), sh(2, 1), sh(3, 0)), (sh(0, 1), sh(1, 1), sh(2, 1), sh(3, 1))]
        blocks = []
        for qt in quartets:
            blocks.append(skew_block(shells, qt))
            print(name, "quartet", qt, blocks[-1]["L"], "stride", blocks[-1]["stride"], flush=True)
        oneel = []
        for a, b in ((sh(0, 3), sh(1, 3)), (sh(0, 3), sh(2, 2)), (sh(1, 2), sh(3, 1))):
            ss, tt, vv = one_electron_block(shells[a], shells[b], atoms)
            oneel.append(dict(shells=[int(a), int(b)], S=ss.tolist(), T=tt.tolist(), V=vv.tolist()))
        gold[name] = dict(n=n, eri_blocks=blocks, one_electron_blocks=oneel)
    m = syn.far(syn.far_distance(SKEW_T))[0]
    s, shells, off, n, atoms = build_system(m)
    blocks = [skew_block(shells, qt) for qt in ((sh(0, 3), sh(0, 3), sh(1, 3), sh(1, 3)), (sh(0, 2), sh(0, 3), sh(1, 3), sh(1, 2)))]
    gold["far"] = dict(n=n, boys_argument=syn.far_boys_argument(m), eri_blocks=blocks)
    path = os.path.join(out_dir, "skew_quartets_golden.json")
    with open(path, "w") as f:
        json.dump(gold, f)
    print("written", path)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/golden/schwarz_golden.json: the Schwarz factor sqrt(max_ab (ab|ab)) of every shell pair A >= B of spread() and deep()
# (tests/synthetic_systems.py), from eri_block above; for the ss pairs a second value from the closed form
#   (ab|ab) = sum over primitive quartets of 2 pi^{5/2} / (p q sqrt(p + q)) K_ab K_cd F_0(T),  T = p q / (p + q) |P - Q|^2,
# in mpmath at 50 digits (normalisation included: nothing of it passes through a double before the final rounding).  Factors go down
# to 1e-41, where only a relative comparison means anything - these two columns are what the oracle's factors are measured against.
SCHWARZ_SYSTEMS = ("spread", "deep")
SCHWARZ_DIGITS = 50


def _schwarz_numeric(args):
    name, a, b = args
    import synthetic_systems as syn
    shells = build_system(syn.BUILDERS[name]()[0])[1]
    blk = eri_block(shells[a], shells[b], shells[a], shells[b])
    na, nb = blk.shape[:2]
    return float(math.sqrt(max(blk[i, j, i, j] for i in range(na) for j in range(nb))))


def _schwarz_closed_form(args):
    name, a, b = args
    import mpmath as mp
    import synthetic_systems as syn
    mp.mp.dps = SCHWARZ_DIGITS
    m = syn.BUILDERS[name]()[0]
    first = np.concatenate([[0], np.cumsum(m.shell_nprim)])
    pi = mp.pi

    def s_shell(i):
        """(centre, exponents, coefficients of the normalised contracted s function)"""
        assert m.shell_L[i] == 0
        A = [mp.mpf(float(x)) for x in m.atoms[m.shell_atom[i]].position]
        ex = [mp.mpf(float(x)) for x in m.exponents[first[i]:first[i + 1]]]
        co = [mp.mpf(float(c)) * (2 * e / pi) ** mp.mpf("0.75") for c, e in zip(m.coefficients[first[i]:first[i + 1]], ex)]
        norm2 = sum(ci * cj * (pi / (ei + ej)) ** mp.mpf("1.5") for ci, ei in zip(co, ex) for cj, ej in zip(co, ex))
        return A, ex, [c / mp.sqrt(norm2) for c in co]
    (A, ea, ca), (B, eb, cb) = s_shell(a), s_shell(b)
    R2 = sum((x - y) ** 2 for x, y in zip(A, B))
    prims = []                                            # (p, P, K) of every primitive pair
    for x, cx in zip(ea, ca):
        for y, cy in zip(eb, cb):
            p = x + y
            prims.append((p, [(x * u + y * v) / p for u, v in zip(A, B)], cx * cy * mp.exp(-x * y / p * R2)))
    total = mp.mpf(0)
    for p, P, Kab in prims:
        for q, Q, Kcd in prims:
            T = p * q / (p + q) * sum((u - v) ** 2 for u, v in zip(P, Q))
            total += 2 * pi ** mp.mpf("2.5") / (p * q * mp.sqrt(p + q)) * Kab * Kcd * mp.hyp1f1(mp.mpf("0.5"), mp.mpf("1.5"), -T)
    return float(mp.sqrt(total))


def main_schwarz(out_dir):
    from multiprocessing import Pool
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synthetic_systems as syn
    gold = {"_generator": "tools/gen_golden.py schwarz (eri_block of the independent numpy/scipy implementation; ss pairs also in closed "
                          "form, mpmath at %d digits; NOT reference output)" % SCHWARZ_DIGITS}
    jobs, jobs_ss = [], []
    for name in SCHWARZ_SYSTEMS:
        m = syn.BUILDERS[name]()[0]
        for a in range(m.n_shells):
            for b in range(a + 1):
                jobs.append((name, a, b))
                if m.shell_L[a] == 0 and m.shell_L[b] == 0:
                    jobs_ss.append((name, a, b))
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool:          # (one shell pair per task: the values do not depend on the pool)
        r_ss = pool.map_async(_schwarz_closed_form, jobs_ss, chunksize=1)
        r = pool.map_async(_schwarz_numeric, jobs, chunksize=1)
        q_ss, qs = r_ss.get(), r.get()
    for name in SCHWARZ_SYSTEMS:
        pick = lambda js, vals: ([[a, b] for n_, a, b in js if n_ == name], [v for (n_, _, _), v in zip(js, vals) if n_ == name])
        pairs, Q = pick(jobs, qs)
        pairs_ss, Q_ss = pick(jobs_ss, q_ss)
        gold[name] = dict(pairs=pairs, Q=Q, ss_pairs=pairs_ss, ss_Q_closed_form=Q_ss)
        print(name, len(pairs), "pairs, Q from %.3e to %.3e;" % (min(Q), max(Q)), len(pairs_ss), "ss pairs in closed form", flush=True)
    path = os.path.join(out_dir, "schwarz_golden.json")
    with open(path, "w") as f:
        json.dump(gold, f)
    print("written", path)


def main():
    out_dir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    if sys.argv[1:] == ["schwarz"]:              # (the Schwarz file alone: the 13-primitive pairs of deep() make it a few minutes)
        main_schwarz(out_dir)
        return
    main_skew(out_dir)
    if sys.argv[1:] == ["skew"]:                 # (the skew file alone: seconds instead of a minute)
        return
    gold = {"_generator": "tools/gen_golden.py (independent numpy/scipy implementation; NOT reference output)"}
    # Boys
    xs = [0.0, 1e-7, 0.003, 0.5, 1.0, 2.7, 9.9, 17.0, 25.0, 34.9, 35.1, 50.0, 120.0, 1000.0]
    gold["boys"] = {"nmax": 16, "x": xs, "F": [[float(boys(n, x)) for n in range(17)] for x in xs]}
    # full small systems
    for mol, basis, eps in (("hydrogen", "STO-3G", 1e-12), ("water", "STO-3G", 1e-11)):
        s, S, T, V, I = full_integrals(mol, basis)
        r = rhf(s, S, T, V, I, eps)
        enuc = sum(a.ordinal * b.ordinal / np.linalg.norm(np.array(a.position) - np.array(b.position))
                   for a, b in itertools.combinations(s.atoms, 2))
        gold[f"{mol}/{basis}"] = dict(n=S.shape[0], overlap=S.tolist(), kinetic=T.tolist(), nuclear=V.tolist(),
                                     eri=I.reshape(-1).tolist(), epsilon=eps, nuclear_repulsion=enuc, rhf=r)
        print(mol, basis, "E_tot = %.12f" % (r["electronic_energy"] + enuc), "it", r["iterations"], flush=True)
    # selected high-L shell quartets of the headline config (water / cc-pVTZ) + one-electron matrices
    s, shells, off, n, atoms = build("water", "cc-pVTZ")
    Ls = [sh.L for sh in shells]
    print("water/cc-pVTZ shells L:", Ls, "n =", n, flush=True)
    first = lambda L, skip=0: [i for i, l in enumerate(Ls) if l == L][skip]
    f_O, d_O, d_O2, p_O, s_O = first(3), first(2), first(2, 1), first(1), first(0)
    d_H = [i for i, l in enumerate(Ls) if l == 2][-1]
    p_H = [i for i, l in enumerate(Ls) if l == 1][-1]
    s_H = [i for i, l in enumerate(Ls) if l == 0][-1]
    quartets = [(f_O, f_O, f_O, f_O), (f_O, d_H, p_H, f_O), (d_H, s_O, f_O, p_O), (d_O, d_O2, d_H, d_O),
                (f_O, s_H, s_O, s_O), (p_H, p_O, d_H, s_H), (d_H, p_H, d_O, p_O), (f_O, p_H, d_H, d_O2),
                (s_O, s_O, s_O, s_O), (p_O, s_O, p_H, s_H)]
    blocks = []
    for q in quartets:
        blk = eri_block(*(shells[i] for i in q))
        blocks.append(dict(shells=list(map(int, q)), L=[Ls[i] for i in q], shape=list(blk.shape),
                           values=blk.reshape(-1).tolist()))
        print("quartet", q, [Ls[i] for i in q], "max|.| = %.3e" % np.abs(blk).max(), flush=True)
    # one-electron blocks for pairs involving d/f
    pairs = [(f_O, f_O), (f_O, d_H), (d_H, p_O), (d_O, s_H), (f_O, s_O), (d_H, d_H)]
    oneel = []
    for a, b in pairs:
        ss, tt, vv = one_electron_block(shells[a], shells[b], atoms)
        oneel.append(dict(shells=[int(a), int(b)], S=ss.tolist(), T=tt.tolist(), V=vv.tolist()))
    gold["water/cc-pVTZ"] = dict(n=n, shell_L=Ls, shell_offset=off, eri_blocks=blocks, one_electron_blocks=oneel)
    with open(os.path.join(out_dir, "integrals_golden.json"), "w") as f:
        json.dump(gold, f)
    print("written", os.path.join(out_dir, "integrals_golden.json"))
    main_schwarz(out_dir)


if __name__ == "__main__":
    main()
