// qc_grad.hip - analytic RHF/UHF nuclear gradient: the fixed-density contraction of the derivative integrals.
//
//   dE/dX = sum P_t dh/dX + 1/2 sum d(mn|ls)/dX Gamma_mnls - sum W dS/dX + dVnn/dX,
//   Gamma_mnls = P_t,mn P_t,ls - 1/2 sum_spin (P_s,ml P_s,ns + P_s,ms P_s,nl)          (exchange symmetrised: 8-fold symmetric)
//
// Every derivative comes from the Gaussian rule d/dA_x G_i = 2a G_{i+1} - i G_{i-1}: in McMurchie-Davidson form it only swaps the
// Hermite expansion E^{ij}_t of one axis for 2a E^{i+1,j}_t - i E^{i-1,j}_t (or the same in j for centre B).  Nothing is new but the
// expansions one order higher and the Hermite-Coulomb table R_tuv one order higher.
//
// The densities are transformed once to the Cartesian basis (P_cart = T^T P T per shell block, cart_transform_kernel); no kernel
// below sees solid harmonics.  All reductions run in a fixed order: no float atomics, so a call is bitwise reproducible.
//  * two-electron term (qc_grad2_kernel): persistent one-wave workgroups walk the Schwarz-screened unique quartets of the handle's
//    work lists (QcClass::tasks), statically dealt (task i -> workgroup i mod grid).  The lanes of a wave form groups of gs lanes, one
//    group per primitive quartet; gs grows with the class (lane per primitive quartet for the low classes, a whole wave for (ff|ff)).
//    Per primitive quartet: E tables of bra and ket, R_tuv to order L_ab + L_cd + 1 (cooperatively, in LDS), then per bra Cartesian
//    pair ab the ket Hermite densities K_ab = sum_cd Gamma_abcd E^cd and KC_ab,x/y/z (centre-C derivative of E^cd), and the bra side
//    against R.  Centres A, B, C directly; D by translational invariance.  Each workgroup keeps its row of the atom gradient in LDS and
//    adds each quartet's twelve numbers with one lane, in task order; rows go to a slab [workgroup][3 natoms].
//  * one-electron terms (qc_grad1_kernel): one wave per shell pair, lanes over primitive pairs (x nuclei for V), the same slab rows.
//  * qc_grad_sum_kernel: one workgroup adds the slab rows in row order.
// Hermite expansions, Boys function (Kummer series + downward recursion, exact to the last digits at every order this needs, up to
// F_13 for (ff|ff); the Fock kernels' interpolation table is not read), the R recurrence step, the sums of one Cartesian pair and the
// Cartesian component order come from qc_md.h, shared with the one-electron kernel and the host; shells and primitives from the
// handle's blob (qc_shell_blob).
#include <algorithm>
#include <cmath>

#include "qc_md.h"

namespace {

// ---- tables --------------------------------------------------------------------------------------------------------------------
constexpr int GL_MAX = 4 * QC_LMAX + 1;                 // highest Hermite order of a derivative ERI
constexpr int NH_MAX = qc_nherm(GL_MAX);

struct HermTab { unsigned char t[NH_MAX], u[NH_MAX], v[NH_MAX]; };
constexpr HermTab make_htab() {
    HermTab h{};
    int k = 0;
    for (int N = 0; N <= GL_MAX; ++N)
        for (int t = N; t >= 0; --t)
            for (int u = N - t; u >= 0; --u, ++k) { h.t[k] = (unsigned char)t; h.u[k] = (unsigned char)u; h.v[k] = (unsigned char)(N - t - u); }
    return h;
}
__constant__ HermTab c_htab = make_htab();

// ---- density transform ---------------------------------------------------------------------------------------------------------
// dst[m][i][j] (nc x nc, Cartesian) = sum_{f,g} T_A[f][x] src[m][offA + f][offB + g] T_B[g][y] for Cartesian i = coffA + x, j = coffB + y
__global__ __launch_bounds__(256) void cart_transform_kernel(int n, int nc, const QcDevShell *__restrict__ sh, const int *__restrict__ cshell,
                                                             const double *__restrict__ Tm, const double *__restrict__ src, double *__restrict__ dst) {
    const size_t ij = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ij >= (size_t)nc * nc) return;
    const int m = blockIdx.y;
    const int i = (int)(ij / nc), j = (int)(ij - (size_t)i * nc);
    const QcDevShell A = sh[cshell[i]], B = sh[cshell[j]];
    const int x = i - A.coff, y = j - B.coff;
    const double *S = src + (size_t)m * n * n, *Ta = Tm + A.toff, *Tb = Tm + B.toff;
    double acc = 0.0;
    for (int f = 0; f < A.nfunc; ++f) {
        double r = 0.0;
        for (int g = 0; g < B.nfunc; ++g) r += S[(size_t)(A.off + f) * n + B.off + g] * Tb[g * B.ncart + y];
        acc += Ta[f * A.ncart + x] * r;
    }
    dst[(size_t)m * nc * nc + ij] = acc;
}

// [Pt, Pa, Pb, W] in the function basis from the caller's densities: nspin 1: Pt = D, Pa = Pb = D / 2; nspin 2: Pt = Da + Db
__global__ void combine_kernel(int nn, int nspin, const double *__restrict__ D, double *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nn) return;
    const double a = nspin == 1 ? 0.5 * D[k] : D[k], b = nspin == 1 ? a : D[nn + k];
    out[k] = nspin == 1 ? D[k] : a + b;
    out[nn + k] = a;
    out[2 * nn + k] = b;
}

// Ce[:, i] = w_i C[:, i] for the occupied columns i < nocc, w_i = occ * eps_i (the energy-weighted density's left factor)
__global__ void scale_cols_kernel(int n, int nocc, double occ, const double *__restrict__ C, const double *__restrict__ eps, double *__restrict__ Ce) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n * n) return;
    const int i = k % n;
    Ce[k] = i < nocc ? occ * eps[i] * C[k] : 0.0;
}

// ---- one-electron terms --------------------------------------------------------------------------------------------------------
constexpr int EI1 = QC_LMAX + 2, EJ1 = QC_LMAX + 3, ET1 = EI1 + EJ1 + 1;   // i <= la + 1, j <= lb + 2

using E1 = QcMdE1<EI1 * EJ1 * ET1>;

// Slab row of workgroup w: [core (3 natoms) | overlap (3 natoms)].  One wave per shell pair (a >= b), statically dealt.
__global__ __launch_bounds__(64) void qc_grad1_kernel(int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps, const double *__restrict__ coefs,
                                                      int natoms, const int *__restrict__ Z, const double *__restrict__ xyz, int nc,
                                                      const double *__restrict__ Pc, const double *__restrict__ Wc, double *__restrict__ slab) {
    extern __shared__ double row[];                   // 6 natoms
    const int lane = threadIdx.x, na3 = 3 * natoms;
    for (int k = lane; k < 2 * na3; k += 64) row[k] = 0.0;
    __syncthreads();
    const int npairs = nshells * (nshells + 1) / 2;
    for (int pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
        int a, b;
        qc_tri_pair(pr, a, b);
        const QcDevShell A = sh[a], B = sh[b];
        const double f = a == b ? 1.0 : 2.0;
        const int npp = A.nprim * B.nprim;
        // overlap (x W) and kinetic (x P): d/dA only, d/dB = -d/dA
        double sA[3] = {0, 0, 0}, tA[3] = {0, 0, 0};
        for (int pp = lane; pp < npp; pp += 64) {
            const int i = pp / B.nprim, j = pp - i * B.nprim;
            const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb, cc = coefs[A.poff + i] * coefs[B.poff + j] * pow(M_PI / p, 1.5);
            E1 E[3];
            for (int k = 0; k < 3; ++k) E[k].fill(A.L + 1, B.L + 2, ea, eb, A.A[k] - B.A[k]);
            for (int x = 0; x < A.ncart; ++x) {
                const unsigned char *ax = qc_md_cart(A.L, x);
                for (int y = 0; y < B.ncart; ++y) {
                    const unsigned char *by = qc_md_cart(B.L, y);
                    const int bi[3] = {by[0], by[1], by[2]};
                    const double w = cc * Wc[(size_t)(A.coff + x) * nc + B.coff + y], pv = cc * Pc[(size_t)(A.coff + x) * nc + B.coff + y];
                    for (int k = 0; k < 3; ++k) {
                        int up[3] = {ax[0], ax[1], ax[2]}, dn[3] = {ax[0], ax[1], ax[2]};
                        ++up[k]; --dn[k];
                        const double lo = ax[k] ? ax[k] * qc_md_ovl(E, dn, bi) : 0.0, klo = ax[k] ? ax[k] * (-0.5 * qc_md_kin(E, dn, bi, eb)) : 0.0;
                        sA[k] += w * (2.0 * ea * qc_md_ovl(E, up, bi) - lo);
                        tA[k] += pv * (2.0 * ea * (-0.5 * qc_md_kin(E, up, bi, eb)) - klo);
                    }
                }
            }
        }
        for (int k = 0; k < 3; ++k) { sA[k] = qc_wave_sum(sA[k]); tA[k] = qc_wave_sum(tA[k]); }
        if (lane == 0)
            for (int k = 0; k < 3; ++k) {
                row[3 * A.atom + k] += f * tA[k]; row[3 * B.atom + k] -= f * tA[k];
                row[na3 + 3 * A.atom + k] -= f * sA[k]; row[na3 + 3 * B.atom + k] += f * sA[k];
            }
        // nuclear attraction, nucleus by nucleus: d/dA and d/dB from the basis functions, d/dC = -(d/dA + d/dB) (Hellmann-Feynman)
        for (int c = 0; c < natoms; ++c) {
            double vA[3] = {0, 0, 0}, vB[3] = {0, 0, 0};
            for (int pp = lane; pp < npp; pp += 64) {
                const int i = pp / B.nprim, j = pp - i * B.nprim;
                const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb;
                const double cc = -(double)Z[c] * 2.0 * M_PI / p * coefs[A.poff + i] * coefs[B.poff + j];
                E1 E[3];
                double PC[3];
                for (int k = 0; k < 3; ++k) {
                    E[k].fill(A.L + 1, B.L + 2, ea, eb, A.A[k] - B.A[k]);
                    PC[k] = (ea * A.A[k] + eb * B.A[k]) / p - xyz[3 * c + k];
                }
                const int L = A.L + B.L + 1;
                double Rb[2][qc_nherm(QC_LPAIR + 1)], F[QC_LPAIR + 2];
                qc_md_boys(L, p * (PC[0] * PC[0] + PC[1] * PC[1] + PC[2] * PC[2]), F);
                for (int n = L; n >= 0; --n) {
                    double *Rn = Rb[n & 1];
                    const double *Rn1 = Rb[(n + 1) & 1];
                    Rn[0] = pow(-2.0 * p, n) * F[n];          // (the seeds: pow here, see qc_md.h)
                    for (int h = 1; h < qc_nherm(L - n); ++h) Rn[h] = qc_md_r_step(Rn1, c_htab.t[h], c_htab.u[h], c_htab.v[h], PC);
                }
                qc_md_nuc_grad(E, A.L, A.ncart, B.L, B.ncart, ea, eb, Rb[0], cc, Pc + (size_t)A.coff * nc + B.coff, nc, vA, vB);
            }
            for (int k = 0; k < 3; ++k) { vA[k] = qc_wave_sum(vA[k]); vB[k] = qc_wave_sum(vB[k]); }
            if (lane == 0)
                for (int k = 0; k < 3; ++k) {
                    row[3 * A.atom + k] += f * vA[k];
                    row[3 * B.atom + k] += f * vB[k];
                    row[3 * c + k] -= f * (vA[k] + vB[k]);
                }
        }
    }
    __syncthreads();
    for (int k = lane; k < 2 * na3; k += 64) slab[(size_t)blockIdx.x * 2 * na3 + k] = row[k];
}

// ---- two-electron term ---------------------------------------------------------------------------------------------------------
struct GTask { int sa, sb, sc, sd; };

__host__ __device__ inline int esize(int li, int lj) { return (li + 2) * (lj + 2) * (li + lj + 3); }   // one axis, i <= li + 1, j <= lj + 1
// LDS doubles of one lane group for a quartet of these orders
__host__ __device__ inline int group_words(int la, int lb, int lc, int ld) {
    const int lab = la + lb, lcd = lc + ld, L = lab + lcd + 1;
    return 3 * esize(la, lb) + 3 * esize(lc, ld) + 2 * qc_nherm(L) + qc_nherm(lcd) + 3 * qc_nherm(lcd + 1) + GL_MAX + 3;
}

// Dynamic LDS: [Gamma block gmax][groups x ws][atom row 3 natoms].  One wave per workgroup; groups of gs = 64 >> glog lanes.
// The slab row of the workgroup is read at the start and written back at the end (one row across the launches of all classes).
__global__ __launch_bounds__(64) void qc_grad2_kernel(const GTask *__restrict__ tasks, int ntasks, int glog, int ws, int gmax,
                                                      const QcDevShell *__restrict__ sh, const double *__restrict__ exps, const double *__restrict__ coefs,
                                                      int nc, const double *__restrict__ Pt, const double *__restrict__ Pa, const double *__restrict__ Pb,
                                                      int natoms, double *__restrict__ slab) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, gs = 64 >> glog, ngroups = 1 << glog, g = lane / gs, gl = lane - g * gs, na3 = 3 * natoms;
    double *gam = lds, *W = lds + gmax + (size_t)g * ws, *row = lds + gmax + (size_t)ngroups * ws;
    for (int k = lane; k < na3; k += 64) row[k] = slab[(size_t)blockIdx.x * na3 + k];
    for (int ti = blockIdx.x; ti < ntasks; ti += gridDim.x) {
        const GTask tk = tasks[ti];
        const QcDevShell A = sh[tk.sa], B = sh[tk.sb], Cs = sh[tk.sc], D = sh[tk.sd];
        const int nab = A.ncart * B.ncart, ncd = Cs.ncart * D.ncart;
        const int lab = A.L + B.L, lcd = Cs.L + D.L, L = lab + lcd + 1;
        // Gamma_abcd of the block (Cartesian), exchange symmetrised
        __syncthreads();
        for (int e = lane; e < nab * ncd; e += 64) {
            const int ab = e / ncd, cd = e - ab * ncd;
            const int i = A.coff + ab / B.ncart, j = B.coff + ab % B.ncart, k = Cs.coff + cd / D.ncart, l = D.coff + cd % D.ncart;
            const size_t ij = (size_t)i * nc + j, kl = (size_t)k * nc + l, ik = (size_t)i * nc + k, jl = (size_t)j * nc + l, il = (size_t)i * nc + l,
                         jk = (size_t)j * nc + k;
            gam[e] = Pt[ij] * Pt[kl] - 0.5 * (Pa[ik] * Pa[jl] + Pa[il] * Pa[jk] + Pb[ik] * Pb[jl] + Pb[il] * Pb[jk]);
        }
        // lane group layout
        const int sEb = esize(A.L, B.L), sEk = esize(Cs.L, D.L), nhL = qc_nherm(L);
        const int tb = lab + 3, tk_ = lcd + 3, jb = B.L + 2, jd = D.L + 2;   // t extent, j extent of the tables
        double *Eb = W, *Ek = Eb + 3 * sEb, *R0 = Ek + 3 * sEk, *R1 = R0 + nhL, *K = R1 + nhL, *KC = K + qc_nherm(lcd), *Fv = KC + 3 * qc_nherm(lcd + 1);
        const int nhK = qc_nherm(lcd), nhK1 = qc_nherm(lcd + 1), nhB = qc_nherm(lab), nhB1 = qc_nherm(lab + 1);
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int KB = A.nprim * B.nprim, KK = Cs.nprim * D.nprim, npq = KB * KK;
        const int rounds = (npq + ngroups - 1) / ngroups;
        __syncthreads();
        for (int r = 0; r < rounds; ++r) {
            const int pq = r * ngroups + g;
            const bool act = pq < npq;
            const int ib = act ? pq / KK : 0, ik = act ? pq - ib * KK : 0;
            const int i = ib / B.nprim, j = ib - i * B.nprim, k = ik / D.nprim, l = ik - k * D.nprim;
            const double ea = exps[A.poff + i], eb = exps[B.poff + j], ec = exps[Cs.poff + k], ed = exps[D.poff + l];
            const double p = ea + eb, q = ec + ed, alpha = p * q / (p + q);
            double PQ[3];
            for (int x = 0; x < 3; ++x) PQ[x] = (ea * A.A[x] + eb * B.A[x]) / p - (ec * Cs.A[x] + ed * D.A[x]) / q;
            const double pref = 2.0 * pow(M_PI, 2.5) / (p * q * sqrt(p + q)) * coefs[A.poff + i] * coefs[B.poff + j] * coefs[Cs.poff + k] * coefs[D.poff + l];
            if (act) {
                for (int e = gl; e < 6; e += gs) {
                    if (e < 3) qc_md_herm_e(Eb + e * sEb, A.L + 1, B.L + 1, tb, ea, eb, A.A[e] - B.A[e]);
                    else qc_md_herm_e(Ek + (e - 3) * sEk, Cs.L + 1, D.L + 1, tk_, ec, ed, Cs.A[e - 3] - D.A[e - 3]);
                }
                if (gl == 0) qc_md_boys(L, alpha * (PQ[0] * PQ[0] + PQ[1] * PQ[1] + PQ[2] * PQ[2]), Fv);
            }
            __syncthreads();
            for (int n = L; n >= 0; --n) {          // R^n from R^{n+1}; R^0 ends in R0
                double *Rn = (n & 1) ? R1 : R0;
                const double *Rn1 = (n & 1) ? R0 : R1;
                if (act)
                    for (int h = gl; h < qc_nherm(L - n); h += gs)
                        Rn[h] = h == 0 ? pow(-2.0 * alpha, n) * Fv[n] : qc_md_r_step(Rn1, c_htab.t[h], c_htab.u[h], c_htab.v[h], PQ);
                __syncthreads();
            }
            for (int ab = 0; ab < nab; ++ab) {
                const unsigned char *ax = qc_md_cart(A.L, ab / B.ncart), *bx = qc_md_cart(B.L, ab % B.ncart);
                if (act)
                    for (int h = gl; h < nhK1; h += gs) {       // ket Hermite densities of this bra pair
                        const int tt[3] = {c_htab.t[h], c_htab.u[h], c_htab.v[h]};
                        double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
                        for (int cd = 0; cd < ncd; ++cd) {
                            const unsigned char *cx = qc_md_cart(Cs.L, cd / D.ncart), *dx = qc_md_cart(D.L, cd % D.ncart);
                            double e[3], de[3];
                            for (int x = 0; x < 3; ++x) {
                                const double *Ex = Ek + x * sEk;
                                const int ci = cx[x], di = dx[x];
                                e[x] = Ex[(ci * jd + di) * tk_ + tt[x]];
                                de[x] = 2.0 * ec * Ex[((ci + 1) * jd + di) * tk_ + tt[x]] - (ci ? ci * Ex[((ci - 1) * jd + di) * tk_ + tt[x]] : 0.0);
                            }
                            const double gv = gam[ab * ncd + cd];
                            k0 += gv * e[0] * e[1] * e[2];
                            k1 += gv * de[0] * e[1] * e[2];
                            k2 += gv * e[0] * de[1] * e[2];
                            k3 += gv * e[0] * e[1] * de[2];
                        }
                        const double s = ((tt[0] + tt[1] + tt[2]) & 1) ? -pref : pref;
                        if (h < nhK) K[h] = s * k0;
                        KC[h] = s * k1; KC[nhK1 + h] = s * k2; KC[2 * nhK1 + h] = s * k3;
                    }
                __syncthreads();
                if (act)
                    for (int h = gl; h < nhB1; h += gs) {       // bra side against R
                        const int t = c_htab.t[h], u = c_htab.u[h], v = c_htab.v[h];
                        const bool low = h < nhB;
                        double V = 0.0, V1 = 0.0, V2 = 0.0, V3 = 0.0;
                        for (int hk = 0; hk < (low ? nhK1 : nhK); ++hk) {
                            const double rv = R0[qc_hidx(t + c_htab.t[hk], u + c_htab.u[hk], v + c_htab.v[hk])];
                            if (hk < nhK) V += K[hk] * rv;
                            if (low) { V1 += KC[hk] * rv; V2 += KC[nhK1 + hk] * rv; V3 += KC[2 * nhK1 + hk] * rv; }
                        }
                        const int tt[3] = {t, u, v};
                        double e[3], dA[3], dB[3];
                        for (int x = 0; x < 3; ++x) {
                            const double *Ex = Eb + x * sEb;
                            const int ai = ax[x], bi = bx[x];
                            e[x] = Ex[(ai * jb + bi) * tb + tt[x]];
                            dA[x] = 2.0 * ea * Ex[((ai + 1) * jb + bi) * tb + tt[x]] - (ai ? ai * Ex[((ai - 1) * jb + bi) * tb + tt[x]] : 0.0);
                            dB[x] = 2.0 * eb * Ex[(ai * jb + bi + 1) * tb + tt[x]] - (bi ? bi * Ex[(ai * jb + bi - 1) * tb + tt[x]] : 0.0);
                        }
                        acc[0] += dA[0] * e[1] * e[2] * V; acc[1] += e[0] * dA[1] * e[2] * V; acc[2] += e[0] * e[1] * dA[2] * V;
                        acc[3] += dB[0] * e[1] * e[2] * V; acc[4] += e[0] * dB[1] * e[2] * V; acc[5] += e[0] * e[1] * dB[2] * V;
                        if (low) {
                            const double e3 = e[0] * e[1] * e[2];
                            acc[6] += e3 * V1; acc[7] += e3 * V2; acc[8] += e3 * V3;
                        }
                    }
                __syncthreads();
            }
        }
        for (int x = 0; x < 9; ++x) acc[x] = qc_wave_sum(acc[x]);
        if (lane == 0) {
            // degeneracy of the unique quartet (pair A>=B, pair C>=D, bra pair vs ket pair) x the 1/2 of the energy expression
            const bool bra_eq_ket = (tk.sa == tk.sc && tk.sb == tk.sd) || (tk.sa == tk.sd && tk.sb == tk.sc);
            const double f = 0.5 * (tk.sa == tk.sb ? 1.0 : 2.0) * (tk.sc == tk.sd ? 1.0 : 2.0) * (bra_eq_ket ? 1.0 : 2.0);
            for (int x = 0; x < 3; ++x) {
                row[3 * A.atom + x] += f * acc[x];
                row[3 * B.atom + x] += f * acc[3 + x];
                row[3 * Cs.atom + x] += f * acc[6 + x];
                row[3 * D.atom + x] -= f * (acc[x] + acc[3 + x] + acc[6 + x]);      // translational invariance
            }
        }
    }
    __syncthreads();
    for (int k = lane; k < na3; k += 64) slab[(size_t)blockIdx.x * na3 + k] = row[k];
}

// out[term][k], term 0 core, 1 overlap, 2 two-electron: rows added in row order
__global__ __launch_bounds__(256) void qc_grad_sum_kernel(int na3, int rows1, const double *__restrict__ slab1, int rows2, const double *__restrict__ slab2,
                                                          double *__restrict__ out) {
    for (int idx = threadIdx.x; idx < 3 * na3; idx += blockDim.x) {
        const int term = idx / na3, k = idx - term * na3;
        double s = 0.0;
        if (term < 2) for (int w = 0; w < rows1; ++w) s += slab1[(size_t)w * 2 * na3 + term * na3 + k];
        else for (int w = 0; w < rows2; ++w) s += slab2[(size_t)w * na3 + k];
        out[idx] = s;
    }
}

constexpr int G1_ROWS = 512, G2_ROWS = 1024;
constexpr size_t LDS_LIMIT = 160 * 1024, LDS_GROUPS = 64 * 1024;

}  // namespace

// The terms core / overlap / two-electron of the gradient (3 x 3 natoms doubles, host `terms3`) from function-basis densities on the
// device: dP = [D] (nspin 1) or [Da; Db] (nspin 2), dW = W.  Phase times (ms, stream events) go to ms[4] when it is not null.
int qc_gradient_device(qc_system *S, int nspin, const double *dP, const double *dW, double *terms3, double *ms) {
    const int n = S->nbasis, na = S->natoms, na3 = 3 * na, nsh = S->nshells;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    if ((size_t)2 * na3 * 8 > 32 * 1024) return QC_ERR_UNSUPPORTED;          // the atom rows live in LDS
    const QcShellBlob *B;
    int rc = qc_shell_blob(S, &B);
    if (rc != QC_OK) return rc;
    const int nc = B->nc;
    const size_t ncc = (size_t)nc * nc;
    // the two-electron work: the handle's unique quartets after Schwarz screening, bucketed by total order (one launch each)
    const bool screen = !S->pairQ.empty() && S->schwarz_tau > 0.0;
    std::vector<std::vector<GTask>> bucket(4 * QC_LMAX + 1);
    std::vector<int> bws(bucket.size(), 0), bg(bucket.size(), 0);
    for (const auto &c : S->classes)
        for (const auto &t : c.tasks) {
            if (screen && !(S->pairQ[t.bra] * S->pairQ[t.ket] >= S->schwarz_tau)) continue;
            const GTask g{S->pairA[t.bra], S->pairB[t.bra], S->pairA[t.ket], S->pairB[t.ket]};
            const QcShell &a = S->shells[g.sa], &b = S->shells[g.sb], &c2 = S->shells[g.sc], &d = S->shells[g.sd];
            const int Lt = a.L + b.L + c2.L + d.L;
            bucket[Lt].push_back(g);
            bws[Lt] = std::max(bws[Lt], group_words(a.L, b.L, c2.L, d.L));
            bg[Lt] = std::max(bg[Lt], a.ncart * b.ncart * c2.ncart * d.ncart);
        }
    std::vector<size_t> boff(bucket.size() + 1, 0);
    for (size_t b = 0; b < bucket.size(); ++b) boff[b + 1] = boff[b] + bucket[b].size();
    std::vector<GTask> flat;
    flat.reserve(boff.back());
    for (const auto &v : bucket) flat.insert(flat.end(), v.begin(), v.end());

    // (the task list follows the current Schwarz threshold: built and uploaded per call)
    QcDev<GTask> tasks;
    DevBuf fb, cb, s1, s2, out;
    if (tasks.alloc(flat.size()) != QC_OK || fb.alloc(4 * nn) != QC_OK || cb.alloc(4 * ncc) != QC_OK || s1.alloc((size_t)G1_ROWS * 2 * na3) != QC_OK ||
        s2.alloc((size_t)G2_ROWS * na3) != QC_OK || out.alloc(3 * na3) != QC_OK)
        return QC_ERR_HIP;
    if (!flat.empty()) QC_HIP_CHECK(hipMemcpyAsync(tasks.p, flat.data(), flat.size() * sizeof(GTask), hipMemcpyHostToDevice, st));

    hipEvent_t ev[5];
    for (auto &e : ev) QC_HIP_CHECK(hipEventCreate(&e));
    struct EvDel { hipEvent_t *e; ~EvDel() { for (int i = 0; i < 5; ++i) (void)hipEventDestroy(e[i]); } } evdel{ev};
    QC_HIP_CHECK(hipEventRecord(ev[0], st));
    // 1. [Pt, Pa, Pb, W] -> Cartesian
    double *F = fb.p, *Cc = cb.p;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, (int)nn, nspin, dP, F);
    QC_HIP_CHECK(hipMemcpyAsync(F + 3 * nn, dW, nn * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(cart_transform_kernel, dim3((unsigned)((ncc + 255) / 256), 4), dim3(256), 0, st, n, nc, B->sh, B->cshell, B->T, F, Cc);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipEventRecord(ev[1], st));
    // 2. one-electron terms
    const int npairs = nsh * (nsh + 1) / 2, g1 = std::min(npairs, G1_ROWS);
    QC_HIP_CHECK(hipMemsetAsync(s1.p, 0, (size_t)G1_ROWS * 2 * na3 * 8, st));
    hipLaunchKernelGGL(qc_grad1_kernel, dim3(g1), dim3(64), 2 * na3 * 8, st, nsh, B->sh, B->exps, B->coefs, na, B->Z, B->xyz, nc, Cc, Cc + 3 * ncc, s1.p);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipEventRecord(ev[2], st));
    // 3. two-electron term, one launch per total order
    // (set on every call: the attribute is per device, and handles may live on several devices and threads)
    QC_HIP_CHECK(hipFuncSetAttribute((const void *)qc_grad2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
    QC_HIP_CHECK(hipMemsetAsync(s2.p, 0, (size_t)G2_ROWS * na3 * 8, st));
    for (size_t b = 0; b < bucket.size(); ++b) {
        const int nt = (int)bucket[b].size();
        if (!nt) continue;
        int glog = 6;                                 // most groups whose tables fit LDS_GROUPS
        while (glog > 0 && ((size_t)bws[b] << glog) * 8 > LDS_GROUPS) --glog;
        const size_t lds = ((size_t)bg[b] + ((size_t)bws[b] << glog) + na3) * 8;
        if (lds > LDS_LIMIT) return QC_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(qc_grad2_kernel, dim3(std::min(nt, G2_ROWS)), dim3(64), lds, st, tasks.p + boff[b], nt, glog, bws[b], bg[b], B->sh, B->exps,
                           B->coefs, nc, Cc, Cc + ncc, Cc + 2 * ncc, na, s2.p);
        QC_HIP_CHECK(hipGetLastError());
    }
    QC_HIP_CHECK(hipEventRecord(ev[3], st));
    // 4. fixed-order sum of the slab rows
    hipLaunchKernelGGL(qc_grad_sum_kernel, dim3(1), dim3(256), 0, st, na3, g1, s1.p, G2_ROWS, s2.p, out.p);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipEventRecord(ev[4], st));
    QC_HIP_CHECK(hipMemcpyAsync(terms3, out.p, 3 * na3 * 8, hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    if (ms) for (int i = 0; i < 4; ++i) { float t = 0.f; QC_HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1])); ms[i] = t; }
    return QC_OK;
}

// W = sum_spin sum_{i occ} n_i eps_i c_i c_i^T from the coefficients / orbital energies of an SCF state (nspin * n*n, nspin * n), on the
// device, into dW (n*n), enqueued on the handle's stream
int qc_gradient_w_device(qc_system *S, int nspin, const double *dC, const double *dEps, const int *nocc, double *dW) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    DevBuf Ce;
    if (Ce.alloc(nn) != QC_OK) return QC_ERR_HIP;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};     // before Ce is freed: the work below reads it
    const double occ = nspin == 1 ? 2.0 : 1.0;
    QC_HIP_CHECK(hipMemsetAsync(dW, 0, nn * 8, st));
    for (int s = 0; s < nspin; ++s) {
        if (nocc[s] <= 0) continue;
        hipLaunchKernelGGL(scale_cols_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, n, nocc[s], occ, dC + s * nn, dEps + (size_t)s * n, Ce.p);
        QC_HIP_CHECK(hipGetLastError());
        qc_gemm(st, n, n, nocc[s], 1.0, Ce.p, n, false, dC + s * nn, n, true, 1.0, dW, n);
    }
    return QC_OK;
}

// dVnn/dX, 3 natoms doubles (host)
void qc_nuclear_gradient(const qc_system *S, double *g) {
    for (int a = 0; a < 3 * S->natoms; ++a) g[a] = 0.0;
    for (int a = 0; a < S->natoms; ++a)
        for (int b = 0; b < S->natoms; ++b) {
            if (a == b) continue;
            double d[3], r2 = 0.0;
            for (int k = 0; k < 3; ++k) { d[k] = S->xyz[3 * a + k] - S->xyz[3 * b + k]; r2 += d[k] * d[k]; }
            const double f = -(double)(S->Z[a] * S->Z[b]) / (r2 * std::sqrt(r2));
            for (int k = 0; k < 3; ++k) g[3 * a + k] += f * d[k];
        }
}
