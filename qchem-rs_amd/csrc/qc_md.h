// qc_md.h - the McMurchie-Davidson primitives every integral consumer outside the Fock kernels shares, host and device:
// Hermite expansion E^{ij}_t, Boys function, the Hermite-Coulomb recurrence step, the overlap / kinetic / nuclear-attraction / dipole sums of
// one Cartesian pair, the Hermite moments behind the Cartesian multipoles, and the order of the Cartesian components.  Users: the host model and host one-electron matrices
// (qc_system.cpp), the one-electron kernel (qc_one_electron.hip), the gradient kernels (qc_grad.hip).  The Fock kernels keep their
// own interpolated Boys function and staged tables.
//
// S, T and V decide the open-shell SCF trajectories to the last bit, so every expression here has the shape its
// users had when they each carried a copy, and what differed between the copies stays with the callers:
//  * prefactors ((pi/p)^{3/2}, -1/2, contraction coefficients, -Z 2 pi / p) multiply the sums below at the call sites (but see qc_md_ovl);
//  * the seeds R^n_000 = (-2 alpha)^n F_n: the SCF path (host and one-electron kernel) forms (-2 alpha)^n as a running product,
//    the gradient calls pow(-2 alpha, n) - these round differently, so qc_md_r_step is the recurrence step only;
//  * which products of the E recurrence the device compiler fuses into the adds follows the guards around them: see qc_md_herm_e.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "qc_internal.h"

// ---- Cartesian components (lx, ly, lz) of a shell of order L <= QC_LMAX: lx descending, then ly descending
struct QcMdCartTab { unsigned char l[qc_nherm(QC_LMAX)][3]; };
constexpr QcMdCartTab qc_md_make_cart() {
    QcMdCartTab c{};
    int k = 0;
    for (int L = 0; L <= QC_LMAX; ++L)
        for (int lx = L; lx >= 0; --lx)
            for (int ly = L - lx; ly >= 0; --ly, ++k) { c.l[k][0] = (unsigned char)lx; c.l[k][1] = (unsigned char)ly; c.l[k][2] = (unsigned char)(L - lx - ly); }
    return c;
}
constexpr QcMdCartTab qc_md_cart_tab = qc_md_make_cart();
__host__ __device__ constexpr int qc_md_cartoff(int L) { return L * (L + 1) * (L + 2) / 6; }
// exponents of component x of order L
__host__ __device__ inline const unsigned char *qc_md_cart(int L, int x) { return qc_md_cart_tab.l[qc_md_cartoff(L) + x]; }

// ---- 1-D Hermite expansion E^{ij}_t of x_A^i x_B^j exp(-a x_A^2 - b x_B^2), i <= imax, j <= jmax, t < tdim (>= imax + jmax + 1),
// stored E[(i * (jmax + 1) + j) * tdim + t]; every entry with t > i + j is zero.
// The two device users' old copies differed in the guards of a step, and with them in what the device compiler makes of it:
//  * FUSED (the one-electron kernel): each neighbour is read through a guard (outside 0 <= t <= i + j - 1 it is zero), the three
//    products sit in one expression: mul x e_t, fma h e_{t-1}, fma (t+1) e_{t+1};
//  * otherwise (the gradient kernels): the outer products are formed under their guards: mul h e_{t-1}, fma x e_t, mul, add.
// Without contraction (the host) both give the same bits.  The step is spelled out in place, as a macro: handed to the loops through
// a function or a lambda, the same text came back from the compiler with the other product fused, and S, T, V moved in the last bit.
#define QC_MD_E_GET(tt) (((tt) < 0 || (tt) > lim) ? 0.0 : e[tt])
#define QC_MD_E_STEP(x)                                                                                          \
    (FUSED ? h * QC_MD_E_GET(t - 1) + x * QC_MD_E_GET(t) + (t + 1) * QC_MD_E_GET(t + 1)                \
           : (t > 0 ? h * e[t - 1] : 0.0) + x * e[t] + (t + 1 < tdim ? (t + 1) * e[t + 1] : 0.0))
template <bool FUSED = false>
__host__ __device__ inline void qc_md_herm_e(double *E, int imax, int jmax, int tdim, double a, double b, double Q) {
    const double p = a + b, h = 0.5 / p, xpa = -b / p * Q, xpb = a / p * Q;
    const int sj = tdim, si = (jmax + 1) * tdim;
    for (int k = 0; k < (imax + 1) * si; ++k) E[k] = 0.0;
    E[0] = exp(-a * b / p * Q * Q);
    for (int i = 1; i <= imax; ++i)
        for (int t = 0; t <= i; ++t) {
            const double *e = E + (i - 1) * si;
            const int lim = i - 1; (void)lim;
            E[i * si + t] = QC_MD_E_STEP(xpa);
        }
    for (int i = 0; i <= imax; ++i)
        for (int j = 1; j <= jmax; ++j)
            for (int t = 0; t <= i + j; ++t) {
                const double *e = E + i * si + (j - 1) * sj;
                const int lim = i + j - 1; (void)lim;
                E[i * si + j * sj + t] = QC_MD_E_STEP(xpb);
            }
}
#undef QC_MD_E_STEP
#undef QC_MD_E_GET

// The table of one axis with its accessor: N doubles of storage, filled for i <= imax, j <= jmax
template <int N, bool FUSED = false> struct QcMdE1 {
    double v[N];
    int jm, td;
    __host__ __device__ void fill(int imax, int jmax, double a, double b, double Q) {
        jm = jmax; td = imax + jmax + 1;
        qc_md_herm_e<FUSED>(v, imax, jmax, td, a, b, Q);
    }
    __host__ __device__ double g(int i, int j, int t) const { return (i < 0 || j < 0 || t < 0 || t > i + j) ? 0.0 : v[(i * (jm + 1) + j) * td + t]; }
};

// ---- F_n(x), n = 0..nmax: Kummer series at nmax + downward recursion; erf + upward recursion for large x (exact to the last digits at
// every order its users need, up to F_13 for the (ff|ff) gradient)
__host__ __device__ inline void qc_md_boys(int nmax, double x, double *F) {
    const double ex = exp(-x);
    if (x < 38.0) {
        double term = 1.0 / (2 * nmax + 1), sum = term;
        for (int k = 1; k < 500; ++k) { term *= 2.0 * x / (2 * nmax + 2 * k + 1); sum += term; if (term < 1e-18 * sum) break; }
        F[nmax] = ex * sum;
        for (int n = nmax; n > 0; --n) F[n - 1] = (2.0 * x * F[n] + ex) / (2 * n - 1);
    } else {
        F[0] = 0.5 * sqrt(M_PI / x) * erf(sqrt(x));
        for (int n = 0; n < nmax; ++n) F[n + 1] = ((2 * n + 1) * F[n] - ex) / (2.0 * x);
    }
}

// ---- R^n_tuv from the table of order n + 1 (Rn1, indexed by qc_hidx; X = P - C or P - Q), t + u + v >= 1.  The seeds R^n_000 are the
// callers' (see the head of this file).
__host__ __device__ inline double qc_md_r_step(const double *Rn1, int t, int u, int v, const double *X) {
    if (t) return X[0] * Rn1[qc_hidx(t - 1, u, v)] + (t > 1 ? (t - 1) * Rn1[qc_hidx(t - 2, u, v)] : 0.0);
    if (u) return X[1] * Rn1[qc_hidx(t, u - 1, v)] + (u > 1 ? (u - 1) * Rn1[qc_hidx(t, u - 2, v)] : 0.0);
    return X[2] * Rn1[qc_hidx(t, u, v - 1)] + (v > 1 ? (v - 1) * Rn1[qc_hidx(t, u, v - 2)] : 0.0);
}

// ---- sums of one Cartesian pair (a | b) over the three axis tables E[3], without any prefactor
// (f: a factor that enters the product first - the SCF side's (pi/p)^{3/2}, whose products have always rounded in that order)
template <class E1> __host__ __device__ inline double qc_md_ovl(const E1 *E, const int *a, const int *b, double f = 1.0) {
    return f * E[0].g(a[0], b[0], 0) * E[1].g(a[1], b[1], 0) * E[2].g(a[2], b[2], 0);
}
// <a| (r - O)_k |b> / (pi/p)^{3/2}: one more entry of the table of axis k, [E^k_1 + (P - O)_k E^k_0] E_0 E_0 (PO = (P - O)_k; f as in qc_md_ovl)
template <class E1> __host__ __device__ inline double qc_md_dip(const E1 *E, const int *a, const int *b, int k, double PO, double f = 1.0) {
    double s[3];
    for (int q = 0; q < 3; ++q) s[q] = E[q].g(a[q], b[q], 0);
    s[k] = E[k].g(a[k], b[k], 1) + PO * s[k];
    return f * s[0] * s[1] * s[2];
}
// ---- Cartesian multipole moments <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b>, i + j + k <= QC_MOM_MAX.  Components by total order
// ascending, inside an order as qc_md_cart (its table ends at QC_LMAX, hence one of its own here).
constexpr int QC_MOM_MAX = 4;
struct QcMdMomTab { unsigned char l[qc_nherm(QC_MOM_MAX)][3]; };
constexpr QcMdMomTab qc_md_make_mom() {
    QcMdMomTab c{};
    int k = 0;
    for (int L = 0; L <= QC_MOM_MAX; ++L)
        for (int lx = L; lx >= 0; --lx)
            for (int ly = L - lx; ly >= 0; --ly, ++k) { c.l[k][0] = (unsigned char)lx; c.l[k][1] = (unsigned char)ly; c.l[k][2] = (unsigned char)(L - lx - ly); }
    return c;
}
constexpr QcMdMomTab qc_md_mom_tab = qc_md_make_mom();
__host__ __device__ inline const unsigned char *qc_md_mom_comp(int c) { return qc_md_mom_tab.l[c]; }
// Hermite moments of one axis, M[m * (QC_MOM_MAX + 1) + t] = int (x - O)^m Lambda_t dx / sqrt(pi/p), m <= mmax (X = P - O):
//   M^0_t = delta_t0,  M^(m+1)_t = X M^m_t + t M^m_(t-1) + M^m_(t+1) / 2p,  M^m_t = 0 for t > m
__host__ __device__ inline void qc_md_mom_herm(int mmax, double X, double p, double *M) {
    constexpr int W = QC_MOM_MAX + 1;
    const double h = 0.5 / p;
    for (int k = 0; k < W * W; ++k) M[k] = 0.0;
    M[0] = 1.0;
    for (int m = 0; m < mmax; ++m)
        for (int t = 0; t <= m + 1; ++t)
            M[(m + 1) * W + t] = X * M[m * W + t] + (t > 0 ? t * M[m * W + t - 1] : 0.0) + (t < m ? h * M[m * W + t + 1] : 0.0);
}
// the 1-D factors of one axis for the pair (i, j): F[m] = sum_{t <= min(m, i + j)} E^{ij}_t M^m_t, m <= mmax; m = 1 is E_1 + X E_0
template <class E1> __host__ __device__ inline void qc_md_mom_1d(const E1 &E, int i, int j, int mmax, const double *M, double *F) {
    constexpr int W = QC_MOM_MAX + 1;
    for (int m = 0; m <= mmax; ++m) {
        double s = 0.0;
        for (int t = 0; t <= m && t <= i + j; ++t) s += E.g(i, j, t) * M[m * W + t];
        F[m] = s;
    }
}
// sum_axis <a| d^2/dx^2 |b> (second derivative of the ket primitive: b + 2, b, b - 2 terms; eb: its exponent); T = -1/2 (pi/p)^{3/2} x this
template <class E1> __host__ __device__ inline double qc_md_kin(const E1 *E, const int *a, const int *b, double eb) {
    double s1[3], t1[3];
    for (int k = 0; k < 3; ++k) {
        s1[k] = E[k].g(a[k], b[k], 0);
        t1[k] = 4.0 * eb * eb * E[k].g(a[k], b[k] + 2, 0) - 2.0 * eb * (2 * b[k] + 1) * s1[k];
        if (b[k] >= 2) t1[k] += b[k] * (b[k] - 1) * E[k].g(a[k], b[k] - 2, 0);
    }
    return t1[0] * s1[1] * s1[2] + s1[0] * t1[1] * s1[2] + s1[0] * s1[1] * t1[2];
}
// sum_tuv E^x_t E^y_u E^z_v R_tuv (R: the table R^0, indexed by qc_hidx)
template <class E1> __host__ __device__ inline double qc_md_nuc(const E1 *E, const int *a, const int *b, const double *R) {
    if (a[0] < 0 || a[1] < 0 || a[2] < 0 || b[0] < 0 || b[1] < 0 || b[2] < 0) return 0.0;
    double acc = 0.0;
    for (int t = 0; t <= a[0] + b[0]; ++t)
        for (int u = 0; u <= a[1] + b[1]; ++u)
            for (int v = 0; v <= a[2] + b[2]; ++v) acc += E[0].g(a[0], b[0], t) * E[1].g(a[1], b[1], u) * E[2].g(a[2], b[2], v) * R[qc_hidx(t, u, v)];
    return acc;
}

// ---- what the gradient kernels of the nuclear attraction share (qc_grad1_kernel: R of one nucleus; qc_pc_grad_kernel: Lambda, the sum over
// the point charges).  For every Cartesian pair (x | y) of a shell pair and every axis k, d/dA_k and d/dB_k of its integral by the Gaussian
// rule - E filled to la + 1, lb + 1, R of order la + lb + 1 - weighted with cc P[x * ldp + y]:  vA[k] += pv dA,  vB[k] += pv dB.
template <class E1>
__device__ __forceinline__ void qc_md_nuc_grad(const E1 *E, int la, int nca, int lb, int ncb, double ea, double eb, const double *R, double cc,
                                               const double *P, int ldp, double (&vA)[3], double (&vB)[3]) {
    for (int x = 0; x < nca; ++x) {
        const unsigned char *ax = qc_md_cart(la, x);
        for (int y = 0; y < ncb; ++y) {
            const unsigned char *by = qc_md_cart(lb, y);
            const double pv = cc * P[(size_t)x * ldp + y];
            for (int k = 0; k < 3; ++k) {
                int ai[3] = {ax[0], ax[1], ax[2]}, bi[3] = {by[0], by[1], by[2]};
                ++ai[k];
                double dA = 2.0 * ea * qc_md_nuc(E, ai, bi, R);
                ai[k] -= 2;
                if (ax[k]) dA -= ax[k] * qc_md_nuc(E, ai, bi, R);
                ai[k] += 1;
                ++bi[k];
                double dB = 2.0 * eb * qc_md_nuc(E, ai, bi, R);
                bi[k] -= 2;
                if (by[k]) dB -= by[k] * qc_md_nuc(E, ai, bi, R);
                vA[k] += pv * dA;
                vB[k] += pv * dB;
            }
        }
    }
}
#ifdef __HIPCC__                                     // (the host tests compile this header with a plain C++ compiler)
// sum over the lanes of a wave by a fixed butterfly: every lane ends with the same, order-independent value
__device__ inline double qc_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
#endif
// shell pair pr = a (a + 1) / 2 + b of the triangle a >= b
__host__ __device__ inline void qc_tri_pair(int pr, int &a, int &b) {
    a = 0;
    while (pr > a) { pr -= a + 1; ++a; }
    b = pr;
}
