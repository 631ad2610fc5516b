// qc_subspace_host.h - the host numerics of the reduced-space solvers (qc_subspace.h): the small dense problems they solve on the host each
// round.  Standard library only: the file compiles without HIP, and tests/host/subspace_host_main.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <vector>

constexpr double QC_STAB_KEEP = 1e-4;         // a correction vector that loses more than this factor to the orthogonalisation is dropped

// eigenpairs of a small symmetric matrix on the host: cyclic Jacobi, ascending eigenvalues, vectors as the ROWS of Vr (Vr[k * m + i]).
// The sweeps end once |off-diagonal|^2 <= rel_stop |diagonal|^2.  Rounding alone keeps that ratio near (m - 1) u^2 = 5e-31 at m = 40,
// so the default runs all 100 sweeps on a full subspace (22 ms at m = 40) - the stability analysis keeps it, since its results are
// pinned bit for bit; a caller that solves two such problems per round (TDHF) passes a ratio above the rounding floor.
inline void host_sym_eig(int m, std::vector<double> A, std::vector<double> &w, std::vector<double> &Vr, double rel_stop = 1e-32) {
    std::vector<double> V((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1.0;
    for (int i = 0; i < m; ++i) for (int j = 0; j < i; ++j) A[(size_t)j * m + i] = A[(size_t)i * m + j];      // (the lower triangle counts)
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) (i == j ? diag : off) += A[(size_t)i * m + j] * A[(size_t)i * m + j];
        if (off <= rel_stop * diag || off == 0.0) break;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[(size_t)p * m + q];
                if (apq == 0.0) continue;
                const double tau = (A[(size_t)q * m + q] - A[(size_t)p * m + p]) / (2.0 * apq);
                const double tn = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + tn * tn), sn = tn * c;
                for (int k = 0; k < m; ++k) {
                    const double akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
                    A[(size_t)k * m + p] = c * akp - sn * akq; A[(size_t)k * m + q] = sn * akp + c * akq;
                }
                for (int k = 0; k < m; ++k) {
                    const double apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
                    A[(size_t)p * m + k] = c * apk - sn * aqk; A[(size_t)q * m + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < m; ++k) {
                    const double vkp = V[(size_t)k * m + p], vkq = V[(size_t)k * m + q];
                    V[(size_t)k * m + p] = c * vkp - sn * vkq; V[(size_t)k * m + q] = sn * vkp + c * vkq;
                }
            }
    }
    std::vector<int> idx(m);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return A[(size_t)a * m + a] < A[(size_t)b * m + b]; });
    w.resize(m); Vr.assign((size_t)m * m, 0.0);
    for (int k = 0; k < m; ++k) {
        w[k] = A[(size_t)idx[k] * m + idx[k]];
        for (int i = 0; i < m; ++i) Vr[(size_t)k * m + i] = V[(size_t)i * m + idx[k]];
    }
}

// A y = b for nrhs right-hand sides (b, y: nrhs rows of m) by LU with partial pivoting; false: a pivot vanished against the matrix
inline bool host_lu_solve(int m, std::vector<double> A, int nrhs, const double *b, double *y) {
    std::vector<int> piv(m);
    double amax = 0.0;
    for (double a : A) amax = std::max(amax, std::fabs(a));
    for (int k = 0; k < m; ++k) {
        int p = k;
        for (int i = k + 1; i < m; ++i) if (std::fabs(A[(size_t)i * m + k]) > std::fabs(A[(size_t)p * m + k])) p = i;
        if (!(std::fabs(A[(size_t)p * m + k]) > 1e-14 * amax)) return false;
        piv[k] = p;
        if (p != k) for (int j = 0; j < m; ++j) std::swap(A[(size_t)k * m + j], A[(size_t)p * m + j]);
        for (int i = k + 1; i < m; ++i) {
            const double l = A[(size_t)i * m + k] / A[(size_t)k * m + k];
            A[(size_t)i * m + k] = l;
            for (int j = k + 1; j < m; ++j) A[(size_t)i * m + j] -= l * A[(size_t)k * m + j];
        }
    }
    for (int q = 0; q < nrhs; ++q) {
        double *x = y + (size_t)q * m;
        for (int i = 0; i < m; ++i) x[i] = b[(size_t)q * m + i];
        for (int k = 0; k < m; ++k) if (piv[k] != k) std::swap(x[k], x[piv[k]]);      // (whole rows were swapped: all of P first, then L)
        for (int k = 0; k < m; ++k)
            for (int i = k + 1; i < m; ++i) x[i] -= A[(size_t)i * m + k] * x[k];
        for (int i = m - 1; i >= 0; --i) {
            for (int j = i + 1; j < m; ++j) x[i] -= A[(size_t)i * m + j] * x[j];
            x[i] /= A[(size_t)i * m + i];
        }
    }
    return true;
}

// stop ratio of the host Jacobi eigensolves of the TDHF subspace problems: off-diagonal norm <= 3e-14 of the diagonal's - above the rounding
// floor of a 40 x 40 problem (where the default never stops before its 100th sweep), far below what the residuals resolve
constexpr double kJacobiStop = 1e-27;

// TDHF: the reduced generalised problem on the host.  Mp, Mm: m x m (row-major, symmetric).  Out: omega (ascending), Rt, Lt (rows of m,
// nroots each).  false: M- or H is not positive definite in this subspace.
inline bool tdhf_reduced(int m, const std::vector<double> &Mp, const std::vector<double> &Mm, int nroots, double *omega, std::vector<double> &Rt,
                         std::vector<double> &Lt) {
    std::vector<double> s, U, w2, T;
    host_sym_eig(m, Mm, s, U, kJacobiStop);                        // rows of U: eigenvectors of M-
    if (!(s[0] > 0.0)) return false;
    std::vector<double> Sh((size_t)m * m, 0.0), X((size_t)m * m, 0.0), H((size_t)m * m, 0.0);
    for (int k = 0; k < m; ++k) {
        const double r = std::sqrt(s[k]);
        for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) Sh[(size_t)i * m + j] += r * U[(size_t)k * m + i] * U[(size_t)k * m + j];
    }
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) { double t = 0.0; for (int k = 0; k < m; ++k) t += Mp[(size_t)i * m + k] * Sh[(size_t)k * m + j]; X[(size_t)i * m + j] = t; }
    for (int i = 0; i < m; ++i) for (int j = 0; j <= i; ++j) { double t = 0.0; for (int k = 0; k < m; ++k) t += Sh[(size_t)i * m + k] * X[(size_t)k * m + j]; H[(size_t)i * m + j] = H[(size_t)j * m + i] = t; }
    host_sym_eig(m, H, w2, T, kJacobiStop);
    if (!(w2[0] > 0.0)) return false;
    Rt.assign((size_t)nroots * m, 0.0); Lt.assign((size_t)nroots * m, 0.0);
    for (int r = 0; r < nroots; ++r) {
        const double w = std::sqrt(w2[r]), is = 1.0 / std::sqrt(w);
        omega[r] = w;
        for (int i = 0; i < m; ++i) { double t = 0.0; for (int k = 0; k < m; ++k) t += Sh[(size_t)i * m + k] * T[(size_t)r * m + k]; Rt[(size_t)r * m + i] = t * is; }
        for (int i = 0; i < m; ++i) { double t = 0.0; for (int k = 0; k < m; ++k) t += Mp[(size_t)i * m + k] * Rt[(size_t)r * m + k]; Lt[(size_t)r * m + i] = t / w; }
    }
    return true;
}

// Row k of Z (rows of ld doubles) = src[0 .. m) made orthogonal to rows 0 .. k - 1 (orthonormal) by two passes of modified Gram-Schmidt in
// coefficient space, then normalised.  false: the row lost more than QC_STAB_KEEP of its length - it is zeroed and does not count.
inline bool qc_orthonormalize_row(double *Z, int ld, int m, int k, const double *src) {
    double *z = Z + (size_t)k * ld;
    double before = 0.0, after = 0.0;
    for (int j = 0; j < m; ++j) { z[j] = src[j]; before += z[j] * z[j]; }
    for (int pass = 0; pass < 2; ++pass)
        for (int r = 0; r < k; ++r) {
            double d = 0.0;
            for (int j = 0; j < m; ++j) d += z[j] * Z[(size_t)r * ld + j];
            for (int j = 0; j < m; ++j) z[j] -= d * Z[(size_t)r * ld + j];
        }
    for (int j = 0; j < m; ++j) after += z[j] * z[j];
    if (!(after > QC_STAB_KEEP * QC_STAB_KEEP * before)) { std::fill(z, z + ld, 0.0); return false; }
    const double inv = 1.0 / std::sqrt(after);
    for (int j = 0; j < m; ++j) z[j] *= inv;
    return true;
}

// out[q * ld + r] = Z_r . Y_q over j < m for q < nrows, r < k: rows of coefficients Y in the coordinates of the orthonormal rows Z; the rest of out is zero
inline void qc_rows_in_basis(const double *Z, int ld, int m, int k, const double *Y, int nrows, double *out) {
    std::fill(out, out + (size_t)nrows * ld, 0.0);
    for (int q = 0; q < nrows; ++q)
        for (int r = 0; r < k; ++r) {
            double d = 0.0;
            for (int j = 0; j < m; ++j) d += Z[(size_t)r * ld + j] * Y[(size_t)q * ld + j];
            out[(size_t)q * ld + r] = d;
        }
}
