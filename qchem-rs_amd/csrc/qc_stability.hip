// qc_stability.hip - SCF wave-function stability analysis: the lowest eigenpairs of the real orbital Hessian (A + B) by a block
// Davidson iteration whose Hessian-vector product is the direct Fock build, and the orbital rotation that follows an eigenvector.
//
// For real orbitals and a trial vector x^s_ia (s = spin, i occupied, a virtual, laid out x[i * v + a]) the symmetric pseudo-density
//   D1^s = C_occ^s x^s C_virt^s^T + transpose
// turns the two-electron part of (A + B) x into one Fock build:
//   UHF internal      sigma^s = (e_a - e_i) x^s + [C_virt^s^T (J[D1^a + D1^b] - K[D1^s]) C_occ^s]_ai      one UHF build of (D1^a, D1^b)
//   RHF singlet       the bracket is 2 J[D1] - K[D1]: one RHF build of 2 D1
//   RHF -> UHF        the bracket is -K[D1]: the alpha output of one UHF build of (D1, -D1)
// Trial vectors, sigma vectors and the correction vector live in HBM (msub + 1 rows of `dim` doubles each); the subspace matrix
// (at most QC_STAB_MAXSUB rows) is diagonalised on the host.  Every dot product is a fixed-order reduction (a thread's elements in
// index order, the 64 lanes of a wave by a shuffle tree, the waves in order) and the Fock build accumulates integers: a call is bitwise
// reproducible.  The layout of a vector, the Hessian-vector product and the subspace kernels are in qc_stab_shared.h (shared with the
// response solver, qc_response.hip); this file keeps the Davidson driver, the host eigenproblem and the rotation.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "qc_stab_shared.h"

namespace {

// eigenpairs of a small symmetric matrix on the host: cyclic Jacobi, ascending eigenvalues, vectors as the ROWS of Vr (Vr[k * m + i])
void host_sym_eig(int m, std::vector<double> A, std::vector<double> &w, std::vector<double> &Vr) {
    std::vector<double> V((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1.0;
    for (int i = 0; i < m; ++i) for (int j = 0; j < i; ++j) A[(size_t)j * m + i] = A[(size_t)i * m + j];      // (the lower triangle counts)
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) (i == j ? diag : off) += A[(size_t)i * m + j] * A[(size_t)i * m + j];
        if (off <= 1e-32 * diag || off == 0.0) break;
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

}  // namespace

int qc_stability_dim(int n, bool uhf, const int *nocc) { return StabLayout(n, uhf, nocc).dim; }

// Lowest `nroots` eigenpairs of (A + B) at the orbitals dC / energies dEps (device; nblk blocks).  io: kind, nroots, tol, max_iterations
// checked by the caller.  vectors (host, nullable): nroots x dim.
int qc_stability_device(qc_system *S, bool uhf, const int *nocc, const double *dC, const double *dEps, qc_stability *io, double *vectors) {
    const double t_begin = qc_now_ms();
    const int n = S->nbasis, nroots = io->nroots;
    const StabLayout L(n, uhf, nocc);
    const int dim = L.dim;
    const double tol = io->tol > 0.0 ? io->tol : 1e-6;
    const int maxit = io->max_iterations > 0 ? io->max_iterations : 100;
    hipStream_t st = S->stream;
    const int msub = std::min(dim, QC_STAB_MAXSUB);

    // diagonal e_a - e_i, on the device and on the host (start vectors)
    DevBuf dDe;
    if (dDe.alloc(dim) != QC_OK) return QC_ERR_HIP;
    for (int b = 0; b < L.nblk; ++b) {
        const int ov = L.o[b] * L.v[b];
        if (ov > 0) hipLaunchKernelGGL(qc_stab_delta_kernel, dim3((ov + 255) / 256), dim3(256), 0, st, L.o[b], L.v[b], dEps + (size_t)b * n, dDe.p + L.off[b]);
    }
    std::vector<double> de(dim);
    QC_HIP_CHECK(hipMemcpyAsync(de.data(), dDe.p, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));

    StabSigma sigma(S, L, uhf, io->kind, dC, dDe.p);
    DevBuf V, Sg, Wk, dM, dY, dTheta, dInfo;
    QcDev<int> dCnt;
    const size_t rows = (size_t)msub + 1;
    if (sigma.alloc() != QC_OK || V.alloc(rows * dim) != QC_OK || Sg.alloc(rows * dim) != QC_OK || Wk.alloc(2 * (size_t)QC_STAB_MAXROOTS * dim) != QC_OK ||
        dM.alloc((size_t)QC_STAB_MAXSUB * QC_STAB_MAXSUB) != QC_OK || dY.alloc((size_t)QC_STAB_MAXROOTS * QC_STAB_MAXSUB) != QC_OK ||
        dTheta.alloc(QC_STAB_MAXROOTS) != QC_OK || dInfo.alloc(2 * (QC_STAB_MAXSUB + 1)) != QC_OK || dCnt.alloc(1) != QC_OK) return QC_ERR_HIP;

    // Start vectors: unit vectors on the smallest e_a - e_i (ties: lower index first); a subspace that can hold the whole space starts as
    // the whole space.  Unit vectors carry the symmetry of one orbital pair, and a Krylov space never leaves the symmetries it starts
    // with - so one more start vector has a fixed pseudo-random component on every orbital pair.
    std::vector<int> order(dim);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return de[a] < de[b]; });
    const bool whole = dim <= QC_STAB_MAXSUB;
    const int nunit = whole ? dim : std::min(dim, 2 * nroots);
    const int nstart = whole ? dim : nunit + 1;
    {
        std::vector<double> start((size_t)nstart * dim, 0.0);
        for (int k = 0; k < nunit; ++k) start[(size_t)k * dim + order[k]] = 1.0;
        if (!whole) {
            uint32_t lcg = 12345u;
            for (int e = 0; e < dim; ++e) { lcg = lcg * 1664525u + 1013904223u; start[(size_t)nunit * dim + e] = (double)(lcg >> 8) / 8388608.0 - 1.0; }
        }
        // (staged behind the subspace rows: Sg is not in use yet)
        if (nstart > (int)rows) return QC_ERR_INVALID;
        QC_HIP_CHECK(hipMemcpyAsync(Sg.p, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemsetAsync(dCnt.p, 0, sizeof(int), st));
        for (int k = 0; k < nstart; ++k)
            hipLaunchKernelGGL(qc_stab_expand_kernel<false>, dim3(1), dim3(1024), 0, st, dim, 0, msub, V.p, (const double *)nullptr, (const double *)nullptr,
                               (const double *)nullptr, (const double *)nullptr, (const double *)(Sg.p + (size_t)k * dim), (const double *)nullptr, 0.0, dCnt.p, dInfo.p + 2 * k);
        QC_HIP_CHECK(hipStreamSynchronize(st));      // (the staged vectors have been read before the first sigma vector overwrites them)
    }
    int m = 0;
    QC_HIP_CHECK(hipMemcpy(&m, dCnt.p, sizeof(int), hipMemcpyDeviceToHost));
    if (m < nroots) return QC_ERR_INVALID;

    std::vector<double> M((size_t)QC_STAB_MAXSUB * QC_STAB_MAXSUB, 0.0), w, Y, theta(nroots, 0.0), rnorm(nroots, 0.0), info(2 * QC_STAB_MAXROOTS);
    std::vector<double> Ysel((size_t)QC_STAB_MAXROOTS * QC_STAB_MAXSUB, 0.0);
    int m_done = 0, it = 0, nconv = 0, rc = QC_OK;
    bool converged = false;
    for (it = 1; it <= maxit; ++it) {
        for (int k = m_done; k < m; ++k)
            if ((rc = sigma.apply(V.p + (size_t)k * dim, Sg.p + (size_t)k * dim)) != QC_OK) return rc;
        // new rows of the subspace matrix: M[k][j] = <V_j, Sg_k>, j <= k
        hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, m - m_done), dim3(256), 0, st, dim, V.p, Sg.p, m_done, QC_STAB_MAXSUB, dM.p);
        QC_HIP_CHECK(hipMemcpyAsync(M.data() + (size_t)m_done * QC_STAB_MAXSUB, dM.p + (size_t)m_done * QC_STAB_MAXSUB,
                                    (size_t)(m - m_done) * QC_STAB_MAXSUB * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        m_done = m;
        std::vector<double> A((size_t)m * m);
        for (int i = 0; i < m; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * m + j] = A[(size_t)j * m + i] = M[(size_t)i * QC_STAB_MAXSUB + j];
        host_sym_eig(m, A, w, Y);
        for (int r = 0; r < nroots; ++r) {
            theta[r] = w[r];
            for (int j = 0; j < QC_STAB_MAXSUB; ++j) Ysel[(size_t)r * QC_STAB_MAXSUB + j] = j < m ? Y[(size_t)r * m + j] : 0.0;
        }
        QC_HIP_CHECK(hipMemcpyAsync(dY.p, Ysel.data(), Ysel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dTheta.p, theta.data(), nroots * sizeof(double), hipMemcpyHostToDevice, st));
        // the subspace is full: collapse onto the Ritz vectors of the requested roots (their sigma vectors follow by linearity)
        if (m + nroots > msub && m > nroots && m < dim) {
            dim3 grid((dim + 255) / 256, nroots);
            hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m, QC_STAB_MAXSUB, dY.p, V.p, Wk.p);
            hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m, QC_STAB_MAXSUB, dY.p, Sg.p, Wk.p + (size_t)QC_STAB_MAXROOTS * dim);
            QC_HIP_CHECK(hipMemcpyAsync(V.p, Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
            QC_HIP_CHECK(hipMemcpyAsync(Sg.p, Wk.p + (size_t)QC_STAB_MAXROOTS * dim, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
            m = m_done = nroots;
            hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, m), dim3(256), 0, st, dim, V.p, Sg.p, 0, QC_STAB_MAXSUB, dM.p);
            QC_HIP_CHECK(hipMemcpyAsync(M.data(), dM.p, (size_t)m * QC_STAB_MAXSUB * sizeof(double), hipMemcpyDeviceToHost, st));
            std::fill(Ysel.begin(), Ysel.end(), 0.0);
            for (int r = 0; r < nroots; ++r) Ysel[(size_t)r * QC_STAB_MAXSUB + r] = 1.0;
            QC_HIP_CHECK(hipMemcpyAsync(dY.p, Ysel.data(), Ysel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        }
        // residual | preconditioner | orthogonalisation of every requested root, one launch each; the device counts the vectors it added
        QC_HIP_CHECK(hipMemsetAsync(dCnt.p, 0, sizeof(int), st));
        for (int r = 0; r < nroots; ++r)
            hipLaunchKernelGGL(qc_stab_expand_kernel<false>, dim3(1), dim3(1024), 0, st, dim, m, msub, V.p, (const double *)Sg.p,
                               (const double *)(dY.p + (size_t)r * QC_STAB_MAXSUB), (const double *)(dTheta.p + r), (const double *)dDe.p,
                               (const double *)nullptr, (const double *)nullptr, tol, dCnt.p, dInfo.p + 2 * r);
        int added = 0;
        QC_HIP_CHECK(hipMemcpyAsync(info.data(), dInfo.p, 2 * nroots * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipMemcpyAsync(&added, dCnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        nconv = 0;
        for (int r = 0; r < nroots; ++r) { rnorm[r] = std::sqrt(info[2 * r]); if (rnorm[r] <= tol) ++nconv; }
        if (nconv == nroots) { converged = true; break; }
        if (added == 0) break;                           // (nothing left to add: the residuals are as small as this arithmetic makes them)
        m += added;
    }
    if (it > maxit) it = maxit;
    for (int r = 0; r < QC_STAB_MAXROOTS; ++r) { io->eigenvalues[r] = r < nroots ? theta[r] : 0.0; io->residuals[r] = r < nroots ? rnorm[r] : 0.0; }
    io->nconverged = nconv; io->iterations = it; io->builds = sigma.builds;
    if (vectors) {
        dim3 grid((dim + 255) / 256, nroots);
        hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m_done, QC_STAB_MAXSUB, dY.p, V.p, Wk.p);
        QC_HIP_CHECK(hipMemcpyAsync(vectors, Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
    }
    QC_HIP_CHECK(hipGetLastError());
    io->ms_builds = sigma.ms_builds;
    io->ms_total = qc_now_ms() - t_begin;
    return converged ? QC_OK : QC_NOT_CONVERGED;
}

// ---- rotation along a vector.  In the MO basis (occupied first) kappa = [[0, -x], [x^T, 0]] with x the o x v block, so kappa_ai = x_ia.
// exp(theta kappa) applied to the occupied columns, with x x^T = U diag(s^2) U^T:
//   C_occ' = C_occ U cos(theta s) U^T + C_virt x^T U (sin(theta s) / s) U^T
// - an exact orthogonal rotation for any theta.  Host arithmetic (n x o matrices); hD = C_occ' C_occ'^T.
static void rotate_block(int n, int o, const double *C, const double *x, double theta, double *hD) {
    const int v = n - o;
    std::fill(hD, hD + (size_t)n * n, 0.0);
    if (o == 0) return;
    std::vector<double> Co((size_t)n * o);
    for (int mu = 0; mu < n; ++mu) for (int i = 0; i < o; ++i) Co[(size_t)mu * o + i] = C[(size_t)mu * n + i];
    if (v > 0) {
        std::vector<double> XX((size_t)o * o, 0.0), s2, U;
        for (int i = 0; i < o; ++i) for (int j = 0; j <= i; ++j) {
            double t = 0.0;
            for (int a = 0; a < v; ++a) t += x[(size_t)i * v + a] * x[(size_t)j * v + a];
            XX[(size_t)i * o + j] = XX[(size_t)j * o + i] = t;
        }
        host_sym_eig(o, XX, s2, U);                          // rows of U: eigenvectors
        // Fc = U cos U^T, Fs = U (sin / s) U^T (o x o)
        std::vector<double> Fc((size_t)o * o, 0.0), Fs((size_t)o * o, 0.0);
        for (int k = 0; k < o; ++k) {
            const double sk = std::sqrt(std::max(s2[k], 0.0)), ck = std::cos(theta * sk), sn = sk > 1e-8 ? std::sin(theta * sk) / sk : theta;
            for (int i = 0; i < o; ++i) for (int j = 0; j < o; ++j) {
                const double uu = U[(size_t)k * o + i] * U[(size_t)k * o + j];
                Fc[(size_t)i * o + j] += ck * uu; Fs[(size_t)i * o + j] += sn * uu;
            }
        }
        // xf = x^T Fs (v x o); Co' = Co Fc + C_virt xf
        std::vector<double> xf((size_t)v * o, 0.0), Cn((size_t)n * o, 0.0);
        for (int a = 0; a < v; ++a) for (int i = 0; i < o; ++i) { const double xa = x[(size_t)i * v + a]; if (xa != 0.0) for (int j = 0; j < o; ++j) xf[(size_t)a * o + j] += xa * Fs[(size_t)i * o + j]; }
        for (int mu = 0; mu < n; ++mu) {
            double *row = &Cn[(size_t)mu * o];
            for (int i = 0; i < o; ++i) { const double c = Co[(size_t)mu * o + i]; for (int j = 0; j < o; ++j) row[j] += c * Fc[(size_t)i * o + j]; }
            for (int a = 0; a < v; ++a) { const double c = C[(size_t)mu * n + o + a]; for (int j = 0; j < o; ++j) row[j] += c * xf[(size_t)a * o + j]; }
        }
        Co.swap(Cn);
    }
    for (int mu = 0; mu < n; ++mu) for (int nu = 0; nu <= mu; ++nu) {
        double t = 0.0;
        for (int i = 0; i < o; ++i) t += Co[(size_t)mu * o + i] * Co[(size_t)nu * o + i];
        hD[(size_t)mu * n + nu] = hD[(size_t)nu * n + mu] = t;
    }
}

// Densities (host, per spin, n x n) of the determinant rotated along x, and its electronic energy 1/2 sum_s tr(D_s (2 H + G_s)) from one UHF
// build.  angle <= 0: the lowest of theta = +-0.1 * 2^k, k = 0..4.
int qc_rotated_density_device(qc_system *S, bool uhf, int kind, const int *nocc, const double *dC, const double *dH, const double *x, double angle,
                              double *hDa, double *hDb, double *energy) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    const StabLayout L(n, uhf, nocc);
    hipStream_t st = S->stream;
    std::vector<double> C((uhf ? 2 : 1) * nn);
    QC_HIP_CHECK(hipMemcpyAsync(C.data(), dC, C.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    DevBuf dD, dG, dE;
    if (dD.alloc(2 * nn) != QC_OK || dG.alloc(2 * nn) != QC_OK || dE.alloc(4) != QC_OK) return QC_ERR_HIP;
    std::vector<double> Da(nn), Db(nn);
    auto eval = [&](double theta, double *e) -> int {
        rotate_block(n, L.o[0], C.data(), x, theta, Da.data());
        if (uhf) rotate_block(n, L.o[1], C.data() + nn, x + L.off[1], theta, Db.data());
        else if (kind == 1) rotate_block(n, L.o[0], C.data(), x, -theta, Db.data());
        else Db = Da;
        QC_HIP_CHECK(hipMemcpyAsync(dD.p, Da.data(), nn * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dD.p + nn, Db.data(), nn * sizeof(double), hipMemcpyHostToDevice, st));
        int rc = qc_fock_build_device(S, dD.p, dD.p + nn, dG.p, dG.p + nn, true);
        if (rc != QC_OK) return rc;
        for (int s = 0; s < 2; ++s) qc_energy_rms(st, n, dD.p + s * nn, dD.p + s * nn, dH, dG.p + s * nn, dE.p + 2 * s);
        double h[4];
        QC_HIP_CHECK(hipMemcpyAsync(h, dE.p, sizeof(h), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        if ((rc = qc_join_check(S)) != QC_OK) return rc;
        qc_gate_quiet(S);
        *e = h[0] + h[2];
        return QC_OK;
    };
    double best_e = 0.0, best_theta = angle;
    int rc;
    if (angle > 0.0) { if ((rc = eval(angle, &best_e)) != QC_OK) return rc; }
    else {
        bool first = true;
        const bool mirror = !uhf && kind == 1;           // (alpha by +theta and beta by -theta: the sign of theta only swaps the spins)
        std::vector<double> keep_a, keep_b;
        for (int k = 0; k < 5; ++k)
            for (int sgn = 0; sgn < (mirror ? 1 : 2); ++sgn) {
                const double theta = (sgn ? -0.1 : 0.1) * (double)(1 << k);
                double e = 0.0;
                if ((rc = eval(theta, &e)) != QC_OK) return rc;
                if (first || e < best_e) { best_e = e; best_theta = theta; first = false; keep_a = Da; keep_b = Db; }
            }
        Da.swap(keep_a); Db.swap(keep_b);
    }
    (void)best_theta;
    std::memcpy(hDa, Da.data(), nn * sizeof(double));
    std::memcpy(hDb, Db.data(), nn * sizeof(double));
    if (energy) *energy = best_e;
    return QC_OK;
}
