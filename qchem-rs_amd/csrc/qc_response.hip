// qc_response.hip - first-order properties and static response of an SCF state: the trace of the density with the dipole matrices, and the
// static dipole polarizability by coupled-perturbed Hartree-Fock.
//
// For a static, real perturbation the first-order orbital rotations U^q solve (A + B) U^q = r^q with r^q = C_occ^T M_q C_virt per spin
// block (M_q: dipole matrix of direction q; vectors laid out x[i * v + a] as in qc_stability.hip), and
//   alpha_pq = c r^p . U^q,   c = 4 for an RHF state (singlet operator), c = 2 for a UHF state (internal operator, vector [x^a; x^b]).
// (A + B) x is the Hessian-vector product of the stability analysis - one direct Fock build of the symmetric pseudo-density, qc_stab_shared.h.
// The three systems share one orthonormal subspace V (reduced-space iteration): per round one build per new vector, the projected
// matrix V^T (A + B) V and V^T r by fixed-order dot products, the small systems solved on the host, and per right-hand side one launch that
// forms the residual, preconditions it with 1 / (e_a - e_i) and orthogonalises it into V.  A Galerkin solve needs the projected matrix
// to be non-singular, not (A + B) to be positive definite: at a saddle the iteration works as long as no projected matrix is singular.
// Every sum is a fixed-order reduction and the Fock build accumulates integers: a call is bitwise reproducible.
#include <cmath>
#include <cstring>
#include <vector>

#include "qc_stab_shared.h"

namespace {

constexpr int QC_CPHF_NRHS = 3;

// out[k] = sum_e (Pa[e] + Pb[e]) M_k[e] = tr(P_t M_k) (M_k symmetric): workgroup k, 256 threads, fixed-order sums
__global__ __launch_bounds__(256) void qc_dipole_trace_kernel(size_t nn, const double *__restrict__ Pa, const double *__restrict__ Pb,
                                                              const double *__restrict__ M, double *__restrict__ out) {
    __shared__ double sh[16];
    const double *m = M + (size_t)blockIdx.x * nn;
    double s = 0.0;
    for (size_t e = threadIdx.x; e < nn; e += 256) s = fma(Pb ? Pa[e] + Pb[e] : Pa[e], m[e], s);
    s = qc_stab_block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// start vectors: x = r / (e_a - e_i) with the floor on the denominator
__global__ void qc_cphf_precond_kernel(int dim, const double *__restrict__ de, const double *__restrict__ r, double *__restrict__ x) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= dim) return;
    double d = de[e];
    if (fabs(d) < QC_STAB_DENOM_FLOOR) d = d < 0.0 ? -QC_STAB_DENOM_FLOOR : QC_STAB_DENOM_FLOOR;
    x[e] = r[e] / d;
}

// A y = b for nrhs right-hand sides (b, y: nrhs rows of m) by LU with partial pivoting; false: a pivot vanished against the matrix
bool host_lu_solve(int m, std::vector<double> A, int nrhs, const double *b, double *y) {
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

}  // namespace

int qc_dipole_trace_device(qc_system *S, const double *dPa, const double *dPb, const double *dM, double *tr3) {
    DevBuf out;
    if (out.alloc(3) != QC_OK) return QC_ERR_HIP;
    hipLaunchKernelGGL(qc_dipole_trace_kernel, dim3(3), dim3(256), 0, S->stream, (size_t)S->nbasis * S->nbasis, dPa, dPb, dM, out.p);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipMemcpyAsync(tr3, out.p, 3 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

int qc_polarizability_device(qc_system *S, bool uhf, const int *nocc, const double *dC, const double *dEps, qc_polarizability *io, double *response) {
    const double t_begin = qc_now_ms();
    constexpr int NR = QC_CPHF_NRHS, LD = QC_STAB_MAXSUB;
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    const StabLayout L(n, uhf, nocc);
    const int dim = L.dim;
    const double tol = io->tol > 0.0 ? io->tol : 1e-6, c_alpha = uhf ? 2.0 : 4.0;
    const int maxit = io->max_iterations > 0 ? io->max_iterations : 100;
    hipStream_t st = S->stream;
    for (double &a : io->alpha) a = 0.0;
    for (double &r : io->residuals) r = 0.0;
    io->asymmetry = 0.0; io->nconverged = NR; io->iterations = 0; io->builds = 0; io->ms_builds = 0.0; io->ms_total = 0.0;
    if (response) std::fill(response, response + (size_t)NR * dim, 0.0);
    if (dim == 0) { io->ms_total = qc_now_ms() - t_begin; return QC_OK; }
    const int msub = std::min(dim, QC_STAB_MAXSUB);
    const size_t rows = (size_t)msub + 1;

    DevBuf dDe, dM3, Rh, V, Sg, Wk, dA, dB, dY, dInfo, dOut;
    QcDev<int> dCnt;
    StabSigma sigma(S, L, uhf, 0, dC, nullptr);
    if (dDe.alloc(dim) != QC_OK || dM3.alloc(3 * nn) != QC_OK || Rh.alloc((size_t)NR * dim) != QC_OK || V.alloc(rows * dim) != QC_OK ||
        Sg.alloc(rows * dim) != QC_OK || Wk.alloc(2 * (size_t)NR * dim) != QC_OK || dA.alloc((size_t)LD * LD) != QC_OK || dB.alloc((size_t)NR * LD) != QC_OK ||
        dY.alloc((size_t)NR * LD) != QC_OK || dInfo.alloc(2 * NR) != QC_OK || dOut.alloc(NR * NR) != QC_OK || dCnt.alloc(1) != QC_OK || sigma.alloc() != QC_OK)
        return QC_ERR_HIP;
    sigma.dDe = dDe.p;
    for (int b = 0; b < L.nblk; ++b) {
        const int ov = L.o[b] * L.v[b];
        if (ov > 0) hipLaunchKernelGGL(qc_stab_delta_kernel, dim3((ov + 255) / 256), dim3(256), 0, st, L.o[b], L.v[b], dEps + (size_t)b * n, dDe.p + L.off[b]);
    }

    // right-hand sides r^q = C_occ^T M_q C_virt per block (origin 0: occupied and virtual orbitals are orthogonal), and their squared norms
    const double origin[3] = {0.0, 0.0, 0.0};
    int rc = qc_dipole_device(S, origin, dM3.p);
    if (rc != QC_OK) return rc;
    for (int q = 0; q < NR; ++q)
        for (int b = 0; b < L.nblk; ++b) {
            if (L.o[b] == 0 || L.v[b] == 0) continue;
            const double *Cb = dC + b * nn;
            qc_gemm(st, n, L.v[b], n, 1.0, dM3.p + q * nn, n, false, Cb + L.o[b], n, false, 0.0, sigma.P.p, L.v[b]);                       // M C_virt
            qc_gemm(st, L.o[b], L.v[b], n, 1.0, Cb, n, true, sigma.P.p, L.v[b], false, 0.0, Rh.p + (size_t)q * dim + L.off[b], L.v[b]);    // C_occ^T (.)
        }
    hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(NR, NR), dim3(256), 0, st, dim, Rh.p, Rh.p, 0, NR, dOut.p);
    double rr[NR * NR];
    QC_HIP_CHECK(hipMemcpyAsync(rr, dOut.p, sizeof(rr), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    bool active[NR];
    int nactive = 0;
    for (int q = 0; q < NR; ++q) { active[q] = rr[q * NR + q] > 0.0; nactive += active[q] ? 1 : 0; }

    // start vectors: the preconditioned right-hand sides, orthonormalised (staged in Wk)
    QC_HIP_CHECK(hipMemsetAsync(dCnt.p, 0, sizeof(int), st));
    for (int q = 0; q < NR; ++q) {
        if (!active[q]) continue;
        hipLaunchKernelGGL(qc_cphf_precond_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, dim, dDe.p, Rh.p + (size_t)q * dim, Wk.p + (size_t)q * dim);
        hipLaunchKernelGGL(qc_stab_expand_kernel<false>, dim3(1), dim3(1024), 0, st, dim, 0, msub, V.p, (const double *)nullptr, (const double *)nullptr,
                           (const double *)nullptr, (const double *)nullptr, (const double *)(Wk.p + (size_t)q * dim), (const double *)nullptr, 0.0,
                           dCnt.p, dInfo.p + 2 * q);
    }
    int m = 0;
    QC_HIP_CHECK(hipMemcpyAsync(&m, dCnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));

    // (Z, Yn: the collapse's coefficient arrays; they are sources of enqueued copies and live as long as the stream may read them)
    std::vector<double> M((size_t)LD * LD, 0.0), B((size_t)NR * LD, 0.0), Y((size_t)NR * LD, 0.0), info(2 * NR, 0.0);
    std::vector<double> Z((size_t)NR * LD, 0.0), Yn((size_t)NR * LD, 0.0);
    // the residual norms always belong to the estimate that is returned: before the first solve that is U = 0, whose residual is r itself
    double rnorm[NR];
    for (int q = 0; q < NR; ++q) rnorm[q] = active[q] ? std::sqrt(rr[q * NR + q]) : 0.0;
    int m_done = 0, it = 0, nconv = NR - nactive;
    bool converged = nactive == 0;
    for (it = 1; m > 0 && !converged && it <= maxit; ++it) {
        for (int k = m_done; k < m; ++k)
            if ((rc = sigma.apply(V.p + (size_t)k * dim, Sg.p + (size_t)k * dim)) != QC_OK) return rc;
        // new rows of the projected matrix, M[k][j] = <V_j, Sg_k>, j <= k, and the new entries of V^T r, B[q][j] = <V_j, r^q>
        hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, m - m_done), dim3(256), 0, st, dim, V.p, Sg.p, m_done, LD, dA.p);
        hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m - m_done, NR), dim3(256), 0, st, dim, V.p + (size_t)m_done * dim, Rh.p, 0, LD, dB.p + m_done);
        QC_HIP_CHECK(hipMemcpyAsync(M.data() + (size_t)m_done * LD, dA.p + (size_t)m_done * LD, (size_t)(m - m_done) * LD * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipMemcpyAsync(B.data(), dB.p, B.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        m_done = m;
        std::vector<double> A((size_t)m * m), b((size_t)NR * m, 0.0), y((size_t)NR * m, 0.0);
        for (int i = 0; i < m; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * m + j] = A[(size_t)j * m + i] = M[(size_t)i * LD + j];
        for (int q = 0; q < NR; ++q) if (active[q]) for (int j = 0; j < m; ++j) b[(size_t)q * m + j] = B[(size_t)q * LD + j];
        if (!host_lu_solve(m, A, NR, b.data(), y.data())) break;   // (a singular projected system: the last estimates and their residuals stand)
        std::fill(Y.begin(), Y.end(), 0.0);
        for (int q = 0; q < NR; ++q) for (int j = 0; j < m; ++j) Y[(size_t)q * LD + j] = y[(size_t)q * m + j];
        QC_HIP_CHECK(hipMemcpyAsync(dY.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
        // the subspace is full: collapse onto the current solutions, orthonormalised in coefficient space (V is orthonormal); their sigma
        // vectors follow by linearity, and the Galerkin solutions in the smaller space are the same vectors.  Only a space larger than the
        // subspace collapses: with dim <= QC_STAB_MAXSUB the basis grows until it spans the whole space, where the solve is exact
        // (at most dim builds).
        if (dim > msub && m + nactive > msub && m > nactive) {
            std::fill(Z.begin(), Z.end(), 0.0);
            int k = 0;
            for (int q = 0; q < NR; ++q) {
                if (!active[q]) continue;
                double *z = &Z[(size_t)k * LD];
                double before = 0.0, after = 0.0;
                for (int j = 0; j < m; ++j) { z[j] = Y[(size_t)q * LD + j]; before += z[j] * z[j]; }
                for (int pass = 0; pass < 2; ++pass)
                    for (int r = 0; r < k; ++r) {
                        double d = 0.0;
                        for (int j = 0; j < m; ++j) d += z[j] * Z[(size_t)r * LD + j];
                        for (int j = 0; j < m; ++j) z[j] -= d * Z[(size_t)r * LD + j];
                    }
                for (int j = 0; j < m; ++j) after += z[j] * z[j];
                if (!(after > QC_STAB_KEEP * QC_STAB_KEEP * before)) { std::fill(z, z + LD, 0.0); continue; }
                const double inv = 1.0 / std::sqrt(after);
                for (int j = 0; j < m; ++j) z[j] *= inv;
                ++k;
            }
            if (k > 0) {
                QC_HIP_CHECK(hipMemcpyAsync(dY.p, Z.data(), Z.size() * sizeof(double), hipMemcpyHostToDevice, st));
                dim3 grid((dim + 255) / 256, k);
                hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m, LD, dY.p, V.p, Wk.p);
                hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m, LD, dY.p, Sg.p, Wk.p + (size_t)NR * dim);
                QC_HIP_CHECK(hipMemcpyAsync(V.p, Wk.p, (size_t)k * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
                QC_HIP_CHECK(hipMemcpyAsync(Sg.p, Wk.p + (size_t)NR * dim, (size_t)k * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
                // coefficients of the solutions in the new basis, and its projected matrix and right-hand sides
                std::fill(Yn.begin(), Yn.end(), 0.0);
                for (int q = 0; q < NR; ++q)
                    for (int r = 0; r < k; ++r) {
                        double d = 0.0;
                        for (int j = 0; j < m; ++j) d += Z[(size_t)r * LD + j] * Y[(size_t)q * LD + j];
                        Yn[(size_t)q * LD + r] = d;
                    }
                Y.swap(Yn);
                m = m_done = k;
                hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, m), dim3(256), 0, st, dim, V.p, Sg.p, 0, LD, dA.p);
                hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, NR), dim3(256), 0, st, dim, V.p, Rh.p, 0, LD, dB.p);
                QC_HIP_CHECK(hipMemcpyAsync(M.data(), dA.p, (size_t)m * LD * sizeof(double), hipMemcpyDeviceToHost, st));
                QC_HIP_CHECK(hipMemcpyAsync(dY.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
            }
        }
        // residual | preconditioner | orthogonalisation of every right-hand side, one launch each; the device counts the vectors it added
        QC_HIP_CHECK(hipMemsetAsync(dCnt.p, 0, sizeof(int), st));
        for (int q = 0; q < NR; ++q)
            if (active[q])
                hipLaunchKernelGGL(qc_stab_expand_kernel<true>, dim3(1), dim3(1024), 0, st, dim, m, msub, V.p, (const double *)Sg.p,
                                   (const double *)(dY.p + (size_t)q * LD), (const double *)nullptr, (const double *)dDe.p, (const double *)nullptr,
                                   (const double *)(Rh.p + (size_t)q * dim), tol, dCnt.p, dInfo.p + 2 * q);
        int added = 0;
        QC_HIP_CHECK(hipMemcpyAsync(info.data(), dInfo.p, 2 * NR * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipMemcpyAsync(&added, dCnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        nconv = 0;
        for (int q = 0; q < NR; ++q) { rnorm[q] = active[q] ? std::sqrt(info[2 * q]) : 0.0; if (rnorm[q] <= tol) ++nconv; }
        if (nconv == NR) { converged = true; break; }
        if (added == 0) break;                           // (nothing left to add: the residuals are as small as this arithmetic makes them)
        m += added;
    }
    if (it > maxit) it = maxit;
    if (nactive == 0 || m == 0) it = 0;

    // U^q = sum_j y^q_j V_j, alpha_pq = c <r^p, U^q> by the fixed-order dot products; symmetrised on the host
    if (m_done > 0) {
        QC_HIP_CHECK(hipMemcpyAsync(dY.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(qc_stab_lincomb_kernel, dim3((dim + 255) / 256, NR), dim3(256), 0, st, dim, m_done, LD, dY.p, V.p, Wk.p);
        hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(NR, NR), dim3(256), 0, st, dim, Rh.p, Wk.p, 0, NR, dOut.p);       // out[q * 3 + p] = <r^p, U^q>
        double ru[NR * NR];
        QC_HIP_CHECK(hipMemcpyAsync(ru, dOut.p, sizeof(ru), hipMemcpyDeviceToHost, st));
        if (response) QC_HIP_CHECK(hipMemcpyAsync(response, Wk.p, (size_t)NR * dim * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        for (int p = 0; p < NR; ++p)
            for (int q = 0; q < NR; ++q) {
                const double apq = c_alpha * ru[q * NR + p], aqp = c_alpha * ru[p * NR + q];
                io->alpha[p * NR + q] = 0.5 * (apq + aqp);
                io->asymmetry = std::max(io->asymmetry, std::fabs(apq - aqp));
            }
    }
    QC_HIP_CHECK(hipGetLastError());
    for (int q = 0; q < NR; ++q) io->residuals[q] = rnorm[q];
    io->nconverged = nconv; io->iterations = it; io->builds = sigma.builds;
    io->ms_builds = sigma.ms_builds;
    io->ms_total = qc_now_ms() - t_begin;
    return converged ? QC_OK : QC_NOT_CONVERGED;
}
