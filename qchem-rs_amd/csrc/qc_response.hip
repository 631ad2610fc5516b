// qc_response.hip - first-order properties and static response of an SCF state: the trace of the density with the dipole matrices, and the
// static dipole polarizability by coupled-perturbed Hartree-Fock.
//
// For a static, real perturbation the first-order orbital rotations U^q solve (A + B) U^q = r^q with r^q = C_occ^T M_q C_virt per spin
// block (M_q: dipole matrix of direction q; vectors laid out x[i * v + a] as in qc_stability.hip), and
//   alpha_pq = c r^p . U^q,   c = 4 for an RHF state (singlet operator), c = 2 for a UHF state (internal operator, vector [x^a; x^b]).
// (A + B) x is the Hessian-vector product of the stability analysis - one direct Fock build of the symmetric pseudo-density, StabSigma in qc_subspace.h.
// The three systems share one orthonormal subspace (QcSubspace, qc_subspace.h; reduced-space iteration): per round one build per new vector, the projected
// matrix V^T (A + B) V and V^T r by fixed-order dot products, the small systems solved on the host, and per right-hand side one launch that
// forms the residual, preconditions it with 1 / (e_a - e_i) and orthogonalises it into V.  A Galerkin solve needs the projected matrix
// to be non-singular, not (A + B) to be positive definite: at a saddle the iteration works as long as no projected matrix is singular.
// Every sum is a fixed-order reduction and the Fock build accumulates integers: a call is bitwise reproducible.
#include "qc_subspace.h"

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

// the same trace for `count` matrices (the Cartesian multipoles): one workgroup per matrix
int qc_multipole_trace_device(qc_system *S, int count, const double *dPa, const double *dPb, const double *dM, double *tr) {
    DevBuf out;
    if (out.alloc(count) != QC_OK) return QC_ERR_HIP;
    hipLaunchKernelGGL(qc_dipole_trace_kernel, dim3(count), dim3(256), 0, S->stream, (size_t)S->nbasis * S->nbasis, dPa, dPb, dM, out.p);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipMemcpyAsync(tr, out.p, count * sizeof(double), hipMemcpyDeviceToHost, S->stream));
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
    DevBuf dDe, dM3, Rh, dB, dOut;
    QcSubspace sub;
    StabSigma sigma(S, L, uhf, 0, dC, nullptr);
    if (dDe.alloc(dim) != QC_OK || dM3.alloc(3 * nn) != QC_OK || Rh.alloc((size_t)NR * dim) != QC_OK || sub.alloc(st, dim, 1, NR) != QC_OK ||
        dB.alloc((size_t)NR * LD) != QC_OK || dOut.alloc(NR * NR) != QC_OK || sigma.alloc() != QC_OK) return QC_ERR_HIP;
    sigma.dDe = dDe.p;
    qc_stab_fill_delta(st, L, n, dEps, dDe.p);

    // right-hand sides r^q = C_occ^T M_q C_virt per block (origin 0: occupied and virtual orbitals are orthogonal), and their squared norms
    const double origin[3] = {0.0, 0.0, 0.0};
    int rc = qc_dipole_device(S, origin, dM3.p);
    if (rc != QC_OK) return rc;
    for (int q = 0; q < NR; ++q)
        for (int b = 0; b < L.nblk; ++b)
            if (L.o[b] > 0 && L.v[b] > 0) qc_ao_to_ov(st, n, L.o[b], L.v[b], dC + b * nn, dM3.p + q * nn, sigma.P.p, Rh.p + (size_t)q * dim + L.off[b]);
    qc_stab_dots(st, dim, Rh.p, NR, Rh.p, 0, NR, NR, dOut.p);
    double rr[NR * NR];
    QC_HIP_CHECK(hipMemcpyAsync(rr, dOut.p, sizeof(rr), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    bool active[NR]; int nactive = 0;
    for (int q = 0; q < NR; ++q) { active[q] = rr[q * NR + q] > 0.0; nactive += active[q] ? 1 : 0; }

    // start vectors: the preconditioned right-hand sides, orthonormalised (staged in the work rows)
    for (int q = 0; q < NR; ++q) {
        if (!active[q]) continue;
        hipLaunchKernelGGL(qc_cphf_precond_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, dim, dDe.p, Rh.p + (size_t)q * dim, sub.Wk.p + (size_t)q * dim);
        sub.seed(sub.Wk.p + (size_t)q * dim, q);
    }
    if ((rc = sub.added(&sub.m)) != QC_OK) return rc;

    // (Z: the collapse's coefficient array; Y and Z are sources of enqueued copies and live as long as the stream may read them)
    std::vector<double> B((size_t)NR * LD, 0.0), Y((size_t)NR * LD, 0.0), info(2 * NR, 0.0), Z((size_t)NR * LD, 0.0), Yn((size_t)NR * LD, 0.0);
    // the residual norms always belong to the estimate that is returned: before the first solve that is U = 0, whose residual is r itself
    double rnorm[NR];
    for (int q = 0; q < NR; ++q) rnorm[q] = active[q] ? std::sqrt(rr[q * NR + q]) : 0.0;
    int it = 0, nconv = NR - nactive; bool converged = nactive == 0;
    for (it = 1; sub.m > 0 && !converged && it <= maxit; ++it) {
        for (int k = sub.m_done; k < sub.m; ++k)
            if ((rc = sigma.apply(sub.V.p + (size_t)k * dim, sub.Sg[0].p + (size_t)k * dim)) != QC_OK) return rc;
        // new entries of V^T r, B[q][j] = <V_j, r^q>, then the new rows of the projected matrix (B's launch and copy stood behind the matrix's: nothing in common; the one wait is still project()'s)
        qc_stab_dots(st, dim, sub.V.p + (size_t)sub.m_done * dim, sub.m - sub.m_done, Rh.p, 0, NR, LD, dB.p + sub.m_done);
        QC_HIP_CHECK(hipMemcpyAsync(B.data(), dB.p, B.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if ((rc = sub.project()) != QC_OK) return rc;
        const int m = sub.m;
        std::vector<double> b((size_t)NR * m, 0.0), y((size_t)NR * m, 0.0);
        for (int q = 0; q < NR; ++q) if (active[q]) for (int j = 0; j < m; ++j) b[(size_t)q * m + j] = B[(size_t)q * LD + j];
        if (!host_lu_solve(m, sub.reduced(0), NR, b.data(), y.data())) break;   // (a singular projected system: the last estimates and their residuals stand)
        std::fill(Y.begin(), Y.end(), 0.0);
        for (int q = 0; q < NR; ++q) for (int j = 0; j < m; ++j) Y[(size_t)q * LD + j] = y[(size_t)q * m + j];
        QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
        // the subspace is full: collapse onto the current solutions, orthonormalised in coefficient space (V is orthonormal); their sigma
        // vectors follow by linearity, and the Galerkin solutions in the smaller space are the same vectors.  Only a space larger than the
        // subspace collapses: with dim <= QC_STAB_MAXSUB the basis grows until it spans the whole space, where the solve is exact
        // (at most dim builds).
        if (dim > sub.msub && m + nactive > sub.msub && m > nactive) {
            std::fill(Z.begin(), Z.end(), 0.0);
            int k = 0;
            for (int q = 0; q < NR; ++q)
                if (active[q] && qc_orthonormalize_row(Z.data(), LD, m, k, &Y[(size_t)q * LD])) ++k;
            if (k > 0) {
                if ((rc = sub.collapse(Z.data(), k)) != QC_OK) return rc;
                // the solutions' coefficients and V^T r in the new basis (V^T r's launch stood before the matrix's copy to the host, which collapse() enqueues: nothing in common)
                qc_rows_in_basis(Z.data(), LD, m, k, Y.data(), NR, Yn.data());
                Y.swap(Yn);
                qc_stab_dots(st, dim, sub.V.p, k, Rh.p, 0, NR, LD, dB.p);
                QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
            }
        }
        // residual | preconditioner | orthogonalisation of every right-hand side, one launch each; the device counts the vectors it added
        for (int q = 0; q < NR; ++q)
            if (active[q]) sub.expand_residual(sub.coef.p + (size_t)q * LD, nullptr, dDe.p, Rh.p + (size_t)q * dim, tol, q);
        int added = 0;
        QC_HIP_CHECK(hipMemcpyAsync(info.data(), sub.info.p, 2 * NR * sizeof(double), hipMemcpyDeviceToHost, st));
        if ((rc = sub.added(&added)) != QC_OK) return rc;
        nconv = 0;
        for (int q = 0; q < NR; ++q) { rnorm[q] = active[q] ? std::sqrt(info[2 * q]) : 0.0; if (rnorm[q] <= tol) ++nconv; }
        if (nconv == NR) { converged = true; break; }
        if (added == 0) break;                           // (nothing left to add: the residuals are as small as this arithmetic makes them)
        sub.m += added;
    }
    if (it > maxit) it = maxit;
    if (nactive == 0 || sub.m == 0) it = 0;

    // U^q = sum_j y^q_j V_j, alpha_pq = c <r^p, U^q> by the fixed-order dot products; symmetrised on the host
    if (sub.m_done > 0) {
        QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Y.data(), Y.size() * sizeof(double), hipMemcpyHostToDevice, st));
        sub.combine(sub.coef.p, NR, 0, sub.Wk.p);
        qc_stab_dots(st, dim, Rh.p, NR, sub.Wk.p, 0, NR, NR, dOut.p);       // out[q * 3 + p] = <r^p, U^q>
        double ru[NR * NR];
        QC_HIP_CHECK(hipMemcpyAsync(ru, dOut.p, sizeof(ru), hipMemcpyDeviceToHost, st));
        if (response) QC_HIP_CHECK(hipMemcpyAsync(response, sub.Wk.p, (size_t)NR * dim * sizeof(double), hipMemcpyDeviceToHost, st));
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
