// qc_subspace.h - what the stability analysis (qc_stability.hip), the response solver (qc_response.hip) and the excited states
// (qc_excited.hip) share: the reduced-space subspace (QcSubspace, qc_subspace.hip), the layout of a vector and the Hessian-vector product
// sigma = (A + B) x as one direct Fock build (StabLayout, StabSigma, qc_stability.hip), the fixed-order workgroup sum and the block Davidson
// loop over an abstract product.  Host numerics: qc_subspace_host.h.  Every kernel is compiled once, in the file named.
#pragma once
#include "qc_internal.h"
#include "qc_subspace_host.h"

constexpr int QC_STAB_MAXROOTS = 8;
constexpr int QC_STAB_MAXSUB = 40;            // rows of the subspace: full -> collapse onto the Ritz vectors of the requested roots
constexpr double QC_STAB_DENOM_FLOOR = 1e-4;  // |e_a - e_i - theta| of the diagonal preconditioner is not allowed below this

// sum of `s` over the workgroup, the same bits in every thread: lanes by a shuffle tree, waves in index order (sh: 16 doubles)
__device__ __forceinline__ double qc_stab_block_sum(double s, double *sh) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __syncthreads();                                    // (the previous sum has been read by everybody)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    const int nw = (int)(blockDim.x >> 6);
    for (int k = 0; k < nw; ++k) t += sh[k];
    return t;
}

// M[(k0 + k) * ldm + j] = <V_j, Sg_(k0 + k)>, j < nv, k < nk, by the fixed-order dot products (qc_stab_dots_kernel)
void qc_stab_dots(hipStream_t st, int dim, const double *V, int nv, const double *Sg, int k0, int nk, int ldm, double *M);

// The state of a reduced-space iteration: an orthonormal basis V of at most msub = min(dim, QC_STAB_MAXSUB) rows of `dim` doubles, the products of its rows
// with one or two operators (Sg), the projected matrices V^T Sg (device and host, leading dimension LD, the lower triangle counts) and the scratch of the
// kernels.  m rows are in the basis, m_done of them have their products and their rows of the projected matrices: the caller forms the products of rows
// m_done .. m - 1 and calls project().  The reduced problem, the rows a restart keeps and the stop rule are the solver's.  Device pointers unless noted.
struct QcSubspace {
    static constexpr int LD = QC_STAB_MAXSUB;
    hipStream_t st = nullptr;
    int dim = 0, msub = 0, nops = 0, work_rows = 0, m = 0, m_done = 0;
    DevBuf V, Sg[2];               // msub + 1 rows each: row m of V is the work array of the expand kernel
    DevBuf Wk;                     // (1 + nops) blocks of work_rows rows: the targets of a collapse, staging for the caller
    DevBuf dM[2];                  // LD x LD per operator ...
    std::vector<double> M[2];      // ... and on the host
    DevBuf coef, info;             // LD x LD coefficient rows; 2 (LD + 1) words: slot s = {|t|^2 before, length after (0: not added)} of a launch
    QcDev<int> cnt;                // vectors added since the last added() (zero after alloc)
    int alloc(hipStream_t st_, int dim_, int nops_, int work_rows_);
    // one launch of the expand kernel, info slot s.  seed: src is orthogonalised against the basis and, if enough is left and there is room, normalised into the next row;
    // expand_residual: the same for t = r / (diag - theta), r = sum_j coef_row[j] (Sg0_j - theta V_j) [- rhs], if |r| > tol (theta null: 0; rhs null: the eigenvalue instance)
    void expand(const double *y, const double *theta, const double *diag, const double *src, const double *rhs, double tol, int info_slot);
    void seed(const double *src, int s) { expand(nullptr, nullptr, nullptr, src, nullptr, 0.0, s); }
    void expand_residual(const double *coef_row, const double *theta, const double *diag, const double *rhs, double tol, int s) { expand(coef_row, theta, diag, nullptr, rhs, tol, s); }
    int added(int *count);         // rows added since the last call (host): waits for the stream, clears the counter; the caller adds them to m
    int project();                 // rows m_done .. m - 1 of every projected matrix, to the host; waits for the stream; m_done = m
    int project_rows(int k0);      // (rows k0 .. m - 1: the dot products and their copies to the host, enqueued)
    std::vector<double> reduced(int op) const;            // the dense symmetric m_done x m_done projected matrix of operator `op`
    // out[r] = sum_j coef_rows[r * LD + j] B_j, r < rows, j < m_done; block 0: B = V, block 1 + op: B = Sg[op]
    void combine(const double *coef_rows, int rows, int block, double *out);
    // the basis becomes the k combinations Z (host, k rows of LD, orthonormal; null: the rows already in `coef`) of its rows, the sigma blocks
    // follow by linearity, m = m_done = k and every projected matrix is formed again (its copy to the host is enqueued, not waited for)
    int collapse(const double *Z, int k);
};
// Start vectors of a Davidson iteration for the lowest `nroots` roots of an operator with diagonal `de` (host), orthonormalised into the empty subspace
int qc_stab_start(QcSubspace &sub, int nroots, const std::vector<double> &de);

// blocks of a vector: one per spin of a UHF state, one for an RHF state
struct StabLayout {
    int nblk = 1, o[2] = {0, 0}, v[2] = {0, 0}, off[2] = {0, 0}, dim = 0;
    StabLayout(int n, bool uhf, const int *nocc) {
        nblk = uhf ? 2 : 1;
        for (int b = 0; b < nblk; ++b) { o[b] = nocc[b]; v[b] = n - nocc[b]; off[b] = dim; dim += o[b] * v[b]; }
    }
};

// dDe[off_b + i * v + a] = eps_b[o + a] - eps_b[i] for every block of the layout (dEps: nblk n-vectors), enqueued
void qc_stab_fill_delta(hipStream_t st, const StabLayout &L, int n, const double *dEps, double *dDe);
// out (o x v) = C_occ^T (M C_virt) for an n x n matrix M in the AO basis and orbitals C (columns; occupied first); scratch: n x v
void qc_ao_to_ov(hipStream_t st, int n, int o, int v, const double *C, const double *M_ao, double *scratch, double *out);

// the Hessian-vector product: sigma = (A + B) x, one direct Fock build (qc_stability.hip)
struct StabSigma {
    qc_system *S; StabLayout L; bool uhf; int kind;
    const double *dC;          // nblk blocks of n x n, columns = MOs
    const double *dDe;         // e_a - e_i, `dim` doubles
    DevBuf P, Q, D1, G, R;
    double ms_builds = 0.0; int builds = 0;
    StabSigma(qc_system *S_, const StabLayout &L_, bool uhf_, int kind_, const double *dC_, const double *dDe_) : S(S_), L(L_), uhf(uhf_), kind(kind_), dC(dC_), dDe(dDe_) {}
    int alloc();
    int apply(const double *dx, double *dsg);
};

struct StabDavidsonOut { double theta[QC_STAB_MAXROOTS], rnorm[QC_STAB_MAXROOTS]; int nconv = 0, iterations = 0; };
// Block Davidson iteration for the lowest `nroots` eigenpairs of a symmetric operator of order `dim` (nroots <= dim, <= QC_STAB_MAXROOTS).
// apply(V, Sg, k0, k1) writes the products of rows k0 .. k1 - 1 of V into the same rows of Sg (both device, rows of `dim` doubles) on the
// handle's stream and returns a status; dDiag / de: the diagonal of the preconditioner on the device and on the host.  Ritz vectors
// (nroots x dim) go to `vectors` (host) and `d_vectors` (device), both nullable.  eig_stop: the stop ratio of host_sym_eig for the
// subspace matrix.  QC_OK, QC_NOT_CONVERGED (out is filled with the best estimates) or an error.
template <class Apply>
int qc_stab_davidson(qc_system *S, int dim, int nroots, double tol, int maxit, const double *dDiag, const std::vector<double> &de, Apply &&apply,
                     StabDavidsonOut &out, double *vectors, double *d_vectors, double eig_stop = 1e-32) {
    constexpr int LD = QcSubspace::LD;
    hipStream_t st = S->stream;
    QcSubspace sub; DevBuf dTheta;
    if (sub.alloc(st, dim, 1, QC_STAB_MAXROOTS) != QC_OK || dTheta.alloc(QC_STAB_MAXROOTS) != QC_OK) return QC_ERR_HIP;
    int rc = qc_stab_start(sub, nroots, de);
    if (rc != QC_OK) return rc;
    std::vector<double> w, Y, theta(nroots, 0.0), rnorm(nroots, 0.0), info(2 * QC_STAB_MAXROOTS), Ysel((size_t)QC_STAB_MAXROOTS * LD, 0.0);
    int it = 0, nconv = 0; bool converged = false;
    for (it = 1; it <= maxit; ++it) {
        if ((rc = apply((const double *)sub.V.p, sub.Sg[0].p, sub.m_done, sub.m)) != QC_OK) return rc;
        if ((rc = sub.project()) != QC_OK) return rc;
        const int m = sub.m;
        host_sym_eig(m, sub.reduced(0), w, Y, eig_stop);
        for (int r = 0; r < nroots; ++r) {
            theta[r] = w[r];
            for (int j = 0; j < LD; ++j) Ysel[(size_t)r * LD + j] = j < m ? Y[(size_t)r * m + j] : 0.0;
        }
        QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Ysel.data(), Ysel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dTheta.p, theta.data(), nroots * sizeof(double), hipMemcpyHostToDevice, st));
        // the subspace is full: collapse onto the requested Ritz vectors (coefficients already in `coef`; unit rows afterwards); nothing waits before the expand launches
        if (m + nroots > sub.msub && m > nroots && m < dim) {
            if ((rc = sub.collapse(nullptr, nroots)) != QC_OK) return rc;
            std::fill(Ysel.begin(), Ysel.end(), 0.0);
            for (int r = 0; r < nroots; ++r) Ysel[(size_t)r * LD + r] = 1.0;
            QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Ysel.data(), Ysel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        }
        // residual | preconditioner | orthogonalisation of every requested root, one launch each; the device counts the vectors it added
        for (int r = 0; r < nroots; ++r) sub.expand_residual(sub.coef.p + (size_t)r * LD, dTheta.p + r, dDiag, nullptr, tol, r);
        int added = 0;
        QC_HIP_CHECK(hipMemcpyAsync(info.data(), sub.info.p, 2 * nroots * sizeof(double), hipMemcpyDeviceToHost, st));
        if ((rc = sub.added(&added)) != QC_OK) return rc;
        nconv = 0;
        for (int r = 0; r < nroots; ++r) { rnorm[r] = std::sqrt(info[2 * r]); if (rnorm[r] <= tol) ++nconv; }
        if (nconv == nroots) { converged = true; break; }
        if (added == 0) break;                           // (nothing left to add: the residuals are as small as this arithmetic makes them)
        sub.m += added;
    }
    if (it > maxit) it = maxit;
    for (int r = 0; r < QC_STAB_MAXROOTS; ++r) { out.theta[r] = r < nroots ? theta[r] : 0.0; out.rnorm[r] = r < nroots ? rnorm[r] : 0.0; }
    out.nconv = nconv; out.iterations = it;
    if (vectors || d_vectors) {
        sub.combine(sub.coef.p, nroots, 0, sub.Wk.p);
        if (vectors) QC_HIP_CHECK(hipMemcpyAsync(vectors, sub.Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToHost, st));
        if (d_vectors) QC_HIP_CHECK(hipMemcpyAsync(d_vectors, sub.Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
    }
    QC_HIP_CHECK(hipGetLastError());
    return converged ? QC_OK : QC_NOT_CONVERGED;
}
