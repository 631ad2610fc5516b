// qc_stab_shared.h - what the stability analysis (qc_stability.hip), the response solver (qc_response.hip) and the excited states
// (qc_excited.hip) share: the layout of a vector, the Hessian-vector product sigma = (A + B) x as one direct Fock build, the fixed-order
// reductions, the subspace kernels, the host eigensolver of the subspace matrix and the block Davidson loop over an abstract product.
// Everything sits in an anonymous namespace: each of the files compiles its own copy of the kernels from this one text.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "qc_internal.h"

namespace {

constexpr int QC_STAB_MAXROOTS = 8;
constexpr int QC_STAB_MAXSUB = 40;            // rows of the subspace: full -> collapse onto the Ritz vectors of the requested roots
constexpr double QC_STAB_DENOM_FLOOR = 1e-4;  // |e_a - e_i - theta| of the diagonal preconditioner is not allowed below this
constexpr double QC_STAB_KEEP = 1e-4;         // a correction vector that loses more than this factor to the orthogonalisation is dropped

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

// de[i * v + a] = eps[o + a] - eps[i]
__global__ void qc_stab_delta_kernel(int o, int v, const double *__restrict__ eps, double *__restrict__ de) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < o * v) de[e] = eps[o + e % v] - eps[e / v];
}

// pseudo-density: D = s (Q + Q^T) with Q = C_occ x C_virt^T; Dneg (nullable) = -D
__global__ void qc_stab_symmetrize_kernel(int n, double s, const double *__restrict__ Q, double *__restrict__ D, double *__restrict__ Dneg) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * n) return;
    const int r = e / n, c = e % n;
    const double d = s * (Q[e] + Q[(size_t)c * n + r]);
    D[e] = d;
    if (Dneg) Dneg[e] = -d;
}

// sigma = de * x + R, R = the occupied-virtual block of the two-electron matrix
__global__ void qc_stab_sigma_kernel(int dim, const double *__restrict__ de, const double *__restrict__ x, const double *__restrict__ R,
                                     double *__restrict__ sg) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < dim) sg[e] = fma(de[e], x[e], R[e]);
}

// M[(k0 + k) * ldm + j] = <V_j, Sg_(k0 + k)>: workgroup (j, k), 256 threads
__global__ __launch_bounds__(256) void qc_stab_dots_kernel(int dim, const double *__restrict__ V, const double *__restrict__ Sg, int k0, int ldm,
                                                           double *__restrict__ M) {
    __shared__ double sh[16];
    const int j = blockIdx.x, k = k0 + blockIdx.y;
    const double *a = V + (size_t)j * dim, *b = Sg + (size_t)k * dim;
    double s = 0.0;
    for (int e = threadIdx.x; e < dim; e += 256) s = fma(a[e], b[e], s);
    s = qc_stab_block_sum(s, sh);
    if (threadIdx.x == 0) M[(size_t)k * ldm + j] = s;
}

// out[r * dim + e] = sum_j Y[r * ldy + j] In[j * dim + e], j < m (Ritz vectors and their sigma vectors)
__global__ void qc_stab_lincomb_kernel(int dim, int m, int ldy, const double *__restrict__ Y, const double *__restrict__ In, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (e >= dim) return;
    double s = 0.0;
    for (int j = 0; j < m; ++j) s = fma(Y[(size_t)r * ldy + j], In[(size_t)j * dim + e], s);
    out[(size_t)r * dim + e] = s;
}

// One new basis vector, one workgroup.  With m = m0 + *cnt vectors in V (m0 spanned by the Ritz coefficients y, *cnt added by earlier
// launches of this round):
//   src == null:  r = sum_j y_j (Sg_j - theta V_j) [- rhs], info[0] = |r|^2; if |r| > tol: t = r / (de - theta) with the floor on the denominator
//                 (RHS false: the residual of a Ritz pair; RHS true, theta_p == null: the residual of the linear system
//                 (A + B) u = rhs at u = sum_j y_j V_j - an instance of its own, so that the eigenvalue instance stays the code it was)
//   src != null:  t = src (start vectors), info[0] = |t|^2
// then t is orthogonalised against V_0 .. V_(m-1) twice (modified Gram-Schmidt), and if it keeps more than QC_STAB_KEEP of its length and
// the subspace has room it is normalised into row m and *cnt goes up.  info[1] = its length after the orthogonalisation (0: not added).
// Row m of V is the work array (V has msub + 1 rows).
template <bool RHS>
__global__ __launch_bounds__(1024) void qc_stab_expand_kernel(int dim, int m0, int msub, double *__restrict__ V, const double *__restrict__ Sg,
                                                              const double *__restrict__ y, const double *__restrict__ theta_p,
                                                              const double *__restrict__ de, const double *__restrict__ src,
                                                              const double *__restrict__ rhs, double tol, int *cnt, double *__restrict__ info) {
    __shared__ double sh[16];
    const int m = m0 + *cnt;
    double *t = V + (size_t)m * dim;
    const double theta = theta_p ? *theta_p : 0.0;
    double s = 0.0;
    for (int e = threadIdx.x; e < dim; e += 1024) {
        double r;
        if (src) r = src[e];
        else {
            r = 0.0;
            for (int j = 0; j < m0; ++j) r = fma(y[j], Sg[(size_t)j * dim + e] - theta * V[(size_t)j * dim + e], r);
            if (RHS) r -= rhs[e];
        }
        s = fma(r, r, s);
        t[e] = r;
    }
    const double rn2 = qc_stab_block_sum(s, sh);
    if (threadIdx.x == 0) { info[0] = rn2; info[1] = 0.0; }
    if (m >= msub || !(rn2 > 0.0) || (!src && sqrt(rn2) <= tol)) return;            // (uniform: every thread holds the same sum)
    s = 0.0;
    if (!src)
        for (int e = threadIdx.x; e < dim; e += 1024) {
            double d = de[e] - theta;
            if (fabs(d) < QC_STAB_DENOM_FLOOR) d = d < 0.0 ? -QC_STAB_DENOM_FLOOR : QC_STAB_DENOM_FLOOR;
            const double x = t[e] / d;
            t[e] = x;
            s = fma(x, x, s);
        }
    const double before = src ? rn2 : qc_stab_block_sum(s, sh);
    for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < m; ++j) {
            const double *vj = V + (size_t)j * dim;
            s = 0.0;
            for (int e = threadIdx.x; e < dim; e += 1024) s = fma(t[e], vj[e], s);
            const double c = qc_stab_block_sum(s, sh);
            for (int e = threadIdx.x; e < dim; e += 1024) t[e] = fma(-c, vj[e], t[e]);
        }
    s = 0.0;
    for (int e = threadIdx.x; e < dim; e += 1024) s = fma(t[e], t[e], s);
    const double after = qc_stab_block_sum(s, sh);
    if (!(after > QC_STAB_KEEP * QC_STAB_KEEP * before)) return;
    const double inv = 1.0 / sqrt(after);
    for (int e = threadIdx.x; e < dim; e += 1024) t[e] *= inv;
    if (threadIdx.x == 0) { info[1] = sqrt(after); *cnt = m - m0 + 1; }
}

// blocks of a vector: one per spin of a UHF state, one for an RHF state
struct StabLayout {
    int nblk = 1, o[2] = {0, 0}, v[2] = {0, 0}, off[2] = {0, 0}, dim = 0;
    StabLayout(int n, bool uhf, const int *nocc) {
        nblk = uhf ? 2 : 1;
        for (int b = 0; b < nblk; ++b) { o[b] = nocc[b]; v[b] = n - nocc[b]; off[b] = dim; dim += o[b] * v[b]; }
    }
};

// the Hessian-vector product: sigma = (A + B) x, one direct Fock build
struct StabSigma {
    qc_system *S;
    StabLayout L;
    bool uhf;
    int kind;
    const double *dC;          // nblk blocks of n x n, columns = MOs
    const double *dDe;         // e_a - e_i, `dim` doubles
    DevBuf P, Q, D1, G, R;
    double ms_builds = 0.0;
    int builds = 0;
    StabSigma(qc_system *S_, const StabLayout &L_, bool uhf_, int kind_, const double *dC_, const double *dDe_) : S(S_), L(L_), uhf(uhf_), kind(kind_), dC(dC_), dDe(dDe_) {}
    int alloc() {
        const size_t n = S->nbasis, nn = n * n;
        if (P.alloc(nn) != QC_OK || Q.alloc(nn) != QC_OK || D1.alloc(2 * nn) != QC_OK || G.alloc(2 * nn) != QC_OK || R.alloc(std::max<size_t>(L.dim, 1)) != QC_OK) return QC_ERR_HIP;
        return QC_OK;
    }
    int apply(const double *dx, double *dsg) {
        const int n = S->nbasis;
        const size_t nn = (size_t)n * n;
        hipStream_t st = S->stream;
        const bool triplet = !uhf && kind == 1, rhf_build = !uhf && kind == 0;
        for (int b = 0; b < L.nblk; ++b) {
            const double *Cb = dC + b * nn;
            double *Db = D1.p + b * nn;
            if (L.o[b] == 0 || L.v[b] == 0) { QC_HIP_CHECK(hipMemsetAsync(Db, 0, nn * sizeof(double), st)); continue; }
            qc_gemm(st, n, L.v[b], L.o[b], 1.0, Cb, n, false, dx + L.off[b], L.v[b], false, 0.0, P.p, L.v[b]);          // C_occ x
            qc_gemm(st, n, n, L.v[b], 1.0, P.p, L.v[b], false, Cb + L.o[b], n, true, 0.0, Q.p, n);                       // (.) C_virt^T
            hipLaunchKernelGGL(qc_stab_symmetrize_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, n, rhf_build ? 2.0 : 1.0, Q.p, Db,
                               triplet ? D1.p + nn : nullptr);
        }
        const double t0 = qc_now_ms();
        int rc = rhf_build ? qc_fock_build_device(S, D1.p, nullptr, G.p, nullptr, false)
                           : qc_fock_build_device(S, D1.p, D1.p + nn, G.p, G.p + nn, true);
        if (rc != QC_OK) return rc;
        QC_HIP_CHECK(hipStreamSynchronize(st));
        if ((rc = qc_join_check(S)) != QC_OK) return rc;
        qc_gate_quiet(S);
        ms_builds += qc_now_ms() - t0; builds += 1;
        for (int b = 0; b < L.nblk; ++b) {
            if (L.o[b] == 0 || L.v[b] == 0) continue;
            const double *Cb = dC + b * nn;
            const int ov = L.o[b] * L.v[b];
            qc_gemm(st, n, L.v[b], n, 1.0, G.p + b * nn, n, false, Cb + L.o[b], n, false, 0.0, P.p, L.v[b]);             // G C_virt
            qc_gemm(st, L.o[b], L.v[b], n, 1.0, Cb, n, true, P.p, L.v[b], false, 0.0, R.p + L.off[b], L.v[b]);            // C_occ^T (.)
            hipLaunchKernelGGL(qc_stab_sigma_kernel, dim3((ov + 255) / 256), dim3(256), 0, st, ov, dDe + L.off[b], dx + L.off[b], R.p + L.off[b],
                               dsg + L.off[b]);
        }
        QC_HIP_CHECK(hipGetLastError());
        return QC_OK;
    }
};

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

// Start vectors of a Davidson iteration for the lowest `nroots` roots of a symmetric operator with diagonal `de` (host), orthonormalised
// into rows 0 .. *m_out - 1 of V (msub + 1 rows).  stage: msub + 1 rows of scratch; cnt, info: the counter and the 2 (msub + 1) info words
// of the expand kernel.
inline int qc_stab_start(hipStream_t st, int dim, int nroots, int msub, const std::vector<double> &de, double *V, double *stage, int *cnt, double *info,
                         int *m_out) {
    // Unit vectors on the smallest e_a - e_i (ties: lower index first); a subspace that can hold the whole space starts as
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
        if (nstart > msub + 1) return QC_ERR_INVALID;
        QC_HIP_CHECK(hipMemcpyAsync(stage, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int), st));
        for (int k = 0; k < nstart; ++k)
            hipLaunchKernelGGL(qc_stab_expand_kernel<false>, dim3(1), dim3(1024), 0, st, dim, 0, msub, V, (const double *)nullptr, (const double *)nullptr,
                               (const double *)nullptr, (const double *)nullptr, (const double *)(stage + (size_t)k * dim), (const double *)nullptr, 0.0, cnt, info + 2 * k);
        QC_HIP_CHECK(hipStreamSynchronize(st));      // (the staged vectors have been read before the first sigma vector overwrites them)
    }
    QC_HIP_CHECK(hipMemcpy(m_out, cnt, sizeof(int), hipMemcpyDeviceToHost));
    if (*m_out < nroots) return QC_ERR_INVALID;
    return QC_OK;
}

struct StabDavidsonOut { double theta[QC_STAB_MAXROOTS], rnorm[QC_STAB_MAXROOTS]; int nconv = 0, iterations = 0; };

// Block Davidson iteration for the lowest `nroots` eigenpairs of a symmetric operator of order `dim` (nroots <= dim, <= QC_STAB_MAXROOTS).
// apply(V, Sg, k0, k1) writes the products of rows k0 .. k1 - 1 of V into the same rows of Sg (both device, rows of `dim` doubles) on the
// handle's stream and returns a status; dDiag / de: the diagonal of the preconditioner on the device and on the host.  Ritz vectors
// (nroots x dim) go to `vectors` (host) and `d_vectors` (device), both nullable.  eig_stop: the stop ratio of host_sym_eig for the
// subspace matrix.  QC_OK, QC_NOT_CONVERGED (out is filled with the best estimates) or an error.
template <class Apply>
int qc_stab_davidson(qc_system *S, int dim, int nroots, double tol, int maxit, const double *dDiag, const std::vector<double> &de, Apply &&apply,
                     StabDavidsonOut &out, double *vectors, double *d_vectors, double eig_stop = 1e-32) {
    hipStream_t st = S->stream;
    const int msub = std::min(dim, QC_STAB_MAXSUB);
    DevBuf V, Sg, Wk, dM, dY, dTheta, dInfo;
    QcDev<int> dCnt;
    const size_t rows = (size_t)msub + 1;
    if (V.alloc(rows * dim) != QC_OK || Sg.alloc(rows * dim) != QC_OK || Wk.alloc(2 * (size_t)QC_STAB_MAXROOTS * dim) != QC_OK ||
        dM.alloc((size_t)QC_STAB_MAXSUB * QC_STAB_MAXSUB) != QC_OK || dY.alloc((size_t)QC_STAB_MAXROOTS * QC_STAB_MAXSUB) != QC_OK ||
        dTheta.alloc(QC_STAB_MAXROOTS) != QC_OK || dInfo.alloc(2 * (QC_STAB_MAXSUB + 1)) != QC_OK || dCnt.alloc(1) != QC_OK) return QC_ERR_HIP;

    int m = 0;
    int rc = qc_stab_start(st, dim, nroots, msub, de, V.p, Sg.p, dCnt.p, dInfo.p, &m);
    if (rc != QC_OK) return rc;

    std::vector<double> M((size_t)QC_STAB_MAXSUB * QC_STAB_MAXSUB, 0.0), w, Y, theta(nroots, 0.0), rnorm(nroots, 0.0), info(2 * QC_STAB_MAXROOTS);
    std::vector<double> Ysel((size_t)QC_STAB_MAXROOTS * QC_STAB_MAXSUB, 0.0);
    int m_done = 0, it = 0, nconv = 0;
    bool converged = false;
    for (it = 1; it <= maxit; ++it) {
        if ((rc = apply((const double *)V.p, Sg.p, m_done, m)) != QC_OK) return rc;
        // new rows of the subspace matrix: M[k][j] = <V_j, Sg_k>, j <= k
        hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(m, m - m_done), dim3(256), 0, st, dim, V.p, Sg.p, m_done, QC_STAB_MAXSUB, dM.p);
        QC_HIP_CHECK(hipMemcpyAsync(M.data() + (size_t)m_done * QC_STAB_MAXSUB, dM.p + (size_t)m_done * QC_STAB_MAXSUB,
                                    (size_t)(m - m_done) * QC_STAB_MAXSUB * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        m_done = m;
        std::vector<double> A((size_t)m * m);
        for (int i = 0; i < m; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * m + j] = A[(size_t)j * m + i] = M[(size_t)i * QC_STAB_MAXSUB + j];
        host_sym_eig(m, A, w, Y, eig_stop);
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
                               (const double *)(dY.p + (size_t)r * QC_STAB_MAXSUB), (const double *)(dTheta.p + r), dDiag,
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
    for (int r = 0; r < QC_STAB_MAXROOTS; ++r) { out.theta[r] = r < nroots ? theta[r] : 0.0; out.rnorm[r] = r < nroots ? rnorm[r] : 0.0; }
    out.nconv = nconv; out.iterations = it;
    if (vectors || d_vectors) {
        dim3 grid((dim + 255) / 256, nroots);
        hipLaunchKernelGGL(qc_stab_lincomb_kernel, grid, dim3(256), 0, st, dim, m_done, QC_STAB_MAXSUB, dY.p, V.p, Wk.p);
        if (vectors) QC_HIP_CHECK(hipMemcpyAsync(vectors, Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToHost, st));
        if (d_vectors) QC_HIP_CHECK(hipMemcpyAsync(d_vectors, Wk.p, (size_t)nroots * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
    }
    QC_HIP_CHECK(hipGetLastError());
    return converged ? QC_OK : QC_NOT_CONVERGED;
}

}  // namespace
