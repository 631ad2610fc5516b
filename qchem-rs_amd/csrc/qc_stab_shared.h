// qc_stab_shared.h - what the stability analysis (qc_stability.hip) and the response solver (qc_response.hip) share: the layout of a
// vector, the Hessian-vector product sigma = (A + B) x as one direct Fock build, the fixed-order reductions and the subspace kernels.
// Everything sits in an anonymous namespace: each of the two files compiles its own copy of the kernels from this one text.
#pragma once
#include <algorithm>

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

}  // namespace
