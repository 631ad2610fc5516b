// qc_subspace.hip - the subspace kernels of the reduced-space solvers and the QcSubspace operations that launch them (qc_subspace.h): fixed-order dot
// products, linear combinations of rows, one workgroup that makes a residual or a staged vector the next basis vector.  Nothing depends on scheduling.
#include "qc_subspace.h"

namespace {

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

}  // namespace

void qc_stab_dots(hipStream_t st, int dim, const double *V, int nv, const double *Sg, int k0, int nk, int ldm, double *M) { hipLaunchKernelGGL(qc_stab_dots_kernel, dim3(nv, nk), dim3(256), 0, st, dim, V, Sg, k0, ldm, M); }

int QcSubspace::alloc(hipStream_t st_, int dim_, int nops_, int work_rows_) {
    st = st_; dim = dim_; nops = nops_; work_rows = work_rows_; m = m_done = 0; msub = std::min(dim, QC_STAB_MAXSUB);
    const size_t rows = (size_t)msub + 1;
    if (V.alloc(rows * dim) != QC_OK || Wk.alloc((size_t)(1 + nops) * work_rows * dim) != QC_OK || coef.alloc((size_t)LD * LD) != QC_OK ||
        info.alloc(2 * (LD + 1)) != QC_OK || cnt.alloc(1) != QC_OK) return QC_ERR_HIP;
    for (int op = 0; op < nops; ++op) {
        if (Sg[op].alloc(rows * dim) != QC_OK || dM[op].alloc((size_t)LD * LD) != QC_OK) return QC_ERR_HIP;
        M[op].assign((size_t)LD * LD, 0.0);
    }
    QC_HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int), st));
    return QC_OK;
}

void QcSubspace::expand(const double *y, const double *theta, const double *diag, const double *src, const double *rhs, double tol, int info_slot) {
    hipLaunchKernelGGL(rhs ? qc_stab_expand_kernel<true> : qc_stab_expand_kernel<false>, dim3(1), dim3(1024), 0, st, dim, m, msub, V.p,
                       src ? nullptr : (const double *)Sg[0].p, y, theta, diag, src, rhs, tol, cnt.p, info.p + 2 * info_slot);
}

int QcSubspace::added(int *count) {
    QC_HIP_CHECK(hipMemcpyAsync(count, cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    // (cleared here, behind the read, where every solver cleared it in front of its next round of launches: they find the same zero)
    QC_HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(int), st));
    return QC_OK;
}

int QcSubspace::project_rows(int k0) {
    for (int op = 0; op < nops; ++op) qc_stab_dots(st, dim, V.p, m, Sg[op].p, k0, m - k0, LD, dM[op].p);
    for (int op = 0; op < nops; ++op)
        QC_HIP_CHECK(hipMemcpyAsync(M[op].data() + (size_t)k0 * LD, dM[op].p + (size_t)k0 * LD, (size_t)(m - k0) * LD * sizeof(double), hipMemcpyDeviceToHost, st));
    return QC_OK;
}

int QcSubspace::project() {
    if (m > m_done && project_rows(m_done) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipStreamSynchronize(st));
    m_done = m;
    return QC_OK;
}

std::vector<double> QcSubspace::reduced(int op) const {
    std::vector<double> A((size_t)m_done * m_done);
    for (int i = 0; i < m_done; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * m_done + j] = A[(size_t)j * m_done + i] = M[op][(size_t)i * LD + j];
    return A;
}

void QcSubspace::combine(const double *coef_rows, int rows, int block, double *out) {
    hipLaunchKernelGGL(qc_stab_lincomb_kernel, dim3((dim + 255) / 256, rows), dim3(256), 0, st, dim, m_done, LD, coef_rows,
                       (const double *)(block ? Sg[block - 1].p : V.p), out);
}

int QcSubspace::collapse(const double *Z, int k) {
    // (the k rows the launches below read; the solvers used to send their whole, otherwise zero, arrays)
    if (Z) QC_HIP_CHECK(hipMemcpyAsync(coef.p, Z, (size_t)k * LD * sizeof(double), hipMemcpyHostToDevice, st));
    const size_t blk = (size_t)work_rows * dim;
    for (int b = 0; b <= nops; ++b) combine(coef.p, k, b, Wk.p + b * blk);
    QC_HIP_CHECK(hipMemcpyAsync(V.p, Wk.p, (size_t)k * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int op = 0; op < nops; ++op)
        QC_HIP_CHECK(hipMemcpyAsync(Sg[op].p, Wk.p + (1 + op) * blk, (size_t)k * dim * sizeof(double), hipMemcpyDeviceToDevice, st));
    m = m_done = k;
    return project_rows(0);
}

int qc_stab_start(QcSubspace &sub, int nroots, const std::vector<double> &de) {
    // Unit vectors on the smallest e_a - e_i (ties: lower index first); a subspace that can hold the whole space starts as
    // the whole space.  Unit vectors carry the symmetry of one orbital pair, and a Krylov space never leaves the symmetries it starts
    // with - so one more start vector has a fixed pseudo-random component on every orbital pair.
    const int dim = sub.dim;
    std::vector<int> order(dim);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return de[a] < de[b]; });
    const bool whole = dim <= QC_STAB_MAXSUB;
    const int nunit = whole ? dim : std::min(dim, 2 * nroots);
    const int nstart = whole ? dim : nunit + 1;
    std::vector<double> start((size_t)nstart * dim, 0.0);
    for (int k = 0; k < nunit; ++k) start[(size_t)k * dim + order[k]] = 1.0;
    if (!whole) {
        uint32_t lcg = 12345u;
        for (int e = 0; e < dim; ++e) { lcg = lcg * 1664525u + 1013904223u; start[(size_t)nunit * dim + e] = (double)(lcg >> 8) / 8388608.0 - 1.0; }
    }
    // (staged behind the subspace rows: Sg is not in use yet)
    if (nstart > sub.msub + 1) return QC_ERR_INVALID;
    double *stage = sub.Sg[0].p;
    QC_HIP_CHECK(hipMemcpyAsync(stage, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, sub.st));
    for (int k = 0; k < nstart; ++k) sub.seed(stage + (size_t)k * dim, k);
    // (a copy on the stream and a wait, where a wait and a blocking copy stood: the same value; the staged vectors have been read, the first sigma vector may overwrite them)
    if (sub.added(&sub.m) != QC_OK) return QC_ERR_HIP;
    if (sub.m < nroots) return QC_ERR_INVALID;
    return QC_OK;
}
