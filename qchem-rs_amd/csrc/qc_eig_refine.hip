// qc_eig_refine.hip - the eigensolve of almost every SCF pass: Ogita-Aishima refinement (rule: qc_refine_rule.h) of the previous pass's
// or the tridiagonal path's eigenvectors, as one workgroup + host decisions (synchronous) or chip-wide A / B kernels + control words.
#include <cstdlib>
#include <vector>

#include "qc_internal.h"
#include "qc_refine_rule.h"

// ---------------------------------------------------------------------------------------------------------------
// Statistics of a refinement pass in one workgroup, for the synchronous variant (qc_eig_device_refine takes the decisions on the host):
// Rayleigh quotients, partner list and stats[0..6] as described in qc_refine_rule.h, with stats[5] = max a / g.
__global__ __launch_bounds__(1024) void qc_refine_stats_kernel(int n, const double *__restrict__ S, const double *__restrict__ XtX,
                                                                double *__restrict__ lam, double *__restrict__ stats, int *__restrict__ partner) {
    __shared__ double red[4 * 16];
    __shared__ double sh_scale;
    __shared__ int sh_multi, sh_nstrong;
    const int tid = threadIdx.x;
    double off = 0.0, rr = 0.0, amax = 0.0;
    for (int x = tid; x < n * n; x += 1024) {
        const int i = x / n, j = x - i * n;
        const double r = (i == j ? 1.0 : 0.0) - XtX[x];
        rr = fma(r, r, rr);
        if (i != j) off = fma(S[x], S[x], off);
        else { const double l = qc_ref_quotient(S[x], r); lam[i] = l; amax = fmax(amax, fabs(l)); }
    }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_down(off, o, 64); rr += __shfl_down(rr, o, 64); amax = fmax(amax, __shfl_down(amax, o, 64)); }
    if ((tid & 63) == 0) { red[tid >> 6] = off; red[16 + (tid >> 6)] = rr; red[32 + (tid >> 6)] = amax; }
    if (tid == 0) { sh_multi = 0; sh_nstrong = 0; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = 0; k < 16; ++k) { a += red[k]; b += red[16 + k]; c = fmax(c, red[32 + k]); }
        stats[0] = sqrt(a); stats[1] = sqrt(b); stats[2] = c;
        sh_scale = c;
    }
    __syncthreads();                                         // lam[] (global, written by this workgroup) is visible
    const double scale = sh_scale, tiny = QC_REF_TINY * scale, gfloor = QC_REF_GFLOOR * scale;
    double cmax = 0.0, emax = 0.0;
    for (int i = tid >> 4; i < n; i += 64) {                 // one row per team of 16 lanes
        int cnt = 0, who = -1;
        for (int j = tid & 15; j < n; j += 16) {
            if (j == i) continue;
            const double r = -XtX[(size_t)i * n + j];
            const double sij = 0.5 * (S[(size_t)i * n + j] + S[(size_t)j * n + i]);   // A is symmetric only to rounding
            const double a = fabs(QC_REF_COUPLING(sij, lam[i], lam[j], r)), g = fabs(lam[j] - lam[i]);
            if (!qc_ref_coupled(a, tiny)) continue;
            if (qc_ref_strong(a, g, gfloor)) { ++cnt; who = j; }
            else if (qc_ref_degenerate(g, gfloor)) cmax = fmax(cmax, a);
            else emax = fmax(emax, a / g);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 16); who = max(who, __shfl_xor(who, o, 16)); }
        if ((tid & 15) == 0) {
            partner[i] = qc_ref_partner(cnt, who);
            if (cnt > 1) sh_multi = 1;
            if (cnt == 1) atomicAdd(&sh_nstrong, 1);
        }
    }
    for (int o = 32; o > 0; o >>= 1) { cmax = fmax(cmax, __shfl_down(cmax, o, 64)); emax = fmax(emax, __shfl_down(emax, o, 64)); }
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = cmax; red[16 + (tid >> 6)] = emax; }
    // a strong pair must be mutual; one index per thread (partner[] was written by this workgroup before the barrier above) - as a
    // loop of thread 0 these dependent loads were half of the kernel's 18 us
    for (int i = tid; i < n; i += 1024) if (qc_ref_not_mutual(partner, i)) sh_multi = 1;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < 16; ++k) { a = fmax(a, red[k]); b = fmax(b, red[16 + k]); }
        stats[3] = 0.5 * sh_nstrong; stats[4] = a; stats[5] = b; stats[6] = sh_multi;
    }
}

// The statistics / decisions / update matrix of a refinement pass spread over the chip (round 3).  As one workgroup
// (qc_refine_stats_kernel above, kept for the synchronous variant) this took 28 us per pass at n = 114 - 74 us of benzene's 340 us Roothaan
// step: ~2000 f64-heavy instructions per wave for sixteen waves on ONE compute unit.  Now two launches of ceil(n / 8) workgroups of 256
// threads, eight rows each (32 lanes per row, columns l + 32 q):
//   A  every workgroup forms all n Rayleigh quotients itself (n loads: cheaper than a grid barrier), classifies the pairs of its rows,
//      fixes their partner[] entries and leaves its partial sums / maxima / flags in `part` (8 doubles per workgroup);
//   B  every workgroup folds the partials in a fixed order and takes the decisions itself (workgroup 0 publishes them), then writes
//      its rows of M = I + E.
// The size of the first-order update is tested as |a| <= tau g (no division; stats[5] reports the threshold exceeded).
constexpr int QC_STATS_ROWS = 8;
__global__ __launch_bounds__(256) void qc_refine_statsA_kernel(int n, const double *__restrict__ S, const double *__restrict__ XtX,
                                                                double *__restrict__ lam, int *__restrict__ partner, double *__restrict__ part,
                                                                const int *__restrict__ ctl) {
    if (ctl && ctl[QC_EIG_STATE] != QC_EIG_RUNNING) return;
    extern __shared__ double sh_lam[];                       // n
    __shared__ double red[3][4];
    __shared__ double sh_scale;
    __shared__ int sh_multi, sh_nstrong, sh_big, sh_notlast;
    const int tid = threadIdx.x, r = tid >> 5, l = tid & 31;
    double amax = 0.0;
    for (int t = tid; t < n; t += 256) {
        const double lv = qc_ref_quotient(S[(size_t)t * n + t], 1.0 - XtX[(size_t)t * n + t]);
        sh_lam[t] = lv; amax = fmax(amax, fabs(lv));
        if (blockIdx.x == 0) lam[t] = lv;
    }
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_down(amax, o, 64));
    if ((tid & 63) == 0) red[0][tid >> 6] = amax;
    if (tid == 0) { sh_multi = 0; sh_nstrong = 0; sh_big = 0; sh_notlast = 0; }
    __syncthreads();
    if (tid == 0) sh_scale = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    __syncthreads();
    const double scale = sh_scale, tiny = QC_REF_TINY * scale, gfloor = QC_REF_GFLOOR * scale;
    const int i = blockIdx.x * QC_STATS_ROWS + r;
    const bool iok = i < n;
    const double li = sh_lam[iok ? i : 0];
    double off = 0.0, rsum = 0.0, cmax = 0.0;
    int cnt = 0, who = -1, big = 0, notlast = 0;
    for (int j0 = l; j0 < n; j0 += 128) {                    // four columns of the row at a time
        double sij[4], sji[4], xij[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 32 * u;
            const bool ok = iok && j < n;
            sij[u] = S[ok ? (size_t)i * n + j : 0]; sji[u] = S[ok ? (size_t)j * n + i : 0]; xij[u] = XtX[ok ? (size_t)i * n + j : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 32 * u;
            if (iok && j < n) {
                const double rv = (i == j ? 1.0 : 0.0) - xij[u];
                rsum = fma(rv, rv, rsum);
                if (i != j) {
                    off = fma(sij[u], sij[u], off);
                    const double lj = sh_lam[j];
                    const double av = fabs(QC_REF_COUPLING(0.5 * (sij[u] + sji[u]), li, lj, rv)), g = fabs(lj - li);
                    if (qc_ref_coupled(av, tiny)) {
                        if (qc_ref_strong(av, g, gfloor)) { ++cnt; who = j; }
                        else if (qc_ref_degenerate(g, gfloor)) cmax = fmax(cmax, av);
                        else { big |= qc_ref_pair_big(av, g) ? 1 : 0; notlast |= qc_ref_pair_notlast(av, g) ? 1 : 0; }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 32); who = max(who, __shfl_xor(who, o, 32)); }
    if (l == 0 && iok) {
        partner[i] = qc_ref_partner(cnt, who);
        if (cnt > 1) sh_multi = 1;
        if (cnt == 1) atomicAdd(&sh_nstrong, 1);
    }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_down(off, o, 64); rsum += __shfl_down(rsum, o, 64); cmax = fmax(cmax, __shfl_down(cmax, o, 64)); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = off; red[1][tid >> 6] = rsum; red[2][tid >> 6] = cmax; }
    if (big) sh_big = 1;
    if (notlast) sh_notlast = 1;
    __syncthreads();
    if (tid == 0) {
        double *p = part + 8 * blockIdx.x;
        p[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        p[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        p[2] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
        p[3] = sh_nstrong; p[4] = sh_multi; p[5] = sh_big; p[6] = sh_notlast; p[7] = scale;
    }
}
__global__ __launch_bounds__(256) void qc_refine_statsB_kernel(int n, const double *__restrict__ S, const double *__restrict__ XtX,
                                                                const double *__restrict__ lam, double *__restrict__ stats,
                                                                const int *__restrict__ partner, const double *__restrict__ part, int nwg,
                                                                int *__restrict__ ctl, double *__restrict__ M) {
    if (ctl[QC_EIG_STATE] != QC_EIG_RUNNING) return;
    extern __shared__ double shb[];                          // lam[n], then partner[n] as ints
    double *sh_lam = shb;
    int *sh_partner = reinterpret_cast<int *>(shb + n);
    __shared__ int sh_go, sh_multi;
    __shared__ double sh_scale;
    const int tid = threadIdx.x, r = tid >> 5, l = tid & 31;
    for (int t = tid; t < n; t += 256) { sh_lam[t] = lam[t]; sh_partner[t] = partner[t]; }
    if (tid == 0) sh_multi = 0;
    __syncthreads();
    for (int t = tid; t < n; t += 256) if (qc_ref_not_mutual(sh_partner, t)) sh_multi = 1;
    __syncthreads();
    if (tid == 0) {
        double off = 0.0, rs = 0.0, cm = 0.0, nstrong = 0.0;
        int multi = sh_multi, big = 0, notlast = 0;
        for (int w = 0; w < nwg; ++w) {
            const double *p = part + 8 * w;
            off += p[0]; rs += p[1]; cm = fmax(cm, p[2]); nstrong += p[3];
            multi |= p[4] != 0.0; big |= p[5] != 0.0; notlast |= p[6] != 0.0;
        }
        const double scale = part[7], orth = sqrt(rs), scl = fmax(scale, QC_REF_SCALE_FLOOR);
        sh_scale = scale;
        int c0 = 0, c1 = 0, c2 = 0;
        if (QC_REF_ROTATE(big, orth, multi)) c0 = QC_EIG_ROTATE;
        else { c1 = QC_REF_IS_LAST(notlast, orth, nstrong != 0.0) ? 1 : 0; c2 = QC_REF_IS_CLEAN(cm, scl) ? 1 : 0; }
        sh_go = c0 == 0;
        if (blockIdx.x == 0) {
            stats[0] = sqrt(off); stats[1] = orth; stats[2] = scale; stats[3] = 0.5 * nstrong; stats[4] = cm;
            stats[5] = big ? 1.0 : (notlast ? 1e-6 : 0.0); stats[6] = multi;
            if (c0) ctl[QC_EIG_STATE] = c0; else { ctl[QC_EIG_LAST] = c1; ctl[QC_EIG_CLEAN] = c2; }
        }
    }
    __syncthreads();
    if (!sh_go) return;
    const double scale = sh_scale, tiny = QC_REF_TINY * scale, gfloor = QC_REF_GFLOOR * scale;
    const int i = blockIdx.x * QC_STATS_ROWS + r;
    if (i >= n) return;
    const double li = sh_lam[i];
    const int pi_ = sh_partner[i];
    for (int j0 = l; j0 < n; j0 += 128) {
        double sij[4], sji[4], xij[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 32 * u;
            const bool ok = j < n;
            sij[u] = S[ok ? (size_t)i * n + j : 0]; sji[u] = S[ok ? (size_t)j * n + i : 0]; xij[u] = XtX[ok ? (size_t)i * n + j : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 32 * u;
            if (j < n) {
                const double lj = sh_lam[j];
                const double rv = (i == j ? 1.0 : 0.0) - xij[u];
                const double sy = 0.5 * (sij[u] + sji[u]);
                const double av = QC_REF_COUPLING(sy, li, lj, rv), g = lj - li;
                double mm;
                if (i == j) {
                    mm = qc_ref_m_diag(rv);
                    if (pi_ >= 0) {                              // cosine of this index's rotation
                        const double avp = QC_REF_COUPLING(0.5 * (S[(size_t)i * n + pi_] + S[(size_t)pi_ * n + i]), li, sh_lam[pi_], -XtX[(size_t)i * n + pi_]);
                        mm = qc_ref_m_diag_rot(rv, avp, sh_lam[pi_] - li);
                    }
                } else if (pi_ == j) mm = qc_ref_m_rot(av, g);
                else mm = QC_REF_M_WEAK(sy, rv, lj, av, g, tiny, gfloor);
                M[(size_t)i * n + j] = mm;
            }
        }
    }
}
// doubles of the scratch behind lam / stats / partner that the two kernels need
size_t qc_refine_part_doubles(int n) { return 8 * (size_t)((n + QC_STATS_ROWS - 1) / QC_STATS_ROWS); }

// element x of M = I + E, with exact rotations on the strong pairs
__device__ __forceinline__ double qc_refine_m(int n, int x, const double *__restrict__ S, const double *__restrict__ XtX,
                                              const double *__restrict__ lam, double tiny, double gfloor, const int *__restrict__ partner) {
    const int i = x / n, j = x - i * n;
    const double r = (i == j ? 1.0 : 0.0) - XtX[x];
    if (i == j) {
        const int pj = partner[i];
        if (pj < 0) return qc_ref_m_diag(r);
        const double a = QC_REF_COUPLING(0.5 * (S[(size_t)i * n + pj] + S[(size_t)pj * n + i]), lam[i], lam[pj], -XtX[(size_t)i * n + pj]);
        return qc_ref_m_diag_rot(r, a, lam[pj] - lam[i]);      // cosine of this index's rotation
    }
    const double sij = 0.5 * (S[x] + S[(size_t)j * n + i]), a = QC_REF_COUPLING(sij, lam[i], lam[j], r), g = lam[j] - lam[i];
    return partner[i] == j ? qc_ref_m_rot(a, g) : QC_REF_M_WEAK(sij, r, lam[j], a, g, tiny, gfloor);
}

__global__ void qc_refine_update_kernel(int n, const double *__restrict__ S, const double *__restrict__ XtX, const double *__restrict__ lam,
                                        const double *__restrict__ stats, const int *__restrict__ partner, double *__restrict__ M) {
    const double scale = stats[2], tiny = QC_REF_TINY * scale, gfloor = QC_REF_GFLOOR * scale;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n * n; x += gridDim.x * blockDim.x) M[x] = qc_refine_m(n, x, S, XtX, lam, tiny, gfloor, partner);
}

// ascending eigenvalues + columns permuted alongside (utils.rs:28)
__global__ __launch_bounds__(1024) void qc_sort_columns_kernel(int n, const double *__restrict__ lam, const double *__restrict__ X,
                                                                double *__restrict__ w, double *__restrict__ Xs) {
    extern __shared__ int rank_s[];
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 1024) {
        const double wi = lam[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += QC_REF_BEFORE(lam, j, wi, i) ? 1 : 0;
        rank_s[i] = r;
        w[r] = wi;
    }
    __syncthreads();
    for (int x = tid; x < n * n; x += 1024) {
        const int i = x / n, j = x - i * n;
        Xs[(size_t)i * n + rank_s[j]] = X[x];
    }
}

// Eigen-decomposition of dA starting from the eigenvectors dV0 of a nearby matrix.
//   pass: S = X^T A X, X^T X, stats -> host (one small sync).
//     * update size max|E| > QC_REF_BIG (not perturbative), orthogonality lost, or passes exhausted -> Jacobi kernel on S
//       (nearly diagonal => few sweeps), V = X Q;
//     * max|E| <= QC_REF_LAST: one more update leaves ~1e-14 (quadratic) - unless a cluster still carries coupling, which only
//       rotations can remove -> Jacobi on S;
//     * otherwise apply X <- X (I + E) and take another pass.
int qc_eig_device_refine(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *notconv) {
    const size_t nn = (size_t)n * n;
    double *const d_work = E.work.p, *const t1 = E.t1.p, *const t2 = E.t2.p, *const t3 = E.t3.p, *const t4 = E.t4.p, *const small = E.small.p;
    double *lam = small, *stats = small + n;
    double *X = t4;                                            // current eigenvector estimate
    if (hipMemcpyAsync(X, dV0, nn * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return QC_ERR_HIP;
    double hs[8];
    int *partner = reinterpret_cast<int *>(small + n + 8);
    if (const char *dump = getenv("QC_EIG_DUMP")) {           // debugging aid: append (n, A, V0) of every call to a file
        static int ncall = 0;
        std::vector<double> h(2 * nn);
        (void)hipMemcpy(h.data(), dA, nn * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipMemcpy(h.data() + nn, dV0, nn * sizeof(double), hipMemcpyDeviceToHost);
        if (FILE *f = fopen(dump, ncall++ ? "ab" : "wb")) { double dn = n; fwrite(&dn, 8, 1, f); fwrite(h.data(), 8, 2 * nn, f); fclose(f); }
    }
    constexpr int MAXPASS = 5;
    static const bool dbg = getenv("QC_EIG_DEBUG") != nullptr;
    for (int pass = 0; pass < MAXPASS; ++pass) {
        qc_gemm(st, n, n, n, 1.0, dA, n, false, X, n, false, 0.0, t1, n);          // A X
        qc_gemm(st, n, n, n, 1.0, X, n, true, t1, n, false, 0.0, t2, n);           // S = X^T A X
        qc_gemm(st, n, n, n, 1.0, X, n, true, X, n, false, 0.0, t3, n);            // X^T X
        hipLaunchKernelGGL(qc_refine_stats_kernel, dim3(1), dim3(1024), 0, st, n, t2, t3, lam, stats, partner);
        if (hipMemcpyAsync(hs, stats, 7 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) return QC_ERR_HIP;
        if (hipStreamSynchronize(st) != hipSuccess) return QC_ERR_HIP;
        const double scale = fmax(hs[2], QC_REF_SCALE_FLOOR), orth = hs[1], nstrong = hs[3], cmax = hs[4], emax = hs[5], multi = hs[6];
        if (dbg) fprintf(stderr, "[eig n=%d pass %d] off %.2e orth %.2e scale %.1f strong %.0f multi %.0f cmax %.2e emax %.2e\n", n, pass, hs[0], orth, scale, nstrong, multi, cmax, emax);
        if (QC_REF_ROTATE(!(emax <= QC_REF_BIG), orth, multi != 0.0) || pass == MAXPASS - 1) {
            // not perturbative (or not converging): rotations.  Always from the orthonormal start V0 (pass 0: t2 holds V0^T A V0 already).
            if (pass > 0) return qc_eig_device_warm(st, n, dA, dV0, dV, dw, E, notconv);
            int rc = qc_eig_device(st, n, t2, t1, dw, E, notconv);      // Q -> t1 (sorted), eigenvalues -> dw
            if (rc != QC_OK) return rc;
            qc_gemm(st, n, n, n, 1.0, dV0, n, false, t1, n, false, 0.0, dV, n);    // V = V0 Q
            return QC_OK;
        }
        const bool last = QC_REF_IS_LAST(!(emax <= QC_REF_LAST), orth, nstrong != 0.0);
        hipLaunchKernelGGL(qc_refine_update_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, n, t2, t3, lam, stats, partner, t1);
        qc_gemm(st, n, n, n, 1.0, X, n, false, t1, n, false, 0.0, d_work, n);      // X (I + E): error now ~ emax^2
        if (last && QC_REF_IS_CLEAN(cmax, scale)) {   // lam is second-order accurate already; d_work holds the final vectors
            hipLaunchKernelGGL(qc_sort_columns_kernel, dim3(1), dim3(1024), n * sizeof(int), st, n, lam, d_work, dw, dV);
            return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
        }
        if (hipMemcpyAsync(X, d_work, nn * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return QC_ERR_HIP;
        if (last) {
            // converged except for coupling left inside degenerate pairs, which only rotations remove:
            // X is orthonormal to ~1e-14 now, so Jacobi on X^T A X (a handful of non-trivial rotations) finishes the job
            return qc_eig_device_warm(st, n, dA, X, dV, dw, E, notconv);
        }
    }
    return QC_ERR_HIP;   // not reached
}

// Sync-free variant for the SCF loop: a fixed number of passes is enqueued, every kernel looks at the device-side control
// word ctl[QC_EIG_STATE] and returns at once when the refinement has ended.  The caller reads it together with the iteration's
// energy; on QC_EIG_ROTATE it repeats the eigensolve with rotations.
__global__ __launch_bounds__(1024) void qc_refine_finish_kernel(int n, const double *__restrict__ lam, const double *__restrict__ Xn,
                                                                 double *__restrict__ X, double *__restrict__ w, double *__restrict__ Xs,
                                                                 int *__restrict__ ctl, int final_pass) {
    if (ctl[QC_EIG_STATE] != QC_EIG_RUNNING) return;
    extern __shared__ int rank_s[];
    const int tid = threadIdx.x;
    const int last = ctl[QC_EIG_LAST], clean = ctl[QC_EIG_CLEAN];
    __syncthreads();
    if (tid == 0) ctl[QC_EIG_PASSES] += 1;                              // passes used (the host sizes the next step's pipeline with it)
    if (last && clean) {                                    // Xn holds the final vectors: ascending eigenvalues, columns alongside
        double *lam_s = reinterpret_cast<double *>(rank_s + ((n + 1) & ~1));      // (the n quotients once, not n times per thread, from L2)
        for (int i = tid; i < n; i += 1024) lam_s[i] = lam[i];
        __syncthreads();
        for (int i = tid; i < n; i += 1024) {
            const double wi = lam_s[i];
            int r = 0;
            for (int j = 0; j < n; ++j) r += QC_REF_BEFORE(lam_s, j, wi, i) ? 1 : 0;
            rank_s[i] = r;
            w[r] = wi;
        }
        __syncthreads();
        // thread (row group, column): eight elements requested at a time, no index division
        const int c = tid & 127, rg = tid >> 7;
        for (int c0 = 0; c0 < n; c0 += 128) {
            const int j = c0 + c;
            const int rj = j < n ? rank_s[j] : 0;
            for (int i0 = rg; i0 < n; i0 += 64) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int i = i0 + 8 * u; v[u] = Xn[(j < n && i < n) ? (size_t)i * n + j : 0]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) { const int i = i0 + 8 * u; if (j < n && i < n) Xs[(size_t)i * n + rj] = v[u]; }
            }
        }
        __syncthreads();
        if (tid == 0) ctl[QC_EIG_STATE] = QC_EIG_DONE;
    } else if (last || final_pass) {
        __syncthreads();
        if (tid == 0) ctl[QC_EIG_STATE] = QC_EIG_ROTATE;                           // coupling inside a degenerate cluster, or passes exhausted
    }
    // (otherwise the next pass reads Xn in place: the passes alternate between two buffers, no copy)
}

int qc_eig_refine_async(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *ctl, int npass) {
    double *const d_work = E.work.p, *const t1 = E.t1.p, *const t2 = E.t2.p, *const t3 = E.t3.p, *const t4 = E.t4.p, *const small = E.small.p;
    double *lam = small, *stats = small + n;
    int *partner = reinterpret_cast<int *>(small + n + 8);
    // the four words of ctl must be zero on entry (the SCF step clears all control words with one memset)
    const double *X = dV0;                                    // pass 0 reads the start vectors in place
    for (int pass = 0; pass < npass; ++pass) {
        qc_gemm_pair(st, n, dA, false, X, t1, X, true, X, t3, ctl);                     // A X  and  X^T X in one launch
        qc_gemm(st, n, n, n, 1.0, X, n, true, t1, n, false, 0.0, t2, n, ctl);           // S = X^T A X
        {   // statistics, decisions, M = I + E -> t1
            const int nwg = (n + QC_STATS_ROWS - 1) / QC_STATS_ROWS;
            double *part = small + 2 * n + 16;                // (behind lam[n], stats[8], partner[n]: qc_eig_small_doubles(n))
            hipLaunchKernelGGL(qc_refine_statsA_kernel, dim3(nwg), dim3(256), n * sizeof(double), st, n, t2, t3, lam, partner, part, ctl);
            hipLaunchKernelGGL(qc_refine_statsB_kernel, dim3(nwg), dim3(256), n * sizeof(double) + n * sizeof(int) + 8, st, n, t2, t3, lam, stats, partner,
                               part, nwg, ctl, t1);
        }
        double *Xn = (pass & 1) ? t4 : d_work;                // (passes alternate between d_work and t4; pass 0 reads the start vectors in place)
        qc_gemm(st, n, n, n, 1.0, X, n, false, t1, n, false, 0.0, Xn, n, ctl);          // X (I + E)
        hipLaunchKernelGGL(qc_refine_finish_kernel, dim3(1), dim3(1024), ((n + 1) & ~1) * sizeof(int) + n * sizeof(double), st, n, lam, Xn, (double *)nullptr, dw, dV, ctl, pass == npass - 1 ? 1 : 0);
        X = Xn;
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

int qc_eig_cold_async(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *ctl, int npass) {
    int rc = qc_eig_tridiag_start(st, n, dA, E);
    if (rc != QC_OK) return rc;
    return qc_eig_refine_async(st, n, dA, E.x0.p, dV, dw, E, ctl, npass);
}

int qc_eig_cold_sync(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *ctl, int *notconv) {
    if (!qc_tri_ok(n) || qc_eig_force_jacobi()) return qc_eig_device(st, n, dA, dV, dw, E, notconv);
    if (hipMemsetAsync(ctl, 0, QC_CTL_EIG_STRIDE * sizeof(int), st) != hipSuccess) return QC_ERR_HIP;
    int rc = qc_eig_cold_async(st, n, dA, dV, dw, E, ctl, 4);
    if (rc != QC_OK) return rc;
    int h[QC_CTL_EIG_STRIDE] = {0, 0, 0, 0};
    if (hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return QC_ERR_HIP;
    static const bool dbg = getenv("QC_EIG_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[eig cold n=%d] ctl %d %d %d passes %d\n", n, h[QC_EIG_STATE], h[QC_EIG_LAST], h[QC_EIG_CLEAN], h[QC_EIG_PASSES]);
    if (h[QC_EIG_STATE] == QC_EIG_DONE) return QC_OK;
    if (hipMemsetAsync(ctl, 0, QC_CTL_EIG_STRIDE * sizeof(int), st) != hipSuccess) return QC_ERR_HIP;
    return qc_eig_device(st, n, dA, dV, dw, E, notconv);      // rotations: the start was not good enough
}
