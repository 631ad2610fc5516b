// qc_chol.hip - dense symmetric positive-definite inverse on gfx950: what the continuum's K = -f S^-1 needs, and the
// library's only dense SPD solve.  Blocked right-looking Cholesky A = L L^T with QC_CHOL_NB = 64:
//   per block column k   L_kk, X_kk = L_kk^-1     one workgroup, the block and its inverse in LDS           (qc_chol_diag_kernel)
//                        L_ik = W_ik X_kk^T       the panel, one MFMA GEMM
//                        W_ij -= L_ik L_jk^T      the trailing square, one MFMA GEMM (alpha = -1, beta = 1)
//   then X = L^-1 by block forward substitution, block row i:  X_i,<i = -X_ii (L_i,<i X_<i,<i)        two GEMMs per block row
//   and  A^-1 = X^T X, one GEMM, mirrored from its lower triangle so that it is exactly symmetric.
// The inverse is formed because its user applies it once per SCF pass: with A^-1 that is one matrix-vector product, with the factor two
// triangular chains of n dependent steps each.  Every sum has a fixed order (no atomics; the flag word is a plain store of 1): a call is
// bit for bit repeatable.  A pivot that is <= 0 or not finite sets the flag and is replaced by 1, so no loop depends on a NaN.
#include <cmath>

#include "qc_solvent.h"

namespace {

constexpr int NB = QC_CHOL_NB;
constexpr int DIAG_THREADS = 256;

// Factor and invert the b x b diagonal block at (k0, k0) of W (b <= NB; rows / columns beyond b do not exist: the loops stop at b).
// Ld: the block, then its factor (lower triangle), rows LD = NB + 1 doubles apart so that a column read by consecutive lanes falls
// into distinct LDS banks; Li: its inverse, the lower triangle packed by rows (entry (k, c) at k (k + 1) / 2 + c).  50 KB of static
// LDS.  L_kk goes to L, X_kk to X, both with zeros above the diagonal.
constexpr int LD = NB + 1;
__device__ __forceinline__ int qc_tri(int k, int c) { return k * (k + 1) / 2 + c; }
__global__ __launch_bounds__(DIAG_THREADS) void qc_chol_diag_kernel(int n, int k0, const double *__restrict__ W, double *__restrict__ L,
                                                                     double *__restrict__ X, int *__restrict__ flag) {
    __shared__ double Ld[NB * LD], Li[NB * (NB + 1) / 2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = min(NB, n - k0);
    for (int e = t; e < NB * NB; e += DIAG_THREADS) {
        const int r = e / NB, c = e % NB;
        Ld[r * LD + c] = (r < b && c <= r) ? W[(size_t)(k0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < b; ++j) {
        double d = Ld[j * LD + j];
        const bool bad = !(d > 0.0) || !(d <= 1.79769313486231570815e308);     // <= 0, NaN or inf
        if (bad) d = 1.0;
        const double s = sqrt(d);
        __syncthreads();                                     // (every thread has read the pivot)
        if (t == 0) { Ld[j * LD + j] = s; if (bad) *flag = 1; }
        for (int r = j + 1 + t; r < b; r += DIAG_THREADS) Ld[r * LD + j] /= s;
        __syncthreads();
        // rank-1 update of the trailing triangle: a wave per row (rows in turn over the waves), a lane per column up to the diagonal
        const int c = j + 1 + lane;
        for (int r = j + 1 + wave; r < b; r += DIAG_THREADS / 64)
            if (c <= r) Ld[r * LD + c] -= Ld[r * LD + j] * Ld[c * LD + j];
        __syncthreads();
    }
    // X_kk: thread c owns column c, rows in turn (row i needs the rows before it of the same column only)
    if (t < b) {
        const int c = t;
        for (int i = c; i < b; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= Ld[i * LD + k] * Li[qc_tri(k, c)];
            Li[qc_tri(i, c)] = s / Ld[i * LD + i];
        }
    }
    __syncthreads();
    for (int e = t; e < NB * NB; e += DIAG_THREADS) {
        const int r = e / NB, c = e % NB;
        if (r >= b || c >= b) continue;
        const size_t g = (size_t)(k0 + r) * n + k0 + c;
        L[g] = c <= r ? Ld[r * LD + c] : 0.0;
        X[g] = c <= r ? Li[qc_tri(r, c)] : 0.0;
    }
}

// out[j][i] = out[i][j] for j > i: the mirror of the lower triangle
__global__ __launch_bounds__(256) void qc_chol_mirror_kernel(int n, double *__restrict__ A) {
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (r < n && c < r) A[(size_t)c * n + r] = A[(size_t)r * n + c];
}

}  // namespace

int qc_spd_inverse_device(qc_system *S, int n, const double *dA, double scale, double *dAinv) {
    if (n < 1) return QC_ERR_INVALID;
    hipStream_t st = S->stream;
    const size_t nn = (size_t)n * n;
    DevBuf W, L, X, T;
    QcDev<int> dflag;
    if (W.alloc(nn) != QC_OK || L.alloc(nn) != QC_OK || X.alloc(nn) != QC_OK || T.alloc((size_t)NB * n) != QC_OK || dflag.alloc(4) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(W.p, dA, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    QC_HIP_CHECK(hipMemsetAsync(L.p, 0, nn * sizeof(double), st));
    QC_HIP_CHECK(hipMemsetAsync(X.p, 0, nn * sizeof(double), st));
    QC_HIP_CHECK(hipMemsetAsync(dflag.p, 0, 4 * sizeof(int), st));
    for (int k0 = 0; k0 < n; k0 += NB) {
        const int b = std::min(NB, n - k0), k1 = k0 + b, rest = n - k1;
        hipLaunchKernelGGL(qc_chol_diag_kernel, dim3(1), dim3(DIAG_THREADS), 0, st, n, k0, W.p, L.p, X.p, dflag.p);
        if (rest <= 0) break;
        double *Lp = L.p + (size_t)k1 * n + k0;                             // the panel below the block
        qc_gemm(st, rest, b, b, 1.0, W.p + (size_t)k1 * n + k0, n, false, X.p + (size_t)k0 * n + k0, n, true, 0.0, Lp, n);    // W_ik X_kk^T
        qc_gemm(st, rest, rest, b, -1.0, Lp, n, false, Lp, n, true, 1.0, W.p + (size_t)k1 * n + k1, n);                      // W_ij -= L_ik L_jk^T
    }
    for (int i0 = NB; i0 < n; i0 += NB) {                                   // block rows of X below the first
        const int b = std::min(NB, n - i0);
        qc_gemm(st, b, i0, i0, 1.0, L.p + (size_t)i0 * n, n, false, X.p, n, false, 0.0, T.p, n);                             // L_i,<i X_<i,<i
        qc_gemm(st, b, i0, b, -1.0, X.p + (size_t)i0 * n + i0, n, false, T.p, n, false, 0.0, X.p + (size_t)i0 * n, n);       // -X_ii (.)
    }
    qc_gemm(st, n, n, n, scale, X.p, n, true, X.p, n, false, 0.0, dAinv, n);                                                 // scale X^T X
    hipLaunchKernelGGL(qc_chol_mirror_kernel, dim3((n + 15) / 16, (n + 15) / 16), dim3(256), 0, st, n, dAinv);
    int flag = 0;
    QC_HIP_CHECK(hipMemcpyAsync(&flag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return QC_ERR_HIP;
    return flag ? QC_ERR_INVALID : QC_OK;
}

extern "C" int qc_spd_inverse(qc_system *S, int n, const double *A, double *Ainv) {
    if (!S || !A || !Ainv || n < 1) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)n * n;
    DevBuf dA, dI;
    if (dA.alloc(nn) != QC_OK || dI.alloc(nn) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dA.p, A, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    rc = qc_spd_inverse_device(S, n, dA.p, 1.0, dI.p);
    if (rc != QC_OK && rc != QC_ERR_INVALID) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(Ainv, dI.p, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return rc;
}
