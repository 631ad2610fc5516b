// qc_linalg.hip - dense f64 linear algebra of the SCF iteration on gfx950: MFMA GEMM, the DIIS solve, element-wise, tensor and
// reduction kernels.  All matrices row-major, device pointers, on the caller's stream.  (The eigensolvers: qc_eig_*.hip.)
//
// Replaces the nalgebra operations in the reference's loop body: the `*` products at rhf.rs:71,74,76,85, the Frobenius dots of
// diis.rs:43-45 and the trace / diagonal-rms at rhf.rs:84-88.
#include <algorithm>

#include "qc_internal.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------
// C = alpha * op(A) * op(B) + beta * C with v_mfma_f64_16x16x4_f64.  One wave per 16x16 tile of C.
// Operand lane maps (cdna_hip_programming.md section 3): lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; result register r holds C[row = (l >> 4) + 4 r][col = l & 15].
struct QcGemmArgs { int m, n, k; double alpha; const double *A; int lda, ta; const double *B; int ldb, tb; double beta; double *C; int ldc; };

__device__ __forceinline__ void qc_gemm_tile(const QcGemmArgs &g) {
    const int m = g.m, n = g.n, k = g.k;
    const double *__restrict__ A = g.A, *__restrict__ B = g.B;
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int row0 = blockIdx.y * 16, col0 = blockIdx.x * 16;
    const int ai = row0 + li, bj = col0 + li;
    const bool aok = ai < m, bok = bj < n;
    const size_t a_i = g.ta ? (size_t)ai : (size_t)ai * g.lda, a_k = g.ta ? (size_t)g.lda : 1;
    const size_t b_j = g.tb ? (size_t)bj * g.ldb : (size_t)bj, b_k = g.tb ? 1 : (size_t)g.ldb;
    // The operands of 64 k-values (4 x 4 MFMA steps) are requested before the first MFMA of the chunk: a tile is a chain of L2
    // round trips otherwise, one per 16 k-values.
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < k; k0 += 64) {
        double av[16], bv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int kk = k0 + 4 * s + lk;
            av[s] = (aok && kk < k) ? A[a_i + kk * a_k] : 0.0;
            bv[s] = (bok && kk < k) ? B[b_j + kk * b_k] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (k0 + 4 * s < k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);     // (uniform)
    }
    if (bok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + lk + 4 * r;
            if (row < m) {
                double *c = &g.C[(size_t)row * g.ldc + bj];
                *c = (g.beta == 0.0) ? g.alpha * acc[r] : fma(g.alpha, acc[r], g.beta * *c);
            }
        }
    }
}

__global__ __launch_bounds__(64) void qc_gemm_kernel(const QcGemmArgs g, const int *__restrict__ skip) {
    if (skip && *skip != 0) return;                        // device-side control flow of the sync-free SCF step
    qc_gemm_tile(g);
}

// two independent products of the same shape in one launch (blockIdx.z picks the problem)
__global__ __launch_bounds__(64) void qc_gemm2_kernel(const QcGemmArgs g0, const QcGemmArgs g1, const int *__restrict__ skip) {
    if (skip && *skip != 0) return;
    qc_gemm_tile(blockIdx.z ? g1 : g0);
}

void qc_gemm(hipStream_t st, int m, int n, int k, double alpha, const double *A, int lda, bool ta, const double *B, int ldb, bool tb,
             double beta, double *C, int ldc, const int *skip) {
    dim3 grid((n + 15) / 16, (m + 15) / 16);
    const QcGemmArgs g{m, n, k, alpha, A, lda, ta ? 1 : 0, B, ldb, tb ? 1 : 0, beta, C, ldc};
    hipLaunchKernelGGL(qc_gemm_kernel, grid, dim3(64), 0, st, g, skip);
}

// C0 = op(A0) op(B0), C1 = op(A1) op(B1), all n x n
void qc_gemm_pair(hipStream_t st, int n, const double *A0, bool ta0, const double *B0, double *C0, const double *A1, bool ta1,
                  const double *B1, double *C1, const int *skip) {
    dim3 grid((n + 15) / 16, (n + 15) / 16, 2);
    const QcGemmArgs g0{n, n, n, 1.0, A0, n, ta0 ? 1 : 0, B0, n, 0, 0.0, C0, n}, g1{n, n, n, 1.0, A1, n, ta1 ? 1 : 0, B1, n, 0, 0.0, C1, n};
    hipLaunchKernelGGL(qc_gemm2_kernel, grid, dim3(64), 0, st, g0, g1, skip);
}

// ---------------------------------------------------------------------------------------------------------------
// DIIS coefficients on the device (diis.rs:40-51): B is kept slot-indexed in HBM, the new row <e_0, e_j> arrives in
// `dots` (window order, newest first); Householder QR with the arithmetic of nalgebra's qr().solve(); one thread.
struct QcDiisArgs { int m, minlen, maxlen; int slot[12]; };
// the (m+1) x (m+1) system entirely in registers: every loop bound is a compile-time constant
template <int M>
__device__ __forceinline__ bool qc_qr_solve_reg(double (&A)[M * M], double (&y)[M], double (&x)[M]) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
        double norm = 0.0;
#pragma unroll
        for (int i = k; i < M; ++i) norm += A[i * M + k] * A[i * M + k];
        norm = sqrt(norm);
        if (norm == 0.0) return false;
        const double alpha = A[k * M + k] > 0 ? -norm : norm;
        double v[M];
        double vn = 0.0;
#pragma unroll
        for (int i = k; i < M; ++i) { v[i] = A[i * M + k] - (i == k ? alpha : 0.0); vn += v[i] * v[i]; }
        if (vn > 0.0) {
#pragma unroll
            for (int j = k; j < M; ++j) {
                double d = 0.0;
#pragma unroll
                for (int i = k; i < M; ++i) d += v[i] * A[i * M + j];
                d *= 2.0 / vn;
#pragma unroll
                for (int i = k; i < M; ++i) A[i * M + j] -= d * v[i];
            }
            double d = 0.0;
#pragma unroll
            for (int i = k; i < M; ++i) d += v[i] * y[i];
            d *= 2.0 / vn;
#pragma unroll
            for (int i = k; i < M; ++i) y[i] -= d * v[i];
        }
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < M; ++j) s -= A[i * M + j] * x[j];
        if (A[i * M + i] == 0.0) return false;
        x[i] = s / A[i * M + i];
    }
    return true;
}

template <int M>
__global__ void qc_diis_solve_kernel(QcDiisArgs a, const double *__restrict__ dots, double *B, double *__restrict__ c, int *__restrict__ flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    constexpr int m = M - 1;
    const int ML = a.maxlen;
#pragma unroll
    for (int j = 0; j < m; ++j) { const double d = dots[j]; B[a.slot[0] * ML + a.slot[j]] = d; B[a.slot[j] * ML + a.slot[0]] = d; }
    c[0] = 1.0;
#pragma unroll
    for (int j = 1; j < 12; ++j) c[j] = 0.0;
    if (m < a.minlen) return;                               // diis.rs:33-38: hand back the newest Fock matrix
    double A[M * M], y[M], x[M];
#pragma unroll
    for (int i = 0; i < m; ++i) {
#pragma unroll
        for (int j = 0; j < m; ++j) A[i * M + j] = B[a.slot[i] * ML + a.slot[j]];
        A[i * M + m] = 1.0; A[m * M + i] = 1.0; y[i] = 0.0;  // border +1, corner 0 (diis.rs:40-46)
    }
    A[m * M + m] = 0.0; y[m] = 1.0;
    if (!qc_qr_solve_reg<M>(A, y, x)) { *flag = 1; return; }   // "DIIS failed" (rhf.rs:73); c stays (1, 0, ...)
#pragma unroll
    for (int j = 0; j < m; ++j) c[j] = x[j];
}
void qc_diis_solve(hipStream_t st, int m, int minlen, int maxlen, const int *slots, const double *dots, double *B, double *c, int *flag) {
    QcDiisArgs a{};
    a.m = m; a.minlen = minlen; a.maxlen = maxlen;
    for (int j = 0; j < m; ++j) a.slot[j] = slots[j];
#define QC_DIIS_CASE(M) case M - 1: hipLaunchKernelGGL(qc_diis_solve_kernel<M>, dim3(1), dim3(64), 0, st, a, dots, B, c, flag); break;
    switch (m) { QC_DIIS_CASE(2) QC_DIIS_CASE(3) QC_DIIS_CASE(4) QC_DIIS_CASE(5) QC_DIIS_CASE(6) QC_DIIS_CASE(7) QC_DIIS_CASE(8) QC_DIIS_CASE(9)
                 QC_DIIS_CASE(10) QC_DIIS_CASE(11) QC_DIIS_CASE(12) default: break; }
#undef QC_DIIS_CASE
}

// ---------------------------------------------------------------------------------------------------------------
__global__ void qc_axpby_kernel(int nn, double a, const double *x, double b, const double *y, double *out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nn; i += gridDim.x * blockDim.x) out[i] = a * x[i] + (y ? b * y[i] : 0.0);
}
void qc_axpby(hipStream_t st, int n, double a, const double *x, double b, const double *y, double *out) {
    const int nn = n * n;
    hipLaunchKernelGGL(qc_axpby_kernel, dim3((nn + 255) / 256), dim3(256), 0, st, nn, a, x, b, y, out);
}

__global__ void qc_sub_transpose_kernel(int n, const double *M, double *out) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n * n; x += gridDim.x * blockDim.x) {
        const int i = x / n, j = x - i * n;
        out[x] = M[x] - M[j * n + i];
    }
}
void qc_sub_transpose(hipStream_t st, int n, const double *M, double *out) {
    hipLaunchKernelGGL(qc_sub_transpose_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, n, M, out);
}

// G = Gt + Gt^T: closes the unique-quartet digestion (fock_finalize)
// (with H and F given, F = H + G - the Fock matrix of rhf.rs:68 - leaves in the same launch)
// FX: Gt = [hi plane | lo plane] of 64-bit fixed-point integers, units fxs[1] = 2^-S and 2^-(S+32) (qc_fock_kernel.h): the two
// halves are added as integers, the planes meet in one fma when the sum becomes a double - G is symmetric bit for bit
template <bool FX>
__global__ void qc_symmetrize_add_kernel(int n, const double *Gt, size_t lo_off, double *G, const double *H, double *F, const double *fxs) {
    const double u1 = FX ? fxs[1] : 1.0, u2 = u1 * 0x1p-32;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n * n; x += gridDim.x * blockDim.x) {
        const int i = x / n, j = x - i * n;
        double g;
        if constexpr (FX) {
            const long long *Gh = reinterpret_cast<const long long *>(Gt), *Gl = Gh + lo_off;
            g = fma((double)(Gl[x] + Gl[j * n + i]), u2, (double)(Gh[x] + Gh[j * n + i]) * u1);
        } else g = Gt[x] + Gt[j * n + i];
        G[x] = g;
        if (F) F[x] = 1.0 * H[x] + 1.0 * g;              // the arithmetic of qc_axpby(1, H, 1, G)
    }
}
// Replica fold and G = Gt + Gt^T (and F = H + G) of a fixed-point build in ONE launch (single-rank builds: the folded planes are not
// needed for an all-reduce): thread (i <= j) sums the `nrep` replicas of the four integers hi[ij], hi[ji], lo[ij], lo[ji] - eight replicas
// requested at a time - and writes the pair; integer sums are exact, so the result is the one of qc_reduce_replicas + qc_symmetrize_add.
// The replicas it has read are zeroed on the way: the next build finds clean accumulator planes without a 1.7 MB memset of its own.
__global__ __launch_bounds__(64) void qc_fold_symmetrize_kernel(int n, int nrep, size_t rep_stride, long long *__restrict__ Gh, size_t lo_off,
                                                                double *__restrict__ G, const double *__restrict__ H, double *__restrict__ F,
                                                                const double *__restrict__ fxs, unsigned long long *tl) {
    if (tl != nullptr && threadIdx.x == 0 && blockIdx.x == 0) tl[0] = wall_clock64();
    struct Leave { unsigned long long *tl; __device__ ~Leave() { if (tl != nullptr && threadIdx.x == 0) tl[1 + (blockIdx.x & 31)] = wall_clock64(); } } leave{tl};
    // lane = (element of this workgroup's 16, quarter of the replicas): one batch of loads per lane, the quarters meet by shuffles
    const int e = threadIdx.x >> 2, part = threadIdx.x & 3;
    const int x = blockIdx.x * 16 + e;
    const bool in = x < n * n;
    const int i = in ? x / n : 0, j = in ? x - i * n : 0;
    const bool act = in && i <= j;
    const int xx = act ? x : 0, xt = act ? j * n + i : 0;
    long long *__restrict__ Gl = Gh + lo_off;
    const int per = (nrep + 3) / 4, r0 = part * per, r1 = min(nrep, r0 + per);
    long long h = 0, l = 0;
    for (int rb = r0; rb < r1; rb += 8) {
        long long a[8], b[8], c[8], d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t o = (size_t)min(rb + u, nrep - 1) * rep_stride;
            a[u] = Gh[o + xx]; b[u] = Gh[o + xt]; c[u] = Gl[o + xx]; d[u] = Gl[o + xt];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (act && rb + u < r1) {
                h += a[u] + (i == j ? 0 : b[u]); l += c[u] + (i == j ? 0 : d[u]);
                const size_t o = (size_t)(rb + u) * rep_stride;
                Gh[o + xx] = 0; Gh[o + xt] = 0; Gl[o + xx] = 0; Gl[o + xt] = 0;
            }
    }
    h += __shfl_xor(h, 1, 4); l += __shfl_xor(l, 1, 4);
    h += __shfl_xor(h, 2, 4); l += __shfl_xor(l, 2, 4);
    if (!act || part != 0) return;
    if (i == j) { h *= 2; l *= 2; }                       // (diagonal: Gt_ii + Gt_ii)
    const double u1 = fxs[1], u2 = u1 * 0x1p-32;
    const double g = fma((double)l, u2, (double)h * u1);
    G[x] = g; G[xt] = g;
    if (F) { F[x] = 1.0 * H[x] + 1.0 * g; F[xt] = 1.0 * H[xt] + 1.0 * g; }
}
void qc_fold_symmetrize(hipStream_t st, int n, int nrep, size_t rep_stride, double *Gt, size_t lo_off, double *G, const double *H, double *F,
                        const double *fxs, unsigned long long *tl) {
    hipLaunchKernelGGL(qc_fold_symmetrize_kernel, dim3((n * n + 15) / 16), dim3(64), 0, st, n, nrep, rep_stride,
                       reinterpret_cast<long long *>(Gt), lo_off, G, H, F, fxs, tl);
}
void qc_symmetrize_add(hipStream_t st, int n, const double *Gt, size_t lo_off, double *G, const double *H, double *F, const double *fxs) {
    if (fxs) hipLaunchKernelGGL(qc_symmetrize_add_kernel<true>, dim3((n * n + 255) / 256), dim3(256), 0, st, n, Gt, lo_off, G, H, F, fxs);
    else hipLaunchKernelGGL(qc_symmetrize_add_kernel<false>, dim3((n * n + 255) / 256), dim3(256), 0, st, n, Gt, lo_off, G, H, F, fxs);
}

// Fixed-point scale of one Fock build.  Every |(ij|kl)| <= imax (Schwarz) and every element of Gt is a sum of terms
// f (ij|kl) D_kl with |f| <= 2 in which each D_kl occurs at most once per kind (J, K), so |Gt_ij| <= 3 imax sum|D| and
// 2^S (4 imax sum|D|) <= 2^60 keeps every partial and final sum inside 62 bits - wrap-around cannot happen.  One workgroup,
// fixed reduction order: the same densities give the same scale on every rank.
__global__ __launch_bounds__(1024) void qc_fx_scale_kernel(int nn, const double *__restrict__ Da, const double *__restrict__ Db, double imax,
                                                           double *__restrict__ out) {
    __shared__ double sh[16];
    double s = 0.0;
    for (int x = threadIdx.x; x < nn; x += 1024) s += fabs(Da[x]) + (Db ? fabs(Db[x]) : 0.0);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += sh[k];
        const double bound = 4.0 * imax * t;
        int e = 0;
        if (bound > 0.0 && bound < 1e300) { (void)frexp(bound, &e); }      // bound < 2^e
        else if (!(bound < 1e300)) e = 1100;                              // inf / nan densities: coarsest scale
        int S = 60 - e;
        S = S > QC_FX_MAXBITS ? QC_FX_MAXBITS : (S < -900 ? -900 : S);
        // non-finite densities must stay visible: integers cannot carry a NaN, so the unit that turns the sums back into doubles
        // (qc_symmetrize_add_kernel) becomes NaN and every element of G with it - what f64 accumulation would have produced
        out[0] = ldexp(1.0, S); out[1] = (bound < 1e300) ? ldexp(1.0, -S) : __builtin_nan("");
    }
}
void qc_fx_scale(hipStream_t st, int n, const double *Da, const double *Db, double imax, double *out) {
    hipLaunchKernelGGL(qc_fx_scale_kernel, dim3(1), dim3(1024), 0, st, n * n, Da, Db, imax, out);
}

// flag[0] = number of positions where a and b differ bitwise (spin-symmetry test of the UHF build)
__global__ void qc_count_diff_kernel(size_t count, const double *a, const double *b, int *flag) {
    int d = 0;
    for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < count; x += (size_t)gridDim.x * blockDim.x)
        d += (__double_as_longlong(a[x]) != __double_as_longlong(b[x])) ? 1 : 0;
    if (d) atomicAdd(flag, d);
}
void qc_count_diff(hipStream_t st, size_t count, const double *a, const double *b, int *flag) {
    hipLaunchKernelGGL(qc_count_diff_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, count, a, b, flag);
}

// out[p][x] = sum_r Gt[p][r][x]: folds the accumulation replicas of the Fock build, plane by plane (f64: one plane; fixed
// point: hi and lo planes, `plane_stride` doubles apart, summed as integers); the sums of the planes land back to back in `out`
// (a small matrix gives only a dozen workgroups, so the kernel is as long as its chain of loads: eight replicas are requested
// at a time - four independent partial sums, combined in a fixed order)
template <typename T>
__global__ void qc_reduce_replicas_kernel(size_t count, int nrep, size_t stride, int nplanes, size_t plane_stride, const T *Gt, T *out) {
    for (size_t y = blockIdx.x * (size_t)blockDim.x + threadIdx.x; y < count * nplanes; y += (size_t)gridDim.x * blockDim.x) {
        const size_t p = y / count, x = y - p * count;
        const T *base = Gt + p * plane_stride + x;
        T s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int r = 0;
        for (; r + 8 <= nrep; r += 8) {
            const T *g = base + (size_t)r * stride;
            const T a0 = g[0], a1 = g[stride], a2 = g[2 * stride], a3 = g[3 * stride];
            const T a4 = g[4 * stride], a5 = g[5 * stride], a6 = g[6 * stride], a7 = g[7 * stride];
            s0 += a0; s1 += a1; s2 += a2; s3 += a3;
            s0 += a4; s1 += a5; s2 += a6; s3 += a7;
        }
        for (; r < nrep; ++r) s0 += base[(size_t)r * stride];
        out[y] = (s0 + s1) + (s2 + s3);
    }
}
void qc_reduce_replicas(hipStream_t st, size_t count, int nrep, size_t stride, const double *Gt, double *out, bool fx, size_t plane_stride) {
    const int nplanes = fx ? 2 : 1;
    const unsigned grid = (unsigned)((count * nplanes + 63) / 64);
    if (fx) hipLaunchKernelGGL(qc_reduce_replicas_kernel<long long>, dim3(grid), dim3(64), 0, st, count, nrep, stride, nplanes, plane_stride,
                               reinterpret_cast<const long long *>(Gt), reinterpret_cast<long long *>(out));
    else hipLaunchKernelGGL(qc_reduce_replicas_kernel<double>, dim3(grid), dim3(64), 0, st, count, nrep, stride, nplanes, plane_stride, Gt, out);
}


// ---------------------------------------------------------------------------------------------------------------
// Stored-tensor ("conventional") Fock build: the reference's own algorithm with the n^4 tensor resident in HBM
// (288 GB hold it up to n ~ 400).  K5a: T[i,j,k,l] = I[i,j,k,l] - c I[i,k,j,l] (rhf.rs:58-62 with c = 1/2; c = 1 gives
// the exchange-permuted copy the UHF contraction of uhf.rs:216-226 needs).  K5b: G[i,j] = sum_kl D[k,l] T[i,j,k,l] for
// i <= j, mirrored (rhf.rs:152-167) - a GEMV over n(n+1)/2 rows of n^2 doubles: pure HBM streaming, 4 n^4 bytes.
__global__ void qc_permute_tensor_kernel(int n, const double *__restrict__ I, double c_direct, double c_exch, double *__restrict__ T) {
    const size_t n1 = n, n2 = n1 * n1, n3 = n2 * n1, n4 = n3 * n1;
    for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < n4; x += (size_t)gridDim.x * blockDim.x) {
        const size_t i = x / n3, r = x - i * n3, j = r / n2, r2 = r - j * n2, k = r2 / n1, l = r2 - k * n1;
        T[x] = c_direct * I[x] + c_exch * I[i * n3 + k * n2 + j * n1 + l];
    }
}
void qc_permute_tensor(hipStream_t st, int n, const double *I, double c_direct, double c_exch, double *T) {
    const size_t n4 = (size_t)n * n * n * n;
    hipLaunchKernelGGL(qc_permute_tensor_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 1u << 20)), dim3(256), 0, st, n, I, c_direct, c_exch,
                       T);
}

// Persistent workgroups, each streaming a strided set of upper-triangle rows (i <= j) of the tensor(s) against the
// density held in LDS (n^2 doubles: 27 KB at n = 58, 104 KB at n = 114; larger n read D through L2 instead).
// G[i,j] = G[j,i] = <T1[i,j,:], D1> + <T2[i,j,:], D2>   (T2/D2 optional).  16-byte loads.
constexpr int QC_GEMV_THREADS = 512;
template <bool D_IN_LDS>
__global__ __launch_bounds__(QC_GEMV_THREADS) void qc_tensor_gemv_kernel(int n, const double *__restrict__ T1, const double *__restrict__ D1,
                                                                         const double *__restrict__ T2, const double *__restrict__ D2,
                                                                         double *__restrict__ G) {
    extern __shared__ double sd[];
    __shared__ double sh[QC_GEMV_THREADS / 64];
    const size_t nn = (size_t)n * n, nv = nn / 2;
    const int tid = threadIdx.x, nrows = n * (n + 1) / 2;
    const double2 *d1 = reinterpret_cast<const double2 *>(D1), *d2 = reinterpret_cast<const double2 *>(D2);
    if (D_IN_LDS) {
        for (size_t x = tid; x < nn; x += QC_GEMV_THREADS) { sd[x] = D1[x]; if (T2) sd[nn + (nn & 1) + x] = D2[x]; }
        __syncthreads();
        d1 = reinterpret_cast<const double2 *>(sd);
        d2 = reinterpret_cast<const double2 *>(sd + nn + (nn & 1));
    }
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        int i = (int)((2.0 * n + 1.0 - sqrt((2.0 * n + 1.0) * (2.0 * n + 1.0) - 8.0 * row)) * 0.5);
        while (i > 0 && (size_t)i * n - (size_t)i * (i - 1) / 2 > (size_t)row) --i;
        while ((size_t)(i + 1) * n - (size_t)(i + 1) * i / 2 <= (size_t)row) ++i;
        const int j = i + (row - (int)((size_t)i * n - (size_t)i * (i - 1) / 2));
        const size_t base = ((size_t)i * n + j) * nn;
        double acc = 0.0;
        {
            const double2 *t1 = reinterpret_cast<const double2 *>(T1 + base);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            size_t x = tid;
            for (; x + 3 * QC_GEMV_THREADS < nv; x += 4 * QC_GEMV_THREADS) {        // 4 independent 16-byte loads in flight per lane
                const double2 p0 = t1[x], p1 = t1[x + QC_GEMV_THREADS], p2 = t1[x + 2 * QC_GEMV_THREADS], p3 = t1[x + 3 * QC_GEMV_THREADS];
                const double2 q0 = d1[x], q1 = d1[x + QC_GEMV_THREADS], q2 = d1[x + 2 * QC_GEMV_THREADS], q3 = d1[x + 3 * QC_GEMV_THREADS];
                a0 = fma(p0.x, q0.x, fma(p0.y, q0.y, a0)); a1 = fma(p1.x, q1.x, fma(p1.y, q1.y, a1));
                a2 = fma(p2.x, q2.x, fma(p2.y, q2.y, a2)); a3 = fma(p3.x, q3.x, fma(p3.y, q3.y, a3));
            }
            for (; x < nv; x += QC_GEMV_THREADS) { const double2 a = t1[x], b = d1[x]; a0 = fma(a.x, b.x, fma(a.y, b.y, a0)); }
            acc = (a0 + a1) + (a2 + a3);
            if ((nn & 1) && tid == 0) acc = fma(T1[base + nn - 1], D1[nn - 1], acc);
        }
        if (T2) {
            const double2 *t2 = reinterpret_cast<const double2 *>(T2 + base);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            size_t x = tid;
            for (; x + 3 * QC_GEMV_THREADS < nv; x += 4 * QC_GEMV_THREADS) {
                const double2 p0 = t2[x], p1 = t2[x + QC_GEMV_THREADS], p2 = t2[x + 2 * QC_GEMV_THREADS], p3 = t2[x + 3 * QC_GEMV_THREADS];
                const double2 q0 = d2[x], q1 = d2[x + QC_GEMV_THREADS], q2 = d2[x + 2 * QC_GEMV_THREADS], q3 = d2[x + 3 * QC_GEMV_THREADS];
                a0 = fma(p0.x, q0.x, fma(p0.y, q0.y, a0)); a1 = fma(p1.x, q1.x, fma(p1.y, q1.y, a1));
                a2 = fma(p2.x, q2.x, fma(p2.y, q2.y, a2)); a3 = fma(p3.x, q3.x, fma(p3.y, q3.y, a3));
            }
            for (; x < nv; x += QC_GEMV_THREADS) { const double2 a = t2[x], b = d2[x]; a0 = fma(a.x, b.x, fma(a.y, b.y, a0)); }
            acc += (a0 + a1) + (a2 + a3);
            if ((nn & 1) && tid == 0) acc = fma(T2[base + nn - 1], D2[nn - 1], acc);
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((tid & 63) == 0) sh[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            double r = 0.0;
            for (int k = 0; k < QC_GEMV_THREADS / 64; ++k) r += sh[k];
            G[(size_t)i * n + j] = r; G[(size_t)j * n + i] = r;
        }
        __syncthreads();
    }
}
// Three forms: D in LDS within the default 48 KB (RHF n <= 78, UHF n <= 55), D in LDS above it after raising the kernel's limit
// (RHF n <= 138, UHF n <= 97), D read through L2.  Returns QC_ERR_HIP if the limit cannot be raised or the launch fails: G is
// then not written.
int qc_tensor_gemv(hipStream_t st, int n, const double *T1, const double *D1, const double *T2, const double *D2, double *G) {
    const size_t nn = (size_t)n * n, lds = (T2 ? 2 : 1) * (nn + 1) * sizeof(double);
    const int nrows = n * (n + 1) / 2;
    if (lds <= 150 * 1024) {
        static size_t allowed = 48 * 1024;
        if (lds > allowed) {
            QC_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(qc_tensor_gemv_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            allowed = lds;
        }
        const int per_cu = std::max<int>(1, std::min<int>(4, (int)(150 * 1024 / lds)));
        hipLaunchKernelGGL(qc_tensor_gemv_kernel<true>, dim3(std::min(nrows, 256 * per_cu)), dim3(QC_GEMV_THREADS), lds, st, n, T1, D1, T2, D2, G);
    } else {
        hipLaunchKernelGGL(qc_tensor_gemv_kernel<false>, dim3(std::min(nrows, 256 * 4)), dim3(QC_GEMV_THREADS), 0, st, n, T1, D1, T2, D2, G);
    }
    QC_HIP_CHECK(hipGetLastError());
    return QC_OK;
}

// out[j] = <x, ys[j]>, one workgroup per j (diis.rs:43-45)
struct QcPtrList { const double *p[16]; };
__global__ __launch_bounds__(1024) void qc_dots_kernel(int nn, const double *x, QcPtrList ys, double *out) {
    __shared__ double sh[16];
    const double *y = ys.p[blockIdx.x];
    double s = 0.0;
    for (int i0 = threadIdx.x; i0 < nn; i0 += 4 * 1024) {       // (four elements of each array requested before the first is used: 16 -> 6 us at n = 114)
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int i = min(i0 + u * 1024, nn - 1); a[u] = x[i]; b[u] = y[i]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i0 + u * 1024 < nn) s = fma(a[u], b[u], s);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; ++k) t += sh[k];
        out[blockIdx.x] = t;
    }
}
void qc_dots(hipStream_t st, int n, const double *x, const double *const *ys, int ny, double *out) {
    QcPtrList l;
    for (int j = 0; j < ny; ++j) l.p[j] = ys[j];
    hipLaunchKernelGGL(qc_dots_kernel, dim3(ny), dim3(1024), 0, st, n * n, x, l, out);
}

// out2[0] = 0.5 tr(Dnew (2H + G)),  out2[1] = sum_i (Dnew - Dold)_ii^2      (rhf.rs:84-88)
// `out2` may be pinned host memory (the SCF pass reads its scalars without a copy); with `ctl` the control words are
// copied next to them (ctl_out) and cleared for the next pass.
// (one workgroup: the kernel is as long as a thread's chain of loads, hence 1024 threads and a separate pass over the diagonal)
__global__ __launch_bounds__(1024) void qc_energy_rms_kernel(int n, const double *Dn, const double *Do, const double *H, const double *G,
                                                             double *out2, int *ctl, int *ctl_out) {
    __shared__ double sh[2][16];
    double e = 0.0, r = 0.0;
    // tr(Dn (2H + G)) = sum_x Dn[x] (2H + G)[x^T]; H and G are symmetric bit for bit (qc_one_electron.hip, qc_symmetrize_add_kernel), so the
    // transposed elements are the elements themselves and every read is coalesced; eight elements per thread are requested at a time
    // (as a chain of thirteen strided trips to L2 this kernel took 25 us at n = 114, now 11)
    const int nn = n * n;
    for (int x0 = threadIdx.x; x0 < nn; x0 += 8 * 1024) {
        double d[8], h[8], g[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int x = min(x0 + u * 1024, nn - 1); d[u] = Dn[x]; h[u] = H[x]; g[u] = G[x]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) if (x0 + u * 1024 < nn) e = fma(d[u], 2.0 * h[u] + g[u], e);
    }
    for (int i = threadIdx.x; i < n; i += 1024) { const double d = Dn[(size_t)i * n + i] - Do[(size_t)i * n + i]; r = fma(d, d, r); }
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_down(e, o, 64); r += __shfl_down(r, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = e; sh[1][threadIdx.x >> 6] = r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        e = 0.0; r = 0.0;
        for (int k = 0; k < 16; ++k) { e += sh[0][k]; r += sh[1][k]; }
        out2[0] = 0.5 * e; out2[1] = r;
    }
    if (ctl && threadIdx.x < QC_CTL_WORDS) { ctl_out[threadIdx.x] = ctl[threadIdx.x]; ctl[threadIdx.x] = 0; }
    __threadfence_system();
}
void qc_energy_rms(hipStream_t st, int n, const double *Dnew, const double *Dold, const double *H, const double *G, double *out2, int *ctl,
                   int *ctl_out) {
    hipLaunchKernelGGL(qc_energy_rms_kernel, dim3(1), dim3(1024), 0, st, n, Dnew, Dold, H, G, out2, ctl, ctl_out);
}

// w[nwords + i] = ~w[i]: the complements that let a max all-reduce over bit patterns reveal a rank whose words differ
__global__ void qc_sync_pack_kernel(unsigned long long *w, int nwords) {
    if ((int)threadIdx.x < nwords) w[nwords + threadIdx.x] = ~w[threadIdx.x];
}
void qc_sync_pack(hipStream_t st, unsigned long long *w, int nwords) { hipLaunchKernelGGL(qc_sync_pack_kernel, dim3(1), dim3(64), 0, st, w, nwords); }

// out = sum_i c[i] * Fs[i]   (diis.rs:52-58)
struct QcCoefList { double c[16]; };
__global__ void qc_lincomb_kernel(int nn, QcPtrList Fs, QcCoefList c, int m, double *out) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < nn; x += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(c.c[i], Fs.p[i][x], s);
        out[x] = s;
    }
}
__global__ void qc_lincomb_dev_kernel(int nn, QcPtrList Fs, const double *__restrict__ c, int m, double *out) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < nn; x += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(c[i], Fs.p[i][x], s);
        out[x] = s;
    }
}
void qc_lincomb_dev(hipStream_t st, int n, const double *const *Fs, const double *c_dev, int m, double *out) {
    QcPtrList l;
    for (int i = 0; i < m; ++i) l.p[i] = Fs[i];
    hipLaunchKernelGGL(qc_lincomb_dev_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, n * n, l, c_dev, m, out);
}
void qc_lincomb(hipStream_t st, int n, const double *const *Fs, const double *c, int m, double *out) {
    QcPtrList l; QcCoefList cl;
    for (int i = 0; i < m; ++i) { l.p[i] = Fs[i]; cl.c[i] = c[i]; }
    hipLaunchKernelGGL(qc_lincomb_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, n * n, l, cl, m, out);
}

// X = U diag(lam_ii^-1/2) U^T helper: out[i][k] = U[i][k] / sqrt(Lam[k][k])   (rhf.rs:128-130)
__global__ void qc_scale_cols_invsqrt_kernel(int n, const double *U, const double *Lam, double *out) {
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < n * n; x += gridDim.x * blockDim.x) {
        const int k = x % n;
        out[x] = U[x] / sqrt(Lam[k * n + k]);
    }
}
void qc_scale_cols_invsqrt(hipStream_t st, int n, const double *U, const double *Lam, double *out) {
    hipLaunchKernelGGL(qc_scale_cols_invsqrt_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, n, U, Lam, out);
}
