// qc_mp2.hip - conventional MP2 correlation energy on the GPU (RHF and UHF references).
//
// The AO tensor (mu nu|la si) is built in HBM by qc_launch_eri_full and transformed to the MO basis by four quarter
// transformations, each one f64 MFMA GEMM that contracts the slowest index of its operand:
//   1. (i nu|la si) = C_occ^T I          M = o,  N = n^3,  K = n
//   2. (i a|la si)                       batched over i:      M = v, N = n^2, K = n
//   3. (i a|j si)                        batched over (i,a):  M = o, N = n,   K = n
//   4. (i a|j b)                         one GEMM:            M = o v o, N = v, K = n   (contracts the last index of step 3's output)
// For UHF steps 1-2 run once per spin; the alpha-beta block applies the beta coefficients to the alpha half-transform.
// A pair kernel then sums e_ij over (a,b) for every occupied pair, and one workgroup adds the pair sums in a fixed order:
// no float atomics, so a call is bitwise reproducible.
#include <algorithm>
#include <cstdint>

#include "qc_internal.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

// ---- batched strided GEMM  C[b] = A[b] B[b]  with v_mfma_f64_16x16x4_f64
//   A[m,k] = A[b a_bs + m a_ms + k a_ks]   (any strides: C^T and plain row-major operands both occur)
//   B[k,j] = B[b b_bs + k ldb + j]         (row-major, unit column stride: streamed with 16-byte loads when aligned)
//   C[m,j] = C[b c_bs + m ldc + j]
// Workgroup tile 32 x 128 (four waves, each 32 x 32 = 2 x 2 MFMA tiles), k-chunks of 16 staged in LDS and prefetched into registers
// while the chunk before is multiplied.  M <= 32 (the o of step 1 and 3) is one M tile: every B element is read from memory once;
// M <= 16 skips the second row of MFMA tiles.  Operand lane maps (cdna_hip_programming.md, f64 16x16x4): lane l holds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register r holds C[row = (l >> 4) + 4 r][col = l & 15].
constexpr int BM = 32, BN = 128, BK = 16;
constexpr int PAD = 16;   // LDS rows of 48 / 144 doubles: the four k-rows one MFMA operand read touches fall on distinct bank halves

struct Mp2Gemm {
    int M, N, K, mtiles, ntiles;
    const double *A; int64_t a_ms, a_ks, a_bs;
    const double *B; int64_t ldb, b_bs;
    double *C; int64_t ldc, c_bs;
};

template <bool VEC>
__global__ __launch_bounds__(256) void qc_mp2_gemm_kernel(const Mp2Gemm g) {
    __shared__ double As[BK][BM + PAD];
    __shared__ double Bs[BK][BN + PAD];
    const int64_t tile = blockIdx.x;                   // M tile fastest: the tiles that share a B tile run side by side
    const int mt = (int)(tile % g.mtiles);
    const int64_t rest = tile / g.mtiles;
    const int nt = (int)(rest % g.ntiles);
    const int64_t b = rest / g.ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const double *__restrict__ A = g.A + b * g.a_bs;
    const double *__restrict__ B = g.B + b * g.b_bs;
    double *__restrict__ C = g.C + b * g.c_bs;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 15, lk = lane >> 4;

    // staging: A chunk 32 x 16 = 2 elements per thread (m fastest); B chunk 16 x 128 = 4 double2 (VEC) or 8 doubles per thread
    double ra[2];
    double rb[8];
    auto load = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int e = t + 256 * p, m = e & 31, k = e >> 5;
            ra[p] = (m0 + m < g.M && k0 + k < g.K) ? A[(int64_t)(m0 + m) * g.a_ms + (int64_t)(k0 + k) * g.a_ks] : 0.0;
        }
        if constexpr (VEC) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int e = t + 256 * p, k = e >> 6, j = n0 + 2 * (e & 63);
                const double *src = B + (int64_t)(k0 + k) * g.ldb + j;
                double2 v = {0.0, 0.0};
                if (k0 + k < g.K) {
                    if (j + 1 < g.N) v = *reinterpret_cast<const double2 *>(src);
                    else if (j < g.N) v.x = src[0];
                }
                rb[2 * p] = v.x; rb[2 * p + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int e = t + 256 * p, k = e >> 7, j = n0 + (e & 127);
                rb[p] = (k0 + k < g.K && j < g.N) ? B[(int64_t)(k0 + k) * g.ldb + j] : 0.0;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) { const int e = t + 256 * p; As[e >> 5][e & 31] = ra[p]; }
        if constexpr (VEC) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int e = t + 256 * p, k = e >> 6, j = 2 * (e & 63);
                Bs[k][j] = rb[2 * p]; Bs[k][j + 1] = rb[2 * p + 1];
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) { const int e = t + 256 * p; Bs[e >> 7][e & 127] = rb[p]; }
        }
    };

    const bool two_m = m0 + 16 < g.M;                  // (uniform)
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = double4_t{0.0, 0.0, 0.0, 0.0};
    load(0);
    for (int k0 = 0; k0 < g.K; k0 += BK) {
        __syncthreads();                               // the chunk before has been read
        store();
        __syncthreads();
        if (k0 + BK < g.K) load(k0 + BK);              // next chunk in flight during this one's MFMAs
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            const int kk = 4 * s + lk;
            const double a0 = As[kk][li], a1 = As[kk][16 + li];
            const double b0 = Bs[kk][32 * w + li], b1 = Bs[kk][32 * w + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            if (two_m) {
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int col = n0 + 32 * w + 16 * y + li;
            if (col >= g.N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + 16 * x + lk + 4 * r;
                if (row < g.M) C[(int64_t)row * g.ldc + col] = acc[x][y][r];
            }
        }
}

}  // namespace

void qc_mp2_gemm(hipStream_t st, int batch, int M, int N, int K, const double *A, int64_t a_ms, int64_t a_ks, int64_t a_bs,
              const double *B, int64_t ldb, int64_t b_bs, double *C, int64_t ldc, int64_t c_bs) {
    if (batch <= 0 || M <= 0 || N <= 0 || K <= 0) return;
    Mp2Gemm g{M, N, K, (M + BM - 1) / BM, (N + BN - 1) / BN, A, a_ms, a_ks, a_bs, B, ldb, b_bs, C, ldc, c_bs};
    const int64_t tiles = (int64_t)g.mtiles * g.ntiles * batch;
    const bool vec = (reinterpret_cast<uintptr_t>(B) % 16) == 0 && ldb % 2 == 0 && b_bs % 2 == 0;
    if (vec) hipLaunchKernelGGL(qc_mp2_gemm_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(qc_mp2_gemm_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, g);
}

// ---- the four quarter transformations: one index of the operand against `m` columns of C from column c0 (A[i,mu] = C[mu, c0 + i]: row stride 1, k stride n)
void qc_quarter_first(hipStream_t st, int n, const double *C, int c0, int m, const double *In, double *Out) {
    const int64_t n3 = (int64_t)n * n * n;
    qc_mp2_gemm(st, 1, m, (int)n3, n, C + c0, 1, n, 0, In, n3, 0, Out, n3, 0);
}
void qc_quarter_second(hipStream_t st, int n, int batch, const double *C, int c0, int m, const double *In, double *Out) {
    const int64_t nn = (int64_t)n * n;
    qc_mp2_gemm(st, batch, m, (int)nn, n, C + c0, 1, n, 0, In, nn, nn * n, Out, nn, (int64_t)m * nn);
}
void qc_quarter_third(hipStream_t st, int n, int batch, const double *C, int c0, int m, const double *In, double *Out) {
    qc_mp2_gemm(st, batch, m, n, n, C + c0, 1, n, 0, In, n, (int64_t)n * n, Out, n, (int64_t)m * n);
}
void qc_quarter_last(hipStream_t st, int n, int rows, const double *C, int c0, int m, const double *In, double *Out) { qc_mp2_gemm(st, 1, rows, m, n, In, n, 1, 0, C + c0, n, 0, Out, m, 0); }

namespace {

// ---- pair energies.  W[i,a,j,b] = (ia|jb) of one spin block, dims (o1, v1, o2, v2); one workgroup per pair (i,j).
//   mode 0 (RHF):        os = sum_ab W^2 / D,  ss = sum_ab W (W - Wx) / D
//   mode 1 (UHF ab):     os = sum_ab W^2 / D
//   mode 2 (UHF aa, bb): ss = 1/2 sum_ab W (W - Wx) / D
// with D = e_i + e_j - e_a - e_b and the exchange integral Wx = (ib|ja) = (ja|ib) = W[j,a,i,b].  Every lane sums a fixed
// subset in a fixed order, then a fixed LDS tree: the result does not depend on scheduling.
__global__ __launch_bounds__(256) void qc_mp2_pair_kernel(const double *__restrict__ W, int o1, int v1, int o2, int v2,
                                                          const double *__restrict__ eo1, const double *__restrict__ ev1,
                                                          const double *__restrict__ eo2, const double *__restrict__ ev2, int mode,
                                                          double *__restrict__ pos, double *__restrict__ pss) {
    __shared__ double r_os[256], r_ss[256];
    const int p = blockIdx.x, i = p / o2, j = p % o2, t = threadIdx.x;
    const int64_t astride = (int64_t)o2 * v2;
    const double *Wij = W + ((int64_t)i * v1 * o2 + j) * v2;
    const double *Wji = W + ((int64_t)j * v1 * o2 + i) * v2;     // (same-spin blocks only: o1 = o2, v1 = v2)
    const double eij = eo1[i] + eo2[j];
    double s_os = 0.0, s_ss = 0.0;
    for (int e = t; e < v1 * v2; e += 256) {
        const int a = e / v2, b = e - a * v2;
        const double x = Wij[a * astride + b];
        const double d = eij - ev1[a] - ev2[b];
        if (mode != 2) s_os += x * x / d;
        if (mode != 1) s_ss += x * (x - Wji[a * astride + b]) / d;
    }
    r_os[t] = s_os; r_ss[t] = s_ss;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { r_os[t] += r_os[t + h]; r_ss[t] += r_ss[t + h]; }
        __syncthreads();
    }
    if (t == 0) { pos[p] = r_os[0]; pss[p] = mode == 2 ? 0.5 * r_ss[0] : r_ss[0]; }
}

// out[0] = sum pos, out[1] = sum pss, in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void qc_mp2_sum_kernel(const double *__restrict__ pos, const double *__restrict__ pss, int np,
                                                         double *__restrict__ out) {
    __shared__ double r_os[256], r_ss[256];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int e = t; e < np; e += 256) { a += pos[e]; b += pss[e]; }
    r_os[t] = a; r_ss[t] = b;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { r_os[t] += r_os[t + h]; r_ss[t] += r_ss[t + h]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = r_os[0]; out[1] = r_ss[0]; }
}

}  // namespace

int qc_mp2_validate(int n, int nspin, const double *eps, const int32_t *nocc, int n_frozen) {
    if (n <= 0 || !eps || !nocc || (nspin != 1 && nspin != 2) || n_frozen < 0) return QC_ERR_INVALID;
    for (int s = 0; s < nspin; ++s) {
        if (nocc[s] < 0 || nocc[s] > n || n_frozen > nocc[s]) return QC_ERR_INVALID;
        const double *e = eps + (size_t)s * n;
        if (n_frozen == nocc[s] || nocc[s] == n) continue;          // no active occupied or no virtual orbital: an empty block
        double hi = e[n_frozen], lo = e[nocc[s]];
        for (int k = n_frozen; k < nocc[s]; ++k) hi = std::max(hi, e[k]);
        for (int k = nocc[s]; k < n; ++k) lo = std::min(lo, e[k]);
        if (!(hi < lo)) return QC_ERR_INVALID;                      // some denominator e_i + e_j - e_a - e_b >= 0 (or NaN)
    }
    return QC_OK;
}

// MP2 of validated orbitals resident in HBM (dC: nspin n x n blocks, dEps: nspin n-vectors) on the handle's stream.
int qc_mp2_device(qc_system *S, int nspin, const double *dC, const double *dEps, const int32_t *nocc, int n_frozen, qc_mp2_output *out) {
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const int n = S->nbasis;
    const int64_t nn = (int64_t)n * n, n3 = nn * n, n4 = nn * nn;
    int o[2] = {0, 0}, v[2] = {0, 0};
    for (int s = 0; s < nspin; ++s) { o[s] = nocc[s] - n_frozen; v[s] = n - nocc[s]; }
    // blocks (s1, s2, mode): RHF one; UHF alpha-alpha, beta-beta, alpha-beta.  Pair sums are laid out in this order.
    struct Blk { int s1, s2, mode; int64_t w_off, p_off; };
    std::vector<Blk> blks;
    if (nspin == 1) blks.push_back({0, 0, 0, 0, 0});
    else { blks.push_back({0, 0, 2, 0, 0}); blks.push_back({1, 1, 2, 0, 0}); blks.push_back({0, 1, 1, 0, 0}); }
    int64_t w_total = 0, p_total = 0, t3_max = 0, t1_max = 0, t2_total = 0;
    int64_t t2_off[2] = {0, 0};
    for (int s = 0; s < nspin; ++s) {
        if (o[s] > 0 && v[s] > 0) { t1_max = std::max(t1_max, o[s] * n3); t2_off[s] = t2_total; t2_total += (int64_t)o[s] * v[s] * nn; }
    }
    for (auto &b : blks) {
        b.w_off = w_total; b.p_off = p_total;
        if (o[b.s1] == 0 || v[b.s1] == 0 || o[b.s2] == 0 || v[b.s2] == 0) continue;
        w_total += (int64_t)o[b.s1] * v[b.s1] * o[b.s2] * v[b.s2];
        p_total += (int64_t)o[b.s1] * o[b.s2];
        t3_max = std::max(t3_max, (int64_t)o[b.s1] * v[b.s1] * o[b.s2] * n);
    }
    out->e_os = out->e_ss = out->e_corr = 0.0;
    out->ms_tensor = out->ms_transform = out->ms_energy = 0.0;
    out->n_frozen = n_frozen;
    if (p_total == 0) return QC_OK;                                   // every block is empty
    hipStream_t st = S->stream;
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double need = 8.0 * ((double)n4 + (double)t1_max + (double)t2_total + (double)t3_max + (double)w_total + 2.0 * p_total + 2);
    size_t free_b = 0, total_b = 0;
    QC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need * 1.05 > (double)free_b) return QC_ERR_UNSUPPORTED;

    // 1. the AO tensor
    const double t0 = qc_now_ms();
    DevBuf I, T1, T2, T3, W, P, R;
    if (I.alloc(n4) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(I.p, 0, n4 * sizeof(double), st));
    int rc = qc_launch_eri_full(S, I.p);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t1 = qc_now_ms();
    // 2. quarter transformations
    if (T1.alloc(t1_max) != QC_OK || T2.alloc(t2_total) != QC_OK || T3.alloc(t3_max) != QC_OK || W.alloc(w_total) != QC_OK ||
        P.alloc(2 * p_total) != QC_OK || R.alloc(2) != QC_OK) return QC_ERR_HIP;
    for (int s = 0; s < nspin; ++s) {
        if (o[s] == 0 || v[s] == 0) continue;
        const double *Cs = dC + s * nn;
        qc_quarter_first(st, n, Cs, n_frozen, o[s], I.p, T1.p);                               // (i nu|la si)
        qc_quarter_second(st, n, o[s], Cs, nocc[s], v[s], T1.p, T2.p + t2_off[s]);            // (i a|la si)
    }
    for (const auto &b : blks) {
        const int o1 = o[b.s1], v1 = v[b.s1], o2 = o[b.s2], v2 = v[b.s2];
        if (o1 == 0 || v1 == 0 || o2 == 0 || v2 == 0) continue;
        const double *C2 = dC + b.s2 * nn;
        qc_quarter_third(st, n, o1 * v1, C2, n_frozen, o2, T2.p + t2_off[b.s1], T3.p);        // (i a|j si), spin s2 on the third index
        qc_quarter_last(st, n, o1 * v1 * o2, C2, nocc[b.s2], v2, T3.p, W.p + b.w_off);        // (i a|j b)
    }
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t2 = qc_now_ms();
    // 3. pair energies, then their fixed-order sum
    for (const auto &b : blks) {
        const int o1 = o[b.s1], v1 = v[b.s1], o2 = o[b.s2], v2 = v[b.s2];
        if (o1 == 0 || v1 == 0 || o2 == 0 || v2 == 0) continue;
        const double *e1 = dEps + b.s1 * n, *e2 = dEps + b.s2 * n;
        hipLaunchKernelGGL(qc_mp2_pair_kernel, dim3(o1 * o2), dim3(256), 0, st, W.p + b.w_off, o1, v1, o2, v2, e1 + n_frozen, e1 + nocc[b.s1],
                           e2 + n_frozen, e2 + nocc[b.s2], b.mode, P.p + b.p_off, P.p + p_total + b.p_off);
    }
    hipLaunchKernelGGL(qc_mp2_sum_kernel, dim3(1), dim3(256), 0, st, P.p, P.p + p_total, (int)p_total, R.p);
    QC_HIP_CHECK(hipGetLastError());
    double e[2] = {0.0, 0.0};
    QC_HIP_CHECK(hipMemcpyAsync(e, R.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t3 = qc_now_ms();
    out->e_os = e[0]; out->e_ss = e[1]; out->e_corr = e[0] + e[1];
    out->ms_tensor = t1 - t0; out->ms_transform = t2 - t1; out->ms_energy = t3 - t2;
    return QC_OK;
}
