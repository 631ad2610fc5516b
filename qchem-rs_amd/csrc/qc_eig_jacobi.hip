// qc_eig_jacobi.hip - symmetric eigensolvers by Jacobi rotations in ONE workgroup (SymmetricEigen behind utils::sorted_eigs,
// hf/utils.rs:20-36): the two-sided kernel, the one-sided (Hestenes) kernels for matrices that do not fit in LDS, their drivers.
#include <cstdlib>

#include "qc_internal.h"
#include "qc_refine_rule.h"      // (the tangent of the 2x2 rotation, the order of the eigenvalues)

// ---------------------------------------------------------------------------------------------------------------
// Symmetric eigensolver: parallel cyclic two-sided Jacobi in ONE workgroup, matrix (and, when it fits, the
// eigenvector matrix) resident in LDS.  Round-robin ("chess tournament") ordering gives m/2 disjoint rotations per
// step and m-1 steps per sweep.  Each step is two phases separated by one barrier each:
//   A. m/2 threads compute the rotations (c_k, s_k) of the step's pairs (p_k, q_k);
//   B. the similarity transform J^T A J is applied as (m/2)^2 independent 2x2 blocks - block (k,l) = rows {p_k,q_k} x
//      columns {p_l,q_l} gets J_k^T . B . J_l - and V <- V J as n x m/2 independent row pairs.
// Output: eigenvalues ascending in w, eigenvectors as the columns of Vout (utils::sorted_eigs, hf/utils.rs:20-36).
constexpr int QC_EIG_THREADS = 1024;

__device__ __forceinline__ void qc_rr_pair(int step, int k, int m, int &p, int &q) {
    if (k == 0) { p = m - 1; q = step; return; }
    p = step + k; if (p >= m - 1) p -= m - 1;
    q = step - k; if (q < 0) q += m - 1;
}

template <bool V_IN_LDS>
__global__ __launch_bounds__(QC_EIG_THREADS) void qc_jacobi_kernel(int n, const double *__restrict__ Ain, double *__restrict__ Vg,
                                                                   double *__restrict__ Vout, double *__restrict__ w, int max_sweeps, double done_tol,
                                                                   int *__restrict__ notconv) {
    extern __shared__ double sm[];
    const int m = (n + 1) & ~1, half = m / 2, ld = m | 1;
    double *A = sm;                                         // m x ld (padding row/column stay zero => identity rotations)
    double *V = V_IN_LDS ? A + (size_t)m * ld : Vg;         // m x ldv
    const int ldv = V_IN_LDS ? ld : n;
    double *cs = A + (size_t)m * ld * (V_IN_LDS ? 2 : 1);   // 2 * half
    double *red = cs + 2 * half;                            // 32
    int *rank = (int *)(red + 32);                          // m
    const int tid = threadIdx.x, nt = blockDim.x;

    double fro = 0.0;
    for (int x = tid; x < m * m; x += nt) {
        const int i = x / m, j = x - i * m;
        const double v = (i < n && j < n) ? Ain[(size_t)i * n + j] : 0.0;
        A[i * ld + j] = v;
        fro = fma(v, v, fro);
        if (V_IN_LDS) V[i * ldv + j] = (i == j) ? 1.0 : 0.0;
        else if (i < n && j < n) V[(size_t)i * ldv + j] = (i == j) ? 1.0 : 0.0;
    }
    for (int o = 32; o > 0; o >>= 1) fro += __shfl_down(fro, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = fro;
    __syncthreads();
    double normF2 = 0.0;
    for (int k = 0; k < nt / 64; ++k) normF2 += red[k];
    __syncthreads();

    bool conv = false;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        double seen = 0.0;                                  // sum of a_pq^2 at the moment each pair is rotated
        for (int step = 0; step < m - 1; ++step) {
            if (tid < half) {                               // phase A
                int p, q;
                qc_rr_pair(step, tid, m, p, q);
                const double apq = A[p * ld + q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double t = qc_ref_tangent(apq, A[q * ld + q] - A[p * ld + p]);
                    c = 1.0 / sqrt(fma(t, t, 1.0));
                    s = t * c;
                    seen = fma(apq, apq, seen);
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            for (int b = tid; b < half * half; b += nt) {   // phase B: 2x2 blocks of J^T A J
                const int k = b / half, l = b - k * half;
                const double ck = cs[2 * k], sk = cs[2 * k + 1], cl = cs[2 * l], sl = cs[2 * l + 1];
                if (sk == 0.0 && sl == 0.0) continue;
                int pk, qk, pl, ql;
                qc_rr_pair(step, k, m, pk, qk);
                qc_rr_pair(step, l, m, pl, ql);
                const double b00 = A[pk * ld + pl], b01 = A[pk * ld + ql], b10 = A[qk * ld + pl], b11 = A[qk * ld + ql];
                const double r00 = ck * b00 - sk * b10, r01 = ck * b01 - sk * b11;      // J_k^T B
                const double r10 = sk * b00 + ck * b10, r11 = sk * b01 + ck * b11;
                A[pk * ld + pl] = cl * r00 - sl * r01; A[pk * ld + ql] = sl * r00 + cl * r01;   // (.) J_l
                A[qk * ld + pl] = cl * r10 - sl * r11; A[qk * ld + ql] = sl * r10 + cl * r11;
            }
            for (int x = tid; x < n * half; x += nt) {      // V <- V J
                const int i = x / half, l = x - i * half;
                const double cl = cs[2 * l], sl = cs[2 * l + 1];
                if (sl == 0.0) continue;
                int pl, ql;
                qc_rr_pair(step, l, m, pl, ql);
                const double vp = V[(size_t)i * ldv + pl], vq = V[(size_t)i * ldv + ql];
                V[(size_t)i * ldv + pl] = cl * vp - sl * vq;
                V[(size_t)i * ldv + ql] = sl * vp + cl * vq;
            }
            __syncthreads();
        }
        // off-diagonal mass met during this sweep; the sweep itself reduced it (quadratically, once small)
        for (int o = 32; o > 0; o >>= 1) seen += __shfl_down(seen, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = seen;
        __syncthreads();
        double off2 = 0.0;
        for (int k = 0; k < nt / 64; ++k) off2 += red[k];
        __syncthreads();
        // Jacobi converges quadratically: a sweep that met a relative off-norm <= done_tol (1e-9) leaves <= ~done_tol^2 behind - when
        // every rotation of it was a small one.  A pair inside a cluster of equal eigenvalues is turned by up to 45 degrees however small
        // its element, and such a turn moves what rows p and q still hold into positions the sweep has already visited: `seen` is what
        // the sweep removed, not what it left (multiplicity 2 at n = 58 left 4e-10, multiplicity 7 at n = 64 left 4e-10 of a scale of 10
        // to 30).  So the sweep that looks like the last one is believed only if what it left is small, element by element.
        if (2.0 * off2 <= done_tol * done_tol * normF2) {
            double left = 0.0;
            for (int x = tid; x < m * m; x += nt) {
                const int i = x / m, j = x - i * m;
                if (i != j) left = fmax(left, fabs(A[i * ld + j]));
            }
            for (int o = 32; o > 0; o >>= 1) left = fmax(left, __shfl_down(left, o, 64));
            if ((tid & 63) == 0) red[tid >> 6] = left;
            __syncthreads();
            left = 0.0;
            for (int k = 0; k < nt / 64; ++k) left = fmax(left, red[k]);
            __syncthreads();
            if (left * left <= QC_JACOBI_LEFT_TOL * QC_JACOBI_LEFT_TOL * normF2) { conv = true; break; }
        }
    }
    if (!conv && notconv && tid == 0) *notconv = 1;         // sweeps exhausted: the caller reports it instead of using the vectors
    // ascending order (utils.rs:28): rank sort, then permute columns
    for (int i = tid; i < n; i += nt) {
        const double wi = A[i * ld + i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const double wj = A[j * ld + j];
            r += (wj < wi || (wj == wi && j < i)) ? 1 : 0;
        }
        rank[i] = r;
        w[r] = wi;
    }
    __syncthreads();
    for (int x = tid; x < n * n; x += nt) {
        const int i = x / n, j = x - i * n;
        Vout[(size_t)i * n + rank[j]] = V[(size_t)i * ldv + j];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One-sided (Hestenes) Jacobi for matrices whose A and V do not both fit in LDS (100 < n <= 128; n = 100 needs 163 072 bytes for both).
// B = A + sigma I is made positive definite with a Gershgorin shift; the columns of G (initially B) are rotated
// pairwise to mutual orthogonality, G <- G J.  At convergence G = U Sigma: the normalised columns are the
// eigenvectors and ||g_i|| - sigma the eigenvalues, so only ONE n x n matrix has to live in LDS (column-major,
// 8 lanes per column pair, conflict-free reads).  One barrier per step.  The rotation parameters are computed by every
// lane of a team, so the kernel is bound by that scalar chain times the number of resident waves: narrow teams (fewer
// waves) and reciprocal-square-root forms (no IEEE divide / sqrt sequences) make the step 2.4x shorter than the
// 16-lane / divide version.
constexpr int QC_EIG1_TEAM = 8;
constexpr int QC_EIG1_ROWS = 128 / QC_EIG1_TEAM;       // rows per lane of the LDS variant (n <= 128)
constexpr int QC_EIG1_THREADS = 64 * QC_EIG1_TEAM;     // 64 teams: one per column pair

// 1 / x to a few ulp: hardware estimate + two Newton steps (the IEEE division sequence is twice as long, and every lane of a
// team runs this chain between the barriers of a step)
__device__ __forceinline__ double qc_fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}
// Jacobi rotation (c, s) that orthogonalises two columns with squared norms a, b and inner product g.  c^2 + s^2 = 1 holds to
// the accuracy of rsqrt whatever the error of t, so the reciprocal shortcuts cost nothing in orthonormality.
__device__ __forceinline__ void qc_hestenes_rotation(double a, double b, double g, double &cs, double &sn) {
    const double zeta = (b - a) * (0.5 * qc_fast_rcp(g));
    const double z2 = fma(zeta, zeta, 1.0);
    const double den = fabs(zeta) + z2 * rsqrt(z2);            // |zeta| + sqrt(zeta^2 + 1)
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) * qc_fast_rcp(den);
    cs = rsqrt(fma(t, t, 1.0));
    sn = cs * t;
}

// End of the one-sided kernels (G: n columns of stride ld): eigenvalues = column norms - sigma; rank sort; normalised, permuted columns out
__device__ __forceinline__ void qc_hestenes_finish(int n, const double *G, int ld, double sigma, double *nrm, int *rank, double *__restrict__ w,
                                                   double *__restrict__ Vout) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int j = tid; j < n; j += nt) {
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) s2 = fma(G[(size_t)j * ld + i], G[(size_t)j * ld + i], s2);
        nrm[j] = sqrt(s2);
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const double wi = nrm[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += QC_REF_BEFORE(nrm, j, wi, i) ? 1 : 0;
        rank[i] = r;
        w[r] = wi - sigma;
    }
    __syncthreads();
    for (int x = tid; x < n * n; x += nt) {
        const int i = x / n, j = x - i * n;
        Vout[(size_t)i * n + rank[j]] = G[(size_t)j * ld + i] / nrm[j];
    }
}

__global__ __launch_bounds__(QC_EIG1_THREADS) void qc_jacobi1_kernel(int n, const double *__restrict__ Ain, double *__restrict__ Vout,
                                                                    double *__restrict__ w, int max_sweeps, double done_tol, int *__restrict__ notconv) {
    extern __shared__ double sm[];
    const int m = (n + 1) & ~1, half = m / 2, ld = n | 1;        // column stride (doubles)
    double *G = sm;                                               // m columns x ld (padding column stays zero)
    double *red = G + (size_t)m * ld;                             // 32
    double *nrm = red + 32;                                       // m column norms
    int *rank = (int *)(nrm + m);                                 // m
    int *flag = rank + m;                                         // rotations done in this sweep
    const int tid = threadIdx.x, nt = blockDim.x;

    // Gershgorin lower bound of the spectrum -> shift
    double low = 1e300, spread = 0.0;
    for (int i = tid; i < n; i += nt) {
        double r = 0.0;
        for (int j = 0; j < n; ++j) if (j != i) r += fabs(Ain[(size_t)i * n + j]);
        low = fmin(low, Ain[(size_t)i * n + i] - r);
        spread = fmax(spread, Ain[(size_t)i * n + i] + r);
    }
    for (int o = 32; o > 0; o >>= 1) { low = fmin(low, __shfl_down(low, o, 64)); spread = fmax(spread, __shfl_down(spread, o, 64)); }
    if ((tid & 63) == 0) { red[tid >> 6] = low; red[16 + (tid >> 6)] = spread; }
    __syncthreads();
    low = red[0]; spread = red[16];
    for (int k = 1; k < nt / 64; ++k) { low = fmin(low, red[k]); spread = fmax(spread, red[16 + k]); }
    __syncthreads();
    const double sigma = fmax(0.0, -low) + 0.05 * (spread - low) + 1e-3;
    for (int x = tid; x < m * ld; x += nt) {
        const int j = x / ld, i = x - j * ld;                     // column j, row i
        G[x] = (i < n && j < n) ? Ain[(size_t)i * n + j] + (i == j ? sigma : 0.0) : 0.0;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();

    const int team = tid / QC_EIG1_TEAM, tl = tid % QC_EIG1_TEAM;
    bool conv = false;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        for (int step = 0; step < m - 1; ++step) {
            if (team < half) {
                int p, q;
                qc_rr_pair(step, team, m, p, q);
                double *gp = G + (size_t)p * ld, *gq = G + (size_t)q * ld;
                double a = 0.0, b = 0.0, c = 0.0, xp[QC_EIG1_ROWS], xq[QC_EIG1_ROWS];
#pragma unroll
                for (int k = 0; k < QC_EIG1_ROWS; ++k) {
                    const int r = tl + k * QC_EIG1_TEAM;
                    xp[k] = (r < n) ? gp[r] : 0.0; xq[k] = (r < n) ? gq[r] : 0.0;
                    a = fma(xp[k], xp[k], a); b = fma(xq[k], xq[k], b); c = fma(xp[k], xq[k], c);
                }
#pragma unroll
                for (int o = QC_EIG1_TEAM / 2; o > 0; o >>= 1) {
                    a += __shfl_xor(a, o, QC_EIG1_TEAM); b += __shfl_xor(b, o, QC_EIG1_TEAM); c += __shfl_xor(c, o, QC_EIG1_TEAM);
                }
                if (c * c > 1e-32 * (a * b)) {                     // team-uniform: |c| / sqrt(a b) > 1e-16
                    double cs, sn;
                    qc_hestenes_rotation(a, b, c, cs, sn);
#pragma unroll
                    for (int k = 0; k < QC_EIG1_ROWS; ++k) {
                        const int r = tl + k * QC_EIG1_TEAM;
                        if (r < n) { gp[r] = cs * xp[k] - sn * xq[k]; gq[r] = sn * xp[k] + cs * xq[k]; }
                    }
                    // pairs whose relative coupling |c| / sqrt(a b) is below done_tol are done after this rotation (QC_JACOBI_LEFT_TOL: a sweep
                    // may leave what it met - qc_internal.h - so what it met has to be as small as what may be left)
                    if (tl == 0 && c * c > done_tol * done_tol * (a * b)) *flag = 1;
                }
            }
            __syncthreads();
        }
        const int any = *flag;
        __syncthreads();
        if (tid == 0) *flag = 0;
        __syncthreads();
        if (!any) { conv = true; break; }
    }
    if (!conv && notconv && tid == 0) *notconv = 1;
    qc_hestenes_finish(n, G, ld, sigma, nrm, rank, w, Vout);
}

// ---------------------------------------------------------------------------------------------------------------
// One-sided Jacobi for n > 128: same algorithm as qc_jacobi1_kernel with G in global memory (d_work, n columns of
// stride n) and the pairs of a step spread over the 64 teams of one workgroup in a loop.  Slow (global read-modify-write
// behind a workgroup barrier per step) but only the cold start and the rare fallback of the refinement use it; the SCF
// loop's eigensolves are GEMMs (qc_eig_device_refine).  Keeps every shipped basis (benzene/6-311++G**: n = 180) usable.
__global__ __launch_bounds__(QC_EIG_THREADS) void qc_jacobi1g_kernel(int n, const double *__restrict__ Ain, double *__restrict__ G,
                                                                     double *__restrict__ Vout, double *__restrict__ w, int max_sweeps, double done_tol,
                                                                     int *__restrict__ notconv) {
    extern __shared__ double sm[];
    __shared__ double red[32];
    __shared__ int flag;
    double *nrm = sm;                                       // n column norms
    int *rank = reinterpret_cast<int *>(sm + n);            // n ranks
    const int m = (n + 1) & ~1, half = m / 2;
    const int tid = threadIdx.x, nt = blockDim.x;
    double low = 1e300, spread = 0.0;
    for (int i = tid; i < n; i += nt) {
        double r = 0.0;
        for (int j = 0; j < n; ++j) if (j != i) r += fabs(Ain[(size_t)i * n + j]);
        low = fmin(low, Ain[(size_t)i * n + i] - r);
        spread = fmax(spread, Ain[(size_t)i * n + i] + r);
    }
    for (int o = 32; o > 0; o >>= 1) { low = fmin(low, __shfl_down(low, o, 64)); spread = fmax(spread, __shfl_down(spread, o, 64)); }
    if ((tid & 63) == 0) { red[tid >> 6] = low; red[16 + (tid >> 6)] = spread; }
    __syncthreads();
    low = red[0]; spread = red[16];
    for (int k = 1; k < nt / 64; ++k) { low = fmin(low, red[k]); spread = fmax(spread, red[16 + k]); }
    __syncthreads();
    const double sigma = fmax(0.0, -low) + 0.05 * (spread - low) + 1e-3;
    for (int x = tid; x < n * n; x += nt) {               // column-major copy of the (symmetric) shifted matrix
        const int j = x / n, i = x - j * n;
        G[x] = 0.5 * (Ain[(size_t)i * n + j] + Ain[(size_t)j * n + i]) + (i == j ? sigma : 0.0);
    }
    if (tid == 0) flag = 0;
    __syncthreads();
    const int team = tid / QC_EIG1_TEAM, tl = tid % QC_EIG1_TEAM, nteams = nt / QC_EIG1_TEAM;
    bool conv = false;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        for (int step = 0; step < m - 1; ++step) {
            for (int pr = team; pr < half; pr += nteams) {
                int p, q;
                qc_rr_pair(step, pr, m, p, q);
                if (p >= n || q >= n) continue;           // padding index of an odd n
                double *gp = G + (size_t)p * n, *gq = G + (size_t)q * n;
                double a = 0.0, b = 0.0, c = 0.0;
                for (int r = tl; r < n; r += QC_EIG1_TEAM) { const double xp = gp[r], xq = gq[r]; a = fma(xp, xp, a); b = fma(xq, xq, b); c = fma(xp, xq, c); }
#pragma unroll
                for (int o = QC_EIG1_TEAM / 2; o > 0; o >>= 1) {
                    a += __shfl_xor(a, o, QC_EIG1_TEAM); b += __shfl_xor(b, o, QC_EIG1_TEAM); c += __shfl_xor(c, o, QC_EIG1_TEAM);
                }
                const double rel = fabs(c) / sqrt(a * b);
                if (rel > 1e-16) {
                    const double t = qc_ref_tangent(c, b - a);
                    const double cs = 1.0 / sqrt(fma(t, t, 1.0)), sn = cs * t;
                    for (int r = tl; r < n; r += QC_EIG1_TEAM) { const double xp = gp[r], xq = gq[r]; gp[r] = cs * xp - sn * xq; gq[r] = sn * xp + cs * xq; }
                    if (tl == 0 && rel > done_tol) flag = 1;
                }
            }
            __syncthreads();
        }
        const int any = flag;
        __syncthreads();
        if (tid == 0) flag = 0;
        __syncthreads();
        if (!any) { conv = true; break; }
    }
    if (!conv && notconv && tid == 0) *notconv = 1;
    qc_hestenes_finish(n, G, n, sigma, nrm, rank, w, Vout);
}

int QcEigWork::alloc(int n) {
    const size_t nn = (size_t)n * n;
    for (DevBuf *b : {&work, &t1, &t2, &t3, &t4, &x0}) if (b->alloc(nn) != QC_OK) return QC_ERR_HIP;
    if (tri.alloc(qc_eig_tridiag_work_doubles(n)) != QC_OK || small.alloc(qc_eig_small_doubles(n)) != QC_OK) return QC_ERR_HIP;
    return ctl.alloc(QC_CTL_EIG_STRIDE);
}

bool qc_eig_force_jacobi() { static const bool force = getenv("QC_EIG_JACOBI") != nullptr; return force; }

// dA: input (left intact), dV: sorted eigenvectors, dw: eigenvalues
int qc_eig_device(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *notconv) {
    double *const d_work = E.work.p;
    const int m = (n + 1) & ~1, ld = m | 1;
    const size_t tail = (2 * (m / 2) + 32) * sizeof(double) + (size_t)m * sizeof(int) + 16;
    const size_t lds2 = 2 * (size_t)m * ld * sizeof(double) + tail, lds1 = (size_t)m * ld * sizeof(double) + tail;
    const bool v_in_lds = lds2 <= QC_LDS_MAX;
    static const bool force1 = getenv("QC_EIG_ONESIDED") != nullptr;
    if ((!v_in_lds || force1) && n <= QC_EIG1_ROWS * QC_EIG1_TEAM) {   // 100 < n <= 128: one-sided variant, a single matrix in LDS
        const size_t l1 = ((size_t)m * (n | 1) + 32 + m) * sizeof(double) + (size_t)(m + 4) * sizeof(int) + 16;
        if (l1 <= QC_LDS_MAX) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(qc_jacobi1_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l1);
            if (e != hipSuccess) return QC_ERR_HIP;
            hipLaunchKernelGGL(qc_jacobi1_kernel, dim3(1), dim3(QC_EIG1_THREADS), l1, st, n, dA, dV, dw, QC_JACOBI_MAX_SWEEPS, QC_JACOBI_LEFT_TOL, notconv);
            return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
        }
    }
    const size_t lds = v_in_lds ? lds2 : lds1;
    if (lds > QC_LDS_MAX || !v_in_lds) {                // n > 128: the global-memory variant
        if (n > 3000) return QC_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(qc_jacobi1g_kernel, dim3(1), dim3(QC_EIG_THREADS), (size_t)n * 12 + 16, st, n, dA, d_work, dV, dw, QC_JACOBI_MAX_SWEEPS, QC_JACOBI_LEFT_TOL, notconv);
        return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
    }
    auto kern = v_in_lds ? qc_jacobi_kernel<true> : qc_jacobi_kernel<false>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return QC_ERR_HIP;
    }
    static const int nthreads = getenv("QC_EIG_THREADS") ? atoi(getenv("QC_EIG_THREADS")) : QC_EIG_THREADS;
    hipLaunchKernelGGL(kern, dim3(1), dim3(nthreads), lds, st, n, dA, d_work, dV, dw, QC_JACOBI_MAX_SWEEPS, QC_JACOBI_DONE_TOL, notconv);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// Warm-started variant for the SCF loop: with V0 the eigenvectors of the previous iteration's matrix,
// B = V0^T A V0 is nearly diagonal, Jacobi needs 1-3 sweeps instead of ~8, and V = V0 Q.  The three products are
// f64 MFMA GEMMs.
int qc_eig_device_warm(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *notconv) {
    double *const t1 = E.t1.p, *const t2 = E.t2.p;
    qc_gemm(st, n, n, n, 1.0, dA, n, false, dV0, n, false, 0.0, t1, n);        // A V0
    qc_gemm(st, n, n, n, 1.0, dV0, n, true, t1, n, false, 0.0, t2, n);         // V0^T (A V0)
    int rc = qc_eig_device(st, n, t2, t1, dw, E, notconv);   // Q -> t1
    if (rc != QC_OK) return rc;
    qc_gemm(st, n, n, n, 1.0, dV0, n, false, t1, n, false, 0.0, dV, n);        // V = V0 Q
    return QC_OK;
}
