// qc_excited.hip - CIS and TDHF excited states of an RHF state from explicit A + B and A - B matrices.
//
// With (pq|rs) in chemists' notation, i j occupied, a b virtual, Delta = delta_ij delta_ab (e_a - e_i), rows and columns laid out
// [i * v + a] as in qc_stability.hip:
//   singlets  A + B = Delta + 4 (ia|jb) - (ib|ja) - (ij|ab)        triplets  A + B = Delta - (ib|ja) - (ij|ab)
//   both      A - B = Delta + (ib|ja) - (ij|ab)                    A = 1/2 [(A + B) + (A - B)]
// The AO tensor is built in HBM (qc_launch_eri_full) and taken to W = (ia|jb) and V = (ij|ab) by the batched MFMA GEMM of the MP2 code
// (qc_mp2_gemm): the first quarter (i nu|la si) is shared, then one chain of three quarters each.  One kernel assembles both matrices
// of order d = o v, a workgroup per occupied pair i >= j and 32 x 32 tile of (a, b): it writes an element of block (i, j) and its
// mirror image in block (j, i) from the same value, so both matrices are exactly symmetric although the GEMM chain rounds
// W[i,a,j,b] and W[j,b,i,a] differently.  After that every product of the iterative solvers is one qc_gemm over all new trial vectors:
//   CIS   block Davidson on A (the loop of the stability analysis, qc_stab_davidson in qc_subspace.h)
//   TDHF  the reduced-space algorithm of Stratmann, Scuseria and Frisch, J. Chem. Phys. 109, 8218 (1998), with P = A + B, M = A - B:
//         one orthonormal basis b with two sigma blocks (QcSubspace), M+ = b^T P b, M- = b^T M b, H = (M-)^1/2 M+ (M-)^1/2, H T = w^2 T,
//         R~ = (M-)^1/2 T w^-1/2, L~ = M+ R~ / w, R = b R~ = X + Y, L = b L~ = X - Y, L . R = 1,
//         residuals W_R = P R - w L and W_L = M L - w R.
// Every sum outside the GEMMs is a fixed-order reduction and no kernel uses atomics: a call is bitwise reproducible.
#include "qc_subspace.h"

namespace {

constexpr int XT = 32;            // tile of the assembly kernel: XT x XT elements of (a, b), 256 threads, four rows each
constexpr int XT_LD = XT + 1;     // LDS row of 33 doubles: a column read by the 32 lanes of a half-wave strides 66 dwords, and
                                  // 66 l mod 64 = 2 l are 32 distinct bank pairs (ds_read_b64 banks by (a / 4) mod 64 per 32-lane group)

// A + B and A - B of one kind.  grid (pairs i >= j, tiles of a, tiles of b: the pair count, o (o + 1) / 2, sits in x, the one grid dimension without a 65535 limit); W[i,a,j,b] = (ia|jb), V[i,j,a,b] = (ij|ab), eps: orbital
// energies (n).  For i = j only the elements a >= b are formed.  The exchange integral (ib|ja) = W[i,b,j,a] is the transpose of the matrix
// W[i,:,j,:]: its tile (b0, a0) is read along rows and turned through LDS.  The mirror block (j, i) takes the tile turned through LDS too,
// so that both stores run along rows.
__global__ __launch_bounds__(256) void qc_exc_assemble_kernel(int o, int v, int kind, const double *__restrict__ W, const double *__restrict__ V,
                                                              const double *__restrict__ eps, double *__restrict__ ApB, double *__restrict__ AmB) {
    __shared__ double tx[XT][XT_LD], tp[XT][XT_LD], tm[XT][XT_LD];
    // pair p -> (i, j), i >= j: p = i (i + 1) / 2 + j
    const int p = blockIdx.x;
    int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    while (i * (i + 1) / 2 > p) --i;
    const int j = p - i * (i + 1) / 2;
    const int a0 = blockIdx.y * XT, b0 = blockIdx.z * XT;
    if (i == j && a0 + XT - 1 < b0) return;                       // (uniform) a tile strictly above the diagonal of a diagonal block
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int64_t d = (int64_t)o * v, astride = d;               // W[i,a,j,b] = W[((i v + a) o + j) v + b]: a strides o v
    const double *Wij = W + ((int64_t)i * v * o + j) * v;
    const double *Vij = V + ((int64_t)i * o + j) * v * v;
    // the exchange tile: rows b0.., columns a0.. of W[i,:,j,:]
#pragma unroll
    for (int q = 0; q < XT / 8; ++q) {
        const int r = r0 + 8 * q, bb = b0 + r, aa = a0 + c;
        tx[r][c] = (bb < v && aa < v) ? Wij[bb * astride + aa] : 0.0;
    }
    __syncthreads();
    const double four = kind == 0 ? 4.0 : 0.0;
#pragma unroll
    for (int q = 0; q < XT / 8; ++q) {
        const int r = r0 + 8 * q, a = a0 + r, b = b0 + c;
        double pv = 0.0, mv = 0.0;
        if (a < v && b < v && (i != j || a >= b)) {
            const double w = Wij[a * astride + b], x = tx[c][r], g = Vij[(int64_t)a * v + b];
            const double de = (i == j && a == b) ? eps[o + a] - eps[i] : 0.0;
            pv = ((four * w - x) - g) + de;
            mv = (x - g) + de;
            const int64_t e = ((int64_t)i * v + a) * d + (int64_t)j * v + b;
            ApB[e] = pv; AmB[e] = mv;
        }
        tp[r][c] = pv; tm[r][c] = mv;
    }
    __syncthreads();
    // mirror image: element (j v + b, i v + a) = element (i v + a, j v + b); this thread stores row b = b0 + r, column a = a0 + c
#pragma unroll
    for (int q = 0; q < XT / 8; ++q) {
        const int r = r0 + 8 * q, b = b0 + r, a = a0 + c;
        if (a < v && b < v && (i != j || a > b)) {
            const int64_t e = ((int64_t)j * v + b) * d + (int64_t)i * v + a;
            ApB[e] = tp[c][r]; AmB[e] = tm[c][r];
        }
    }
}

// A = 1/2 (P + M), written over P (both exactly symmetric, so A is)
__global__ void qc_exc_half_sum_kernel(int64_t n, double *__restrict__ P, const double *__restrict__ M) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) P[e] = 0.5 * (P[e] + M[e]);
}

// out[e] = s (A[e, e] + (B ? B[e, e] : A[e, e]))
__global__ void qc_exc_diag_kernel(int d, double s, const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < d) out[e] = s * (A[(int64_t)e * d + e] + (B ? B[(int64_t)e * d + e] : A[(int64_t)e * d + e]));
}

// TDHF residuals of root k = blockIdx.x >> 1, side s = blockIdx.x & 1 (0: W_R = P R - w L, 1: W_L = M L - w R), one workgroup each:
//   r = sum_j ys_j Sg_j - w sum_j yv_j V_j,   ys / yv = R~ / L~ (side 0, Sg = P b) or L~ / R~ (side 1, Sg = M b)
// info[2 k + s] = |r|^2, and t = r / (diag - w) with the floor of the stability preconditioner goes to T[(2 k + s) * dim ..].
__global__ __launch_bounds__(1024) void qc_tdhf_residual_kernel(int dim, int m, int ldy, const double *__restrict__ V, const double *__restrict__ Sp,
                                                                const double *__restrict__ Sm, const double *__restrict__ Rt, const double *__restrict__ Lt,
                                                                const double *__restrict__ omega, const double *__restrict__ diag, double *__restrict__ T,
                                                                double *__restrict__ info) {
    __shared__ double sh[16];
    const int k = blockIdx.x >> 1, side = blockIdx.x & 1;
    const double *Sg = side ? Sm : Sp;
    const double *ys = (side ? Lt : Rt) + (size_t)k * ldy, *yv = (side ? Rt : Lt) + (size_t)k * ldy;
    const double w = omega[k];
    double *t = T + (size_t)blockIdx.x * dim;
    double s = 0.0;
    for (int e = threadIdx.x; e < dim; e += 1024) {
        double r = 0.0;
        for (int j = 0; j < m; ++j) r = fma(ys[j], Sg[(size_t)j * dim + e], fma(-w * yv[j], V[(size_t)j * dim + e], r));
        s = fma(r, r, s);
        double dd = diag[e] - w;
        if (fabs(dd) < QC_STAB_DENOM_FLOOR) dd = dd < 0.0 ? -QC_STAB_DENOM_FLOOR : QC_STAB_DENOM_FLOOR;
        t[e] = r / dd;
    }
    s = qc_stab_block_sum(s, sh);
    if (threadIdx.x == 0) info[blockIdx.x] = s;
}

// ---- the two matrices in HBM
struct ExcMatrices {
    int o = 0, v = 0, d = 0;
    DevBuf P, M;                       // A + B, A - B (d x d each)
    double ms_tensor = 0.0, ms_transform = 0.0;
};

// bytes the integral phase holds at its peak plus the two matrices, and `extra` doubles of the caller (solver buffers)
double exc_need_bytes(int n, int o, int v, double extra) {
    const double nn = (double)n * n, d = (double)o * v;
    return 8.0 * (nn * nn + o * nn * n + d * nn + (double)o * o * nn + d * o * n + (double)o * o * v * n + d * d + (double)o * o * v * v + 2.0 * d * d + extra);
}

int exc_build_matrices(qc_system *S, int nocc, const double *dC, const double *dEps, int kind, double extra, ExcMatrices &X) {
    const int n = S->nbasis, o = nocc, v = n - nocc;
    const int64_t nn = (int64_t)n * n, n3 = nn * n, n4 = nn * nn, d = (int64_t)o * v;
    X.o = o; X.v = v; X.d = (int)d;
    hipStream_t st = S->stream;
    QC_HIP_CHECK(hipStreamSynchronize(st));
    size_t free_b = 0, total_b = 0;
    QC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (exc_need_bytes(n, o, v, extra) * 1.05 > (double)free_b) return QC_ERR_UNSUPPORTED;

    // 1. the AO tensor
    const double t0 = qc_now_ms();
    DevBuf I, T1, T2, T3, W, U, Y, Vv;
    if (I.alloc(n4) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(I.p, 0, n4 * sizeof(double), st));
    int rc = qc_launch_eri_full(S, I.p);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t1 = qc_now_ms();
    // 2. quarter transformations.  (i nu|la si) is shared; the tensor and every intermediate are freed as soon as nothing reads them.
    if (T1.alloc(o * n3) != QC_OK) return QC_ERR_HIP;
    qc_quarter_first(st, n, dC, 0, o, I.p, T1.p);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    I.reset();
    if (T2.alloc(d * nn) != QC_OK || U.alloc((int64_t)o * o * nn) != QC_OK) return QC_ERR_HIP;
    qc_quarter_second(st, n, o, dC, o, v, T1.p, T2.p);                    // (i a|la si)
    qc_quarter_second(st, n, o, dC, 0, o, T1.p, U.p);                     // (i j|la si)
    QC_HIP_CHECK(hipStreamSynchronize(st));
    T1.reset();
    if (T3.alloc(d * o * n) != QC_OK || Y.alloc((int64_t)o * o * v * n) != QC_OK) return QC_ERR_HIP;
    qc_quarter_third(st, n, (int)d, dC, 0, o, T2.p, T3.p);                // (i a|j si)
    qc_quarter_third(st, n, o * o, dC, o, v, U.p, Y.p);                   // (i j|a si)
    QC_HIP_CHECK(hipStreamSynchronize(st));
    T2.reset(); U.reset();
    if (W.alloc(d * d) != QC_OK || Vv.alloc((int64_t)o * o * v * v) != QC_OK) return QC_ERR_HIP;
    qc_quarter_last(st, n, (int)(d * o), dC, o, v, T3.p, W.p);            // (i a|j b)
    qc_quarter_last(st, n, o * o * v, dC, o, v, Y.p, Vv.p);               // (i j|a b)
    QC_HIP_CHECK(hipStreamSynchronize(st));
    T3.reset(); Y.reset();
    // 3. assembly
    if (X.P.alloc(d * d) != QC_OK || X.M.alloc(d * d) != QC_OK) return QC_ERR_HIP;
    const int vt = (v + XT - 1) / XT;
    hipLaunchKernelGGL(qc_exc_assemble_kernel, dim3(o * (o + 1) / 2, vt, vt), dim3(256), 0, st, o, v, kind, W.p, Vv.p, dEps, X.P.p, X.M.p);
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t2 = qc_now_ms();
    X.ms_tensor = t1 - t0; X.ms_transform = t2 - t1;
    return QC_OK;
}

// the diagonal of `A` (s (A_ee + B_ee)) on the device and on the host
int exc_diagonal(hipStream_t st, int d, double s, const double *A, const double *B, DevBuf &dDiag, std::vector<double> &diag) {
    if (!dDiag.p && dDiag.alloc(d) != QC_OK) return QC_ERR_HIP;
    hipLaunchKernelGGL(qc_exc_diag_kernel, dim3((d + 255) / 256), dim3(256), 0, st, d, s, A, B, dDiag.p);
    diag.resize(d);
    QC_HIP_CHECK(hipMemcpyAsync(diag.data(), dDiag.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    return QC_OK;
}

// the product handed to the Davidson loop: rows k0 .. k1 - 1 of Sg = the same rows of V times the symmetric matrix A, one GEMM
struct ExcProduct {
    hipStream_t st; int d; const double *A; int products = 0;
    int operator()(const double *V, double *Sg, int k0, int k1) {
        if (k1 > k0) qc_gemm(st, k1 - k0, d, d, 1.0, V + (size_t)k0 * d, d, false, A, d, false, 0.0, Sg + (size_t)k0 * d, d);
        products += k1 - k0;
        return QC_OK;
    }
};

// mu[k * 3 + q] = sqrt 2 r^q . x_k for nroots vectors x (device, rows of d), r^q = C_occ^T M_q C_virt
int exc_transition_dipoles(qc_system *S, int o, int v, const double *dC, const double *dX, int nroots, double *mu) {
    const int n = S->nbasis, d = o * v;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    DevBuf dM3, Pb, Rh, dOut;
    if (dM3.alloc(3 * nn) != QC_OK || Pb.alloc((size_t)n * v) != QC_OK || Rh.alloc((size_t)3 * d) != QC_OK || dOut.alloc(3 * QC_STAB_MAXROOTS) != QC_OK) return QC_ERR_HIP;
    const double origin[3] = {0.0, 0.0, 0.0};
    int rc = qc_dipole_device(S, origin, dM3.p);
    if (rc != QC_OK) return rc;
    for (int q = 0; q < 3; ++q) qc_ao_to_ov(st, n, o, v, dC, dM3.p + q * nn, Pb.p, Rh.p + (size_t)q * d);
    qc_stab_dots(st, d, Rh.p, 3, dX, 0, nroots, 3, dOut.p);                                                    // out[k * 3 + q] = <r^q, x_k>
    double h[3 * QC_STAB_MAXROOTS];
    QC_HIP_CHECK(hipMemcpyAsync(h, dOut.p, (size_t)3 * nroots * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    for (int e = 0; e < 3 * nroots; ++e) mu[e] = std::sqrt(2.0) * h[e];
    return QC_OK;
}

// ---- TDHF (the reduced generalised problem on the host: tdhf_reduced, qc_subspace_host.h)
struct TdhfOut { double omega[QC_STAB_MAXROOTS], rnorm[QC_STAB_MAXROOTS]; int nconv = 0, iterations = 0, products = 0; };

// Lowest nroots positive roots of M P R = w^2 R.  dR, dL (device, nroots x dim each): R = X + Y and L = X - Y of the last estimate.
int tdhf_solve(qc_system *S, int dim, int nroots, double tol, int maxit, const double *P, const double *Mx, const double *dDiag,
               const std::vector<double> &diag, TdhfOut &out, double *dR, double *dL) {
    constexpr int LD = QC_STAB_MAXSUB, NR = QC_STAB_MAXROOTS;
    hipStream_t st = S->stream;
    // sigma block 0: P b, block 1: M b; the coefficient rows of the subspace hold R~ (and the Z of a restart), dLt holds L~
    QcSubspace sub;
    DevBuf T, dLt, dW, dNorm;
    if (sub.alloc(st, dim, 2, LD) != QC_OK || T.alloc((size_t)2 * NR * dim) != QC_OK || dLt.alloc((size_t)NR * LD) != QC_OK || dW.alloc(NR) != QC_OK ||
        dNorm.alloc(2 * NR) != QC_OK) return QC_ERR_HIP;
    int rc = qc_stab_start(sub, nroots, diag);
    if (rc != QC_OK) return rc;

    std::vector<double> Rt, Lt, Rsel((size_t)NR * LD, 0.0), Lsel((size_t)NR * LD, 0.0), Z((size_t)LD * LD, 0.0);
    std::vector<double> Rprev((size_t)NR * LD, 0.0), Lprev((size_t)NR * LD, 0.0);      // the estimates of the round before, in the coordinates of b
    double omega[NR] = {0}, rnorm[NR] = {0}, norm2[2 * NR];
    int it = 0, nconv = 0; bool converged = false, have_prev = false;
    for (int r = 0; r < NR; ++r) out.omega[r] = out.rnorm[r] = 0.0;
    for (it = 1; it <= maxit; ++it) {
        // sigma+ = P b and sigma- = M b of the new rows, one GEMM each
        if (sub.m > sub.m_done) {
            const int k0 = sub.m_done, nk = sub.m - sub.m_done;
            qc_gemm(st, nk, dim, dim, 1.0, sub.V.p + (size_t)k0 * dim, dim, false, P, dim, false, 0.0, sub.Sg[0].p + (size_t)k0 * dim, dim);
            qc_gemm(st, nk, dim, dim, 1.0, sub.V.p + (size_t)k0 * dim, dim, false, Mx, dim, false, 0.0, sub.Sg[1].p + (size_t)k0 * dim, dim);
            out.products += 2 * nk;
        }
        if ((rc = sub.project()) != QC_OK) return rc;
        const int m = sub.m;
        if (!tdhf_reduced(m, sub.reduced(0), sub.reduced(1), nroots, omega, Rt, Lt)) break;      // (cannot happen at a reference certified stable; the last estimates stand)
        std::fill(Rsel.begin(), Rsel.end(), 0.0); std::fill(Lsel.begin(), Lsel.end(), 0.0);
        for (int r = 0; r < nroots; ++r) for (int j = 0; j < m; ++j) { Rsel[(size_t)r * LD + j] = Rt[(size_t)r * m + j]; Lsel[(size_t)r * LD + j] = Lt[(size_t)r * m + j]; }
        QC_HIP_CHECK(hipMemcpyAsync(sub.coef.p, Rsel.data(), Rsel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dLt.p, Lsel.data(), Lsel.size() * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dW.p, omega, nroots * sizeof(double), hipMemcpyHostToDevice, st));
        // R = b R~ and L = b L~ of this estimate, both residuals and their preconditioned images
        sub.combine(sub.coef.p, nroots, 0, dR);
        sub.combine(dLt.p, nroots, 0, dL);
        hipLaunchKernelGGL(qc_tdhf_residual_kernel, dim3(2 * nroots), dim3(1024), 0, st, dim, m, LD, sub.V.p, sub.Sg[0].p, sub.Sg[1].p, sub.coef.p, dLt.p, dW.p,
                           dDiag, T.p, dNorm.p);
        QC_HIP_CHECK(hipMemcpyAsync(norm2, dNorm.p, 2 * nroots * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        nconv = 0;
        for (int r = 0; r < nroots; ++r) {
            rnorm[r] = std::sqrt(std::max(norm2[2 * r], norm2[2 * r + 1]));
            out.omega[r] = omega[r]; out.rnorm[r] = rnorm[r];
            if (rnorm[r] <= tol) ++nconv;
        }
        if (nconv == nroots) { converged = true; break; }
        // The subspace cannot take this round's directions: restart from the R and L of the requested roots and, as far as room is left
        // for one more round, from the R and L of the round before (what a conjugate-gradient step keeps), orthonormalised in coefficient
        // space (b is orthonormal).  sigma+ and sigma- follow by linearity; the reduced problem of the smaller space has the same roots.
        const int nadd = 2 * (nroots - nconv);
        bool collapsed = false;
        if (dim > sub.msub && m + nadd > sub.msub && m > 2 * nroots) {
            std::fill(Z.begin(), Z.end(), 0.0);
            int k = 0;
            for (int q = 0; q < 2 * nroots; ++q)
                if (qc_orthonormalize_row(Z.data(), LD, m, k, (q & 1) ? &Lsel[(size_t)(q >> 1) * LD] : &Rsel[(size_t)(q >> 1) * LD])) ++k;
            if (have_prev)
                for (int side = 0; side < 2; ++side)
                    for (int r = 0; r < nroots; ++r)
                        if (rnorm[r] > tol && k + nadd < sub.msub && qc_orthonormalize_row(Z.data(), LD, m, k, side ? &Lprev[(size_t)r * LD] : &Rprev[(size_t)r * LD])) ++k;
            if ((rc = sub.collapse(Z.data(), k)) != QC_OK) return rc;
            // this round's estimates in the coordinates of the new basis: they are the "round before" of the next restart
            qc_rows_in_basis(Z.data(), LD, m, k, Rsel.data(), NR, Rprev.data());
            qc_rows_in_basis(Z.data(), LD, m, k, Lsel.data(), NR, Lprev.data());
            QC_HIP_CHECK(hipStreamSynchronize(st));          // (Z is read by the enqueued copy; the next round overwrites it)
            collapsed = true;
        }
        if (!collapsed) { Rprev = Rsel; Lprev = Lsel; }
        have_prev = true;
        // new directions: the preconditioned residuals of every root that has not converged, orthogonalised into b (at most two per root)
        for (int r = 0; r < nroots; ++r) {
            if (rnorm[r] <= tol) continue;
            for (int side = 0; side < 2; ++side) sub.seed(T.p + (size_t)(2 * r + side) * dim, 2 * r + side);
        }
        int added = 0;
        if ((rc = sub.added(&added)) != QC_OK) return rc;
        if (added == 0) break;                               // (nothing left to add: the residuals are as small as this arithmetic makes them)
        sub.m += added;
    }
    if (it > maxit) it = maxit;
    out.nconv = nconv; out.iterations = it;
    QC_HIP_CHECK(hipGetLastError());
    return converged ? QC_OK : QC_NOT_CONVERGED;
}

void exc_clear(qc_excitations *io) {
    for (int k = 0; k < 8; ++k) io->energies[k] = io->residuals[k] = io->oscillator[k] = 0.0;
    for (double &t : io->transition_dipole) t = 0.0;
    io->nconverged = io->iterations = io->products = io->reference_unstable = 0;
    io->ms_total = io->ms_tensor = io->ms_transform = io->ms_solve = 0.0;
}

}  // namespace

int qc_excitation_matrices_device(qc_system *S, int nocc, const double *dC, const double *dEps, int kind, double *ApB, double *AmB) {
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    ExcMatrices X;
    int rc = exc_build_matrices(S, nocc, dC, dEps, kind, 0.0, X);
    if (rc != QC_OK) return rc;
    const size_t dd = (size_t)X.d * X.d;
    if (ApB) QC_HIP_CHECK(hipMemcpyAsync(ApB, X.P.p, dd * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    if (AmB) QC_HIP_CHECK(hipMemcpyAsync(AmB, X.M.p, dd * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

int qc_excitations_device(qc_system *S, int nocc, const double *dC, const double *dEps, qc_excitations *io, double *vectors) {
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const double t_begin = qc_now_ms();
    const int n = S->nbasis, o = nocc, v = n - nocc, dim = o * v, nroots = io->nroots;
    const bool tdhf = io->method == 1;
    const double tol = io->tol > 0.0 ? io->tol : 1e-6;
    const int maxit = io->max_iterations > 0 ? io->max_iterations : 100;
    hipStream_t st = S->stream;
    exc_clear(io);
    ExcMatrices X;
    // solver buffers: three blocks of 41 rows, three of 40 work rows for a restart, the states and the staged residuals
    const double extra = (6.0 * (QC_STAB_MAXSUB + 1) + 6.0 * QC_STAB_MAXROOTS + 8.0) * dim + 3.0 * n * n;
    int rc = exc_build_matrices(S, nocc, dC, dEps, io->kind, extra, X);
    if (rc != QC_OK) return rc;
    io->ms_tensor = X.ms_tensor; io->ms_transform = X.ms_transform;
    const double t_solve = qc_now_ms();

    DevBuf dDiag, dVec;
    std::vector<double> diag;
    if (dVec.alloc((size_t)2 * nroots * dim) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(dVec.p, 0, (size_t)2 * nroots * dim * sizeof(double), st));      // (a solver that stops before its first estimate returns zeros)
    int status = QC_OK;
    if (!tdhf) {
        // A = 1/2 (P + M) over P; the preconditioner uses its true diagonal
        const int64_t dd = (int64_t)dim * dim;
        hipLaunchKernelGGL(qc_exc_half_sum_kernel, dim3((unsigned)((dd + 255) / 256)), dim3(256), 0, st, dd, X.P.p, X.M.p);
        X.M.reset();
        if ((rc = exc_diagonal(st, dim, 0.5, X.P.p, nullptr, dDiag, diag)) != QC_OK) return rc;
        ExcProduct prod{st, dim, X.P.p};
        StabDavidsonOut out;
        status = qc_stab_davidson(S, dim, nroots, tol, maxit, dDiag.p, diag, prod, out, vectors, dVec.p, kJacobiStop);
        if (status < 0) return status;
        for (int k = 0; k < nroots; ++k) { io->energies[k] = out.theta[k]; io->residuals[k] = out.rnorm[k]; }
        io->nconverged = out.nconv; io->iterations = out.iterations; io->products = prod.products;
    } else {
        // the reference must be a minimum of both kinds of rotation this matrix pair sees: the lowest root of P and of M, each to its own
        // residual rho, must satisfy theta - rho > 0.  The check has the default budget of 100 rounds whatever max_iterations says: a budget
        // that leaves rho large would report a stable reference as unstable.
        for (int which = 0; which < 2; ++which) {
            const double *A = which ? X.M.p : X.P.p;
            if ((rc = exc_diagonal(st, dim, 0.5, A, nullptr, dDiag, diag)) != QC_OK) return rc;
            ExcProduct prod{st, dim, A};
            StabDavidsonOut out;
            rc = qc_stab_davidson(S, dim, 1, tol, 100, dDiag.p, diag, prod, out, nullptr, nullptr, kJacobiStop);
            if (rc < 0) return rc;
            io->products += prod.products;
            if (!(out.theta[0] - out.rnorm[0] > 0.0)) io->reference_unstable = 1;
        }
        if (io->reference_unstable) {
            io->ms_solve = qc_now_ms() - t_solve; io->ms_total = qc_now_ms() - t_begin;
            if (vectors) std::fill(vectors, vectors + (size_t)2 * nroots * dim, 0.0);
            return QC_NOT_CONVERGED;
        }
        if ((rc = exc_diagonal(st, dim, 0.5, X.P.p, X.M.p, dDiag, diag)) != QC_OK) return rc;          // diagonal of A
        TdhfOut out;
        status = tdhf_solve(S, dim, nroots, tol, maxit, X.P.p, X.M.p, dDiag.p, diag, out, dVec.p, dVec.p + (size_t)nroots * dim);
        if (status < 0) return status;
        for (int k = 0; k < nroots; ++k) { io->energies[k] = out.omega[k]; io->residuals[k] = out.rnorm[k]; }
        io->nconverged = out.nconv; io->iterations = out.iterations; io->products += out.products;
        if (vectors) {
            QC_HIP_CHECK(hipMemcpyAsync(vectors, dVec.p, (size_t)2 * nroots * dim * sizeof(double), hipMemcpyDeviceToHost, st));
            QC_HIP_CHECK(hipStreamSynchronize(st));
        }
    }
    io->ms_solve = qc_now_ms() - t_solve;
    // transition dipoles and oscillator strengths of the singlets (triplets: exactly zero)
    if (io->kind == 0) {
        double mu[3 * QC_STAB_MAXROOTS];
        if ((rc = exc_transition_dipoles(S, o, v, dC, dVec.p, nroots, mu)) != QC_OK) return rc;
        for (int k = 0; k < nroots; ++k) {
            double s = 0.0;
            for (int q = 0; q < 3; ++q) { io->transition_dipole[3 * k + q] = mu[3 * k + q]; s += mu[3 * k + q] * mu[3 * k + q]; }
            io->oscillator[k] = 2.0 / 3.0 * io->energies[k] * s;
        }
    }
    io->ms_total = qc_now_ms() - t_begin;
    return status;
}
