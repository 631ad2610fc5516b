// qc_population.hip - population analysis of a determinant on the device: Mulliken and Loewdin charges and spin
// populations, gross populations per basis function, Mayer and Wiberg bond orders.
//
// With P_t = P_alpha + P_beta, P_s = P_alpha - P_beta and a in A meaning "function a sits on atom A":
//   Mulliken  A_x = P_x S              N_A = sum_{a in A} (A_t)_aa     B_AB = sum_{a in A, b in B} (A_t)_ab (A_t)_ba + (A_s)_ab (A_s)_ba   (Mayer)
//   Loewdin   A_x = S^1/2 P_x S^1/2    N_A = sum_{a in A} (A_t)_aa     B_AB = the same expression - A_x is symmetric, so it is sum (A_x)_ab^2  (Wiberg)
// S^1/2 = S X with X = S^-1/2 the symmetric orthogonaliser of the SCF set-up (resident in a state; built the same way here for a call
// without one): no second eigensolve and no square roots of small eigenvalues; A_x = (S X) P_x (S X)^T is symmetric to rounding.
// The products are qc_gemm calls; the atom sums are fixed-order reductions - one workgroup per atom (pair), the atom's functions walked
// in ascending order from the lists that sit in the shell blob, qc_stab_block_sum, no float atomics: two calls give the same bits.
#include "qc_subspace.h"

namespace {

// workgroup A: out[A] = sum_{a in A} At_aa, out[natoms + A] = the same of As (0 without As); orb[a] = At_aa
__global__ __launch_bounds__(256) void qc_pop_atom_kernel(int n, const int *__restrict__ aoff, const int *__restrict__ flist, const double *__restrict__ At,
                                                          const double *__restrict__ As, int natoms, double *__restrict__ out, double *__restrict__ orb) {
    __shared__ double sh[16];
    const int A = blockIdx.x, lo = aoff[A], hi = aoff[A + 1];
    double st = 0.0, ss = 0.0;
    for (int k = lo + (int)threadIdx.x; k < hi; k += 256) {
        const int a = flist[k];
        const double d = At[(size_t)a * n + a];
        orb[a] = d;
        st += d;
        if (As) ss += As[(size_t)a * n + a];
    }
    st = qc_stab_block_sum(st, sh);
    ss = qc_stab_block_sum(ss, sh);
    if (threadIdx.x == 0) { out[A] = st; out[natoms + A] = ss; }
}

// workgroup = atom pair A >= B: bo[A, B] = bo[B, A] = sum_{a in A, b in B} At_ab At_ba + As_ab As_ba
__global__ __launch_bounds__(256) void qc_pop_bond_kernel(int n, const int *__restrict__ aoff, const int *__restrict__ flist, const double *__restrict__ At,
                                                          const double *__restrict__ As, int natoms, double *__restrict__ bo) {
    __shared__ double sh[16];
    int A = 0, rem = blockIdx.x;
    while (rem > A) { rem -= A + 1; ++A; }
    const int B = rem;
    if (A >= natoms) return;
    const int la = aoff[A], na = aoff[A + 1] - la, lb = aoff[B], nb = aoff[B + 1] - lb;
    double s = 0.0;
    for (int e = threadIdx.x; e < na * nb; e += 256) {
        const int a = flist[la + e / nb], b = flist[lb + e % nb];
        s = fma(At[(size_t)a * n + b], At[(size_t)b * n + a], s);
        if (As) s = fma(As[(size_t)a * n + b], As[(size_t)b * n + a], s);
    }
    s = qc_stab_block_sum(s, sh);
    if (threadIdx.x == 0) { bo[(size_t)A * natoms + B] = s; bo[(size_t)B * natoms + A] = s; }
}

}  // namespace

// X = S^-1/2 from S as the SCF set-up forms it: U diag((U^T S U)_ii^-1/2) U^T with U the eigenvectors of S (dS is left intact)
int qc_population_x_device(qc_system *S, const double *dS, double *dX) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    DevBuf dA, dU, dw;
    QcEigWork E;
    QcDev<int> notconv;
    if (dA.alloc(nn) != QC_OK || dU.alloc(nn) != QC_OK || dw.alloc(n) != QC_OK || E.alloc(n) != QC_OK || notconv.alloc(1) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dA.p, dS, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    QC_HIP_CHECK(hipMemsetAsync(E.ctl.p, 0, 4 * sizeof(int), st));
    QC_HIP_CHECK(hipMemsetAsync(notconv.p, 0, sizeof(int), st));
    int rc = qc_eig_cold_sync(st, n, dA.p, dU.p, dw.p, E, E.ctl.p, notconv.p);
    if (rc != QC_OK) return rc;
    int flag = 0;
    QC_HIP_CHECK(hipMemcpyAsync(&flag, notconv.p, sizeof(int), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    if (flag) return QC_EIG_NOT_CONVERGED;
    qc_gemm(st, n, n, n, 1.0, dS, n, false, dU.p, n, false, 0.0, E.t1.p, n);          // S U
    qc_gemm(st, n, n, n, 1.0, dU.p, n, true, E.t1.p, n, false, 0.0, E.t2.p, n);       // U^T (S U)
    qc_scale_cols_invsqrt(st, n, dU.p, E.t2.p, E.t1.p);                               // U diag^-1/2
    qc_gemm(st, n, n, n, 1.0, E.t1.p, n, false, dU.p, n, true, 0.0, dX, n);           // (.) U^T
    QC_HIP_CHECK(hipStreamSynchronize(st));                                           // (the scratch goes away with this frame)
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// scheme 0 Mulliken, 1 Loewdin (dX needed).  dPa, dPb: the two spin densities; dPb null: dPa is P_t of a closed shell (P_s = 0, nothing is
// computed for it).  Host outputs: N_t, N_s (natoms each), orbital (n, nullable), bond_orders (natoms^2, nullable).  Reads its inputs only.
int qc_population_device(qc_system *S, int scheme, const double *dPa, const double *dPb, const double *dS, const double *dX, double *Nt, double *Ns,
                         double *orbital, double *bond_orders) {
    const int n = S->nbasis, na = S->natoms;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    const QcShellBlob *B;
    int rc = qc_shell_blob(S, &B);
    if (rc != QC_OK) return rc;
    const bool open = dPb != nullptr;
    DevBuf Pt, Ps, At, As, Sh, T, dOut, dOrb, dBo;
    if (At.alloc(nn) != QC_OK || dOut.alloc(2 * (size_t)na) != QC_OK || dOrb.alloc(n) != QC_OK || (bond_orders && dBo.alloc((size_t)na * na) != QC_OK)) return QC_ERR_HIP;
    if (open && (Pt.alloc(nn) != QC_OK || Ps.alloc(nn) != QC_OK || As.alloc(nn) != QC_OK)) return QC_ERR_HIP;
    if (scheme == 1 && (Sh.alloc(nn) != QC_OK || T.alloc(nn) != QC_OK)) return QC_ERR_HIP;
    const double *pt = dPa, *ps = nullptr;
    if (open) {
        qc_axpby(st, n, 1.0, dPa, 1.0, dPb, Pt.p);
        qc_axpby(st, n, 1.0, dPa, -1.0, dPb, Ps.p);
        pt = Pt.p; ps = Ps.p;
    }
    if (scheme == 0) {
        qc_gemm(st, n, n, n, 1.0, pt, n, false, dS, n, false, 0.0, At.p, n);
        if (open) qc_gemm(st, n, n, n, 1.0, ps, n, false, dS, n, false, 0.0, As.p, n);
    } else {
        qc_gemm(st, n, n, n, 1.0, dS, n, false, dX, n, false, 0.0, Sh.p, n);              // S^1/2 = S X
        qc_gemm(st, n, n, n, 1.0, Sh.p, n, false, pt, n, false, 0.0, T.p, n);
        qc_gemm(st, n, n, n, 1.0, T.p, n, false, Sh.p, n, true, 0.0, At.p, n);            // (S X) P (S X)^T
        if (open) {
            qc_gemm(st, n, n, n, 1.0, Sh.p, n, false, ps, n, false, 0.0, T.p, n);
            qc_gemm(st, n, n, n, 1.0, T.p, n, false, Sh.p, n, true, 0.0, As.p, n);
        }
    }
    hipLaunchKernelGGL(qc_pop_atom_kernel, dim3(na), dim3(256), 0, st, n, B->aoff, B->flist, At.p, open ? As.p : nullptr, na, dOut.p, dOrb.p);
    QC_HIP_CHECK(hipGetLastError());
    if (bond_orders) {
        hipLaunchKernelGGL(qc_pop_bond_kernel, dim3(na * (na + 1) / 2), dim3(256), 0, st, n, B->aoff, B->flist, At.p, open ? As.p : nullptr, na, dBo.p);
        QC_HIP_CHECK(hipGetLastError());
    }
    std::vector<double> out(2 * (size_t)na);
    QC_HIP_CHECK(hipMemcpyAsync(out.data(), dOut.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (orbital) QC_HIP_CHECK(hipMemcpyAsync(orbital, dOrb.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (bond_orders) QC_HIP_CHECK(hipMemcpyAsync(bond_orders, dBo.p, (size_t)na * na * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    for (int a = 0; a < na; ++a) { Nt[a] = out[a]; Ns[a] = open ? out[na + a] : 0.0; }
    return QC_OK;
}
