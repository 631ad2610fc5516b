// qc_stability.hip - SCF wave-function stability analysis: the lowest eigenpairs of the real orbital Hessian (A + B) by a block
// Davidson iteration whose Hessian-vector product is the direct Fock build, and the orbital rotation that follows an eigenvector.
//
// For real orbitals and a trial vector x^s_ia (s = spin, i occupied, a virtual, laid out x[i * v + a]) the symmetric pseudo-density
//   D1^s = C_occ^s x^s C_virt^s^T + transpose
// turns the two-electron part of (A + B) x into one Fock build:
//   UHF internal      sigma^s = (e_a - e_i) x^s + [C_virt^s^T (J[D1^a + D1^b] - K[D1^s]) C_occ^s]_ai      one UHF build of (D1^a, D1^b)
//   RHF singlet       the bracket is 2 J[D1] - K[D1]: one RHF build of 2 D1
//   RHF -> UHF        the bracket is -K[D1]: the alpha output of one UHF build of (D1, -D1)
// Trial vectors, sigma vectors and the correction vector live in HBM (msub + 1 rows of `dim` doubles each); the subspace matrix
// (at most QC_STAB_MAXSUB rows) is diagonalised on the host.  Every dot product is a fixed-order reduction (a thread's elements in
// index order, the 64 lanes of a wave by a shuffle tree, the waves in order) and the Fock build accumulates integers: a call is bitwise
// reproducible.  The subspace, its kernels and the Davidson loop are in qc_subspace.h / qc_subspace.hip (shared with qc_response.hip and qc_excited.hip);
// this file defines the Hessian-vector product declared there (StabSigma, its kernels, qc_ao_to_ov), the product handed to that loop and the rotation.
#include "qc_subspace.h"

namespace {

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

}  // namespace

void qc_stab_fill_delta(hipStream_t st, const StabLayout &L, int n, const double *dEps, double *dDe) {
    for (int b = 0; b < L.nblk; ++b)
        if (L.o[b] * L.v[b] > 0) hipLaunchKernelGGL(qc_stab_delta_kernel, dim3((L.o[b] * L.v[b] + 255) / 256), dim3(256), 0, st, L.o[b], L.v[b], dEps + (size_t)b * n, dDe + L.off[b]);
}

void qc_ao_to_ov(hipStream_t st, int n, int o, int v, const double *C, const double *M_ao, double *scratch, double *out) {
    qc_gemm(st, n, v, n, 1.0, M_ao, n, false, C + o, n, false, 0.0, scratch, v);      // M C_virt
    qc_gemm(st, o, v, n, 1.0, C, n, true, scratch, v, false, 0.0, out, v);            // C_occ^T (.)
}

int StabSigma::alloc() {
    const size_t n = S->nbasis, nn = n * n;
    return P.alloc(nn) != QC_OK || Q.alloc(nn) != QC_OK || D1.alloc(2 * nn) != QC_OK || G.alloc(2 * nn) != QC_OK || R.alloc(std::max<size_t>(L.dim, 1)) != QC_OK ? QC_ERR_HIP : QC_OK;
}

int StabSigma::apply(const double *dx, double *dsg) {
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
        qc_ao_to_ov(st, n, L.o[b], L.v[b], dC + b * nn, G.p + b * nn, P.p, R.p + L.off[b]);                           // C_occ^T G C_virt
        const int ov = L.o[b] * L.v[b];
        hipLaunchKernelGGL(qc_stab_sigma_kernel, dim3((ov + 255) / 256), dim3(256), 0, st, ov, dDe + L.off[b], dx + L.off[b], R.p + L.off[b],
                           dsg + L.off[b]);
    }
    QC_HIP_CHECK(hipGetLastError());
    return QC_OK;
}

int qc_stability_dim(int n, bool uhf, const int *nocc) { return StabLayout(n, uhf, nocc).dim; }

// Lowest `nroots` eigenpairs of (A + B) at the orbitals dC / energies dEps (device; nblk blocks).  io: kind, nroots, tol, max_iterations
// checked by the caller.  vectors (host, nullable): nroots x dim.
int qc_stability_device(qc_system *S, bool uhf, const int *nocc, const double *dC, const double *dEps, qc_stability *io, double *vectors) {
    const double t_begin = qc_now_ms();
    const int n = S->nbasis, nroots = io->nroots;
    const StabLayout L(n, uhf, nocc);
    const int dim = L.dim;
    const double tol = io->tol > 0.0 ? io->tol : 1e-6;
    const int maxit = io->max_iterations > 0 ? io->max_iterations : 100;
    hipStream_t st = S->stream;

    // diagonal e_a - e_i, on the device and on the host (start vectors)
    DevBuf dDe;
    if (dDe.alloc(dim) != QC_OK) return QC_ERR_HIP;
    qc_stab_fill_delta(st, L, n, dEps, dDe.p);
    std::vector<double> de(dim);
    QC_HIP_CHECK(hipMemcpyAsync(de.data(), dDe.p, (size_t)dim * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));

    StabSigma sigma(S, L, uhf, io->kind, dC, dDe.p);
    if (sigma.alloc() != QC_OK) return QC_ERR_HIP;
    StabDavidsonOut out;
    const int rc = qc_stab_davidson(S, dim, nroots, tol, maxit, dDe.p, de, [&](const double *V, double *Sg, int k0, int k1) {
        for (int k = k0; k < k1; ++k) {
            const int r = sigma.apply(V + (size_t)k * dim, Sg + (size_t)k * dim);
            if (r != QC_OK) return r;
        }
        return (int)QC_OK;
    }, out, vectors, nullptr);
    if (rc < 0) return rc;
    for (int r = 0; r < QC_STAB_MAXROOTS; ++r) { io->eigenvalues[r] = r < nroots ? out.theta[r] : 0.0; io->residuals[r] = r < nroots ? out.rnorm[r] : 0.0; }
    io->nconverged = out.nconv; io->iterations = out.iterations; io->builds = sigma.builds;
    io->ms_builds = sigma.ms_builds;
    io->ms_total = qc_now_ms() - t_begin;
    return rc;
}

// ---- rotation along a vector.  In the MO basis (occupied first) kappa = [[0, -x], [x^T, 0]] with x the o x v block, so kappa_ai = x_ia.
// exp(theta kappa) applied to the occupied columns, with x x^T = U diag(s^2) U^T:
//   C_occ' = C_occ U cos(theta s) U^T + C_virt x^T U (sin(theta s) / s) U^T
// - an exact orthogonal rotation for any theta.  Host arithmetic (n x o matrices); hD = C_occ' C_occ'^T.
static void rotate_block(int n, int o, const double *C, const double *x, double theta, double *hD) {
    const int v = n - o;
    std::fill(hD, hD + (size_t)n * n, 0.0);
    if (o == 0) return;
    std::vector<double> Co((size_t)n * o);
    for (int mu = 0; mu < n; ++mu) for (int i = 0; i < o; ++i) Co[(size_t)mu * o + i] = C[(size_t)mu * n + i];
    if (v > 0) {
        std::vector<double> XX((size_t)o * o, 0.0), s2, U;
        for (int i = 0; i < o; ++i) for (int j = 0; j <= i; ++j) {
            double t = 0.0;
            for (int a = 0; a < v; ++a) t += x[(size_t)i * v + a] * x[(size_t)j * v + a];
            XX[(size_t)i * o + j] = XX[(size_t)j * o + i] = t;
        }
        host_sym_eig(o, XX, s2, U);                          // rows of U: eigenvectors
        // Fc = U cos U^T, Fs = U (sin / s) U^T (o x o)
        std::vector<double> Fc((size_t)o * o, 0.0), Fs((size_t)o * o, 0.0);
        for (int k = 0; k < o; ++k) {
            const double sk = std::sqrt(std::max(s2[k], 0.0)), ck = std::cos(theta * sk), sn = sk > 1e-8 ? std::sin(theta * sk) / sk : theta;
            for (int i = 0; i < o; ++i) for (int j = 0; j < o; ++j) {
                const double uu = U[(size_t)k * o + i] * U[(size_t)k * o + j];
                Fc[(size_t)i * o + j] += ck * uu; Fs[(size_t)i * o + j] += sn * uu;
            }
        }
        // xf = x^T Fs (v x o); Co' = Co Fc + C_virt xf
        std::vector<double> xf((size_t)v * o, 0.0), Cn((size_t)n * o, 0.0);
        for (int a = 0; a < v; ++a) for (int i = 0; i < o; ++i) { const double xa = x[(size_t)i * v + a]; if (xa != 0.0) for (int j = 0; j < o; ++j) xf[(size_t)a * o + j] += xa * Fs[(size_t)i * o + j]; }
        for (int mu = 0; mu < n; ++mu) {
            double *row = &Cn[(size_t)mu * o];
            for (int i = 0; i < o; ++i) { const double c = Co[(size_t)mu * o + i]; for (int j = 0; j < o; ++j) row[j] += c * Fc[(size_t)i * o + j]; }
            for (int a = 0; a < v; ++a) { const double c = C[(size_t)mu * n + o + a]; for (int j = 0; j < o; ++j) row[j] += c * xf[(size_t)a * o + j]; }
        }
        Co.swap(Cn);
    }
    for (int mu = 0; mu < n; ++mu) for (int nu = 0; nu <= mu; ++nu) {
        double t = 0.0;
        for (int i = 0; i < o; ++i) t += Co[(size_t)mu * o + i] * Co[(size_t)nu * o + i];
        hD[(size_t)mu * n + nu] = hD[(size_t)nu * n + mu] = t;
    }
}

// Densities (host, per spin, n x n) of the determinant rotated along x, and its electronic energy 1/2 sum_s tr(D_s (2 H + G_s)) from one UHF
// build.  angle <= 0: the lowest of theta = +-0.1 * 2^k, k = 0..4.
int qc_rotated_density_device(qc_system *S, bool uhf, int kind, const int *nocc, const double *dC, const double *dH, const double *x, double angle,
                              double *hDa, double *hDb, double *energy) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    const StabLayout L(n, uhf, nocc);
    hipStream_t st = S->stream;
    std::vector<double> C((uhf ? 2 : 1) * nn);
    QC_HIP_CHECK(hipMemcpyAsync(C.data(), dC, C.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    DevBuf dD, dG, dE;
    if (dD.alloc(2 * nn) != QC_OK || dG.alloc(2 * nn) != QC_OK || dE.alloc(4) != QC_OK) return QC_ERR_HIP;
    std::vector<double> Da(nn), Db(nn);
    auto eval = [&](double theta, double *e) -> int {
        rotate_block(n, L.o[0], C.data(), x, theta, Da.data());
        if (uhf) rotate_block(n, L.o[1], C.data() + nn, x + L.off[1], theta, Db.data());
        else if (kind == 1) rotate_block(n, L.o[0], C.data(), x, -theta, Db.data());
        else Db = Da;
        QC_HIP_CHECK(hipMemcpyAsync(dD.p, Da.data(), nn * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemcpyAsync(dD.p + nn, Db.data(), nn * sizeof(double), hipMemcpyHostToDevice, st));
        int rc = qc_fock_build_device(S, dD.p, dD.p + nn, dG.p, dG.p + nn, true);
        if (rc != QC_OK) return rc;
        for (int s = 0; s < 2; ++s) qc_energy_rms(st, n, dD.p + s * nn, dD.p + s * nn, dH, dG.p + s * nn, dE.p + 2 * s);
        double h[4];
        QC_HIP_CHECK(hipMemcpyAsync(h, dE.p, sizeof(h), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        if ((rc = qc_join_check(S)) != QC_OK) return rc;
        qc_gate_quiet(S);
        *e = h[0] + h[2];
        return QC_OK;
    };
    double best_e = 0.0, best_theta = angle;
    int rc;
    if (angle > 0.0) { if ((rc = eval(angle, &best_e)) != QC_OK) return rc; }
    else {
        bool first = true;
        const bool mirror = !uhf && kind == 1;           // (alpha by +theta and beta by -theta: the sign of theta only swaps the spins)
        std::vector<double> keep_a, keep_b;
        for (int k = 0; k < 5; ++k)
            for (int sgn = 0; sgn < (mirror ? 1 : 2); ++sgn) {
                const double theta = (sgn ? -0.1 : 0.1) * (double)(1 << k);
                double e = 0.0;
                if ((rc = eval(theta, &e)) != QC_OK) return rc;
                if (first || e < best_e) { best_e = e; best_theta = theta; first = false; keep_a = Da; keep_b = Db; }
            }
        Da.swap(keep_a); Db.swap(keep_b);
    }
    (void)best_theta;
    std::memcpy(hDa, Da.data(), nn * sizeof(double));
    std::memcpy(hDb, Db.data(), nn * sizeof(double));
    if (energy) *energy = best_e;
    return QC_OK;
}
