// qc_one_electron.hip - overlap, kinetic-energy, nuclear-attraction, dipole and Cartesian multipole matrices on the GPU.
//
// Replaces molint::overlap / kinetic / nuclear (call sites rhf.rs:41-43, uhf.rs:52-54) - the first "next" row of the
// scope table: the last CPU-only start-up phase of an SCF run.  Same McMurchie-Davidson formulas as the
// host version (qc_host_one_electron, qc_system.cpp), which stays as the GPU-free entry point of the C ABI:
//   S_ab = (pi/p)^{3/2} E^x_0 E^y_0 E^z_0,
//   T_ab = -1/2 sum_axis <a| d^2/dx^2 |b>   (second derivative of the ket primitive: b+2, b, b-2 terms),
//   V_ab = - sum_C Z_C (2 pi / p) sum_tuv E^x_t E^y_u E^z_v R_tuv(p, P - C).
// One wave per shell pair; the lanes share out its work items - primitive pairs (S, T) or primitive pair x nucleus (V) -
// and add their Cartesian blocks into LDS (ds_add_f64); the block is then transformed to the shells' functions.
// This is set-up code, run once per geometry: it is written for clarity, not tuned (tables in scratch memory).
// The formulas' pieces (E, Boys, R step, pair sums, Cartesian order) are those of qc_md.h, shared with the host and the gradient
// kernels; this file also owns the handle's shell blob (qc_shell_blob), which the gradient reads too.
#include <cstring>
#include <memory>

#include "qc_md.h"

namespace {

constexpr int MAXC = 10;          // Cartesian components of an f shell
// one axis' expansion table, i <= la, j <= lb + 2 (kinetic energy); its recurrence step in the fused form (qc_md_herm_e)
using E1 = QcMdE1<(QC_LMAX + 1) * (QC_LMAX + 3) * (2 * QC_LMAX + 3), true>;

// Hermite Coulomb integrals R^0_tuv, t+u+v <= L
__device__ void hermite_r(int L, double alpha, const double *PC, double (*W)[qc_nherm(QC_LPAIR)]) {
    double F[QC_LPAIR + 1];
    qc_md_boys(L, alpha * (PC[0] * PC[0] + PC[1] * PC[1] + PC[2] * PC[2]), F);
    double f = 1.0;
    for (int n = 0; n <= L; ++n) { W[n][0] = f * F[n]; f *= -2.0 * alpha; }      // (the seeds: a running product here, see qc_md.h)
    for (int N = 1; N <= L; ++N)
        for (int n = 0; n + N <= L; ++n)
            for (int t = N; t >= 0; --t)
                for (int u = N - t; u >= 0; --u) W[n][qc_hidx(t, u, N - t - u)] = qc_md_r_step(W[n + 1], t, u, N - t - u, PC);
}

typedef __attribute__((address_space(3))) double lds_double;

__global__ __launch_bounds__(64) void qc_one_electron_kernel(int which, int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                             const double *__restrict__ coefs, const double *__restrict__ Tm, int natoms,
                                                             const int *__restrict__ Z, const double *__restrict__ xyz, int n, double *__restrict__ out) {
    __shared__ double cart[MAXC * MAXC];
    // shell pair (a >= b) of this workgroup
    int a = 0, rem = blockIdx.x;
    while (rem > a) { rem -= a + 1; ++a; }
    const int b = rem;
    const QcDevShell A = sh[a], B = sh[b];
    const int lane = threadIdx.x, nca = A.ncart, ncb = B.ncart;
    for (int i = lane; i < MAXC * MAXC; i += 64) cart[i] = 0.0;
    __syncthreads();
    const int npp = A.nprim * B.nprim, nitems = (which == 2) ? npp * natoms : npp;
    for (int item = lane; item < nitems; item += 64) {
        const int pp = (which == 2) ? item / natoms : item, c = (which == 2) ? item - pp * natoms : 0;
        const int i = pp / B.nprim, j = pp - i * B.nprim;
        const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb, cc = coefs[A.poff + i] * coefs[B.poff + j];
        double P[3];
        for (int k = 0; k < 3; ++k) P[k] = (ea * A.A[k] + eb * B.A[k]) / p;
        E1 E[3];
        for (int k = 0; k < 3; ++k) E[k].fill(A.L, B.L + 2, ea, eb, A.A[k] - B.A[k]);
        const double s3 = pow(M_PI / p, 1.5);
        double W[QC_LPAIR + 1][qc_nherm(QC_LPAIR)];
        double vpref = 0.0;
        if (which == 2) {
            const double PC[3] = {P[0] - xyz[3 * c], P[1] - xyz[3 * c + 1], P[2] - xyz[3 * c + 2]};
            hermite_r(A.L + B.L, p, PC, W);
            vpref = -(double)Z[c] * 2.0 * M_PI / p;
        }
        for (int x = 0; x < nca; ++x) {
            const unsigned char *ax = qc_md_cart(A.L, x);
            const int ai[3] = {ax[0], ax[1], ax[2]};
            for (int y = 0; y < ncb; ++y) {
                const unsigned char *by = qc_md_cart(B.L, y);
                const int bi[3] = {by[0], by[1], by[2]};
                double val;
                if (which == 0) val = qc_md_ovl(E, ai, bi, s3);
                else if (which == 1) val = -0.5 * s3 * qc_md_kin(E, ai, bi, eb);
                else val = vpref * qc_md_nuc(E, ai, bi, W[0]);
                (void)__builtin_amdgcn_ds_atomic_fadd_f64((lds_double *)&cart[x * ncb + y], cc * val);
            }
        }
    }
    __syncthreads();
    // Cartesian -> the shells' functions (solid harmonics or scaled monomials), both triangles
    const double *Ta = Tm + A.toff, *Tb = Tm + B.toff;
    for (int f = lane; f < A.nfunc * B.nfunc; f += 64) {
        const int fa = f / B.nfunc, fb = f - fa * B.nfunc;
        if (a == b && fb > fa) continue;                   // diagonal blocks: one triangle, mirrored (exactly symmetric output)
        double v = 0.0;
        for (int x = 0; x < nca; ++x)
            for (int y = 0; y < ncb; ++y) v += Ta[fa * nca + x] * Tb[fb * ncb + y] * cart[x * ncb + y];
        out[(size_t)(A.off + fa) * n + B.off + fb] = v;
        out[(size_t)(B.off + fb) * n + A.off + fa] = v;
    }
}

// Dipole matrices out[k * n * n + ..] = <a| (r - O)_k |b>, k = x, y, z, in one launch: the same wave-per-shell-pair shape, the lanes share
// out the primitive pairs and add into three Cartesian LDS blocks; the three components share the E tables (j <= L_b, t <= 1 is read).
__global__ __launch_bounds__(64) void qc_dipole_kernel(int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                       const double *__restrict__ coefs, const double *__restrict__ Tm, double ox, double oy, double oz,
                                                       int n, double *__restrict__ out) {
    __shared__ double cart[3 * MAXC * MAXC];
    int a = 0, rem = blockIdx.x;
    while (rem > a) { rem -= a + 1; ++a; }
    const int b = rem;
    if (a >= nshells) return;
    const QcDevShell A = sh[a], B = sh[b];
    const int lane = threadIdx.x, nca = A.ncart, ncb = B.ncart;
    for (int i = lane; i < 3 * MAXC * MAXC; i += 64) cart[i] = 0.0;
    __syncthreads();
    const double O[3] = {ox, oy, oz};
    const int npp = A.nprim * B.nprim;
    for (int pp = lane; pp < npp; pp += 64) {
        const int i = pp / B.nprim, j = pp - i * B.nprim;
        const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb, cc = coefs[A.poff + i] * coefs[B.poff + j];
        double PO[3];
        for (int k = 0; k < 3; ++k) PO[k] = (ea * A.A[k] + eb * B.A[k]) / p - O[k];
        E1 E[3];
        for (int k = 0; k < 3; ++k) E[k].fill(A.L, B.L, ea, eb, A.A[k] - B.A[k]);
        const double s3 = pow(M_PI / p, 1.5);
        for (int x = 0; x < nca; ++x) {
            const unsigned char *ax = qc_md_cart(A.L, x);
            const int ai[3] = {ax[0], ax[1], ax[2]};
            for (int y = 0; y < ncb; ++y) {
                const unsigned char *by = qc_md_cart(B.L, y);
                const int bi[3] = {by[0], by[1], by[2]};
                for (int k = 0; k < 3; ++k)
                    (void)__builtin_amdgcn_ds_atomic_fadd_f64((lds_double *)&cart[(k * MAXC + x) * MAXC + y], cc * qc_md_dip(E, ai, bi, k, PO[k], s3));
            }
        }
    }
    __syncthreads();
    // Cartesian -> the shells' functions, both triangles, as above
    const double *Ta = Tm + A.toff, *Tb = Tm + B.toff;
    const size_t nn = (size_t)n * n;
    for (int f = lane; f < 3 * A.nfunc * B.nfunc; f += 64) {
        const int k = f / (A.nfunc * B.nfunc), fab = f - k * A.nfunc * B.nfunc, fa = fab / B.nfunc, fb = fab - fa * B.nfunc;
        if (a == b && fb > fa) continue;
        double v = 0.0;
        for (int x = 0; x < nca; ++x)
            for (int y = 0; y < ncb; ++y) v += Ta[fa * nca + x] * Tb[fb * ncb + y] * cart[(k * MAXC + x) * MAXC + y];
        out[k * nn + (size_t)(A.off + fa) * n + B.off + fb] = v;
        out[k * nn + (size_t)(B.off + fb) * n + A.off + fa] = v;
    }
}

// Cartesian multipole matrices out[c * n * n + ..] = <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b>, the count = qc_nherm(order) components of
// qc_md_mom_comp in one launch: the shape of the dipole kernel with `count` Cartesian LDS blocks (dynamic: count x 10 x 10 doubles, 28 KB at
// order 4).  Per primitive pair the Hermite moments of the three axes, per Cartesian pair the 1-D factors of every power - shared by all
// components.
__global__ __launch_bounds__(64) void qc_multipole_kernel(int nshells, int order, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                          const double *__restrict__ coefs, const double *__restrict__ Tm, double ox, double oy, double oz,
                                                          int n, double *__restrict__ out) {
    extern __shared__ double mcart[];
    constexpr int W = QC_MOM_MAX + 1;
    int a = 0, rem = blockIdx.x;
    while (rem > a) { rem -= a + 1; ++a; }
    const int b = rem;
    if (a >= nshells) return;
    const QcDevShell A = sh[a], B = sh[b];
    const int lane = threadIdx.x, nca = A.ncart, ncb = B.ncart, count = qc_nherm(order);
    for (int i = lane; i < count * MAXC * MAXC; i += 64) mcart[i] = 0.0;
    __syncthreads();
    const double O[3] = {ox, oy, oz};
    const int npp = A.nprim * B.nprim;
    for (int pp = lane; pp < npp; pp += 64) {
        const int i = pp / B.nprim, j = pp - i * B.nprim;
        const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb, cc = coefs[A.poff + i] * coefs[B.poff + j];
        E1 E[3];
        double M[3][W * W];
        for (int k = 0; k < 3; ++k) {
            E[k].fill(A.L, B.L, ea, eb, A.A[k] - B.A[k]);
            qc_md_mom_herm(order, (ea * A.A[k] + eb * B.A[k]) / p - O[k], p, M[k]);
        }
        const double s3 = pow(M_PI / p, 1.5);
        for (int x = 0; x < nca; ++x) {
            const unsigned char *ax = qc_md_cart(A.L, x);
            for (int y = 0; y < ncb; ++y) {
                const unsigned char *by = qc_md_cart(B.L, y);
                double F[3][W];
                for (int k = 0; k < 3; ++k) qc_md_mom_1d(E[k], ax[k], by[k], order, M[k], F[k]);
                for (int c = 0; c < count; ++c) {
                    const unsigned char *m = qc_md_mom_comp(c);
                    (void)__builtin_amdgcn_ds_atomic_fadd_f64((lds_double *)&mcart[(c * MAXC + x) * MAXC + y], cc * (s3 * F[0][m[0]] * F[1][m[1]] * F[2][m[2]]));
                }
            }
        }
    }
    __syncthreads();
    // Cartesian -> the shells' functions, both triangles, as above
    const double *Ta = Tm + A.toff, *Tb = Tm + B.toff;
    const size_t nn = (size_t)n * n;
    for (int f = lane; f < count * A.nfunc * B.nfunc; f += 64) {
        const int c = f / (A.nfunc * B.nfunc), fab = f - c * A.nfunc * B.nfunc, fa = fab / B.nfunc, fb = fab - fa * B.nfunc;
        if (a == b && fb > fa) continue;
        double v = 0.0;
        for (int x = 0; x < nca; ++x)
            for (int y = 0; y < ncb; ++y) v += Ta[fa * nca + x] * Tb[fb * ncb + y] * mcart[(c * MAXC + x) * MAXC + y];
        out[c * nn + (size_t)(A.off + fa) * n + B.off + fb] = v;
        out[c * nn + (size_t)(B.off + fb) * n + A.off + fa] = v;
    }
}

}  // namespace

// The handle's shell blob: uploaded at the first call, in one allocation and one copy; a failure leaves the handle without one.
int qc_shell_blob(qc_system *S, const QcShellBlob **out) {
    if (!S->shell_blob) {
        std::vector<QcDevShell> hs(S->nshells);
        std::vector<double> ex, co, tm;
        std::vector<int> cshell;
        for (int s = 0; s < S->nshells; ++s) {
            const QcShell &q = S->shells[s];
            QcDevShell d{};
            for (int k = 0; k < 3; ++k) d.A[k] = q.A[k];
            d.L = q.L; d.nprim = q.nprim; d.ncart = q.ncart; d.nfunc = q.nfunc; d.off = q.off; d.atom = q.atom;
            d.coff = (int)cshell.size(); d.poff = (int)ex.size(); d.toff = (int)tm.size();
            cshell.insert(cshell.end(), q.ncart, s);
            ex.insert(ex.end(), q.exps.begin(), q.exps.end());
            co.insert(co.end(), q.coefs.begin(), q.coefs.end());
            tm.insert(tm.end(), q.T.begin(), q.T.end());
            hs[s] = d;
        }
        // sections in 256-byte steps: [shells | exps | coefs | T | cshell | Z | xyz | aoff | flist]
        std::vector<unsigned char> host;
        auto put = [&host](const void *src, size_t bytes) {
            const size_t at = host.size();
            host.resize(at + ((bytes + 255) & ~(size_t)255));
            if (bytes) std::memcpy(host.data() + at, src, bytes);
            return at;
        };
        const size_t o_sh = put(hs.data(), hs.size() * sizeof(QcDevShell)), o_ex = put(ex.data(), ex.size() * sizeof(double));
        const size_t o_co = put(co.data(), co.size() * sizeof(double)), o_tm = put(tm.data(), tm.size() * sizeof(double));
        const size_t o_cs = put(cshell.data(), cshell.size() * sizeof(int)), o_z = put(S->Z.data(), S->Z.size() * sizeof(int));
        const size_t o_x = put(S->xyz.data(), S->xyz.size() * sizeof(double));
        // the basis functions of each atom, ascending: atom A owns flist[aoff[A] .. aoff[A + 1])  (population analysis)
        std::vector<int> aoff(S->natoms + 1, 0), flist;
        for (int at = 0; at < S->natoms; ++at) {
            for (const QcShell &q : S->shells)
                if (q.atom == at) for (int f = 0; f < q.nfunc; ++f) flist.push_back(q.off + f);
            aoff[at + 1] = (int)flist.size();
        }
        const size_t o_ao = put(aoff.data(), aoff.size() * sizeof(int)), o_fl = put(flist.data(), flist.size() * sizeof(int));
        std::unique_ptr<QcShellBlob> B(new QcShellBlob{});
        if (B->mem.alloc(host.size()) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemcpy(B->mem.p, host.data(), host.size(), hipMemcpyHostToDevice));
        const unsigned char *m = B->mem.p;
        B->sh = reinterpret_cast<const QcDevShell *>(m + o_sh);
        B->exps = reinterpret_cast<const double *>(m + o_ex); B->coefs = reinterpret_cast<const double *>(m + o_co);
        B->T = reinterpret_cast<const double *>(m + o_tm); B->xyz = reinterpret_cast<const double *>(m + o_x);
        B->cshell = reinterpret_cast<const int *>(m + o_cs); B->Z = reinterpret_cast<const int *>(m + o_z);
        B->aoff = reinterpret_cast<const int *>(m + o_ao); B->flist = reinterpret_cast<const int *>(m + o_fl);
        B->nc = (int)cshell.size();
        S->shell_blob = B.release();
    }
    *out = S->shell_blob;
    return QC_OK;
}

// which: 0 overlap, 1 kinetic, 2 nuclear attraction; d_out: n x n device matrix
int qc_one_electron_device(qc_system *S, int which, double *d_out) {
    if (which < 0 || which > 2) return QC_ERR_INVALID;
    const QcShellBlob *B;
    const int rc = qc_shell_blob(S, &B);
    if (rc != QC_OK) return rc;
    const int npairs = S->nshells * (S->nshells + 1) / 2;
    hipLaunchKernelGGL(qc_one_electron_kernel, dim3(npairs), dim3(64), 0, S->stream, which, S->nshells, B->sh, B->exps, B->coefs, B->T, S->natoms, B->Z, B->xyz,
                       S->nbasis, d_out);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// origin: three doubles on the host; d_out: 3 n x n device matrices (x, y, z)
int qc_dipole_device(qc_system *S, const double *origin, double *d_out) {
    const QcShellBlob *B;
    const int rc = qc_shell_blob(S, &B);
    if (rc != QC_OK) return rc;
    const int npairs = S->nshells * (S->nshells + 1) / 2;
    hipLaunchKernelGGL(qc_dipole_kernel, dim3(npairs), dim3(64), 0, S->stream, S->nshells, B->sh, B->exps, B->coefs, B->T, origin[0], origin[1], origin[2],
                       S->nbasis, d_out);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// order 0 .. QC_MOM_MAX; origin: three doubles on the host; d_out: qc_nherm(order) n x n device matrices
int qc_multipole_device(qc_system *S, int order, const double *origin, double *d_out) {
    if (order < 0 || order > QC_MOM_MAX) return QC_ERR_INVALID;
    const QcShellBlob *B;
    const int rc = qc_shell_blob(S, &B);
    if (rc != QC_OK) return rc;
    const int npairs = S->nshells * (S->nshells + 1) / 2;
    const size_t lds = (size_t)qc_nherm(order) * MAXC * MAXC * sizeof(double);
    hipLaunchKernelGGL(qc_multipole_kernel, dim3(npairs), dim3(64), lds, S->stream, S->nshells, order, B->sh, B->exps, B->coefs, B->T, origin[0], origin[1],
                       origin[2], S->nbasis, d_out);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}
