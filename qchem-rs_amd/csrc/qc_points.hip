// qc_points.hip - the wave function in space: basis functions, density, orbitals and the electrostatic potential on caller-given points
// (DESIGN.md 3.11).  Not in the reference.  Lane = point throughout, 256 points per workgroup, no atomics anywhere.
//   rho(r)    = sum_ab D_ab phi_a(r) phi_b(r)          Phi (function-major) -> Y = D Phi (qc_gemm) -> column dots
//   psi_k(r)  = sum_a C_ak phi_a(r)                    Phi -> C^T Phi (qc_gemm)
//   v_elec(r) = -sum_ab D_ab (a| 1/|r' - r| |b)        the J-engine way: Hermite densities of the stored primitive pairs once per call
//                                                      (qc_esp_hermite_kernel), then per point and record Boys + R_tuv + a dot
//                                                      (qc_esp_points_kernel<L>, tables in registers, records broadcast from LDS)
// Every value of a point is a fixed-order sum that no other point of the call enters, so results do not depend on how the points are
// batched.  The host model's versions of the first and of the point-potential matrix (no device): qc_host_basis_on_points /
// qc_host_potential_matrix in qc_system.cpp.
#include <algorithm>
#include <cstdlib>
#include <utility>

#include "qc_esp.h"

namespace {

constexpr int PT_WG = 256;                 // points per workgroup
constexpr int PT_SPLIT_MAX = 4096;         // batches of at most this many points split the record list over gridDim.y (qc_points_esp_device) ...
constexpr size_t PT_SPLIT_WORDS = (size_t)1 << 25;   // ... as long as their tile sums fit into this many doubles (256 MB)
constexpr int64_t PT_BATCH_CAP = 1 << 20;  // points of a batch at the most (whatever hipMemGetInfo allows)

// ---- basis functions: Phi[a * B + k] = phi_a(r_k).  Per shell the contracted radial part, the monomials as running products
// (x^0 = 1 at a point on the centre without pow), the rows of the shell's transform.
template <int L>
__device__ __forceinline__ void shell_on_point(const QcDevShell &S, const double *__restrict__ Tm, double dx, double dy, double dz, double radial,
                                               int B, double *__restrict__ out /* Phi + S.off * B + k */) {
    constexpr int NC = qc_ncart(L);
    double px[L + 1], py[L + 1], pz[L + 1];
    px[0] = py[0] = pz[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= L; ++i) { px[i] = px[i - 1] * dx; py[i] = py[i - 1] * dy; pz[i] = pz[i - 1] * dz; }
    double mono[NC];
#pragma unroll
    for (int x = 0; x < NC; ++x) {
        const unsigned char *c = qc_md_cart(L, x);         // (constants once the loop is unrolled)
        mono[x] = px[c[0]] * py[c[1]] * pz[c[2]] * radial;
    }
    const double *__restrict__ T = Tm + S.toff;
    for (int f = 0; f < S.nfunc; ++f) {
        double v = 0.0;
#pragma unroll
        for (int x = 0; x < NC; ++x) v += T[f * NC + x] * mono[x];
        out[(size_t)f * B] = v;
    }
}

__global__ __launch_bounds__(PT_WG) void qc_basis_points_kernel(int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                                const double *__restrict__ coefs, const double *__restrict__ Tm, int B,
                                                                const double *__restrict__ xyz, double *__restrict__ Phi) {
    const int k = blockIdx.x * PT_WG + threadIdx.x;
    if (k >= B) return;                                    // the partial last workgroup (no barrier in this kernel)
    const double rx = xyz[3 * (size_t)k], ry = xyz[3 * (size_t)k + 1], rz = xyz[3 * (size_t)k + 2];
    for (int s = 0; s < nshells; ++s) {
        const QcDevShell S = sh[s];
        const double dx = rx - S.A[0], dy = ry - S.A[1], dz = rz - S.A[2], r2 = dx * dx + dy * dy + dz * dz;
        double radial = 0.0;
        for (int i = 0; i < S.nprim; ++i) radial += coefs[S.poff + i] * exp(-exps[S.poff + i] * r2);
        double *out = Phi + (size_t)S.off * B + k;
        switch (S.L) {
            case 0: shell_on_point<0>(S, Tm, dx, dy, dz, radial, B, out); break;
            case 1: shell_on_point<1>(S, Tm, dx, dy, dz, radial, B, out); break;
            case 2: shell_on_point<2>(S, Tm, dx, dy, dz, radial, B, out); break;
            default: shell_on_point<3>(S, Tm, dx, dy, dz, radial, B, out); break;
        }
    }
}

// rho_k = sum_a Phi[a][k] Y[a][k], a ascending
__global__ __launch_bounds__(PT_WG) void qc_points_rowdot_kernel(int n, int B, const double *__restrict__ Phi, const double *__restrict__ Y,
                                                                 double *__restrict__ rho) {
    const int k = blockIdx.x * PT_WG + threadIdx.x;
    if (k >= B) return;
    double acc = 0.0;
    for (int a = 0; a < n; ++a) acc += Phi[(size_t)a * B + k] * Y[(size_t)a * B + k];
    rho[k] = acc;
}

// ---- Hermite densities (the rescaling of the stored blocks: ESP_RESCALE, qc_esp.h).  The records carry MINUS Lambda, so that
// v_elec = sum_h rec_h R_h.
// One workgroup per stored shell pair A >= B; item (primitive pair, word of its record) per lane, every Lambda_h one sequential sum over
// ab.  D need not be symmetric: an off-diagonal pair takes D_ab + D_ba (= 2 D_ab for a symmetric D, exactly), a diagonal pair's block
// holds both orders itself.
__global__ __launch_bounds__(64) void qc_esp_hermite_kernel(const QcPairDesc *__restrict__ pairs, const double *__restrict__ pairdata,
                                                            const int *__restrict__ recstart, const EspGroups g, int n, const double *__restrict__ D,
                                                            double *__restrict__ rec) {
    __shared__ double Dab[100];
    const QcPairDesc d = pairs[blockIdx.x];
    const int lane = threadIdx.x, nab = d.na * d.nb;
    for (int i = lane; i < nab; i += 64) {
        const int fa = i / d.nb, fb = i - fa * d.nb;
        const double dab = D[(size_t)(d.offa + fa) * n + d.offb + fb];
        Dab[i] = d.shA_eq_shB ? dab : dab + D[(size_t)(d.offb + fb) * n + d.offa + fa];
    }
    __syncthreads();
    const int nh = qc_nherm(d.L), RL = 4 + nh, stride = qc_pair_stride(d.L, nab);
    double *__restrict__ out = rec + g.off[d.L] + (size_t)recstart[blockIdx.x] * RL;
    for (int item = lane; item < d.K * RL; item += 64) {
        const int kp = item / RL, j = item - kp * RL;
        const double *__restrict__ blk = pairdata + d.doff + (size_t)kp * stride;
        if (j < 4) { out[item] = blk[j]; continue; }
        const double *__restrict__ E = blk + 4 + (size_t)(j - 4) * nab;
        double s = 0.0;
        for (int ab = 0; ab < nab; ++ab) s += E[ab] * Dab[ab];
        out[item] = -ESP_RESCALE * s;
    }
}

// ---- the potential: the table R^0_tuv of a (record, point) by the compile-time plan of qc_esp.h, records in LDS tiles of esp_tile(L)
// v[k] += sum over the records of order L.  The sum of a point is  (((v + c_0) + c_1) + ...)  over the tiles' sums c_i, each tile summed
// from zero in list order: the same additions whether one workgroup walks all tiles (partial == null, gridDim.y = 1) or the tiles are
// spread over gridDim.y and qc_esp_sum_kernel adds their sums afterwards in the same order (few points: the chip would starve).
template <int L>
__global__ __launch_bounds__(PT_WG) void qc_esp_points_kernel(int nrec, const double *__restrict__ rec, const double *__restrict__ boys, int B,
                                                              const double *__restrict__ xyz, double *__restrict__ v, double *__restrict__ partial,
                                                              int tile0) {
    constexpr int NH = qc_nherm(L), RL = 4 + NH, TR = esp_tile(L);
    __shared__ double tile[TR * RL];
    const int k = blockIdx.x * PT_WG + threadIdx.x;
    const bool live = k < B;                               // (lanes past the end of the partial last workgroup stage tiles and store nothing)
    const double rx = live ? xyz[3 * (size_t)k] : 0.0, ry = live ? xyz[3 * (size_t)k + 1] : 0.0, rz = live ? xyz[3 * (size_t)k + 2] : 0.0;
    const int ntiles = (nrec + TR - 1) / TR;
    double total = (!partial && live) ? v[k] : 0.0;
    for (int c = blockIdx.y; c < ntiles; c += gridDim.y) {
        const int r0 = c * TR, nr = min(TR, nrec - r0);
        __syncthreads();
        for (int i = threadIdx.x; i < nr * RL; i += PT_WG) tile[i] = rec[(size_t)r0 * RL + i];
        __syncthreads();
        double acc = 0.0;
        for (int r = 0; r < nr; ++r) {
            const double *q = tile + r * RL;               // the same address in every lane: a broadcast
            const double p = q[0];
            const double X[3] = {q[1] - rx, q[2] - ry, q[3] - rz};
            double F[L + 1], seed[L + 1], R[NH];
            qc_boys<L>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), boys, F);
            double f = 1.0;
#pragma unroll
            for (int m = 0; m <= L; ++m) { seed[m] = f * F[m]; f *= -2.0 * p; }
            esp_rtable<L>(R, seed, X, std::make_integer_sequence<int, qc_rwork(L)>{});
#pragma unroll
            for (int h = 0; h < NH; ++h) acc += q[4 + h] * R[h];
        }
        if (partial) { if (live) partial[(size_t)(tile0 + c) * B + k] = acc; }
        else total += acc;
    }
    if (!partial && live) v[k] = total;
}

__global__ __launch_bounds__(PT_WG) void qc_esp_sum_kernel(int ntiles, int B, const double *__restrict__ partial, double *__restrict__ v) {
    const int k = blockIdx.x * PT_WG + threadIdx.x;
    if (k >= B) return;
    double total = v[k];
    for (int c = 0; c < ntiles; ++c) total += partial[(size_t)c * B + k];
    v[k] = total;
}

template <int L>
void esp_launch(hipStream_t st, dim3 grid, int nrec, const double *rec, const double *boys, int B, const double *xyz, double *v, double *partial, int tile0) {
    hipLaunchKernelGGL(qc_esp_points_kernel<L>, grid, dim3(PT_WG), 0, st, nrec, rec, boys, B, xyz, v, partial, tile0);
}

// Points of a batch: what a quarter of the free device memory holds at `doubles_per_point`, a multiple of the workgroup, within
// [256, PT_BATCH_CAP].  QC_POINTS_BATCH=<points> (a test switch, read once per handle at its first point call) replaces it.
// QC_POINTS_SPLIT=<points> (read with it) replaces PT_SPLIT_MAX; 0: the potential never splits its record list.
int64_t batch_points(qc_system *S, int64_t npts, size_t doubles_per_point) {
    if (S->points_batch < 0) {
        const char *e = getenv("QC_POINTS_BATCH"), *sp = getenv("QC_POINTS_SPLIT");
        S->points_batch = e ? std::max(0L, atol(e)) : 0;
        S->points_split = sp ? std::max(0L, atol(sp)) : PT_SPLIT_MAX;
    }
    if (S->points_batch > 0) return std::min<int64_t>(npts, S->points_batch);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 30;
    int64_t b = (int64_t)(free_b / 4 / (8 * doubles_per_point));
    b = std::max<int64_t>(PT_WG, std::min<int64_t>(PT_BATCH_CAP, b / PT_WG * PT_WG));
    return std::min(npts, b);
}

int launch_basis(qc_system *S, const QcShellBlob *Bl, int nb, const double *dxyz, double *Phi) {
    hipLaunchKernelGGL(qc_basis_points_kernel, dim3((nb + PT_WG - 1) / PT_WG), dim3(PT_WG), 0, S->stream, S->nshells, Bl->sh, Bl->exps, Bl->coefs, Bl->T,
                       nb, dxyz, Phi);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

}  // namespace

// rho on npts > 0 host points from a device density (n x n); the caller has checked the arguments
int qc_points_density_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *rho) {
    const int n = S->nbasis;
    const QcShellBlob *Bl;
    int rc = qc_shell_blob(S, &Bl);
    if (rc != QC_OK) return rc;
    const int64_t bmax = batch_points(S, npts, 2 * (size_t)n + 4);
    DevBuf dxyz, Phi, Y, dr;
    if (dxyz.alloc(3 * bmax) != QC_OK || Phi.alloc((size_t)n * bmax) != QC_OK || Y.alloc((size_t)n * bmax) != QC_OK || dr.alloc(bmax) != QC_OK) return QC_ERR_HIP;
    PhaseClock clk(S->points_ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    hipStream_t st = S->stream;
    for (int64_t k0 = 0; k0 < npts; k0 += bmax) {
        const int nb = (int)std::min(bmax, npts - k0);
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dxyz.p, xyz + 3 * k0, 3 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        clk.mark(1, st);
        if ((rc = launch_basis(S, Bl, nb, dxyz.p, Phi.p)) != QC_OK) return rc;
        clk.mark(2, st);
        qc_gemm(st, n, nb, n, 1.0, dD, n, false, Phi.p, nb, false, 0.0, Y.p, nb);
        hipLaunchKernelGGL(qc_points_rowdot_kernel, dim3((nb + PT_WG - 1) / PT_WG), dim3(PT_WG), 0, st, n, nb, Phi.p, Y.p, dr.p);
        clk.mark(3, st);
        QC_HIP_CHECK(hipMemcpyAsync(rho + k0, dr.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        clk.mark(4, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        clk.add(0, 4);
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// out[j * npts + k] = sum_a C[a * ldc + j] phi_a(r_k), j < m: columns of a device matrix (n rows, leading dimension ldc)
int qc_points_orbitals_device(qc_system *S, int m, const double *dC, int ldc, int64_t npts, const double *xyz, double *out) {
    const int n = S->nbasis;
    const QcShellBlob *Bl;
    int rc = qc_shell_blob(S, &Bl);
    if (rc != QC_OK) return rc;
    const int64_t bmax = batch_points(S, npts, (size_t)n + m + 4);
    DevBuf dxyz, Phi, Y;
    if (dxyz.alloc(3 * bmax) != QC_OK || Phi.alloc((size_t)n * bmax) != QC_OK || Y.alloc((size_t)m * bmax) != QC_OK) return QC_ERR_HIP;
    PhaseClock clk(S->points_ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    hipStream_t st = S->stream;
    for (int64_t k0 = 0; k0 < npts; k0 += bmax) {
        const int nb = (int)std::min(bmax, npts - k0);
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dxyz.p, xyz + 3 * k0, 3 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        clk.mark(1, st);
        if ((rc = launch_basis(S, Bl, nb, dxyz.p, Phi.p)) != QC_OK) return rc;
        clk.mark(2, st);
        qc_gemm(st, m, nb, n, 1.0, dC, ldc, true, Phi.p, nb, false, 0.0, Y.p, nb);
        clk.mark(3, st);
        QC_HIP_CHECK(hipMemcpy2DAsync(out + k0, (size_t)npts * sizeof(double), Y.p, (size_t)nb * sizeof(double), (size_t)nb * sizeof(double), m,
                                      hipMemcpyDeviceToHost, st));
        clk.mark(4, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        clk.add(0, 4);
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// records of each pair order L = 0..6 of the handle's stored primitive pairs (host model only)
void qc_esp_record_counts(const qc_system *S, int64_t counts[QC_LPAIR + 1]) {
    for (int L = 0; L <= QC_LPAIR; ++L) counts[L] = 0;
    for (const QcPairDesc &d : S->pairs) counts[d.L] += d.K;
}

// the records of dD (EspRecords, qc_esp.h)
int EspRecords::build(qc_system *S, const double *dD, PhaseClock &clk) {
    const int n = S->nbasis, npairs = (int)S->pairs.size();
    qc_esp_record_counts(S, cnt);
    size_t words = 0;
    tiles_all = 0;
    for (int L = 0; L <= QC_LPAIR; ++L) {
        g.off[L] = (long long)words; words += (size_t)cnt[L] * (4 + qc_nherm(L));
        tile0[L] = tiles_all; ntiles[L] = (int)((cnt[L] + esp_tile(L) - 1) / esp_tile(L)); tiles_all += ntiles[L];
    }
    std::vector<int> recstart(npairs);
    { int64_t run[QC_LPAIR + 1] = {}; for (int i = 0; i < npairs; ++i) { recstart[i] = (int)run[S->pairs[i].L]; run[S->pairs[i].L] += S->pairs[i].K; } }
    QcDev<int> drs;
    if (rec.alloc(words) != QC_OK || drs.alloc(npairs) != QC_OK) return QC_ERR_HIP;
    hipStream_t st = S->stream;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    if (npairs > 0)
        hipLaunchKernelGGL(qc_esp_hermite_kernel, dim3(npairs), dim3(64), 0, st, S->dev.d_pairs.p, S->dev.d_pairdata.p, drs.p, g, n, dD, rec.p);
    clk.mark(2, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));                 // (recstart is read by the copy until here)
    clk.add(0, 2);
    return QC_OK;
}

// v_elec on npts > 0 host points from a device density; the device side of the handle is initialised (pair data, Boys tables)
int qc_points_esp_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *v_elec) {
    PhaseClock clk(S->points_ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    EspRecords E;
    int rc = E.build(S, dD, clk);
    if (rc != QC_OK) return rc;
    const DevBuf &rec = E.rec;
    const EspGroups &g = E.g;
    const int64_t *cnt = E.cnt;
    const int *ntiles = E.ntiles, *tile0 = E.tile0, tiles_all = E.tiles_all;
    const int64_t bmax = batch_points(S, npts, 8);
    // few points: the tiles go to workgroups of their own.  The largest batch that does so, and the most points such a batch has
    const int64_t split_max = std::min<int64_t>(S->points_split, (int64_t)(PT_SPLIT_WORDS / (size_t)std::max(tiles_all, 1)));
    const int64_t rem = npts % bmax, split_pts = bmax <= split_max ? bmax : (rem > 0 && rem <= split_max ? rem : 0);
    DevBuf dxyz, dv, partial;
    if (dxyz.alloc(3 * bmax) != QC_OK || dv.alloc(bmax) != QC_OK || partial.alloc((size_t)tiles_all * split_pts) != QC_OK) return QC_ERR_HIP;
    hipStream_t st = S->stream;
    for (int64_t k0 = 0; k0 < npts; k0 += bmax) {
        const int nb = (int)std::min(bmax, npts - k0);
        const bool split = nb <= split_pts;
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dxyz.p, xyz + 3 * k0, 3 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemsetAsync(dv.p, 0, (size_t)nb * sizeof(double), st));
        clk.mark(1, st);
        clk.mark(2, st);
        const int gx = (nb + PT_WG - 1) / PT_WG;
        for (int L = 0; L <= QC_LPAIR; ++L) {              // the seven groups in a fixed order, each adding into dv (or its tiles into `partial`)
            if (!cnt[L]) continue;
            const dim3 grid(gx, split ? std::min(ntiles[L], 65535) : 1);
            const double *r = rec.p + g.off[L];
            double *pp = split ? partial.p : nullptr;
            switch (L) {
                case 0: esp_launch<0>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                case 1: esp_launch<1>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                case 2: esp_launch<2>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                case 3: esp_launch<3>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                case 4: esp_launch<4>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                case 5: esp_launch<5>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
                default: esp_launch<6>(st, grid, (int)cnt[L], r, S->dev.d_boys.p, nb, dxyz.p, dv.p, pp, tile0[L]); break;
            }
        }
        if (split && tiles_all > 0) hipLaunchKernelGGL(qc_esp_sum_kernel, dim3(gx), dim3(PT_WG), 0, st, tiles_all, nb, partial.p, dv.p);
        clk.mark(3, st);
        QC_HIP_CHECK(hipMemcpyAsync(v_elec + k0, dv.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        clk.mark(4, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        clk.add(0, 1); clk.add(2, 4);
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// v_nuc(r) = sum_A Z_A / |r - R_A| on the host, plain IEEE division (a point on a nucleus: +inf)
void qc_points_vnuc(const qc_system *S, int64_t npts, const double *xyz, double *v) {
    for (int64_t k = 0; k < npts; ++k) {
        double s = 0.0;
        for (int a = 0; a < S->natoms; ++a) {
            const double dx = xyz[3 * k] - S->xyz[3 * a], dy = xyz[3 * k + 1] - S->xyz[3 * a + 1], dz = xyz[3 * k + 2] - S->xyz[3 * a + 2];
            s += (double)S->Z[a] / std::sqrt(dx * dx + dy * dy + dz * dz);
        }
        v[k] = s;
    }
}
