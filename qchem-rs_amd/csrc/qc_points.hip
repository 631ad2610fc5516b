// qc_points.hip - the wave function in space: basis functions, density, orbitals, the electrostatic potential and the electric field on
// caller-given points.  Not in the reference.  Lane = point throughout, 256 points per workgroup, no atomics anywhere.
//   rho(r)    = sum_ab D_ab phi_a(r) phi_b(r)          Phi (function-major) -> Y = D Phi (qc_gemm) -> column dots
//   psi_k(r)  = sum_a C_ak phi_a(r)                    Phi -> C^T Phi (qc_gemm)
//   v_elec(r) = -sum_ab D_ab (a| 1/|r' - r| |b)        the J-engine way: Hermite densities of the stored primitive pairs once per call
//                                                      (qc_esp_hermite_kernel), then per point and record Boys + R_tuv + a dot
//                                                      (qc_esp_walk_kernel<L, 1>, tables in registers, records broadcast from LDS)
//   e_elec(r) = -grad v_elec(r)                        the same walk with the table of order L + 1 and the dot shifted by one unit per
//                                                      axis (qc_esp_walk_kernel<L, 3>); one driver for both (points_walk_device)
// Every value of a point is a fixed-order sum that no other point of the call enters, so results do not depend on how the points are
// batched.  The host model's versions of the first and of the point-potential matrix (no device): qc_host_basis_on_points /
// qc_host_potential_matrix in qc_system.cpp.
#include <algorithm>
#include <cstdlib>
#include <utility>

#include "qc_esp.h"

namespace {

constexpr int PT_WG = 256;                 // points per workgroup
constexpr int PT_SPLIT_MAX = 4096;         // batches of at most this many points split the record list over gridDim.y (points_walk_device) ...
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
        esp_dispatch<QC_LMAX>(S.L, [&](auto Lc) { shell_on_point<decltype(Lc)::value>(S, Tm, dx, dy, dz, radial, B, out); });
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

// ---- the field's dot product: d/dr_x R_tuv(P - r) = -R_{t+1,u,v}, so E_x(r) = -dv/dr_x = sum_h rec_h R_{h + e_x}: the potential's dot
// product against the table of order L + 1, shifted by one unit per axis.  The shifted indices are a compile-time list like the table's plan.
struct FieldShift { short x, y, z; };
template <int L> struct FieldShiftTab { FieldShift s[qc_nherm(L)]; };
template <int L> constexpr FieldShiftTab<L> field_make_shift() {
    FieldShiftTab<L> T{};
    for (int N = 0; N <= L; ++N)
        for (int t = N; t >= 0; --t)
            for (int u = N - t; u >= 0; --u) {
                const int v = N - t - u;
                T.s[qc_hidx(t, u, v)] = FieldShift{(short)qc_hidx(t + 1, u, v), (short)qc_hidx(t, u + 1, v), (short)qc_hidx(t, u, v + 1)};
            }
    return T;
}
template <int L> inline constexpr FieldShiftTab<L> field_shift = field_make_shift<L>();
template <int L, int H>
__device__ __forceinline__ void field_term(const double (&R)[qc_nherm(L + 1)], double w, double (&a)[3]) {
    constexpr FieldShift s = field_shift<L>.s[H];
    a[0] += w * R[s.x]; a[1] += w * R[s.y]; a[2] += w * R[s.z];
}
template <int L, int... H>
__device__ __forceinline__ void field_dot(const double (&R)[qc_nherm(L + 1)], const double *q, double (&a)[3], std::integer_sequence<int, H...>) {
    (field_term<L, H>(R, q[4 + H], a), ...);
}

// ---- the record walk: out[x * B + k] += sum over the records of pair order L, x < NV values per point (1: v_elec, 3: e_elec); lane = point,
// the table R^0_tuv of a (record, point) by the compile-time plan of qc_esp.h, records broadcast from LDS tiles of esp_tile(L).  The sum of a
// point is  (((out + c_0) + c_1) + ...)  over the tiles' sums c_i, each tile summed from zero in list order: the same additions whether one
// workgroup walks all tiles (partial == null, gridDim.y = 1) or the tiles are spread over gridDim.y and esp_tile_sum adds their sums
// afterwards in the same order (few points: the chip would starve).  The tile sums and the output are component-major, so the potential
// is the one-component case of the field's stores.
template <int L, int NV>
__global__ __launch_bounds__(PT_WG) void qc_esp_walk_kernel(int nrec, const double *__restrict__ rec, const double *__restrict__ boys, int B,
                                                            const double *__restrict__ xyz, double *__restrict__ out, double *__restrict__ partial,
                                                            int tile0) {
    constexpr int RL = 4 + qc_nherm(L), TR = esp_tile(L);
    __shared__ double tile[TR * RL];
    const int k = blockIdx.x * PT_WG + threadIdx.x;
    const bool live = k < B;                               // (lanes past the end of the partial last workgroup stage tiles and store nothing)
    const double rx = live ? xyz[3 * (size_t)k] : 0.0, ry = live ? xyz[3 * (size_t)k + 1] : 0.0, rz = live ? xyz[3 * (size_t)k + 2] : 0.0;
    const int ntiles = (nrec + TR - 1) / TR;
    double total[NV] = {};
    if (!partial && live) {
#pragma unroll
        for (int x = 0; x < NV; ++x) total[x] = out[x * (size_t)B + k];
    }
    for (int c = blockIdx.y; c < ntiles; c += gridDim.y) {
        const int r0 = c * TR, nr = min(TR, nrec - r0);
        __syncthreads();
        for (int i = threadIdx.x; i < nr * RL; i += PT_WG) tile[i] = rec[(size_t)r0 * RL + i];
        __syncthreads();
        double acc[NV] = {};
        for (int r = 0; r < nr; ++r) {
            const double *q = tile + r * RL;               // the same address in every lane: a broadcast
            const double X[3] = {q[1] - rx, q[2] - ry, q[3] - rz};
            // The per-record step, the one thing in which the uses differ.  Both stay spelled out in the loop: moved into a function, or with
            // the potential's table through esp_table<L> (the statements below are its body), the compiler carries the Boys values of the
            // L = 6 potential as vectors, contracts other products, and v_elec moves in its last bits.
            if constexpr (NV == 1) {                       // the potential: the table of order L and the dot with the record
                const double p = q[0];
                double F[L + 1], seed[L + 1], R[qc_nherm(L)];
                qc_boys<L>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), boys, F);
                double f = 1.0;
#pragma unroll
                for (int m = 0; m <= L; ++m) { seed[m] = f * F[m]; f *= -2.0 * p; }
                esp_rtable<L>(R, seed, X, std::make_integer_sequence<int, qc_rwork(L)>{});
#pragma unroll
                for (int h = 0; h < qc_nherm(L); ++h) acc[0] += q[4 + h] * R[h];
            } else {                                       // the field: the table of order L + 1 and the shifted dot
                double R[qc_nherm(L + 1)];
                esp_table<L + 1>(q[0], X, boys, R);
                field_dot<L>(R, q, acc, std::make_integer_sequence<int, qc_nherm(L)>{});
            }
        }
        if (partial) {
            double *o = partial + (size_t)(tile0 + c) * NV * B + k;
            if (live) {
#pragma unroll
                for (int x = 0; x < NV; ++x) o[x * (size_t)B] = acc[x];
            }
        } else {
#pragma unroll
            for (int x = 0; x < NV; ++x) total[x] += acc[x];
        }
    }
    if (!partial && live) {
#pragma unroll
        for (int x = 0; x < NV; ++x) out[x * (size_t)B + k] = total[x];
    }
}

__global__ __launch_bounds__(256) void qc_esp_tile_sum_kernel(size_t words, int ntiles, const double *__restrict__ partial, double *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    double t = out[i];
    for (int c = 0; c < ntiles; ++c) t += partial[(size_t)c * words + i];
    out[i] = t;
}

// Points of a batch: what a quarter of the free device memory holds at `doubles_per_point`, a multiple of the workgroup, within
// [256, PT_BATCH_CAP].  QC_POINTS_BATCH=<points> (a test switch, read once per handle at its first point call) replaces it.
// QC_POINTS_SPLIT=<points> (read with it) replaces PT_SPLIT_MAX; 0: the potential and the field never split their record list.
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

void esp_tile_sum(hipStream_t st, size_t words, int ntiles, const double *partial, double *out) {
    hipLaunchKernelGGL(qc_esp_tile_sum_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, words, ntiles, partial, out);
}

// records of each pair order L = 0..6 of the handle's stored primitive pairs (host model only)
void qc_esp_record_counts(const qc_system *S, int64_t counts[QC_LPAIR + 1]) {
    EspLayout lay;
    lay.stored_pairs(S, [](int) { return 0; });
    std::copy(lay.cnt, lay.cnt + QC_LPAIR + 1, counts);
}

// the records of dD (EspRecords, qc_esp.h)
int EspRecords::build(qc_system *S, const double *dD, PhaseClock &clk) {
    const int n = S->nbasis, npairs = (int)S->pairs.size();
    const std::vector<int> recstart = lay.stored_pairs(S, [](int L) { return 4 + qc_nherm(L); });
    tiles_all = 0;
    for (int L = 0; L <= QC_LPAIR; ++L) { tile0[L] = tiles_all; ntiles[L] = (int)((lay.cnt[L] + esp_tile(L) - 1) / esp_tile(L)); tiles_all += ntiles[L]; }
    QcDev<int> drs;
    if (rec.alloc(lay.words) != QC_OK || drs.alloc(npairs) != QC_OK) return QC_ERR_HIP;
    hipStream_t st = S->stream;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    if (npairs > 0)
        hipLaunchKernelGGL(qc_esp_hermite_kernel, dim3(npairs), dim3(64), 0, st, S->dev.d_pairs.p, S->dev.d_pairdata.p, drs.p, lay.g, n, dD, rec.p);
    clk.mark(2, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));                 // (recstart is read by the copy until here)
    clk.add(0, 2);
    return QC_OK;
}

namespace {

// NV values per point from the records of a device density on npts > 0 host points (v_elec: NV = 1; e_elec: NV = 3, point-major on the
// host); the device side of the handle is initialised (pair data, Boys tables); phase times into ms[4]
template <int NV>
int points_walk_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *out, double *ms) {
    PhaseClock clk(ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    EspRecords E;
    int rc = E.build(S, dD, clk);
    if (rc != QC_OK) return rc;
    const int64_t bmax = batch_points(S, npts, 8 * NV);
    // few points: the tiles go to workgroups of their own.  The largest batch that does so, and the most points such a batch has
    const int64_t split_max = std::min<int64_t>(S->points_split, (int64_t)(PT_SPLIT_WORDS / (NV * (size_t)std::max(E.tiles_all, 1))));
    const int64_t rem = npts % bmax, split_pts = bmax <= split_max ? bmax : (rem > 0 && rem <= split_max ? rem : 0);
    DevBuf dxyz, dv, partial;
    if (dxyz.alloc(3 * bmax) != QC_OK || dv.alloc(NV * bmax) != QC_OK || partial.alloc((size_t)E.tiles_all * NV * split_pts) != QC_OK) return QC_ERR_HIP;
    std::vector<double> hv(NV > 1 ? NV * (size_t)bmax : 0);   // a batch comes back component-major
    hipStream_t st = S->stream;
    for (int64_t k0 = 0; k0 < npts; k0 += bmax) {
        const int nb = (int)std::min(bmax, npts - k0), gx = (nb + PT_WG - 1) / PT_WG;
        const bool split = nb <= split_pts;
        double *pp = split ? partial.p : nullptr;
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dxyz.p, xyz + 3 * k0, 3 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemsetAsync(dv.p, 0, NV * (size_t)nb * sizeof(double), st));
        clk.mark(1, st);
        clk.mark(2, st);
        for (int L = 0; L <= QC_LPAIR; ++L) {              // the seven groups in a fixed order, each adding into dv (or its tiles into `partial`)
            if (!E.lay.cnt[L]) continue;
            const dim3 grid(gx, split ? std::min(E.ntiles[L], 65535) : 1);
            esp_dispatch<QC_LPAIR>(L, [&](auto Lc) {
                hipLaunchKernelGGL((qc_esp_walk_kernel<decltype(Lc)::value, NV>), grid, dim3(PT_WG), 0, st, (int)E.lay.cnt[L], E.rec.p + E.lay.g.off[L], S->dev.d_boys.p, nb,
                                   dxyz.p, dv.p, pp, E.tile0[L]);
            });
        }
        if (split && E.tiles_all > 0) esp_tile_sum(st, NV * (size_t)nb, E.tiles_all, partial.p, dv.p);
        clk.mark(3, st);
        QC_HIP_CHECK(hipMemcpyAsync(NV > 1 ? hv.data() : out + k0, dv.p, NV * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        clk.mark(4, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        clk.add(0, 1); clk.add(2, 4);
        if (NV > 1)
            for (int k = 0; k < nb; ++k)
                for (int x = 0; x < NV; ++x) out[NV * (k0 + k) + x] = hv[(size_t)x * nb + k];
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

}  // namespace

int qc_points_esp_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *v_elec) {
    return points_walk_device<1>(S, dD, npts, xyz, v_elec, S->points_ms);
}
int qc_points_field_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *e_elec, double *ms) {
    return points_walk_device<3>(S, dD, npts, xyz, e_elec, ms);
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
