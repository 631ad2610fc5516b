// qc_solvent.hip - the device side of the conductor-like continuum (the model: include/qchem_hip.h).
//   qc_solvent_s_kernel        S of the cavity: S_ii = zeta_i sqrt(2 / pi), S_ij = erf(zeta_ij r_ij) / r_ij; one thread per element of the
//                              lower triangle, which also stores the mirror: S is exactly symmetric
//   qc_solvent_reaction_kernel q = K (v_nuc + v_elec), 1/2 q.v_nuc, 1/2 q.v_elec and sum q in one launch, every sum in a fixed order
// K = -f S^-1 comes from qc_chol.hip once per cavity; the potential v_elec and the matrix V_R = -sum_i q_i A(s_i) from the point code
// (qc_points.hip) and the embedding code (qc_embed.hip), whose kernels take the surface elements as points and as charges.
#include <cmath>

#include "qc_embed.h"
#include "qc_md.h"
#include "qc_solvent.h"

namespace {

__global__ __launch_bounds__(256) void qc_solvent_s_kernel(int M, const double *__restrict__ xyz, const double *__restrict__ zeta, double *__restrict__ Smat) {
    if (blockIdx.x > blockIdx.y) return;                  // (tiles above the diagonal are written as mirrors)
    const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (r >= M || c > r) return;
    const double zr = zeta[r];
    if (c == r) { Smat[(size_t)r * M + r] = zr * sqrt(2.0 / M_PI); return; }
    const double zc = zeta[c];
    const double dx = xyz[3 * r] - xyz[3 * c], dy = xyz[3 * r + 1] - xyz[3 * c + 1], dz = xyz[3 * r + 2] - xyz[3 * c + 2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    const double zij = zr * zc / sqrt(zr * zr + zc * zc);
    const double s = erf(zij * d) / d;
    Smat[(size_t)r * M + c] = s;
    Smat[(size_t)c * M + r] = s;
}

// One wave per row of K, RX_ROWS rows per workgroup.  A lane sums its columns j = lane, lane + 64, ... in that order, the lanes are summed by
// the fixed butterfly of qc_wave_sum; a workgroup adds its rows' three products in row order into part[3 b ..]; the workgroup that
// arrives last adds the workgroups' sums - lane l those of b = l, l + 64, ..., then the butterfly - into out = {1/2 q.v_nuc, 1/2 q.v_elec,
// sum q}.  The arrival counter (zeroed by the launch function) decides only WHO adds, never in which order: the sums are the same bits
// whatever the order the workgroups run in.  The hand-off of `part` is an agent-scope release before the counter's add and an
// agent-scope acquire behind it in the last workgroup; nobody waits for anybody.
constexpr int RX_WAVES = 4, RX_ROWS = 16;
__global__ __launch_bounds__(64 * RX_WAVES) void qc_solvent_reaction_kernel(int M, const double *__restrict__ K, const double *__restrict__ v /* [v_nuc | v_elec] */,
                                                                            double *__restrict__ q, double *part, unsigned *cnt, double *__restrict__ out) {
    __shared__ double rows[RX_ROWS][3];
    __shared__ unsigned ticket;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
    const double *__restrict__ vn = v, *__restrict__ ve = v + M;
    for (int k = wave; k < RX_ROWS; k += RX_WAVES) {
        const int i = b * RX_ROWS + k;
        double s = 0.0;
        if (i < M) {
            const double *__restrict__ Ki = K + (size_t)i * M;
            for (int j = lane; j < M; j += 64) s = fma(Ki[j], vn[j] + ve[j], s);
        }
        s = qc_wave_sum(s);
        if (lane == 0) {
            if (i < M) { q[i] = s; rows[k][0] = s * vn[i]; rows[k][1] = s * ve[i]; rows[k][2] = s; }
            else rows[k][0] = rows[k][1] = rows[k][2] = 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double p[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < RX_ROWS; ++k) for (int c = 0; c < 3; ++c) p[c] += rows[k][c];
        for (int c = 0; c < 3; ++c) part[3 * (size_t)b + c] = p[c];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (ticket != gridDim.x - 1) return;                  // (uniform over the workgroup)
    if (wave != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double p[3] = {0.0, 0.0, 0.0};
    const unsigned long long *pw = reinterpret_cast<const unsigned long long *>(part);
    for (int g = lane; g < (int)gridDim.x; g += 64)
        for (int c = 0; c < 3; ++c) p[c] += __longlong_as_double((long long)__hip_atomic_load(pw + 3 * (size_t)g + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (int c = 0; c < 3; ++c) p[c] = qc_wave_sum(p[c]);
    if (lane == 0) { out[0] = 0.5 * p[0]; out[1] = 0.5 * p[1]; out[2] = p[2]; }
}

inline int rx_blocks(int64_t M) { return (int)((M + RX_ROWS - 1) / RX_ROWS); }

}  // namespace

int qc_solvent_matrix_device(qc_system *S, const QcSolvent &Q, double *dS) {
    const int M = (int)Q.M;
    hipStream_t st = S->stream;
    DevBuf dx, dz;
    if (dx.alloc(3 * (size_t)M) != QC_OK || dz.alloc(M) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dx.p, Q.xyz.data(), 3 * (size_t)M * sizeof(double), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dz.p, Q.zeta.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(qc_solvent_s_kernel, dim3((M + 15) / 16, (M + 15) / 16), dim3(256), 0, st, M, dx.p, dz.p, dS);
    QC_HIP_CHECK(hipStreamSynchronize(st));              // (the host vectors and the two buffers are read until here)
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// (a failure leaves the cavity without device buffers: the next call starts again from nothing)
static int solvent_prepare_buffers(qc_system *S, QcSolvent &Q) {
    const size_t M = (size_t)Q.M;
    DevBuf dS;
    if (dS.alloc(M * M) != QC_OK || Q.dK.alloc(M * M) != QC_OK || Q.dv.alloc(2 * M) != QC_OK || Q.dq.alloc(M) != QC_OK || Q.dout.alloc(4) != QC_OK ||
        Q.dpart.alloc(3 * (size_t)rx_blocks(Q.M)) != QC_OK || Q.dcnt.alloc(4) != QC_OK) return QC_ERR_HIP;
    int rc = qc_solvent_matrix_device(S, Q, dS.p);
    if (rc == QC_OK) rc = qc_spd_inverse_device(S, (int)M, dS.p, -Q.f, Q.dK.p);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(Q.dv.p, Q.vnuc.data(), M * sizeof(double), hipMemcpyHostToDevice, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    if (!Q.ev[0]) for (hipEvent_t &e : Q.ev) QC_HIP_CHECK(hipEventCreate(&e));
    return QC_OK;
}
int qc_solvent_prepare(qc_system *S, QcSolvent &Q) {
    if (Q.ready) return QC_OK;
    const double t0 = qc_now_ms();
    const int rc = solvent_prepare_buffers(S, Q);
    if (rc != QC_OK) {
        Q.dK.reset(); Q.dv.reset(); Q.dq.reset(); Q.dout.reset(); Q.dpart.reset(); Q.dcnt.reset();
        return rc;
    }
    Q.ms[0] = qc_now_ms() - t0;
    Q.ready = true;
    return QC_OK;
}

int qc_solvent_response_device(qc_system *S, QcSolvent &Q, const double *dD, double *q, double *v_elec, double *dV, double out3[3]) {
    int rc = qc_solvent_prepare(S, Q);
    if (rc != QC_OK) return rc;
    const size_t M = (size_t)Q.M;
    hipStream_t st = S->stream;
    // (the two drivers report their phase times on the handle: a solvated pass leaves those of the caller's own point and embedding calls alone)
    struct KeepTimes {
        qc_system *S; double points[4], pc[4];
        explicit KeepTimes(qc_system *S_) : S(S_) { std::memcpy(points, S->points_ms, sizeof points); std::memcpy(pc, S->pc_ms, sizeof pc); }
        ~KeepTimes() { std::memcpy(S->points_ms, points, sizeof points); std::memcpy(S->pc_ms, pc, sizeof pc); }
    } keep(S);
    std::vector<double> ve(M), pc(4 * M);
    double t0 = qc_now_ms();
    if ((rc = qc_points_esp_device(S, dD, Q.M, Q.xyz.data(), ve.data())) != QC_OK) return rc;
    Q.ms[1] = qc_now_ms() - t0;
    QC_HIP_CHECK(hipMemcpyAsync(Q.dv.p + M, ve.data(), M * sizeof(double), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemsetAsync(Q.dcnt.p, 0, 4 * sizeof(unsigned), st));
    QC_HIP_CHECK(hipEventRecord(Q.ev[0], st));
    hipLaunchKernelGGL(qc_solvent_reaction_kernel, dim3(rx_blocks(Q.M)), dim3(64 * RX_WAVES), 0, st, (int)M, Q.dK.p, Q.dv.p, Q.dq.p, Q.dpart.p, Q.dcnt.p, Q.dout.p);
    QC_HIP_CHECK(hipEventRecord(Q.ev[1], st));
    std::vector<double> qh(M);
    QC_HIP_CHECK(hipMemcpyAsync(qh.data(), Q.dq.p, M * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipMemcpyAsync(out3, Q.dout.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return QC_ERR_HIP;
    float ms_kernel = 0.f;
    QC_HIP_CHECK(hipEventElapsedTime(&ms_kernel, Q.ev[0], Q.ev[1]));
    Q.ms[2] = ms_kernel;                                                     // (the kernel between two events: not its copies, not the wait)
    Q.ms[3] = 0.0;
    if (dV) {
        t0 = qc_now_ms();
        for (size_t i = 0; i < M; ++i) { for (int k = 0; k < 3; ++k) pc[4 * i + k] = Q.xyz[3 * i + k]; pc[4 * i + 3] = qh[i]; }
        if ((rc = qc_pc_matrix_device(S, pc, dV)) != QC_OK) return rc;        // V_R = -sum_i q_i A(s_i)
        Q.ms[3] = qc_now_ms() - t0;
    }
    if (q) std::copy(qh.begin(), qh.end(), q);
    if (v_elec) std::copy(ve.begin(), ve.end(), v_elec);
    return QC_OK;
}

extern "C" {

int qc_solvent_matrix_gpu(qc_system *S, double *Smat, double *Kmat) {
    if (!S || !S->solvent) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    QcSolvent &Q = *S->solvent;
    const size_t MM = (size_t)Q.M * Q.M;
    if (Smat) {
        DevBuf dS;
        if (dS.alloc(MM) != QC_OK) return QC_ERR_HIP;
        if ((rc = qc_solvent_matrix_device(S, Q, dS.p)) != QC_OK) return rc;
        QC_HIP_CHECK(hipMemcpy(Smat, dS.p, MM * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (Kmat) {
        if ((rc = qc_solvent_prepare(S, Q)) != QC_OK) return rc;
        QC_HIP_CHECK(hipMemcpy(Kmat, Q.dK.p, MM * sizeof(double), hipMemcpyDeviceToHost));
    }
    return QC_OK;
}

int qc_solvent_response(qc_system *S, const double *D, double *q, double *V, double energy[2]) {
    if (!S || !D || !energy || !S->solvent) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    DevBuf dD, dV;
    if (dD.alloc(nn) != QC_OK || (V && dV.alloc(nn) != QC_OK)) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dD.p, D, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    double out3[3];
    if ((rc = qc_solvent_response_device(S, *S->solvent, dD.p, q, nullptr, dV.p, out3)) != QC_OK) return rc;
    energy[0] = out3[0]; energy[1] = out3[1];
    if (V) QC_HIP_CHECK(hipMemcpy(V, dV.p, nn * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}

}  // extern "C"
