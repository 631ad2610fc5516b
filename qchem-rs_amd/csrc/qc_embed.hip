// qc_embed.hip - point-charge embedding on the device.  Not in the reference.  No atomics anywhere: every sum has a
// fixed order.
//   Lambda_h(rec) = sum_c q_c R_h(p_rec, P_rec - R_c)      the adjoint of qc_esp_points_kernel: per stored primitive pair the Hermite-Coulomb
//                                                          tables of all charges, summed.  Charge tiles over gridDim.y in both orientations:
//                                                          qc_pc_lambda_kernel<LT>, lane = record, the charges read through the scalar cache -
//                                                          when its launches fill the chip; qc_pc_lambda_charge_kernel<LT>, lane = charge with
//                                                          a fixed reduction per entry - when they would not (lambda_build).  qc_pc_sum_kernel
//                                                          adds the tiles' sums in ascending order
//   V_pc,ab = -sum_rec sum_h E_h,ab(rec) Lambda_h(rec)     the adjoint of qc_esp_hermite_kernel, from the same pair data (qc_pc_assemble_kernel)
//   E_elec(r) = -grad v_elec(r)                            qc_esp_points_kernel at order L + 1, the dot product shifted by one unit per axis
//                                                          (qc_field_points_kernel<L>); the charges' gradient is -q_c E(R_c)
#include <algorithm>
#include <cstdlib>

#include "qc_embed.h"
#include "qc_esp.h"

namespace {

constexpr int PC_WG = 64;                  // records per workgroup of the Hermite sums: one wave
constexpr int PC_REG_NH = 56;              // tables up to this many entries (LT <= 5) keep their accumulators in registers, larger ones in LDS
constexpr size_t PC_PARTIAL_WORDS = (size_t)1 << 25;     // doubles of tile sums a batch of charges may take (256 MB)
constexpr int PC_BATCH_TILES = 1024;       // tiles of a batch at the most
constexpr int PC_CH_RECORDS = 16;          // records per workgroup of the lane = charge orientation
// lane = record is taken when the Hermite sums of ALL charges are at least this many waves of it, two per SIMD of the chip; below, its
// one-wave workgroups are latency chains of 256 tables each and lane = charge wins (measured, DESIGN.md 5: H2O / cc-pVTZ, 1 482 records,
// 10^4 charges = 1 080 waves: 0.83 against 0.47 ms; 10^5 = 10 557 waves: 1.07 against 1.90 ms; C6H6 / cc-pVDZ from 10^3 charges on: lane = record)
constexpr int64_t PC_FILL_WAVES = 2048;
constexpr int FD_WG = 256;                 // points per workgroup of the field
constexpr int FD_SPLIT_MAX = 4096;         // batches of at most this many points split the record list over gridDim.y, like the potential (PT_SPLIT_MAX) ...
constexpr size_t FD_SPLIT_WORDS = (size_t)1 << 25;   // ... as long as their tile sums fit into this many doubles

struct PcCounts { int n[QC_LPAIR + 1]; };

// partial[tile][goff + h * nrec + r] = sum over the charges of the tile, in list order from zero, of q_c R_h(p_r, P_r - R_c), h < nherm(LT).
// Lane = record r of the group (recoff: where its [p, P] header lies in the pair data); the charge index is the same in every lane, so a
// charge is four scalar loads.  Accumulators + table are 2 nherm(LT) doubles per lane: up to LT = 5 (112) both live in registers, beyond
// (168 at LT = 6, 240 at LT = 7) the accumulators are a column per lane in LDS - no lane reads another's, hence no barrier.
template <int LT>
__global__ __launch_bounds__(PC_WG) void qc_pc_lambda_kernel(int nrec, const int *__restrict__ recoff, const double *__restrict__ pairdata,
                                                             const double *__restrict__ boys, int npc, const double *__restrict__ pc,
                                                             double *__restrict__ partial, size_t words, size_t goff) {
    constexpr int NH = qc_nherm(LT);
    constexpr bool IN_LDS = NH > PC_REG_NH;
    __shared__ double sacc[IN_LDS ? NH * PC_WG : 1];
    const int lane = threadIdx.x, r = blockIdx.x * PC_WG + lane;
    const bool live = r < nrec;
    const double *hd = pairdata + (live ? recoff[r] : recoff[0]);
    const double p = hd[0], Px = hd[1], Py = hd[2], Pz = hd[3];
    const int c0 = blockIdx.y * QC_PC_TILE, c1 = min(npc, c0 + QC_PC_TILE);
    double acc[IN_LDS ? 1 : NH];
    if constexpr (IN_LDS) {
#pragma unroll
        for (int h = 0; h < NH; ++h) sacc[h * PC_WG + lane] = 0.0;
    } else {
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[h] = 0.0;
    }
    for (int c = c0; c < c1; ++c) {
        const double q = pc[4 * (size_t)c + 3];
        const double X[3] = {Px - pc[4 * (size_t)c], Py - pc[4 * (size_t)c + 1], Pz - pc[4 * (size_t)c + 2]};
        double R[NH];
        esp_table<LT>(p, X, boys, R);
        if constexpr (IN_LDS) {
#pragma unroll
            for (int h = 0; h < NH; ++h) sacc[h * PC_WG + lane] += q * R[h];
        } else {
#pragma unroll
            for (int h = 0; h < NH; ++h) acc[h] += q * R[h];
        }
    }
    if (!live) return;
    double *out = partial + (size_t)blockIdx.y * words + goff + r;
    if constexpr (IN_LDS) {
#pragma unroll
        for (int h = 0; h < NH; ++h) out[(size_t)h * nrec] = sacc[h * PC_WG + lane];
    } else {
#pragma unroll
        for (int h = 0; h < NH; ++h) out[(size_t)h * nrec] = acc[h];
    }
}

// lam[i] = ((lam[i] + t_0[i]) + t_1[i]) + ...: the tiles of a batch in ascending order, on top of the batches before it
__global__ __launch_bounds__(256) void qc_pc_sum_kernel(size_t words, int ntiles, const double *__restrict__ partial, double *__restrict__ lam) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    double t = lam[i];
    for (int c = 0; c < ntiles; ++c) t += partial[(size_t)c * words + i];
    lam[i] = t;
}

// One workgroup per stored shell pair A >= B, lane = element (a, b) of its block: the sum over the pair's primitive pairs and their Hermite
// functions in list order, from the pair data as stored (primitive cut-off, contraction, Cartesian-to-pure transform and all).  An element
// and its mirror are written from one value; a diagonal pair's block holds both orders itself: its lower triangle is computed.
__global__ __launch_bounds__(64) void qc_pc_assemble_kernel(const QcPairDesc *__restrict__ pairs, const double *__restrict__ pairdata,
                                                            const int *__restrict__ recstart, const EspGroups g, const PcCounts cnt, int n,
                                                            const double *__restrict__ lam, double *__restrict__ V) {
    const QcPairDesc d = pairs[blockIdx.x];
    const int nab = d.na * d.nb, nh = qc_nherm(d.L), stride = qc_pair_stride(d.L, nab), nrec = cnt.n[d.L];
    const double *__restrict__ L0 = lam + g.off[d.L] + recstart[blockIdx.x];
    for (int i = threadIdx.x; i < nab; i += 64) {
        const int fa = i / d.nb, fb = i - fa * d.nb;
        if (d.shA_eq_shB && fb > fa) continue;
        double s = 0.0;
        for (int kp = 0; kp < d.K; ++kp) {
            const double *__restrict__ E = pairdata + d.doff + (size_t)kp * stride + 4 + i;
            for (int h = 0; h < nh; ++h) s += E[(size_t)h * nab] * L0[(size_t)h * nrec + kp];
        }
        const double v = -ESP_RESCALE * s;
        V[(size_t)(d.offa + fa) * n + d.offb + fb] = v;
        V[(size_t)(d.offb + fb) * n + d.offa + fa] = v;
    }
}

// The other orientation, same output: lane = charge, one 256-lane workgroup per (charge tile, PC_CH_RECORDS records).  A record's header
// is the same in every lane (scalar loads), its table of nherm(LT) registers per lane has no accumulators next to it; per entry the
// lanes' q_c R_h are summed by a fixed butterfly over the wave and the four waves' sums in wave order through LDS: a fixed order too, but
// not the list order of qc_pc_lambda_kernel - the two orientations differ in the last bits, and which one runs is decided from the record
// and charge counts alone (lambda_build), never from the batching.  Lanes past the end of the charges carry q = 0.
template <int LT>
__global__ __launch_bounds__(QC_PC_TILE) void qc_pc_lambda_charge_kernel(int nrec, const int *__restrict__ recoff, const double *__restrict__ pairdata,
                                                                         const double *__restrict__ boys, int npc, const double *__restrict__ pc,
                                                                         double *__restrict__ partial, size_t words, size_t goff) {
    constexpr int NH = qc_nherm(LT);
    __shared__ double ws[QC_PC_TILE / 64][NH];
    const int c = blockIdx.y * QC_PC_TILE + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool live = c < npc;
    const double q = live ? pc[4 * (size_t)c + 3] : 0.0;
    const double cx = live ? pc[4 * (size_t)c] : 0.0, cy = live ? pc[4 * (size_t)c + 1] : 0.0, cz = live ? pc[4 * (size_t)c + 2] : 0.0;
    const int r1 = min(nrec, (int)(blockIdx.x + 1) * PC_CH_RECORDS);
    for (int r = blockIdx.x * PC_CH_RECORDS; r < r1; ++r) {
        const double *hd = pairdata + recoff[r];
        const double X[3] = {hd[1] - cx, hd[2] - cy, hd[3] - cz};
        double R[NH];
        esp_table<LT>(hd[0], X, boys, R);
        __syncthreads();                                   // (the previous record's sums have been read)
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            double v = q * R[h];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) ws[wave][h] = v;
        }
        __syncthreads();
        for (int h = threadIdx.x; h < NH; h += QC_PC_TILE)
            partial[(size_t)blockIdx.y * words + goff + (size_t)h * nrec + r] = ((ws[0][h] + ws[1][h]) + ws[2][h]) + ws[3][h];
    }
}

template <int LT>
void lambda_launch(hipStream_t st, bool by_charge, int nrec, int ntiles, const int *recoff, const double *pairdata, const double *boys, int npc,
                   const double *pc, double *partial, size_t words, size_t goff) {
    if (by_charge)
        hipLaunchKernelGGL(qc_pc_lambda_charge_kernel<LT>, dim3((nrec + PC_CH_RECORDS - 1) / PC_CH_RECORDS, ntiles), dim3(QC_PC_TILE), 0, st, nrec, recoff,
                           pairdata, boys, npc, pc, partial, words, goff);
    else
        hipLaunchKernelGGL(qc_pc_lambda_kernel<LT>, dim3((nrec + PC_WG - 1) / PC_WG, ntiles), dim3(PC_WG), 0, st, nrec, recoff, pairdata, boys, npc, pc,
                           partial, words, goff);
}

// ---- the field: d/dr_x R_tuv(P - r) = -R_{t+1,u,v}, so E_x(r) = -dv/dr_x = sum_h rec_h R_{h + e_x}: the potential's dot product against
// the table of order L + 1, shifted by one unit per axis.  The shifted indices are a compile-time list like the table's plan.
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

// e[x * B + k] += sum over the records of pair order L; lane = point, records broadcast from LDS tiles of esp_tile(L).  The sum of a point
// is (((e + c_0) + c_1) + ...) over the tiles' sums c_i, each tile summed from zero in list order: the same additions whether one workgroup
// walks all tiles (partial == null, gridDim.y = 1) or the tiles are spread over gridDim.y and qc_field_sum_kernel adds their sums
// afterwards in the same order (few points: the chip would starve) - the scheme of qc_esp_points_kernel.
template <int L>
__global__ __launch_bounds__(FD_WG) void qc_field_points_kernel(int nrec, const double *__restrict__ rec, const double *__restrict__ boys, int B,
                                                                const double *__restrict__ xyz, double *__restrict__ e, double *__restrict__ partial,
                                                                int tile0) {
    constexpr int NH = qc_nherm(L), RL = 4 + NH, TR = esp_tile(L);
    __shared__ double tile[TR * RL];
    const int k = blockIdx.x * FD_WG + threadIdx.x;
    const bool live = k < B;                               // (lanes past the end of the partial last workgroup stage tiles and store nothing)
    const double rx = live ? xyz[3 * (size_t)k] : 0.0, ry = live ? xyz[3 * (size_t)k + 1] : 0.0, rz = live ? xyz[3 * (size_t)k + 2] : 0.0;
    const int ntiles = (nrec + TR - 1) / TR;
    double total[3] = {0.0, 0.0, 0.0};
    if (!partial && live) { total[0] = e[k]; total[1] = e[(size_t)B + k]; total[2] = e[2 * (size_t)B + k]; }
    for (int c = blockIdx.y; c < ntiles; c += gridDim.y) {
        const int r0 = c * TR, nr = min(TR, nrec - r0);
        __syncthreads();
        for (int i = threadIdx.x; i < nr * RL; i += FD_WG) tile[i] = rec[(size_t)r0 * RL + i];
        __syncthreads();
        double acc[3] = {0.0, 0.0, 0.0};
        for (int r = 0; r < nr; ++r) {
            const double *q = tile + r * RL;               // the same address in every lane: a broadcast
            const double X[3] = {q[1] - rx, q[2] - ry, q[3] - rz};
            double R[qc_nherm(L + 1)];
            esp_table<L + 1>(q[0], X, boys, R);
            field_dot<L>(R, q, acc, std::make_integer_sequence<int, NH>{});
        }
        if (partial) {
            double *out = partial + (size_t)(tile0 + c) * 3 * B + k;
            if (live) { out[0] = acc[0]; out[(size_t)B] = acc[1]; out[2 * (size_t)B] = acc[2]; }
        } else {
            total[0] += acc[0]; total[1] += acc[1]; total[2] += acc[2];
        }
    }
    if (!partial && live) { e[k] = total[0]; e[(size_t)B + k] = total[1]; e[2 * (size_t)B + k] = total[2]; }
}
// e[j] = ((e[j] + t_0[j]) + t_1[j]) + ..., j < 3 B: all tiles of all groups in ascending order
__global__ __launch_bounds__(FD_WG) void qc_field_sum_kernel(int ntiles, int B3, const double *__restrict__ partial, double *__restrict__ e) {
    const int j = blockIdx.x * FD_WG + threadIdx.x;
    if (j >= B3) return;
    double total = e[j];
    for (int c = 0; c < ntiles; ++c) total += partial[(size_t)c * B3 + j];
    e[j] = total;
}
template <int L>
void field_launch(hipStream_t st, dim3 grid, int nrec, const double *rec, const double *boys, int B, const double *xyz, double *e, double *partial, int tile0) {
    hipLaunchKernelGGL(qc_field_points_kernel<L>, grid, dim3(FD_WG), 0, st, nrec, rec, boys, B, xyz, e, partial, tile0);
}

// Charges of a batch: as many tiles as PC_PARTIAL_WORDS holds tile sums of `words` doubles, PC_BATCH_TILES at the most.  QC_PC_BATCH=<charges>
// (a test switch, read once per handle at its first embedding call) replaces it.
// QC_PC_ORIENT=record|charge (read with it) forces one orientation of the Hermite sums, for the tests of both.
int64_t batch_charges(qc_system *S, int64_t npc, size_t words) {
    if (S->pc_batch < 0) {
        const char *e = getenv("QC_PC_BATCH"), *o = getenv("QC_PC_ORIENT");
        S->pc_batch = e ? std::max(0L, atol(e)) : 0;
        S->pc_orient = !o ? 0 : (o[0] == 'r' ? 1 : (o[0] == 'c' ? 2 : 0));
    }
    if (S->pc_batch > 0) return std::min<int64_t>(npc, S->pc_batch);
    const int64_t tiles = std::max<int64_t>(1, std::min<int64_t>(PC_BATCH_TILES, (int64_t)(PC_PARTIAL_WORDS / std::max<size_t>(words, 1))));
    return std::min<int64_t>(npc, tiles * QC_PC_TILE);
}

// The records of a Lambda build, grouped by the pair order L: headers [p, P(3)] at hdr + recoff[first[L] + r], tables of order L + extra.
// Lambda of group L lies at g.off[L], entry h of record r at h * cnt.n[L] + r.
struct PcLambda {
    PcCounts cnt{};
    EspGroups g{};
    int first[QC_LPAIR + 1], nrec_all = 0, extra = 0;
    size_t words = 0;
    DevBuf lam;
    void layout() {
        for (int L = 0; L <= QC_LPAIR; ++L) {
            g.off[L] = (long long)words; words += (size_t)cnt.n[L] * qc_nherm(L + extra);
            first[L] = nrec_all; nrec_all += cnt.n[L];
        }
    }
};
// lam = sum over all charges, batch by batch: per batch the upload (phase 0), the tile sums of every group and their ordered sum (phase 1)
int lambda_build(qc_system *S, const std::vector<double> &pc, PcLambda &Q, const int *d_recoff, const double *d_hdr, PhaseClock &clk) {
    const int64_t npc = (int64_t)(pc.size() / 4), bmax = batch_charges(S, npc, Q.words);
    const int tmax = (int)((bmax + QC_PC_TILE - 1) / QC_PC_TILE);
    const size_t words = Q.words;
    // the orientation, from the counts of the whole call: the waves lane = record would launch over all charges (not over a batch - the
    // two orientations differ in the last bits, and the result must not depend on the batching)
    int64_t waves = 0;
    for (int L = 0; L <= QC_LPAIR; ++L) waves += (Q.cnt.n[L] + PC_WG - 1) / PC_WG;
    waves *= (npc + QC_PC_TILE - 1) / QC_PC_TILE;
    const bool by_charge = S->pc_orient ? S->pc_orient == 2 : waves < PC_FILL_WAVES;
    hipStream_t st = S->stream;
    DevBuf partial, dpc;
    if (Q.lam.alloc(words) != QC_OK || partial.alloc((size_t)tmax * words) != QC_OK || dpc.alloc(4 * (size_t)bmax) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(Q.lam.p, 0, words * sizeof(double), st));
    for (int64_t c0 = 0; c0 < npc; c0 += bmax) {
        const int nb = (int)std::min(bmax, npc - c0), nt = (nb + QC_PC_TILE - 1) / QC_PC_TILE;
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dpc.p, pc.data() + 4 * c0, 4 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        clk.mark(1, st);
        for (int L = 0; L <= QC_LPAIR; ++L) {
            const int nrec = Q.cnt.n[L];
            if (!nrec) continue;
            const int *ro = d_recoff + Q.first[L];
            const double *boys = S->dev.d_boys.p;
            const size_t goff = (size_t)Q.g.off[L];
            switch (L + Q.extra) {
                case 0: lambda_launch<0>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 1: lambda_launch<1>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 2: lambda_launch<2>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 3: lambda_launch<3>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 4: lambda_launch<4>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 5: lambda_launch<5>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                case 6: lambda_launch<6>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
                default: lambda_launch<7>(st, by_charge, nrec, nt, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff); break;
            }
        }
        hipLaunchKernelGGL(qc_pc_sum_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, words, nt, partial.p, Q.lam.p);
        clk.mark(2, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));             // (the batch's charges are read by the copy until here)
        clk.add(0, 2);
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// ---- the atoms' gradient of tr(P V_pc): the nuclear section of qc_grad1_kernel with the table R of one centre replaced by Lambda, the sum
// over the charges (order L + 1), and without the Hellmann-Feynman row - the charges stay put.  One wave per shell pair a >= b, lanes over
// ALL its primitive pairs (records of their own: the gradient does not go through the stored pair data); the pair's density block is
// transformed to Cartesian components in LDS first.  out[pr][6] = f (dA, dB), f = 2 off the diagonal: added to the atoms on the host, in pair order.
constexpr int GEI = QC_LMAX + 2, GET = 2 * GEI;          // i <= la + 1, j <= lb + 1
using GE1 = QcMdE1<GEI * GEI * GET>;
__device__ inline double pc_wave_sum(double v) {          // fixed butterfly: every lane ends with the same value
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__global__ __launch_bounds__(64) void qc_pc_grad_kernel(int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                        const double *__restrict__ coefs, const double *__restrict__ Tm, int n, const double *__restrict__ P,
                                                        const int *__restrict__ recstart, const EspGroups g, const PcCounts cnt,
                                                        const double *__restrict__ lam, double *__restrict__ out) {
    __shared__ double Pc[qc_ncart(QC_LMAX) * qc_ncart(QC_LMAX)];
    const int lane = threadIdx.x, pr = blockIdx.x;
    int a = 0, rem = pr;
    while (rem > a) { rem -= a + 1; ++a; }
    const int b = rem;
    const QcDevShell A = sh[a], B = sh[b];
    for (int e = lane; e < A.ncart * B.ncart; e += 64) {
        const int x = e / B.ncart, y = e - x * B.ncart;
        double acc = 0.0;
        for (int f = 0; f < A.nfunc; ++f) {
            double r = 0.0;
            for (int gg = 0; gg < B.nfunc; ++gg) r += P[(size_t)(A.off + f) * n + B.off + gg] * Tm[B.toff + gg * B.ncart + y];
            acc += Tm[A.toff + f * A.ncart + x] * r;
        }
        Pc[e] = acc;
    }
    __syncthreads();
    const int L = A.L + B.L, nrec = cnt.n[L], npp = A.nprim * B.nprim, nh = qc_nherm(L + 1);
    const double *__restrict__ L0 = lam + g.off[L] + recstart[pr];
    double vA[3] = {0, 0, 0}, vB[3] = {0, 0, 0};
    for (int pp = lane; pp < npp; pp += 64) {
        const int i = pp / B.nprim, j = pp - i * B.nprim;
        const double ea = exps[A.poff + i], eb = exps[B.poff + j], p = ea + eb;
        const double cc = -2.0 * M_PI / p * coefs[A.poff + i] * coefs[B.poff + j];
        GE1 E[3];
        for (int k = 0; k < 3; ++k) E[k].fill(A.L + 1, B.L + 1, ea, eb, A.A[k] - B.A[k]);
        double R[qc_nherm(QC_LPAIR + 1)];
        for (int h = 0; h < nh; ++h) R[h] = L0[(size_t)h * nrec + pp];
        for (int x = 0; x < A.ncart; ++x) {
            const unsigned char *ax = qc_md_cart(A.L, x);
            for (int y = 0; y < B.ncart; ++y) {
                const unsigned char *by = qc_md_cart(B.L, y);
                const double pv = cc * Pc[x * B.ncart + y];
                for (int k = 0; k < 3; ++k) {
                    int ai[3] = {ax[0], ax[1], ax[2]}, bi[3] = {by[0], by[1], by[2]};
                    ++ai[k];
                    double dA = 2.0 * ea * qc_md_nuc(E, ai, bi, R);
                    ai[k] -= 2;
                    if (ax[k]) dA -= ax[k] * qc_md_nuc(E, ai, bi, R);
                    ai[k] += 1;
                    ++bi[k];
                    double dB = 2.0 * eb * qc_md_nuc(E, ai, bi, R);
                    bi[k] -= 2;
                    if (by[k]) dB -= by[k] * qc_md_nuc(E, ai, bi, R);
                    vA[k] += pv * dA;
                    vB[k] += pv * dB;
                }
            }
        }
    }
    const double f = a == b ? 1.0 : 2.0;
    for (int k = 0; k < 3; ++k) { vA[k] = pc_wave_sum(vA[k]); vB[k] = pc_wave_sum(vB[k]); }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) { out[6 * (size_t)pr + k] = f * vA[k]; out[6 * (size_t)pr + 3 + k] = f * vB[k]; }
}

}  // namespace

int qc_pc_matrix_device(qc_system *S, const std::vector<double> &pc, double *dV) {
    const int n = S->nbasis, npairs = (int)S->pairs.size();
    hipStream_t st = S->stream;
    PhaseClock clk(S->pc_ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(dV, 0, (size_t)n * n * sizeof(double), st));
    if (npairs == 0 || pc.empty()) { QC_HIP_CHECK(hipStreamSynchronize(st)); return QC_OK; }
    // the records: the stored primitive pairs, their headers where they lie in the pair data
    PcLambda Q;
    for (const QcPairDesc &d : S->pairs) Q.cnt.n[d.L] += d.K;
    Q.layout();
    std::vector<int> recstart(npairs), recoff(Q.nrec_all);
    {
        int run[QC_LPAIR + 1] = {};
        for (int i = 0; i < npairs; ++i) {
            const QcPairDesc &d = S->pairs[i];
            const int stride = qc_pair_stride(d.L, d.na * d.nb);
            recstart[i] = run[d.L];
            for (int kp = 0; kp < d.K; ++kp) recoff[Q.first[d.L] + run[d.L]++] = d.doff + kp * stride;
        }
    }
    QcDev<int> drs, dro;
    if (drs.alloc(npairs) != QC_OK || dro.alloc(Q.nrec_all) != QC_OK) return QC_ERR_HIP;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dro.p, recoff.data(), (size_t)Q.nrec_all * sizeof(int), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(0, 1);
    int rc = lambda_build(S, pc, Q, dro.p, S->dev.d_pairdata.p, clk);
    if (rc != QC_OK) return rc;
    clk.mark(2, st);
    hipLaunchKernelGGL(qc_pc_assemble_kernel, dim3(npairs), dim3(64), 0, st, S->dev.d_pairs.p, S->dev.d_pairdata.p, drs.p, Q.g, Q.cnt, n, Q.lam.p, dV);
    clk.mark(3, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(2, 3);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

int qc_pc_atom_gradient_device(qc_system *S, const std::vector<double> &pc, const double *dPt, double *grad) {
    const int n = S->nbasis, nsh = S->nshells, npairs = nsh * (nsh + 1) / 2;
    for (int k = 0; k < 3 * S->natoms; ++k) grad[k] = 0.0;
    if (pc.empty()) return QC_OK;
    const QcShellBlob *Bl;
    int rc = qc_shell_blob(S, &Bl);
    if (rc != QC_OK) return rc;
    hipStream_t st = S->stream;
    PhaseClock clk(S->pc_ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    // the records: every primitive pair of every shell pair a >= b, in the pair order of the kernel
    PcLambda Q;
    Q.extra = 1;
    for (int a = 0; a < nsh; ++a)
        for (int b = 0; b <= a; ++b) Q.cnt.n[S->shells[a].L + S->shells[b].L] += S->shells[a].nprim * S->shells[b].nprim;
    Q.layout();
    std::vector<int> recstart(npairs), recoff(Q.nrec_all);
    std::vector<double> hdr(4 * (size_t)Q.nrec_all);
    {
        int run[QC_LPAIR + 1] = {}, pr = 0;
        for (int a = 0; a < nsh; ++a)
            for (int b = 0; b <= a; ++b, ++pr) {
                const QcShell &A = S->shells[a], &B = S->shells[b];
                const int L = A.L + B.L;
                recstart[pr] = run[L];
                for (int i = 0; i < A.nprim; ++i)
                    for (int j = 0; j < B.nprim; ++j) {
                        const int r = Q.first[L] + run[L]++;
                        const double ea = A.exps[i], eb = B.exps[j], p = ea + eb;
                        recoff[r] = 4 * r;
                        hdr[4 * (size_t)r] = p;
                        for (int k = 0; k < 3; ++k) hdr[4 * (size_t)r + 1 + k] = (ea * A.A[k] + eb * B.A[k]) / p;
                    }
            }
    }
    QcDev<int> drs, dro;
    DevBuf dh, dout;
    if (drs.alloc(npairs) != QC_OK || dro.alloc(Q.nrec_all) != QC_OK || dh.alloc(hdr.size()) != QC_OK || dout.alloc(6 * (size_t)npairs) != QC_OK) return QC_ERR_HIP;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dro.p, recoff.data(), (size_t)Q.nrec_all * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dh.p, hdr.data(), hdr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(0, 1);
    if ((rc = lambda_build(S, pc, Q, dro.p, dh.p, clk)) != QC_OK) return rc;
    std::vector<double> out(6 * (size_t)npairs);
    clk.mark(2, st);
    hipLaunchKernelGGL(qc_pc_grad_kernel, dim3(npairs), dim3(64), 0, st, nsh, Bl->sh, Bl->exps, Bl->coefs, Bl->T, n, dPt, drs.p, Q.g, Q.cnt, Q.lam.p, dout.p);
    clk.mark(3, st);
    QC_HIP_CHECK(hipMemcpyAsync(out.data(), dout.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    clk.mark(4, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(2, 4);
    int pr = 0;
    for (int a = 0; a < nsh; ++a)
        for (int b = 0; b <= a; ++b, ++pr)
            for (int k = 0; k < 3; ++k) {
                grad[3 * S->shells[a].atom + k] += out[6 * (size_t)pr + k];
                grad[3 * S->shells[b].atom + k] += out[6 * (size_t)pr + 3 + k];
            }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

int qc_points_field_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *e_elec, double *ms) {
    PhaseClock clk(ms);
    if (clk.create() != QC_OK) return QC_ERR_HIP;
    EspRecords E;
    int rc = E.build(S, dD, clk);
    if (rc != QC_OK) return rc;
    const int64_t bmax = std::min<int64_t>(npts, (int64_t)1 << 20);
    // few points: the tiles go to workgroups of their own.  The largest batch that does so, and the most points such a batch has
    const int64_t split_max = std::min<int64_t>(FD_SPLIT_MAX, (int64_t)(FD_SPLIT_WORDS / (3 * (size_t)std::max(E.tiles_all, 1))));
    const int64_t rem = npts % bmax, split_pts = bmax <= split_max ? bmax : (rem > 0 && rem <= split_max ? rem : 0);
    DevBuf dxyz, de, partial;
    if (dxyz.alloc(3 * bmax) != QC_OK || de.alloc(3 * bmax) != QC_OK || partial.alloc((size_t)E.tiles_all * 3 * split_pts) != QC_OK) return QC_ERR_HIP;
    std::vector<double> he(3 * (size_t)bmax);
    hipStream_t st = S->stream;
    for (int64_t k0 = 0; k0 < npts; k0 += bmax) {
        const int nb = (int)std::min(bmax, npts - k0), gx = (nb + FD_WG - 1) / FD_WG;
        const bool split = nb <= split_pts;
        double *pp = split ? partial.p : nullptr;
        clk.mark(0, st);
        QC_HIP_CHECK(hipMemcpyAsync(dxyz.p, xyz + 3 * k0, 3 * (size_t)nb * sizeof(double), hipMemcpyHostToDevice, st));
        QC_HIP_CHECK(hipMemsetAsync(de.p, 0, 3 * (size_t)nb * sizeof(double), st));
        clk.mark(1, st);
        clk.mark(2, st);
        for (int L = 0; L <= QC_LPAIR; ++L) {              // the seven groups in a fixed order, each adding into de (or its tiles into `partial`)
            if (!E.cnt[L]) continue;
            const dim3 grid(gx, split ? std::min(E.ntiles[L], 65535) : 1);
            const int t0 = E.tile0[L];
            const double *r = E.rec.p + E.g.off[L], *boys = S->dev.d_boys.p;
            switch (L) {
                case 0: field_launch<0>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                case 1: field_launch<1>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                case 2: field_launch<2>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                case 3: field_launch<3>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                case 4: field_launch<4>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                case 5: field_launch<5>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
                default: field_launch<6>(st, grid, (int)E.cnt[L], r, boys, nb, dxyz.p, de.p, pp, t0); break;
            }
        }
        if (split && E.tiles_all > 0) hipLaunchKernelGGL(qc_field_sum_kernel, dim3((3 * nb + FD_WG - 1) / FD_WG), dim3(FD_WG), 0, st, E.tiles_all, 3 * nb, partial.p, de.p);
        clk.mark(3, st);
        QC_HIP_CHECK(hipMemcpyAsync(he.data(), de.p, 3 * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        clk.mark(4, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        clk.add(0, 1); clk.add(2, 4);
        for (int k = 0; k < nb; ++k)
            for (int x = 0; x < 3; ++x) e_elec[3 * (k0 + k) + x] = he[(size_t)x * nb + k];
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}
