// qc_embed.hip - point-charge embedding on the device.  Not in the reference.  No atomics anywhere: every sum has a
// fixed order.
//   Lambda_h(rec) = sum_c q_c R_h(p_rec, P_rec - R_c)      the adjoint of qc_esp_walk_kernel: per stored primitive pair the Hermite-Coulomb
//                                                          tables of all charges, summed.  Charge tiles over gridDim.y in both orientations:
//                                                          qc_pc_lambda_kernel<LT>, lane = record, the charges read through the scalar cache -
//                                                          when its launches fill the chip; qc_pc_lambda_charge_kernel<LT>, lane = charge with
//                                                          a fixed reduction per entry - when they would not (lambda_build).  esp_tile_sum
//                                                          (qc_esp.h) adds the tiles' sums in ascending order
//   V_pc,ab = -sum_rec sum_h E_h,ab(rec) Lambda_h(rec)     the adjoint of qc_esp_hermite_kernel, from the same pair data (qc_pc_assemble_kernel)
//   d tr(P V_pc) / dR_A                                    the nuclear section of the SCF gradient with Lambda in place of the table of one
//                                                          nucleus (qc_pc_grad_kernel)
// The field on points, whose values at the charges are the charges' gradient -q_c E(R_c), lives with the potential in qc_points.hip.
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

// The records of a Lambda build, grouped by the pair order L (lay): headers [p, P(3)] at hdr + recoff[lay.first[L] + r], tables of order
// L + extra.  Lambda of group L lies at lay.g.off[L], entry h of record r at h * cnt.n[L] + r.
struct PcLambda {
    EspLayout lay;
    PcCounts cnt{};                        // lay.cnt as the kernels take it
    int extra = 0;
    DevBuf lam;
    auto record_words() const { return [e = extra](int L) { return qc_nherm(L + e); }; }
    void counts() { for (int L = 0; L <= QC_LPAIR; ++L) cnt.n[L] = (int)lay.cnt[L]; }
};
// lam = sum over all charges, batch by batch: per batch the upload (phase 0), the tile sums of every group and their ordered sum (phase 1)
int lambda_build(qc_system *S, const std::vector<double> &pc, PcLambda &Q, const int *d_recoff, const double *d_hdr, PhaseClock &clk) {
    const int64_t npc = (int64_t)(pc.size() / 4), bmax = batch_charges(S, npc, Q.lay.words);
    const int tmax = (int)((bmax + QC_PC_TILE - 1) / QC_PC_TILE);
    const size_t words = Q.lay.words;
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
            const int *ro = d_recoff + Q.lay.first[L];
            const double *boys = S->dev.d_boys.p;
            const size_t goff = (size_t)Q.lay.g.off[L];
            esp_dispatch<QC_LPAIR + 1>(L + Q.extra, [&](auto LT) {
                if (by_charge)
                    hipLaunchKernelGGL(qc_pc_lambda_charge_kernel<decltype(LT)::value>, dim3((nrec + PC_CH_RECORDS - 1) / PC_CH_RECORDS, nt), dim3(QC_PC_TILE), 0,
                                       st, nrec, ro, d_hdr, boys, nb, dpc.p, partial.p, words, goff);
                else
                    hipLaunchKernelGGL(qc_pc_lambda_kernel<decltype(LT)::value>, dim3((nrec + PC_WG - 1) / PC_WG, nt), dim3(PC_WG), 0, st, nrec, ro, d_hdr, boys,
                                       nb, dpc.p, partial.p, words, goff);
            });
        }
        esp_tile_sum(st, words, nt, partial.p, Q.lam.p);      // on top of the batches before it
        clk.mark(2, st);
        QC_HIP_CHECK(hipStreamSynchronize(st));             // (the batch's charges are read by the copy until here)
        clk.add(0, 2);
    }
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// ---- the atoms' gradient of tr(P V_pc): the nuclear section of qc_grad1_kernel (the contraction both call: qc_md_nuc_grad, qc_md.h) with
// the table R of one centre replaced by Lambda, the sum over the charges (order L + 1), and without the Hellmann-Feynman row - the charges
// stay put.  One wave per shell pair a >= b, lanes over ALL its primitive pairs (records of their own: the gradient does not go through the stored pair data); the pair's density block is
// transformed to Cartesian components in LDS first.  out[pr][6] = f (dA, dB), f = 2 off the diagonal: added to the atoms on the host, in pair order.
constexpr int GEI = QC_LMAX + 2, GET = 2 * GEI;          // i <= la + 1, j <= lb + 1
using GE1 = QcMdE1<GEI * GEI * GET>;
__global__ __launch_bounds__(64) void qc_pc_grad_kernel(int nshells, const QcDevShell *__restrict__ sh, const double *__restrict__ exps,
                                                        const double *__restrict__ coefs, const double *__restrict__ Tm, int n, const double *__restrict__ P,
                                                        const int *__restrict__ recstart, const EspGroups g, const PcCounts cnt,
                                                        const double *__restrict__ lam, double *__restrict__ out) {
    __shared__ double Pc[qc_ncart(QC_LMAX) * qc_ncart(QC_LMAX)];
    const int lane = threadIdx.x, pr = blockIdx.x;
    int a, b;
    qc_tri_pair(pr, a, b);
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
        qc_md_nuc_grad(E, A.L, A.ncart, B.L, B.ncart, ea, eb, R, cc, Pc, B.ncart, vA, vB);
    }
    const double f = a == b ? 1.0 : 2.0;
    for (int k = 0; k < 3; ++k) { vA[k] = qc_wave_sum(vA[k]); vB[k] = qc_wave_sum(vB[k]); }
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
    const std::vector<int> recstart = Q.lay.stored_pairs(S, Q.record_words());
    Q.counts();
    std::vector<int> recoff(Q.lay.nrec);
    for (int i = 0; i < npairs; ++i) {
        const QcPairDesc &d = S->pairs[i];
        const int stride = qc_pair_stride(d.L, d.na * d.nb);
        for (int kp = 0; kp < d.K; ++kp) recoff[Q.lay.first[d.L] + recstart[i] + kp] = d.doff + kp * stride;
    }
    QcDev<int> drs, dro;
    if (drs.alloc(npairs) != QC_OK || dro.alloc(Q.lay.nrec) != QC_OK) return QC_ERR_HIP;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dro.p, recoff.data(), (size_t)Q.lay.nrec * sizeof(int), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(0, 1);
    int rc = lambda_build(S, pc, Q, dro.p, S->dev.d_pairdata.p, clk);
    if (rc != QC_OK) return rc;
    clk.mark(2, st);
    hipLaunchKernelGGL(qc_pc_assemble_kernel, dim3(npairs), dim3(64), 0, st, S->dev.d_pairs.p, S->dev.d_pairdata.p, drs.p, Q.lay.g, Q.cnt, n, Q.lam.p, dV);
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
    std::vector<int> recstart(npairs);
    {
        int pr = 0;
        for (int a = 0; a < nsh; ++a)
            for (int b = 0; b <= a; ++b, ++pr) recstart[pr] = Q.lay.add(S->shells[a].L + S->shells[b].L, S->shells[a].nprim * S->shells[b].nprim);
    }
    Q.lay.close(Q.record_words());
    Q.counts();
    std::vector<int> recoff(Q.lay.nrec);
    std::vector<double> hdr(4 * (size_t)Q.lay.nrec);
    {
        int pr = 0;
        for (int a = 0; a < nsh; ++a)
            for (int b = 0; b <= a; ++b, ++pr) {
                const QcShell &A = S->shells[a], &B = S->shells[b];
                int r = Q.lay.first[A.L + B.L] + recstart[pr];
                for (int i = 0; i < A.nprim; ++i)
                    for (int j = 0; j < B.nprim; ++j, ++r) {
                        const double ea = A.exps[i], eb = B.exps[j], p = ea + eb;
                        recoff[r] = 4 * r;
                        hdr[4 * (size_t)r] = p;
                        for (int k = 0; k < 3; ++k) hdr[4 * (size_t)r + 1 + k] = (ea * A.A[k] + eb * B.A[k]) / p;
                    }
            }
    }
    QcDev<int> drs, dro;
    DevBuf dh, dout;
    if (drs.alloc(npairs) != QC_OK || dro.alloc(Q.lay.nrec) != QC_OK || dh.alloc(hdr.size()) != QC_OK || dout.alloc(6 * (size_t)npairs) != QC_OK) return QC_ERR_HIP;
    clk.mark(0, st);
    QC_HIP_CHECK(hipMemcpyAsync(drs.p, recstart.data(), (size_t)npairs * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dro.p, recoff.data(), (size_t)Q.lay.nrec * sizeof(int), hipMemcpyHostToDevice, st));
    QC_HIP_CHECK(hipMemcpyAsync(dh.p, hdr.data(), hdr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    clk.mark(1, st);
    QC_HIP_CHECK(hipStreamSynchronize(st));
    clk.add(0, 1);
    if ((rc = lambda_build(S, pc, Q, dro.p, dh.p, clk)) != QC_OK) return rc;
    std::vector<double> out(6 * (size_t)npairs);
    clk.mark(2, st);
    hipLaunchKernelGGL(qc_pc_grad_kernel, dim3(npairs), dim3(64), 0, st, nsh, Bl->sh, Bl->exps, Bl->coefs, Bl->T, n, dPt, drs.p, Q.lay.g, Q.cnt, Q.lam.p, dout.p);
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
