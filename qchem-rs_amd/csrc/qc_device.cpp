// qc_device.cpp - the device side of a handle: set-up (streams, pair data, tables, accumulators, probes, Schwarz pass, work lists),
// teardown, re-sharding.  Host API only; the kernels are launched through their owners' functions.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "qc_internal.h"

int qc_device_ready(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QC_ERR_NO_DEVICE;
    return QC_OK;
}

// Device records of a bra-major work list (QcBundleDev / QcKetUnit, qc_internal.h) from the host lists of qc_make_bundles
void qc_bm_device_lists(const qc_system *S, int lcd, const std::vector<QcBundle> &bundles, const std::vector<int> &ketlist, bool packed,
                               std::vector<QcBundleDev> &db, std::vector<QcKetUnit> &du) {
    db.resize(bundles.size()); du.resize(ketlist.size());
    for (size_t i = 0; i < bundles.size(); ++i) {
        const QcBundle &b = bundles[i];
        const QcPairDesc &p = S->pairs[b.bra];
        db[i] = QcBundleDev{b.bra, b.ij_lo, b.ij_hi, b.first, b.nket, b.maxK, p.doff, p.offa, p.offb, p.na | (p.nb << 8) | ((p.shA_eq_shB ? 1 : 0) << 16), b.pad0, 0};
    }
    for (size_t i = 0; i < ketlist.size(); ++i) {
        int ket, kl0, klen;
        qc_unpack_ket_entry(ketlist[i], packed, &ket, &kl0, &klen);
        const QcPairDesc &p = S->pairs[ket];
        const int stride = lcd == 0 ? qc_pair_stride(0, 1) : (lcd == 1 ? 8 : 16);
        const int K = klen ? klen : p.K;
        // (p.p kets: the columns of a lane are the functions of the SECOND shell - bits 18..23 carry its axis permutation, 24..29 the first shell's)
        const int perm_bits = lcd == 2 ? ((((p.psperm >> 6) & 63) << 18) | ((p.psperm & 63) << 24)) : ((p.psperm & 63) << 18);
        du[i] = QcKetUnit{ket, (lcd == 0 ? p.doff : p.psoff) + kl0 * stride, p.offa | (p.offb << 16),
                          (K & 0xffff) | ((lcd == 1 && p.nb == 1 ? 1 : 0) << 16) | ((p.shA_eq_shB ? 1 : 0) << 17) | perm_bits};
    }
}
// (the work lists of all classes live in ONE device buffer, qc_system::d_lists - the classes' pointers point into it: an allocation and a
// synchronous copy per list, up to three per class, were 2 ms of a cold handle's set-up on H2O/cc-pVTZ)
static void drop_lists(qc_system *S) {
    for (auto &c : S->classes) { c.d_slots = nullptr; c.d_bundles = nullptr; c.d_ketlist = nullptr; }
    S->dev.d_lists.reset();
}
static int upload_slots(qc_system *S) {
    qc_drop_launch_plan(S);
    if (S->stream) (void)hipStreamSynchronize(S->stream);         // (nothing in flight reads the old lists)
    drop_lists(S);
    QcBlob blob;
    struct Where { size_t slots = ~(size_t)0, bundles = ~(size_t)0, kets = ~(size_t)0; };
    std::vector<Where> where(S->classes.size());
    {   // (one allocation for the host copy too: growing it list by list copied benzene's 40 MB several times over)
        size_t est = 0;
        for (const auto &c : S->classes) est += c.slots.size() * sizeof(QcSlot) + c.bundles.size() * sizeof(QcBundleDev) + c.ketlist.size() * sizeof(QcKetUnit) + 3 * 256;
        blob.bytes.reserve(est);
    }
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        auto &c = S->classes[ci];
        if (!c.slots.empty()) where[ci].slots = blob.put(c.slots.data(), c.slots.size() * sizeof(QcSlot));
        if (!c.bundles.empty()) {
            std::vector<QcBundleDev> db; std::vector<QcKetUnit> du;
            qc_bm_device_lists(S, c.LCD, c.bundles, c.ketlist, c.ket_packed, db, du);
            where[ci].bundles = blob.put(db.data(), db.size() * sizeof(QcBundleDev));
            where[ci].kets = blob.put(du.data(), du.size() * sizeof(QcKetUnit));
        }
    }
    if (blob.bytes.empty()) return QC_OK;
    if (S->dev.d_lists.alloc(blob.bytes.size()) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpy(S->dev.d_lists.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice));
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        auto &c = S->classes[ci];
        if (where[ci].slots != ~(size_t)0) c.d_slots = reinterpret_cast<QcSlot *>(S->dev.d_lists.p + where[ci].slots);
        if (where[ci].bundles != ~(size_t)0) c.d_bundles = reinterpret_cast<QcBundleDev *>(S->dev.d_lists.p + where[ci].bundles);
        if (where[ci].kets != ~(size_t)0) c.d_ketlist = reinterpret_cast<QcKetUnit *>(S->dev.d_lists.p + where[ci].kets);
    }
    return QC_OK;
}

int qc_device_reshard(qc_system *S) {
    S->prep.invalidate();                    // a build prepared for the old work lists must not skip the fork of the next one
    S->assign.unit_ms.clear(); S->assign.unit_stream.clear();
    S->assign.cand_skip = false; S->assign.tune_count = 0; S->assign.on = QcOnline{};
    S->assign.gen += 1;
    qc_build_shards(S, !S->device_ready);         // (a handle without its device part builds its lists behind the Schwarz pass, or on demand)
    if (!S->device_ready) return QC_OK;
    return upload_slots(S);
}

// Gather records of the matrix-core classes (qc_fock_body, MFMA branch): step 2's A fragment of k-step ks is, in lane l = 16 q4 + i16 and
// row tile mt, the R value at the Hermite index of h1 + h2 with h1 = 16 mt + i16, h2 = 4 ks + q4.  Which LDS word that is does not
// depend on the quartet: record (ks, l) = eight u16 - byte offsets into the R table for mt = 0..5, one spare, flags (bit 0 = odd ket
// order: the value enters with a minus sign; bit 1 = h2 inside the ket's Hermite range).
static std::vector<unsigned> qc_build_gidx() {
    std::vector<unsigned> out;
    std::vector<int> ht, hu, hv;
    for (int N = 0; N <= QC_LPAIR; ++N)
        for (int t = N; t >= 0; --t)
            for (int u = N - t; u >= 0; --u) { ht.push_back(t); hu.push_back(u); hv.push_back(N - t - u); }
    for (size_t h = 0; h < ht.size(); ++h) if (qc_hidx(ht[h], hu[h], hv[h]) != (int)h) abort();
    for (int LAB = 3; LAB <= 6; ++LAB)
        for (int LCD = 4; LCD <= 6; ++LCD) {
            if ((int)out.size() != 4 * qc_gidx_off(LAB, LCD)) abort();
            const int HAB = qc_nherm(LAB), HCD = qc_nherm(LCD), MT = (HAB + 15) / 16;
            for (int ks = 0; ks < qc_gidx_ksteps(LCD); ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int q4 = lane >> 4, i16 = lane & 15, h2 = 4 * ks + q4;
                    const bool ok = h2 < HCD;
                    unsigned short w[8] = {};
                    for (int mt = 0; mt < MT; ++mt) {
                        const int h1 = std::min(16 * mt + i16, HAB - 1), g = ok ? h2 : 0;
                        w[mt] = (unsigned short)(8 * qc_hidx(ht[h1] + ht[g], hu[h1] + hu[g], hv[h1] + hv[g]));
                    }
                    w[7] = ok ? (unsigned short)(2 | ((ht[h2] + hu[h2] + hv[h2]) & 1)) : 0;
                    for (int k = 0; k < 4; ++k) out.push_back((unsigned)w[2 * k] | ((unsigned)w[2 * k + 1] << 16));
                }
        }
    out.resize(out.size() + 4, 0u);
    return out;
}

// Recurrence plans of the cooperative Hermite-Coulomb tables (qc_build_r in qc_fock_kernel.h), every total order 0..QC_LTOT.  Work array
// of order L: level n (the R^n values) starts at rwork(L) - rwork(L - n), inside a level the Hermite index.  Record = {target | source1 << 16,
// source2 | c << 16 | axis << 24}, byte offsets; entries of stage N = t+u+v are contiguous, levels n = 0 .. L-N, position r inside the order.
static std::vector<int> qc_build_rplan() {
    std::vector<int> plan;
    for (int L = 0; L <= QC_LTOT; ++L) {
        if ((int)plan.size() != 2 * qc_plan_off(L)) abort();
        const int RWL = qc_rwork(L);
        for (int N = 1; N <= L; ++N) {
            const int cnt = (N + 1) * (N + 2) / 2;
            for (int n = 0; n <= L - N; ++n)
                for (int r = 0; r < cnt; ++r) {
                    int s = 0;
                    while ((s + 1) * (s + 2) / 2 <= r) ++s;
                    const int v = r - s * (s + 1) / 2, u = s - v, t = N - s;
                    const int o0 = RWL - qc_rwork(L - n), o1 = RWL - qc_rwork(L - n - 1);
                    int s1, s2, c, ax;
                    if (t > 0) { ax = 0; c = t - 1; s1 = qc_hidx(t - 1, u, v); s2 = t > 1 ? qc_hidx(t - 2, u, v) : s1; }
                    else if (u > 0) { ax = 1; c = u - 1; s1 = qc_hidx(t, u - 1, v); s2 = u > 1 ? qc_hidx(t, u - 2, v) : s1; }
                    else { ax = 2; c = v - 1; s1 = qc_hidx(t, u, v - 1); s2 = v > 1 ? qc_hidx(t, u, v - 2) : s1; }
                    const int dst = 8 * (o0 + qc_hidx(t, u, v)), b1 = 8 * (o1 + s1), b2 = 8 * (o1 + s2);
                    plan.push_back(dst | (b1 << 16));
                    plan.push_back(b2 | (c << 16) | (ax << 24));
                }
        }
    }
    plan.push_back(0); plan.push_back(0);
    return plan;
}

// rows: F_{L+j}(x_k) / j!, j = 0..7, per total order L; then exp(-x_k)
static std::vector<double> qc_build_boys() {
    std::vector<double> tab((size_t)(QC_LTOT + 1) * QC_BOYS_NGRID * 8 + QC_BOYS_NGRID), row(QC_BOYS_NORD);
    for (int k = 0; k < QC_BOYS_NGRID; ++k) {
        qc_boys_host(QC_BOYS_NORD - 1, k * QC_BOYS_DX, row.data());
        for (int L = 0; L <= QC_LTOT; ++L) {
            double fact = 1.0;
            for (int j = 0; j < 8; ++j) { tab[((size_t)L * QC_BOYS_NGRID + k) * 8 + j] = row[L + j] / fact; fact *= (j + 1); }
        }
        tab[(size_t)(QC_LTOT + 1) * QC_BOYS_NGRID * 8 + k] = std::exp(-k * QC_BOYS_DX);
    }
    return tab;
}

// the DS unit's lane order (qc_fock_bm.hip): asked once per device and process
static int qc_ds_order(qc_system *S) {
    static std::mutex mu;
    static int known[64];                          // 0 unknown, 1 fixed order, 2 not
    int dev = S->device >= 0 && S->device < 64 ? S->device : 0;
    std::lock_guard<std::mutex> lk(mu);
    if (known[dev] == 0) {
        QcDev<double> d;
        double h[64];
        if (d.alloc(64) != QC_OK) return QC_ERR_HIP;
        int prc = qc_ds_order_probe(S->stream, d.p);
        hipError_t e = hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, S->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(S->stream);
        if (prc != QC_OK || e != hipSuccess) return QC_ERR_HIP;
        bool same = true;
        for (int i = 1; i < 64; ++i) same = same && std::memcmp(&h[i], &h[0], sizeof(double)) == 0;
        known[dev] = same ? 1 : 2;
        if (!same) fprintf(stderr, "qchem_hip: this device's DS unit does not add the lanes of one instruction in a fixed order: exchange rows go to global memory directly\n");
    }
    S->ds_order_ok = known[dev] == 1 && getenv("QC_DS_ORDER_FAIL") == nullptr;        // (QC_DS_ORDER_FAIL: test hook - as if the probe had failed)
    return QC_OK;
}

template <class T> static int upload(QcDev<T> &d, const std::vector<T> &h, size_t spare = 0) {
    if (d.alloc(h.size() + spare) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return QC_OK;
}

// (creating a stream costs ~2 ms - eight of them 17 ms, three times a whole 15-pass SCF of H2O/cc-pVTZ: a handle that goes away
// leaves its streams, events and measured dispatch lanes in a process-wide pool for the next one)
static int init_streams(qc_system *S, bool *lanes_known) {
    *lanes_known = !S->stream && qc_stream_pool_take(S);
    if (*lanes_known) return QC_OK;
    if (!S->stream) { QC_HIP_CHECK(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking)); S->own_stream = true; }
    for (int i = 0; i < QC_NSTREAMS; ++i) {
        QC_HIP_CHECK(hipStreamCreateWithFlags(&S->lanes.side[i], hipStreamNonBlocking));
        QC_HIP_CHECK(hipEventCreateWithFlags(&S->lanes.ev_join[i], hipEventDisableTiming));
    }
    QC_HIP_CHECK(hipEventCreateWithFlags(&S->lanes.ev_fork, hipEventDisableTiming));
    return QC_OK;
}
static int init_accumulators(qc_system *S) {
    QcDeviceData &D = S->dev;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    if (D.d_D.alloc(2 * nn) != QC_OK || D.d_G.alloc(2 * nn) != QC_OK || D.d_Gtmp.alloc((size_t)2 * QC_NREP * 2 * nn) != QC_OK ||
        D.d_Gred.alloc((size_t)2 * 2 * nn) != QC_OK || D.d_Dj.alloc(nn) != QC_OK || D.d_flag.alloc(4) != QC_OK || D.d_join.alloc(8) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemset(D.d_join.p, 0, 8 * sizeof(unsigned)));
    QC_HIP_CHECK(hipHostMalloc(&S->join.h_timeout, 4 * sizeof(int), hipHostMallocDefault));
    *S->join.h_timeout = 0; S->join.target = 0; S->join.spin_target = 0;
    return QC_OK;
}
// do kernels of different streams run concurrently here, and on which dispatch lanes?
static int init_probes(qc_system *S, bool lanes_known) {
    bool concurrent = true;
    int rc = qc_join_probe(S, &concurrent);
    if (rc != QC_OK) return rc;
    S->join.by_events = !concurrent || getenv("QC_EVENT_JOIN") != nullptr;      // (A/B switch, read per handle: the event join of rounds 1-2)
    if (!concurrent && getenv("QC_SCF_DEBUG")) fprintf(stderr, "qchem_hip: kernels of different streams do not run concurrently here (profiler counters?): event join\n");
    if (concurrent && !lanes_known) { if ((rc = qc_lane_probe(S)) != QC_OK) return rc; S->lanes.lanes_probed = getenv("QC_NO_LANES") == nullptr; }
    return qc_ds_order(S);
}

// The steps of the set-up, in the order of their allocations (cold set-up time is a benchmark figure).  Every step returns at its first
// failure; what the steps before it acquired is released by qc_device_init.
static int device_init_steps(qc_system *S) {
    static const bool sdbg = getenv("QC_SETUP_DEBUG") != nullptr;
    QcLap lap{"setup", sdbg};
    int rc;
    bool lanes_known = false;
    if ((rc = init_streams(S, &lanes_known)) != QC_OK) return rc;
    lap("streams and events");
    QcDeviceData &D = S->dev;
    if (upload(D.d_pairdata, S->pairdata) != QC_OK || upload(D.d_pairdataT, S->pairdataT) != QC_OK || upload(D.d_pspack, S->pspack, 8) != QC_OK ||
        upload(D.d_pairs, S->pairs) != QC_OK) return QC_ERR_HIP;
    lap("pair data upload");
    const std::vector<double> boys = qc_build_boys();
    lap("Boys tables on the host");
    if (upload(D.d_boys, boys) != QC_OK || upload(D.d_rplan, qc_build_rplan()) != QC_OK || upload(D.d_gidx, qc_build_gidx()) != QC_OK) return QC_ERR_HIP;
    if ((rc = init_accumulators(S)) != QC_OK) return rc;
    lap("tables, buffers");
    if ((rc = init_probes(S, lanes_known)) != QC_OK) return rc;
    lap("join + lane probes");
    if (D.d_fxs.alloc(2) != QC_OK) return QC_ERR_HIP;
    // Schwarz factors of the pairs (once per geometry), then the screened work lists
    if ((rc = qc_schwarz_device(S)) != QC_OK) return rc;
    lap("Schwarz pass");
    qc_build_shards(S);
    lap("work lists");
    if ((rc = upload_slots(S)) != QC_OK) return rc;
    lap("upload");
    return QC_OK;
}

// everything the device side of the handle holds, except a stream the caller gave it (qc_set_stream)
static void device_release(qc_system *S) {
    if (S->stream) (void)hipStreamSynchronize(S->stream);
    qc_gate_forget(S);
    drop_lists(S);
    qc_drop_launch_plan(S);
    delete S->shell_blob; S->shell_blob = nullptr;
    qc_renew(S->dev);
    if (S->join.h_timeout) (void)hipHostFree(S->join.h_timeout);
    qc_renew(S->join);
    if (!qc_stream_pool_give(S)) {
        for (int i = 0; i < QC_NSTREAMS; ++i) {
            if (S->lanes.side[i]) (void)hipStreamDestroy(S->lanes.side[i]);
            if (S->lanes.ev_join[i]) (void)hipEventDestroy(S->lanes.ev_join[i]);
        }
        if (S->lanes.ev_fork) (void)hipEventDestroy(S->lanes.ev_fork);
        if (S->own_stream && S->stream) (void)hipStreamDestroy(S->stream);
    }
    S->lanes = QcLanes{};
    if (S->own_stream) S->stream = nullptr;
    S->own_stream = false; S->device_ready = false;
}

int qc_device_init(qc_system *S) {
    if (S->device_ready) return QC_OK;
    if (qc_device_ready() != QC_OK) return QC_ERR_NO_DEVICE;
    QC_HIP_CHECK(hipGetDevice(&S->device));
    hipDeviceProp_t prop;
    QC_HIP_CHECK(hipGetDeviceProperties(&prop, S->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "qchem_hip: device %d is %s, this library is built for gfx950 only\n", S->device, prop.gcnArchName);
        return QC_ERR_NO_DEVICE;
    }
    const int rc = device_init_steps(S);
    if (rc != QC_OK) { device_release(S); return rc; }       // (a second call starts from a clean handle)
    S->device_ready = true;
    return QC_OK;
}

void qc_device_free(qc_system *S) { device_release(S); S->stream = nullptr; }
