// qc_fock.hip - the direct-SCF Fock build: launch plan, issue of a build on the dispatch lanes, the build's entry points, Schwarz pass
// and ERI-tensor launch.  (Device set-up: qc_device.cpp; streams and joins: qc_streams.hip; stream assignment: qc_assign.hip.)
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "qc_fock_build.h"
#include "qc_fock_bm.h"

int qc_launch_tier_lab0(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab1(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab2(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab3(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab4(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab5(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier_lab6(int, int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier1_low(int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier1_mid(int, size_t, hipStream_t, const QcTierArgs &);
int qc_launch_tier1_hi(int, size_t, hipStream_t, const QcTierArgs &);

static int launch_tier(int lab, int tier, int grid, size_t lds, hipStream_t st, const QcTierArgs &a) {
    static int (*const fn[])(int, int, size_t, hipStream_t, const QcTierArgs &) = {qc_launch_tier_lab0, qc_launch_tier_lab1, qc_launch_tier_lab2, qc_launch_tier_lab3,
                                                                                  qc_launch_tier_lab4, qc_launch_tier_lab5, qc_launch_tier_lab6};
    return lab >= 0 && lab <= 6 ? fn[lab](tier, grid, lds, st, a) : QC_ERR_UNSUPPORTED;
}

static QcKernelArgs base_args(qc_system *S, const QcFockArgs &fa) {
    QcKernelArgs a{};
    a.pairs = S->dev.d_pairs.p; a.pairdata = S->dev.d_pairdata.p; a.pairdataT = S->dev.d_pairdataT.p; a.boys = S->dev.d_boys.p; a.rplan = reinterpret_cast<const int2 *>(S->dev.d_rplan.p); a.gidx = reinterpret_cast<const uint4 *>(S->dev.d_gidx.p); a.n = S->nbasis;
    a.Dj = fa.Dj; a.Dk0 = fa.Dk0; a.Dk1 = fa.Dk1; a.G0 = fa.G0; a.G1 = fa.G1; a.cK = fa.cK; a.eri_out = fa.eri_out;
    a.nrep = fa.nrep > 0 ? fa.nrep : 1; a.rep_stride = fa.rep_stride; a.fxs = fa.fxs; a.fx_lo = fa.fx_lo; a.schwarz_out = fa.schwarz_out;
    return a;
}

static Seg seg_of(const QcClass &c) {
    if (c.bm) return Seg{&c, nullptr, (int)c.bundles.size(), c.d_bundles, c.d_ketlist, c.lds_bytes};
    return Seg{&c, c.d_slots, (int)c.slots.size()};
}

void qc_drop_launch_plan(qc_system *S) { delete S->launch_plan; S->launch_plan = nullptr; }

// One launch of the bra-major kernels: workgroups of up to QC_BM_WAVES waves, as many as the LDS blocks of the segments allow
static int launch_bm_segments(qc_system *S, int unit, const std::vector<Seg> &segs, hipStream_t st, const QcKernelArgs &base) {
    QcBmArgs t{};
    t.base = base; t.pairdataT = S->dev.d_pairdataT.p; t.pspack = S->dev.d_pspack.p;
    t.base.tl = S->tl.cur ? S->tl.cur + QC_TL_W * unit : nullptr;
    const int v = unit - 2 * (QC_LPAIR + 1);
    const int lds_max = 160 * 1024 - 512;
    int nw = QC_BM_WAVES, iblock = 0, rows = 0;
    for (const Seg &sg : segs) { iblock = std::max(iblock, sg.lds); rows = std::max(rows, sg.c->bm_rows); }
    // exchange rows of a wave's current bra in LDS: (na + nb) rows x n columns per spin
    const int rowbytes = (base.Dk1 ? 2 : 1) * rows * S->nbasis * 8;
    // (QC_BM_NO_ROWBUF forces the large-n fallback - direct global atomics per bundle - so that tests can reach it)
    t.use_rowbuf = (base.eri_out == nullptr && base.schwarz_out == nullptr && QC_BM_LDS_TABLE + 2 * (iblock + rowbytes) <= lds_max && S->ds_order_ok && !getenv("QC_BM_NO_ROWBUF")) ? 1 : 0;
    const int wbytes = iblock + (t.use_rowbuf ? rowbytes : 0);
    while (nw > 1 && QC_BM_LDS_TABLE + nw * wbytes > lds_max) nw = nw > 4 ? nw - 1 : nw / 2;   // Cartesian d / f bras: 36+ rows of I per wave
    int grid = 0, k = 0;
    for (const Seg &sg : segs) {
        // persistent workgroups of `nw` waves: at most ~12 waves per CU, each wave strides through the bundle list
        grid += std::min((sg.nslots + nw - 1) / nw, 256 * 12 / nw);
        t.seg_end[k] = grid; t.seg_lab[k] = sg.c->LAB; t.seg_lcd[k] = sg.c->LCD; t.seg_bundles[k] = sg.d_bundles; t.seg_ketlist[k] = sg.d_ketlist;
        t.seg_nbundles[k] = sg.nslots; t.seg_iwords[k] = sg.lds / 8;
        t.seg_rows[k] = rows;
        ++k;
    }
    t.nseg = k;
    const int lds = QC_BM_LDS_TABLE + nw * wbytes;
    static const bool lds_dbg = getenv("QC_LDS_DEBUG") != nullptr;
    if (lds_dbg) fprintf(stderr, "[lds] bm<%d,%d>: %d workgroups x %d waves, %d bytes of LDS per workgroup (table %d, per wave %d)\n", v / 2, v % 2, grid, nw, lds, QC_BM_LDS_TABLE, wbytes);
    {   // ss-ket segments in the launch of the ps kets / low bras: the merged kernel
        bool mixed = false;
        for (const Seg &sg : segs) mixed = mixed || sg.c->LCD != v / 2;
        if (mixed) return (v == 2 && k <= QC_MAXSEG) ? qc_launch_bm(3, 0, grid, nw, (size_t)lds, st, t) : QC_ERR_UNSUPPORTED;
    }
    return qc_launch_bm(v / 2, v % 2, grid, nw, (size_t)lds, st, t);
}

// One launch of the column kernels: one-wave workgroups, every segment with the largest segment's LDS
static int launch_column_segments(qc_system *S, int unit, const std::vector<Seg> &segs, hipStream_t st, const QcKernelArgs &base) {
    QcTierArgs t{};
    t.base = base;
    t.base.tl = S->tl.cur ? S->tl.cur + QC_TL_W * unit : nullptr;
    int grid = 0, lds = 0, k = 0;
    for (const Seg &sg : segs) {
        const int G = 64 >> sg.c->LGC;
        const int waves = (sg.nslots + G - 1) / G;
        static const int per_cu = getenv("QC_TIER_WG_PER_CU") ? std::max(1, atoi(getenv("QC_TIER_WG_PER_CU"))) : 32;     // (A/B switch)
        grid += std::min(waves, 256 * per_cu);
        t.seg_end[k] = grid; t.seg_code[k] = (sg.c->LCD << 4) | sg.c->LGC; t.seg_lab[k] = sg.c->LAB;
        t.seg_nslots[k] = sg.nslots; t.seg_words[k] = sg.c->slot_words; t.seg_slots[k] = sg.d_slots;
        lds = std::max(lds, sg.c->lds_bytes);
        ++k;
    }
    t.nseg = k;
    {   // (experiment switch: extra dynamic LDS per workgroup - does the build respond to the LDS the column kernels hold?)
        static const int pad_kb = getenv("QC_LDS_PAD_KB") ? atoi(getenv("QC_LDS_PAD_KB")) : 0;
        if (pad_kb > 0 && lds + pad_kb * 1024 <= QC_LDS_MAX) lds += pad_kb * 1024;
    }
    {   // segments of other bra classes than the unit's own: the merged wide-ket launch of the low bra classes
        bool mixed = false;
        for (const Seg &sg : segs) mixed = mixed || sg.c->LAB != unit / 2;
        if (mixed) {
            if (k > QC_MAXSEG) return QC_ERR_UNSUPPORTED;
            static const bool lds_dbg2 = getenv("QC_LDS_DEBUG") != nullptr;
            if (lds_dbg2) fprintf(stderr, "[lds] merged wide-ket launch of unit %d: %d workgroups (1 wave), %d bytes of LDS per workgroup, %d segments\n", unit, grid, lds, k);
            if (unit == 2 * 2 + 1) return qc_launch_tier1_low(grid, (size_t)lds, st, t);
            if (unit == 2 * 3 + 1) return qc_launch_tier1_mid(grid, (size_t)lds, st, t);
            if (unit == 2 * 5 + 1) return qc_launch_tier1_hi(grid, (size_t)lds, st, t);
            return QC_ERR_UNSUPPORTED;
        }
    }
    // a wide-ket launch made of d.d / f.p-ket buckets only (no basis function above d): the kernel variant without the f-ket bodies
    int tier = unit % 2;
    if (tier == 1) {
        bool only4 = true;
        for (const Seg &sg : segs) only4 = only4 && sg.c->LCD == 4;
        if (only4 && !S->has_fkets) tier = 2;      // (with f kets around, the d.d / f.p-ket classes may be in their matrix-core form: the f-capable kernel)
    }
    static const bool lds_dbg = getenv("QC_LDS_DEBUG") != nullptr;
    if (lds_dbg) {
        fprintf(stderr, "[lds] tier<%d,%d>: %d workgroups (1 wave), %d bytes of LDS per workgroup; segments:", unit / 2, tier, grid, lds);
        for (const Seg &sg : segs) fprintf(stderr, " <%d,%d,%d> %d slots %d B", sg.c->LAB, sg.c->LCD, sg.c->LGC, sg.nslots, sg.c->lds_bytes);
        fprintf(stderr, "\n");
    }
    return launch_tier(unit / 2, tier, grid, (size_t)lds, st, t);
}

static int launch_segments(qc_system *S, int unit, const std::vector<Seg> &segs, hipStream_t st, const QcKernelArgs &base) {
    return unit >= 2 * (QC_LPAIR + 1) ? launch_bm_segments(S, unit, segs, st, base) : launch_column_segments(S, unit, segs, st, base);
}

// Launch units of one build: per bra class LAB, tier 0 (LCD <= 3) and tier 1 (LCD >= 4) of the column kernels, plus
// the four bra-major launches (ket type x bra range); segments heaviest first.
static void tier_units(qc_system *S, std::vector<std::vector<int>> &units) {
    units.assign(QC_NUNITS, {});
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        const QcClass &c = S->classes[ci];
        if (c.slots.empty() && c.bundles.empty()) continue;
        units[qc_build_unit_of(S, c.LAB, c.LCD, c.bm)].push_back((int)ci);
    }
    for (auto &u : units)
        std::stable_sort(u.begin(), u.end(), [&](int x, int y) {
            const QcClass &a_ = S->classes[x], &b_ = S->classes[y];
            if (a_.LCD != b_.LCD) return a_.LCD > b_.LCD;              // long serial chains first
            return a_.flops_alg > b_.flops_alg;
        });
}

// (the launch units and their segments only change with the work lists: kept between builds, dropped by upload_slots)
static const QcLaunchPlan &launch_plan_of(qc_system *S) {
    if (!S->launch_plan) {
        S->launch_plan = new QcLaunchPlan();
        tier_units(S, S->launch_plan->units);
        for (const auto &u : S->launch_plan->units) {
            std::vector<Seg> v;
            for (int ci : u) v.push_back(seg_of(S->classes[ci]));
            S->launch_plan->segs.push_back(std::move(v));
        }
    }
    return *S->launch_plan;
}

// Profiling mode: one single-segment launch per class bucket (class_ms), or the real tier launches (unit_ms, QC_NUNITS entries), serial on
// the handle's stream with a hipEvent between consecutive launches.
int qc_time_units_serial(const QcBuild &b, float *class_ms, float *unit_ms) {
    qc_system *S = b.S;
    const std::vector<std::vector<int>> &units = b.plan.units;
    const size_t nev = (class_ms ? S->classes.size() : units.size()) + 1;
    EventList evl;
    if (evl.create(nev) != QC_OK) return QC_ERR_HIP;
    std::vector<hipEvent_t> &ev = evl.ev;
    QC_HIP_CHECK(hipEventRecord(ev[0], S->stream));
    if (class_ms) {
        for (size_t ci = 0; ci < S->classes.size(); ++ci) {
            const QcClass &c = S->classes[ci];
            if (!c.slots.empty() || !c.bundles.empty()) {
                int rc = launch_segments(S, qc_unit_of(c.LAB, c.LCD, c.bm), {seg_of(c)}, S->stream, b.a);
                if (rc != QC_OK) return rc;
            }
            QC_HIP_CHECK(hipEventRecord(ev[ci + 1], S->stream));
        }
    } else {
        for (size_t u = 0; u < units.size(); ++u) {
            if (!units[u].empty()) { int rc = launch_segments(S, (int)u, b.plan.segs[u], S->stream, b.a); if (rc != QC_OK) return rc; }
            QC_HIP_CHECK(hipEventRecord(ev[u + 1], S->stream));
        }
    }
    QC_HIP_CHECK(hipEventSynchronize(ev.back()));
    float *out = class_ms ? class_ms : unit_ms;
    for (size_t i = 0; i + 1 < nev; ++i) QC_HIP_CHECK(hipEventElapsedTime(&out[i], ev[i], ev[i + 1]));
    return QC_OK;
}

// one concurrent build: fork the side streams off the handle's stream, launch every unit on its stream (heaviest
// first), join.  `ev` (tuning only): [0] fork, [1] join, [2 + 2u], [3 + 2u] around unit u.
// (nofork: everything the launches depend on has completed - the host waited for the handle's stream after it was enqueued)
int qc_issue_build(const QcBuild &b, hipEvent_t *ev, bool per_unit, bool nofork) {
    qc_system *S = b.S;
    qc_stamp("to launch_concurrent");
    QcGateHold gate(S);                        // (cross-stream dependencies are created here and nowhere else: see QcGate)
    qc_stamp("gate");
    if (ev) QC_HIP_CHECK(hipEventRecord(ev[0], S->stream));
    static const bool force_fork = getenv("QC_FORCE_FORK") != nullptr;          // (A/B switch)
    const bool fork = ev != nullptr || !nofork || force_fork;
    if (fork) QC_HIP_CHECK(hipEventRecord(S->lanes.ev_fork, S->stream));
    S->join.wait_limit = qc_wait_limit(S);
    // Issue order (the host needs ~8 us per launch, so it matters): inside a stream heaviest first; across streams the
    // first launch of every stream before any second one, streams in the order of their total load - the chain that
    // ends the build gets going first and no stream sits empty while another one's queue is being filled.
    std::vector<int> q[QC_NSTREAMS];
    int ks[QC_NSTREAMS];
    {
        std::vector<int> byw = b.plan.active();
        // (an entry of unit_stream is lane | rank << 3: inside a lane the launches go out by rank, then heaviest first - the rank is how
        // the assignment search puts a lighter launch in front of a heavier one)
        std::stable_sort(byw.begin(), byw.end(), [&](int x, int y) {
            const int rx = S->assign.unit_stream[x] >> 3, ry = S->assign.unit_stream[y] >> 3;
            return rx != ry ? rx < ry : S->assign.unit_weight[x] > S->assign.unit_weight[y];
        });
        float load[QC_NSTREAMS] = {};
        for (int u : byw) { q[S->assign.unit_stream[u] & 7].push_back(u); load[S->assign.unit_stream[u] & 7] += S->assign.unit_weight[u]; }
        for (int k = 0; k < QC_NSTREAMS; ++k) ks[k] = k;
        std::stable_sort(ks, ks + QC_NSTREAMS, [&](int x, int y) { return load[x] > load[y]; });
    }
    // the most loaded chain runs on the handle's own stream: no fork hop before it, no join after it.
    // (with the dispatch lanes known, slot 0 is the slot on the pipe of the handle's own stream: its chain is the one that runs there -
    // any other choice would put two chains on one pipe; the longest-first rule gives slot 0 the heaviest launch anyway)
    const int kmain = S->lanes.lane0_is_main ? (q[0].empty() ? -1 : 0) : ks[0];
    const bool event_join = S->join.by_events;                   // (QC_EVENT_JOIN, or dispatches are serialised here: qc_device_init)
    // an earlier ASYNCHRONOUS build's wait gave up (qc_fock_*_device return before their build has run; every call that waits on the
    // host has looked at the word itself, qc_join_check): its result was not complete, and this is the first call that can say so
    if (!event_join) { int jrc = qc_join_check(S); if (jrc != QC_OK) return jrc; }
    qc_stamp("sorted");
    // the launches of the streams in use, interleaved (first launch of every stream before any second one), then the streams' markers of
    // the device-side join
    int set[QC_NSTREAMS], nset = 0;
    unsigned nside = 0;
    for (int k : ks) if (!q[k].empty()) { set[nset++] = k; if (k != kmain) ++nside; }
    size_t longest = 0;
    for (int i = 0; i < nset; ++i) longest = std::max(longest, q[set[i]].size());
    for (size_t pos = 0; pos < longest; ++pos)
        for (int i = 0; i < nset; ++i) {
            const int k = set[i];
            if (pos >= q[k].size()) continue;
            const int u = q[k][pos];
            hipStream_t st = k == kmain ? S->stream : S->lanes.side[S->lanes.slot_side[k]];
            if (pos == 0 && k != kmain && fork) QC_HIP_CHECK(hipStreamWaitEvent(st, S->lanes.ev_fork, 0));
            if (ev && per_unit) QC_HIP_CHECK(hipEventRecord(ev[2 + 2 * u], st));
            int rc = launch_segments(S, u, b.plan.segs[u], st, b.a);
            if (rc != QC_OK) return rc;
            qc_stamp("launch");
            if (ev && per_unit) QC_HIP_CHECK(hipEventRecord(ev[3 + 2 * u], st));
        }
    if (event_join) {
        for (int k = 0; k < QC_NSTREAMS; ++k) {
            if (q[k].empty() || k == kmain) continue;
            QC_HIP_CHECK(hipEventRecord(S->lanes.ev_join[k], S->lanes.side[S->lanes.slot_side[k]]));
            QC_HIP_CHECK(hipStreamWaitEvent(S->stream, S->lanes.ev_join[k], 0));
        }
    } else {
        // (test hook QC_JOIN_FAULT: the first side stream's marker is left out - a join that can never complete, as if a launch on
        // that stream had died: the waiting kernel runs into its limit and the call that waits for this build must fail)
        const bool fault = getenv("QC_JOIN_FAULT") != nullptr;
        for (int i = 0; i < nset; ++i)
            if (set[i] != kmain && !(fault && i == (set[0] == kmain ? 1 : 0))) qc_join_mark(S->lanes.side[S->lanes.slot_side[set[i]]], S->dev.d_join.p);
        if (hipGetLastError() != hipSuccess) return QC_ERR_HIP;
        qc_stamp("markers");
        if (nside) {
            S->join.target += nside;
            if (qc_join_wait(S, S->dev.d_join.p, S->join.target, false, S->tl.cur ? S->tl.cur + QC_TL_W * QC_NUNITS : nullptr) != QC_OK) return QC_ERR_HIP;
            gate.waits = true;
            qc_stamp("wait kernel");
        }
    }
    if (ev) QC_HIP_CHECK(hipEventRecord(ev[1], S->stream));
    static const bool join_check = getenv("QC_JOIN_CHECK") != nullptr;       // (diagnostic: after every build the device counter is the host's target)
    if (join_check && !event_join) {
        unsigned c = 0;
        QC_HIP_CHECK(hipDeviceSynchronize());
        QC_HIP_CHECK(hipMemcpy(&c, S->dev.d_join.p, sizeof(c), hipMemcpyDeviceToHost));
        if (c != S->join.target) { fprintf(stderr, "qchem_hip: join counter %u, target %u (%u side streams)\n", c, S->join.target, nside); return QC_ERR_HIP; }
    }
    return QC_OK;
}

// One build: the launch units of the plan on the streams the assignment gives them, joined on the handle's stream.  The first build of
// a shard times the units and assigns them first; later builds may carry an instalment of the assignment search.
// Profiling mode (class_ms or unit_ms non-null): serial timed launches only (time_units_serial).
int qc_launch_fock_classes(qc_system *S, const QcFockArgs &fa, float *class_ms, float *unit_ms, bool nofork) {
    const QcBuild b{S, fa, base_args(S, fa), launch_plan_of(S)};
    if (class_ms || unit_ms) return qc_time_units_serial(b, class_ms, unit_ms);
    int rc;
    if (S->assign.unit_ms.size() != b.plan.units.size()) {
        if ((rc = qc_first_build(b)) != QC_OK) return rc;
        nofork = false;                                  // the side streams must see its memset (and the timing passes) finished
    }
    S->assign.on.builds += 1;
    if (qc_search_due(S, fa)) {
        if ((rc = qc_search_instalment(b)) != QC_OK) return rc;
        nofork = false;
    }
    return qc_issue_build(b, nullptr, false, nofork);
}

// Everything of a fixed-point build that depends on the densities alone, enqueued ahead of time (the SCF pass does this as soon as
// its new density exists, so that it runs while the host turns around): zeroed accumulator planes, this build's fixed-point unit,
// the UHF density sum.  qc_fock_build_device recognises the densities and then goes straight to the class kernels.
int qc_fock_prepare_device(qc_system *S, const double *dDa, const double *dDb, bool uhf, const void *owner, bool scale_done) {
    S->prep.prepared = false;
    S->prep.enqueued = false;
    if (!S->accum_fx) return QC_OK;
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n, plane = (size_t)QC_NREP * (uhf ? 2 : 1) * nn;
    // (the closing fold of the last build zeroes the replicas it reads: no memset then)
    const bool zero = !(S->prep.gt_clean && S->prep.gt_clean_nspin == (uhf ? 2 : 1));
    if (zero) QC_HIP_CHECK(hipMemsetAsync(S->dev.d_Gtmp.p, 0, 2 * plane * sizeof(double), S->stream));
    S->prep.gt_clean = true; S->prep.gt_clean_nspin = uhf ? 2 : 1;
    if (!scale_done) qc_fx_scale(S->stream, n, dDa, uhf ? dDb : nullptr, S->imax, S->dev.d_fxs.p);
    if (uhf) qc_axpby(S->stream, n, 1.0, dDa, 1.0, dDb, S->dev.d_Dj.p);
    // (the build that finds these preliminaries starts its side streams without a fork event: whoever lets the host go on before the
    // handle's stream has drained must know that something was put on it here)
    S->prep.enqueued = zero || !scale_done || uhf;
    S->prep.prepared = true; S->prep.Da = dDa; S->prep.Db = uhf ? dDb : nullptr; S->prep.owner = owner;
    return QC_OK;
}

int qc_fock_build_device(qc_system *S, const double *dDa, const double *dDb, double *dGa, double *dGb, bool uhf, int *twin_cache,
                         const double *dH, double *dFa, double *dFb, bool *f_done, const void *owner) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    const bool fx = S->accum_fx != 0;
    const double *fxs = fx ? S->dev.d_fxs.p : nullptr;
    // Spin symmetry: the reference evaluates both spins with identical arithmetic (uhf.rs:210-227), so bitwise-equal
    // densities give bitwise-equal G (its closed-shell UHF never breaks symmetry).  The fixed-point
    // accumulation keeps that property by construction: every contribution is the same sequence of operations for either
    // spin and integer sums do not depend on their order.  Only the f64-atomic mode (kept for A/B measurements) needs help:
    // there equal spins are detected and digested once.  Inside an SCF run the answer cannot change, so the drivers pass a
    // cache and only their first build pays the host round trip.
    bool twin = false;
    if (uhf && !fx) {
        if (twin_cache && *twin_cache >= 0) twin = *twin_cache != 0;
        else {
            int diff = 1;
            QC_HIP_CHECK(hipMemsetAsync(S->dev.d_flag.p, 0, sizeof(int), st));
            qc_count_diff(st, nn, dDa, dDb, S->dev.d_flag.p);
            QC_HIP_CHECK(hipMemcpyAsync(&diff, S->dev.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
            QC_HIP_CHECK(hipStreamSynchronize(st));
            twin = (diff == 0);
            if (twin_cache) *twin_cache = twin ? 1 : 0;
        }
    }
    const bool two = uhf && !twin;
    const int nspin = two ? 2 : 1;
    // accumulation phase: zero the replicas, density sum, every class kernel on the side streams, replica fold
    const size_t plane = (size_t)QC_NREP * nspin * nn;          // one accumulator plane: [replica][spin][n*n]
    const bool ready = fx && S->prep.prepared && owner != nullptr && S->prep.owner == owner && S->prep.Da == dDa && S->prep.Db == (uhf ? dDb : nullptr);   // qc_fock_prepare_device ran for these
    S->prep.prepared = false;
    QcFockArgs a{};
    // Replicas in use (the planes keep their layout): 8 for n <= 64, all 32 above.  Replicas spread the atomics of hot elements, and the
    // closing fold reads and zeroes every one of them: at n = 58 that is 1.7 MB with 32 replicas, and the H2O/cc-pVTZ iteration takes 0.308 ms
    // with 8 against 0.313 with 32 (0.312 with 16, 0.319 with 4, 0.349 with 2; three alternating runs each); benzene/cc-pVDZ (n = 114) shows
    // no difference between 8, 16 and 32.  QC_NREP_USE: experiment switch.
    const char *nrep_s = getenv("QC_NREP_USE");                 // (read per build: a test switches it inside one process)
    const int nrep_env = nrep_s ? std::max(1, std::min(QC_NREP, atoi(nrep_s))) : 0;
    const int nrep_use = nrep_env ? nrep_env : (n <= 64 ? 8 : QC_NREP);
    a.nrep = nrep_use; a.rep_stride = nspin * nn; a.fxs = fxs; a.fx_lo = plane;
    if (!ready) {
        QC_HIP_CHECK(hipMemsetAsync(S->dev.d_Gtmp.p, 0, (fx ? 2 : 1) * plane * sizeof(double), st));
        if (fx) qc_fx_scale(st, n, dDa, uhf ? dDb : nullptr, S->imax, S->dev.d_fxs.p);      // this build's fixed-point unit, from its densities
    }
    S->prep.gt_clean = false;                                    // (the class kernels are about to accumulate into the planes)
    if (uhf) {
        if (!ready) qc_axpby(st, n, 1.0, dDa, 1.0, dDb, S->dev.d_Dj.p);
        a.Dj = S->dev.d_Dj.p; a.Dk0 = dDa; a.Dk1 = two ? dDb : nullptr; a.cK = 1.0;
    } else {
        a.Dj = dDa; a.Dk0 = dDa; a.Dk1 = nullptr; a.cK = 0.5;
    }
    a.G0 = S->dev.d_Gtmp.p; a.G1 = S->dev.d_Gtmp.p + nn;
    int rc = qc_launch_fock_classes(S, a, nullptr, nullptr, ready);
    if (rc != QC_OK) return rc;
    if (fx && !S->comm && S->nranks == 1) {
        // (one launch instead of fold + symmetrise: nothing needs the folded planes)
        qc_fold_symmetrize(st, n, nrep_use, nspin * nn, S->dev.d_Gtmp.p, plane, dGa, dH, dH ? dFa : nullptr, fxs, S->tl.cur ? S->tl.cur + QC_TL_W * (QC_NUNITS + 1) : nullptr);
        if (two) qc_fold_symmetrize(st, n, nrep_use, nspin * nn, S->dev.d_Gtmp.p + nn, plane, dGb, dH, dH ? dFb : nullptr, fxs);
        S->prep.gt_clean = true; S->prep.gt_clean_nspin = nspin;      // every replica element of the planes in use was read and zeroed
    } else {
        qc_reduce_replicas(st, nspin * nn, nrep_use, nspin * nn, S->dev.d_Gtmp.p, S->dev.d_Gred.p, fx, plane);
        // partial Fock matrices -> full, one all-reduce per build ([Ga|Gb] concatenated for UHF; hi and lo planes back to
        // back).  Fixed-point partials are summed as integers: the result is bit-identical on every rank, whatever the ring
        // order.  (Against a build with another shard layout - the single-GPU build included - it agrees to ~1e-13, not bit for
        // bit: the bra-major kernels pre-sum the exchange rows of a 64-ket bundle in an f64 LDS buffer, and which kets share a
        // bundle depends on the shard.)
        if (S->comm && qc_rccl().AllReduce(S->dev.d_Gred.p, S->dev.d_Gred.p, (fx ? 2 : 1) * nspin * nn, fx ? ncclInt64 : ncclDouble, ncclSum, (ncclComm_t)S->comm, st) != ncclSuccess) return QC_ERR_RCCL;
        qc_symmetrize_add(st, n, S->dev.d_Gred.p, nspin * nn, dGa, dH, dH ? dFa : nullptr, fxs);
        if (two) qc_symmetrize_add(st, n, S->dev.d_Gred.p + nn, nspin * nn, dGb, dH, dH ? dFb : nullptr, fxs);
    }
    if (uhf && !two) QC_HIP_CHECK(hipMemcpyAsync(dGb, dGa, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (f_done) *f_done = dH != nullptr && dFa != nullptr && (!uhf || (two && dFb != nullptr));
    return QC_OK;
}

// ---- Unsplit work lists (every quartet complete in one slot / one-ket bundles) for the passes outside a build: the Schwarz pass takes the
// (P|P) quartets of every class, the ERI-tensor launch all of them.  The lists of all classes are packed into ONE blob, 256-byte aligned -
// one allocation, one copy, one wait for the whole pass: an allocation, two synchronous copies and a wait per class made the Schwarz pass
// 4 ms for H2O/cc-pVTZ, most of a cold handle's set-up; 3.6 ms still with one wait but 35 allocations and 50 copies.
// kind 0: slots, 1: bundles (off_a) + ket units (off_b), 2: p.p kets of a bra-major class through the column kernels, which have these modes
struct UnsplitJob { const QcClass *c; int kind; size_t off_a, off_b; int count, lds; QcClass col; };
static void unsplit_jobs(const qc_system *S, bool diagonal_only, std::vector<UnsplitJob> &jobs, QcBlob &blob) {
    std::vector<QcSlot> slots;
    std::vector<QcBundle> bundles; std::vector<int> ketlist;
    std::vector<QcTask> diag;
    jobs.reserve(S->classes.size());
    for (const auto &c : S->classes) {
        if (diagonal_only) {
            diag.clear();
            for (const auto &t : c.tasks) if (t.bra == t.ket) diag.push_back(t);
        }
        const std::vector<QcTask> &tasks = diagonal_only ? diag : c.tasks;
        if (tasks.empty()) continue;
        UnsplitJob j{&c, 0, 0, 0, 0, 0, QcClass{}};
        if (c.bm && c.LCD != 2) {
            j.kind = 1;
            const bool packed = qc_make_bundles(S, tasks, 0, bundles, ketlist);
            std::vector<QcBundleDev> hb; std::vector<QcKetUnit> hu;
            qc_bm_device_lists(S, c.LCD, bundles, ketlist, packed, hb, hu);
            j.off_a = blob.put(hb.data(), hb.size() * sizeof(QcBundleDev)); j.off_b = blob.put(hu.data(), hu.size() * sizeof(QcKetUnit));
            j.count = (int)bundles.size();
            int mx = 0;
            for (const auto &t : tasks) mx = std::max(mx, qc_bm_wave_words(c.LAB, S->pairs[t.bra].na * S->pairs[t.bra].nb, S->pairs[t.ket].na * S->pairs[t.ket].nb));
            j.lds = mx * 8;
        } else {
            // LDS per lane group over the class's whole task list (qc_build_shards): slot_words / lds_bytes follow the screened shard
            // and are too small - zero for a class that keeps nothing - for the quartets a threshold has dropped from the builds
            if (c.bm) j.kind = 2;
            j.col.LAB = c.LAB; j.col.LCD = c.LCD; j.col.LGC = c.col_lgc; j.col.slot_words = c.col_slot_words; j.col.lds_bytes = c.col_lds_bytes;
            qc_make_slots(S, tasks, 0, false, slots);
            j.off_a = blob.put(slots.data(), slots.size() * sizeof(QcSlot)); j.count = (int)slots.size();
        }
        if (j.count) jobs.push_back(std::move(j));
    }
}
// (`j` must not move while its launch is in flight: the column-kernel copy of its class is referred to by address)
static int launch_unsplit(qc_system *S, const UnsplitJob &j, const unsigned char *d_blob, hipStream_t st, const QcKernelArgs &a) {
    if (j.kind == 1)
        return launch_segments(S, qc_unit_of(j.c->LAB, j.c->LCD, true), {Seg{j.c, nullptr, j.count, reinterpret_cast<const QcBundleDev *>(d_blob + j.off_a),
                                                                            reinterpret_cast<const QcKetUnit *>(d_blob + j.off_b), j.lds}}, st, a);
    const QcClass *cls = &j.col;
    return launch_segments(S, qc_unit_of(cls->LAB, cls->LCD, false), {Seg{cls, reinterpret_cast<const QcSlot *>(d_blob + j.off_a), j.count}}, st, a);
}

// Schwarz pass (the reference's own TODO at uhf.rs:49-50): the (P|P) quartet of every stored pair through the
// class kernels in their `schwarz_out` mode - unsplit slots / one-ket bundles, once per geometry.
int qc_schwarz_device(qc_system *S) {
    const size_t np = S->pairs.size();
    QcDev<double> dq;
    if (dq.alloc(np) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(dq.p, 0, np * sizeof(double), S->stream));
    QcFockArgs fa{};
    fa.schwarz_out = dq.p;
    const QcKernelArgs a = base_args(S, fa);
    std::vector<UnsplitJob> jobs;
    QcBlob blob;
    unsplit_jobs(S, true, jobs, blob);
    QcDev<unsigned char> dblob;
    if (!blob.bytes.empty()) {
        if (dblob.alloc(blob.bytes.size()) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemcpyAsync(dblob.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, S->stream));
    }
    // The launches are independent (each writes its own pairs' entries) and most of them are a few waves working through one long
    // unsplit slot each (an s.s pair of eight primitives: 4096 primitive quartets in one lane group): their durations add up on one
    // stream - 3.5 ms for the 35 classes of H2O/cc-pVTZ - so they go round the dispatch lanes, heaviest classes first.
    const int nl = std::max(1, std::min(S->lanes.nlanes, QC_NSTREAMS));
    if (nl > 1) QC_HIP_CHECK(hipStreamSynchronize(S->stream));    // (the side streams start behind the memset and the copy)
    std::stable_sort(jobs.begin(), jobs.end(), [](const UnsplitJob &x, const UnsplitJob &y) { return x.c->LAB + x.c->LCD > y.c->LAB + y.c->LCD; });
    auto sync_all = [&]() -> hipError_t {
        hipError_t e = hipStreamSynchronize(S->stream);
        for (int k = 1; k < nl; ++k) { const hipError_t e2 = hipStreamSynchronize(S->lanes.side[S->lanes.slot_side[k]]); if (e == hipSuccess) e = e2; }
        return e;
    };
    for (size_t i = 0; i < jobs.size(); ++i) {
        const int lane = (int)(i % nl);
        const int rc = launch_unsplit(S, jobs[i], dblob.p, lane == 0 ? S->stream : S->lanes.side[S->lanes.slot_side[lane]], a);
        if (rc != QC_OK) { (void)sync_all(); return rc; }
    }
    QC_HIP_CHECK(sync_all());
    S->pairQ.assign(np, 0.0);
    QC_HIP_CHECK(hipMemcpy(S->pairQ.data(), dq.p, np * sizeof(double), hipMemcpyDeviceToHost));
    S->imax = 0.0;
    for (double q : S->pairQ) S->imax = std::max(S->imax, q * q);
    return QC_OK;
}

// molint::eri replacement (qc_eri_full, MP2, stored Fock mode): every quartet complete in one slot + plain stores; the classes' launches
// serial on the handle's stream, in class order, one wait at the end
int qc_launch_eri_full(qc_system *S, double *d_out) {
    QcFockArgs fa{};
    fa.eri_out = d_out;
    const QcKernelArgs a = base_args(S, fa);
    std::vector<UnsplitJob> jobs;
    QcBlob blob;
    unsplit_jobs(S, false, jobs, blob);
    if (jobs.empty()) return QC_OK;
    QcDev<unsigned char> dblob;
    if (dblob.alloc(blob.bytes.size()) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dblob.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, S->stream));
    int rc = QC_OK;
    for (size_t i = 0; i < jobs.size() && rc == QC_OK; ++i) rc = launch_unsplit(S, jobs[i], dblob.p, S->stream, a);
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));      // (the blob and the jobs live until their launches have run)
    return rc;
}
