// qc_internal.h - shared declarations of libqchem_hip.so (host model, device buffers, kernel launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/qchem_hip.h"

constexpr int QC_LMAX = 3;              // highest shell angular momentum with kernels (f)
constexpr int QC_LPAIR = 2 * QC_LMAX;   // highest pair angular momentum
constexpr int QC_LTOT = 4 * QC_LMAX;    // highest Hermite order of an ERI
constexpr int QC_SLOT_ITMAX = 128;
constexpr int QC_LREG = 4;               // total Hermite orders up to this keep the R table in registers (bra-major kernels; Boys branch)
constexpr int QC_LHOIST_DPP = 6;         // column kernels: up to this the lanes of a group evaluate several primitive quartets' tables at once
// ... this many per chunk: the parked tables limit the resident waves, and with four groups per wave (16-lane groups) at L = 5
// ((pp|dp), the largest such class) four tables beat eight by 13 %; elsewhere eight win by 3 %
__host__ __device__ constexpr int qc_hoist_chunk(int L, int lgc) { return (L == 5 && lgc == 4) ? 4 : 8; }
__host__ __device__ constexpr bool qc_hoisted(int L) { return L <= QC_LHOIST_DPP; }
// doubles at the head of a lane group's LDS region: the hoisted register tables of one chunk + their (pref, ij/kl)
// records, or the cooperative R work array
__host__ __device__ constexpr int qc_region0(int L, int lgc) {
    return qc_hoisted(L) ? qc_hoist_chunk(L, lgc) * ((((L + 1) * (L + 2) * (L + 3) / 6) | 1) + 2) : (L + 1) * (L + 2) * (L + 3) * (L + 4) / 24;
}
      // primitive quartets per slot
constexpr double QC_PRIM_CUTOFF = 1e-17; // primitive pairs whose Hermite expansion block is entirely below this are dropped (weak shell pairs: QC_PRIM_REL, qc_system.cpp)
constexpr int QC_NREP = 32;             // replicas of the Fock accumulation buffer
constexpr int QC_FX_MAXBITS = 52;       // fixed-point accumulation: finest unit 2^-52 Eh; the scale of a build follows its density (qc_fx_scale)
constexpr double QC_SCHWARZ_TAU = 1e-12; // quartets with sqrt((ab|ab) (cd|cd)) below this are not evaluated (default)
constexpr int QC_LDS_MAX = 160 * 1024;  // LDS of a gfx950 CU, the cap the kernels with dynamic LDS are allowed
#ifndef QC_NSTREAMS_N
#define QC_NSTREAMS_N 7
#endif
constexpr int QC_NSTREAMS = QC_NSTREAMS_N;  // class kernels of one build run concurrently on this many streams (compile-time: A/B builds)
constexpr int QC_NUNITS = 2 * (QC_LPAIR + 1) + 6;   // launch units of one build: (LAB, tier) of the column kernels + the bra-major launches (ket ss / ps / pp x bra range)

__host__ __device__ constexpr int qc_nherm(int L) { return (L + 1) * (L + 2) * (L + 3) / 6; }
// Classes whose two Hermite contractions run as f64 MFMA tiles (one slot per wave): high-order kets against bras with
// enough Hermite functions to fill 16-row tiles.  Measured on H2O/cc-pVTZ and benzene/cc-pVDZ: below these bounds the
// padded tiles and the lost second slot per wave cost more than the LDS reads they save.
// (round 4: d.d / f.p kets - LCD = 4 - too, in their 64-lane instances: a class whose list cannot fill the chip is a latency chain of single
// waves, and there the tile form with one wave per 16-column tile is shorter - (dd|dd) of H2O/cc-pVTZ 57 us per workgroup in the VALU
// form; lists that do fill the chip keep the 32-lane VALU instances with two slots per wave, qc_build_model)
__host__ __device__ constexpr bool qc_use_mfma(int LAB, int LCD) { return LCD >= 4 && LAB >= 3; }
// (... the classes that are ALWAYS on the matrix cores)
__host__ __device__ constexpr bool qc_mfma_always(int LAB, int LCD) { return LCD >= 5 && LAB >= 3; }
// Gather records of the matrix-core classes' step 2 (A operand = R values at h1 + h2): per class (LAB 3..6, LCD 4..6) one 16-byte record
// per (k-step, lane); classes concatenated in (LAB, LCD) order, class (LAB, LCD) starts at record qc_gidx_off(LAB, LCD)
__host__ __device__ constexpr int qc_gidx_ksteps(int LCD) { return ((LCD + 1) * (LCD + 2) * (LCD + 3) / 6 + 3) / 4; }
__host__ __device__ constexpr int qc_gidx_off(int LAB, int LCD) {
    int o = 0;
    for (int a = 3; a <= 6; ++a)
        for (int c = 4; c <= 6; ++c) { if (a == LAB && c == LCD) return o; o += 64 * qc_gidx_ksteps(c); }
    return o;
}
__host__ __device__ constexpr int qc_ncart(int L) { return (L + 1) * (L + 2) / 2; }
// Hermite index of (t,u,v): grouped by total order N = t+u+v, then t descending, then u descending.
__host__ __device__ constexpr int qc_hidx(int t, int u, int v) {
    return (t + u + v) * (t + u + v + 1) * (t + u + v + 2) / 6 + (u + v) * (u + v + 1) / 2 + v;
}
// size of the Hermite-Coulomb work array sum_{n=0..L} nherm(L-n) = C(L+4,4)
// doubles per primitive-pair block: header [p,Px,Py,Pz] + E (nherm x nab), padded to a multiple of 4 (32-byte rows)
__host__ __device__ constexpr int qc_pair_stride(int L, int nab) { return (4 + qc_nherm(L) * nab + 3) & ~3; }
__host__ __device__ constexpr int qc_rwork(int L) { return (L + 1) * (L + 2) * (L + 3) * (L + 4) / 24; }
// Recurrence plan of the cooperative Hermite-Coulomb table (qc_build_r): one 8-byte record per entry (n; t,u,v) with t+u+v >= 1,
// stage by stage; plans of all orders L are concatenated, L's starts at qc_plan_off(L)
__host__ __device__ constexpr int qc_nplan(int L) { return qc_rwork(L) - (L + 1); }
__host__ __device__ constexpr int qc_plan_off(int L) { int o = 0; for (int l = 0; l < L; ++l) o += qc_nplan(l); return o; }

struct QcShell {
    int atom, L, pure, nprim, ncart, nfunc, off;
    double A[3];
    std::vector<double> exps, coefs;  // coefs include the (L,0,0) primitive norm
    std::vector<double> T;            // nfunc x ncart, rows scaled to unit self-overlap
};

// Device-visible pair descriptor (10 ints)
struct QcPairDesc {
    int doff;     // offset (in doubles) of this pair's primitive blocks in the pair-data array
    int K;        // primitive pairs
    int na, nb;   // basis functions of shell A / B
    int offa, offb;
    int L;        // la + lb
    int shA_eq_shB;
    int psoff;    // ps and pp pairs: offset (doubles) of the packed primitive records in the pspack array, else -1
    int psperm;   // ps pairs: basis function of Cartesian axis a = (psperm >> 2a) & 3; pp pairs: the same for shell A, and for shell B from bit 6
};

struct QcTask { int bra, ket; };  // pair indices; (bra|ket) is one unique shell quartet
struct QcSlot { int bra, ket, lo, hi, c0, c1; };  // a quartet restricted to primitive quartets [lo, hi) and ket columns [c0, c1): the kernels' work unit
// Work unit of the bra-major kernels (narrow kets, qc_fock_bm.hip): one wave = one bra pair restricted to the bra
// primitive pairs [ij_lo, ij_hi), against up to 64 ket pairs (one per lane) ketlist[first .. first + nket).
struct QcBundle { int bra, ij_lo, ij_hi, first, nket, maxK, pad0, pad1; };
// Device forms of the bra-major work lists (qc_bm_device_lists): the bundle with what the kernel needs of its bra pair (so that it is
// one scalar load), the lane's unit with what it needs of the ket pair (no look-up in the pair table between the list and the
// primitive records).  nanb = na | nb << 8 | shA_eq_shB << 16;  cd = offa | offb << 16 of the ket pair;
// info = primitives of the unit | (nb == 1) << 16 | shA_eq_shB << 17 | psperm << 18;  koff = offset (doubles) of the unit's first
// primitive record in the pair data (ss kets) or in pspack (ps kets).
// LDS doubles of one wave of a bra-major launch: its block I[nab * ncd][65] and, for the high bras (LAB >= 3) against ss kets, the
// staged expansion block E[nab][HAB] of the current bra primitive pair (step 3 of qc_bm_pass)
inline int qc_bm_wave_words(int LAB, int nab, int ncd) { return nab * ncd * 65 + (LAB >= 3 && ncd == 1 ? ((nab * qc_nherm(LAB) + 1) & ~1) : 0); }
struct alignas(16) QcBundleDev { int bra, ij_lo, ij_hi, first, nket, maxK, bdoff, offa, offb, nanb, pad0, pad1; };
struct alignas(16) QcKetUnit { int ket, koff, cd, info; };

struct QcClass {
    int LAB, LCD, LGC;            // Hermite orders of bra / ket pairs; log2 of the lane-group width C
    std::vector<QcTask> tasks;    // all unique quartets of this launch bucket (full list)
    std::vector<QcTask> shard;    // the ones this rank digests
    std::vector<QcSlot> slots;    // `shard` cut into primitive-quartet ranges of at most QC_SLOT_ITMAX, longest first
    QcSlot *d_slots = nullptr;    // device copy of `slots`
    int slot_words = 0;           // LDS doubles per lane group
    int lds_bytes = 0;
    int col_slot_words = 0, col_lds_bytes = 0, col_lgc = 0;   // the same for the column kernels over the WHOLE task list: what the passes outside a build launch (a pp-ket bra-major class goes through the column kernels there)
    // bra-major classes (ket = ss or ps pair, LAB + LCD <= QC_LREG): `bundles` replace `slots`
    bool bm = false;
    int bm_rows = 0;              // most bra functions (na + nb) of a bundle: rows of the kernels' exchange buffer
    std::vector<QcBundle> bundles;
    std::vector<int> ketlist;
    bool ket_packed = false;      // ketlist entries are packed (pair, first primitive, length) chunks, not plain pair indices (qc_make_bundles)
    QcBundleDev *d_bundles = nullptr;
    QcKetUnit *d_ketlist = nullptr;
    // work model of `shard`
    int64_t prim_quartets = 0;
    double bytes_alg = 0, flops_alg = 0;
};

// Owning device allocation of `count` objects T.  alloc: QC_OK or QC_ERR_HIP; a zero count leaves p null and succeeds.
template <class T> struct QcDev {
    T *p = nullptr;
    QcDev() = default;
    QcDev(const QcDev &) = delete; QcDev &operator=(const QcDev &) = delete;
    int alloc(size_t count) { return !count || hipMalloc(&p, count * sizeof(T)) == hipSuccess ? QC_OK : QC_ERR_HIP; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    ~QcDev() { reset(); }
};
using DevBuf = QcDev<double>;
// host copy of several lists that go to the device in one piece; put: the offset of the copy, 256-byte aligned
struct QcBlob {
    std::vector<unsigned char> bytes;
    size_t put(const void *src, size_t n) { const size_t off = (bytes.size() + 255) & ~(size_t)255; bytes.resize(off + n); if (n) std::memcpy(bytes.data() + off, src, n); return off; }
};
// a member struct of the handle back in its initial state: what it owned is released by its members' destructors
template <class T> void qc_renew(T &x) { x.~T(); new (&x) T(); }
inline double qc_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// QC_SETUP_DEBUG: "[tag] what   ms since the last lap" (qc_build_model, qc_device_init, scf_begin)
struct QcLap {
    const char *tag; bool on; double tt = qc_now_ms();
    void operator()(const char *what) { if (on) { const double t = qc_now_ms(); fprintf(stderr, "[%s] %-28s %.3f ms\n", tag, what, t - tt); tt = t; } }
};

// ---- the device side of a handle, in parts (qc_device.cpp sets them up and tears them down)
// what the kernels read and write: filled by qc_device_init in this order, released as a whole by qc_device_free
struct QcDeviceData {
    QcDev<double> d_pairdata, d_pairdataT, d_pspack;
    QcDev<QcPairDesc> d_pairs;
    QcDev<double> d_boys;
    QcDev<int> d_rplan;          // recurrence plans of the Hermite-Coulomb tables (qc_build_rplan)
    QcDev<unsigned> d_gidx;      // gather records of the matrix-core classes (qc_build_gidx)
    QcDev<double> d_D, d_G;      // 2 * n*n each (alpha/beta or Dj/Dk)
    QcDev<double> d_Gtmp;        // accumulation target: [plane (hi, lo)][replica][spin][n*n]
    QcDev<double> d_Gred;        // replicas folded: [plane][spin][n*n]
    QcDev<double> d_Dj;
    QcDev<double> d_fxs;         // [2^S, 2^-S]: fixed-point scale of the current build
    QcDev<int> d_flag;
    QcDev<unsigned char> d_lists; // the work lists of all classes (QcClass::d_slots / d_bundles / d_ketlist point into it)
    QcDev<unsigned> d_join;      // [0] counter of the device-side join of a build's side streams (qc_join_mark / qc_join_wait);
                                 // [3] scratch of the lane probe's markers, [4] counter of the spin-parallel Roothaan steps
};
// Side streams, their events and the dispatch lanes measured on them (qc_lane_probe): the chip dispatches at most FOUR kernels at a
// time - hardware queues sit in pairs on four pipes, and a pipe works on one dispatch until all its workgroups are launched.
// slot_side[k] = side stream behind assignment slot k; the first `nlanes` slots are on distinct pipes, slot 0 on the pipe of the handle's
// own stream (when one of the side streams shares it).  A handle that goes away leaves this struct, with its own stream, in the stream pool.
struct QcLanes {
    hipStream_t side[QC_NSTREAMS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[QC_NSTREAMS] = {};
    int slot_side[QC_NSTREAMS] = {0, 1, 2, 3, 4, 5, 6};
    int nlanes = QC_NSTREAMS;
    bool lane0_is_main = false;
    bool lanes_probed = false;               // slot_side / nlanes were measured on this handle's own stream set (qc_lane_probe)
};
// device-side joins of the handle's streams (qc_streams.hip); the counters they wait for are d_join
struct QcJoin {
    unsigned target = 0;                     // join counter of a build's side streams (d_join[0])
    unsigned spin_target = 0;                // join counter of the spin-parallel Roothaan steps (d_join[4])
    long long wait_limit = 0;                // device-side waits give up after this many ticks of the 100 MHz clock (qc_wait_limit)
    std::atomic<bool> waits_in_flight{false}; // device-side waits were issued and the host has not seen the handle's stream drained since (qc_gate)
    bool by_events = false;                  // dispatches are serialised here (qc_join_probe): the side streams are joined through events
    int *h_timeout = nullptr;                // pinned (freed by qc_device_free): set by a device-side wait that gave up (the launches it waited for never finished)
};
// accumulators zeroed, fixed-point scale (and the UHF density sum) already enqueued for a build from exactly these densities, and the host
// has waited for the handle's stream since (qc_fock_prepare_device): the build then starts its side streams without a fork
struct QcPrepared {
    bool prepared = false;
    bool gt_clean = false;                   // the accumulator planes (d_Gtmp) are known to be zero for the layout `gt_clean_nspin` (left so by the closing fold)
    int gt_clean_nspin = 0;
    const double *Da = nullptr, *Db = nullptr;
    const void *owner = nullptr;             // the qc_scf_state that enqueued them (addresses alone could be recycled by a later state)
    bool enqueued = false;                   // qc_fock_prepare_device put work on the handle's stream (see scf_iterate)
    void invalidate() { prepared = false; gt_clean = false; }   // nothing on the handle's stream or in the planes may be taken for granted
};
// refinement of the stream assignment in instalments paid for by use (qc_assign.hip, "Refinement of the stream assignment")
struct QcOnline {
    bool frozen = false;
    std::vector<int> best, trial;
    std::vector<std::vector<int>> nb, tried;   // neighbourhood of `best` (swept in order from nb_pos) / every assignment measured so far
    size_t nb_pos = 0;
    std::vector<std::vector<int>> cands;   // proposals of the first build (longest-first on in-build durations): tried before random neighbours
    double base_ms = 0.0;                  // build time of `best` as the search measured it
    bool seeded = false;                   // the proposals of the instrumented builds have been made (first instalment of the search)
    int trials = 0, rejects = 0, kicks = 0;   // (kicks: restarts of the local search from a perturbed copy of the best assignment known)
    long builds = 0, spent = 0;            // builds asked of this handle / extra builds the search has run
    unsigned rng = 2463534242u;
    double seen_sum = 0.0; long seen_n = 0;   // build times reported by SCF passes under the current assignment
    // finals (qc_fock_feedback): the three fastest assignments of the search, sampled inside SCF passes - a build that follows a Roothaan
    // step and a host turn-around is not the back-to-back build the search times, and which of them is fastest THERE differs
    std::vector<std::pair<float, std::vector<int>>> top;
    std::vector<double> fin_sum; std::vector<int> fin_n;
    int fin_cur = 0;
    bool settled = false;                     // search and finals are over
};
struct QcAssign {
    std::vector<float> unit_ms;              // measured serial time of each launch unit (autotuned once per shard)
    std::vector<int> unit_stream;            // side stream of each launch unit (longest-processing-time assignment)
    std::vector<float> unit_weight;          // durations that order the launches (measured inside concurrent builds)
    QcOnline on;
    bool cand_skip = false;                  // the next build is the first under a new assignment: not a sample
    unsigned gen = 0;                        // counts the changes of the stream assignment: a build's time is a sample of the assignment it ran under
    int tune_count = 0;                      // first builds (launches timed alone) on this shard layout
};
// QC_DEV_TIMELINE: ring of QC_TL_PASSES sets of QC_TL_SLOTS kernel slots (QC_TL_W clock words each, qc_tl_stamp), one set per SCF pass; cur = the set
// of the pass being enqueued (null: off, or the ring is full); dumped when an SCF state of the handle ends (qc_tl_dump)
struct QcTimeline {
    QcDev<unsigned long long> d_tl;
    unsigned long long *cur = nullptr;
    int pass = 0;
};

// A/B switches of the work-list planner (qc_plan.cpp; what each one does: DESIGN.md 2), with their defaults.  Read from the environment
// once per handle, at the start of qc_build_model: the classes and every later re-shard of the handle use the same values, a test
// that sets a variable before it creates a System is served, and no getenv runs inside a per-quartet or per-bundle loop.
struct QcPlanSwitches {
    bool no_bm_pp = false, no_bm_ps4 = false, no_t1_merge = false, no_bm_merge = false;
    long bm_pp_min = 8192, mfma4_max = 1024, bm_merge_max = 262144;
    int bm_pq = 32, bm_pp_pq = 96, bm_unit = 8, bm_pp_unit = 8, bm_gain = 0;
    static QcPlanSwitches from_env();
};

struct qc_system {
    int natoms = 0, nshells = 0, nbasis = 0, nelec = 0;
    std::vector<int> Z;
    std::vector<double> xyz;
    std::vector<QcShell> shells;
    // pairs
    std::vector<QcPairDesc> pairs;
    std::vector<int> pairA, pairB, pairKfull;   // shells of each stored pair; its primitive-pair count before the cut-off
    std::vector<double> pairdata;
    std::vector<double> pspack;                 // ps pairs, 8 doubles per primitive: [q, Q(3), E_0[x,y,z], E_1] (see qc_fock_bm.hip)
    std::vector<double> pairdataT;              // same blocks with the expansion stored [ab][h] (bra side of the bra-major kernels)
    std::vector<QcClass> classes;
    QcPlanSwitches plan;
    double grad_ms[4] = {0, 0, 0, 0};         // phase times of the last gradient call (qc_gradient_timings)
    double points_ms[4] = {0, 0, 0, 0};       // phase times of the last point call (qc_points_timings)
    long points_batch = -1;                     // QC_POINTS_BATCH: points per batch of the point calls (0: from the free memory; -1: not read yet)
    long points_split = -1;                     // QC_POINTS_SPLIT: largest batch whose potential splits the record list over workgroups (-1: not read yet)
    // point-charge embedding (qc_embed.h): the handle's current charge set, [x, y, z, q] per charge (qc_set_point_charges)
    std::vector<double> pc;
    double pc_ms[4] = {0, 0, 0, 0};           // phase times of the last embedding call (qc_point_charge_timings)
    long pc_batch = -1;                         // QC_PC_BATCH: charges per batch of the embedding calls (0: the default; -1: not read yet)
    int pc_orient = 0;                          // QC_PC_ORIENT (read with it): 0 chosen from the sizes, 1 lane = record, 2 lane = charge
    std::shared_ptr<struct QcSolvent> solvent;  // continuum solvation (qc_solvent.h): the cavity of the last qc_set_solvent, null without one
    std::vector<double> pairQ;                  // Schwarz factor sqrt(max_ab (ab|ab)) of each stored pair (empty until the device pass has run)
    double imax = 0.0;                          // max pairQ^2: bound on every |(ij|kl)|
    double schwarz_tau = QC_SCHWARZ_TAU;        // 0: no screening
    bool ds_order_ok = true;                    // the DS unit served the lanes of one f64 add in a reproducible order (qc_ds_order_probe, per device)
    bool lists_stale = false;                   // the work lists have not been built since the classes were (qc_build_shards(S, true))
    int64_t nscreened = 0;                      // quartets (of the whole list, all ranks) dropped by the Schwarz bound
    int64_t nquartets = 0;
    int rank = 0, nranks = 1;
    // device (the parts: above)
    bool device_ready = false;
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    QcDeviceData dev;
    QcLanes lanes;
    QcJoin join;
    QcPrepared prep;
    QcAssign assign;
    QcTimeline tl;
    struct QcShellBlob *shell_blob = nullptr; // shells / primitives / transforms / nuclei for the one-electron and gradient kernels (qc_shell_blob)
    struct QcLaunchPlan *launch_plan = nullptr; // launch units and their segments of the current work lists (qc_fock.hip)
    void *comm = nullptr;                    // ncclComm_t
    int live_states = 0;                     // qc_scf_state objects that still point at this handle
    bool zombie = false;                     // qc_system_destroy was called while states were alive: the last qc_scf_end frees the handle
    int fock_mode = 0;                       // 0 direct (default), 1 stored tensor (the reference's own algorithm)
    int accum_fx = 1;                        // 1 (default): fixed-point, order-independent accumulation of G; 0: f64 atomics
    bool merge_bm = false;                    // ... and the ss-ket / high-bra bundles ride in the launch of the ps kets / low bras
    bool merge_t1 = false;                    // the wide-ket launches of the bra classes 0, 1, 2 are one launch (set with the class lists)
    bool has_fkets = false;                   // some class has an f.d / f.f ket (a basis with f functions): the wide-ket launches are the f-capable kernels
    bool pp_ok = true;                        // every p.p pair's expansion blocks have the packed form the pp-ket bra-major kernel assumes
    std::string last_error;
};

// ---- host model (qc_system.cpp) and work-list planner (qc_plan.cpp)
void qc_build_model(qc_system *S);
void qc_build_classes(qc_system *S, QcLap &lap);     // the launch classes with their task lists, has_fkets, merge_t1 / merge_bm
// (meta_only: the classes' LDS / slot sizes only, from the whole task lists - what the Schwarz pass of the device set-up needs before the
// screened lists can exist; the lists are then built once, behind that pass, or on demand: qc_ensure_lists)
void qc_build_shards(qc_system *S, bool meta_only = false);
void qc_host_one_electron(const qc_system *S, int which, double *out);
void qc_host_dipole(const qc_system *S, const double *origin /* 3 */, double *out /* 3 n*n */);
void qc_host_basis_on_points(const qc_system *S, int64_t npts, const double *xyz, double *out /* npts x n, row = point */);
void qc_host_potential_matrix(const qc_system *S, const double *r /* 3 */, double *out /* n*n: (a| 1/|r' - r| |b) */);
void qc_boys_host(int nmax, double x, double *F);

// Boys tables, one per total Hermite order L: row k = F_{L+j}(x_k) / j!, j = 0..7, x_k = k * QC_BOYS_DX (64-byte rows);
// behind them exp(-x_k)
constexpr double QC_BOYS_DX = 0.1;
constexpr int QC_BOYS_NGRID = 421;             // x up to 42
constexpr double QC_BOYS_XMAX = 41.9;          // beyond: asymptotic + upward recursion
constexpr int QC_BOYS_NORD = QC_LTOT + 8;      // orders kept per grid point

// ---- device side of a handle (qc_device.cpp).  init: QC_OK with everything in place, or an error with the handle as it was found
int qc_device_init(qc_system *S);
void qc_device_free(qc_system *S);
int qc_ds_order_probe(hipStream_t st, double *d_out64);      // (qc_fock_bm.hip) 64 sums of the same 64-lane DS add: equal bits = the order is fixed
// Device records of a bra-major work list (QcBundleDev / QcKetUnit) from the host lists of qc_make_bundles
void qc_bm_device_lists(const qc_system *S, int lcd, const std::vector<QcBundle> &bundles, const std::vector<int> &ketlist, bool packed,
                        std::vector<QcBundleDev> &db, std::vector<QcKetUnit> &du);
void qc_drop_launch_plan(qc_system *S);                      // (qc_fock.hip) the launch plan follows the work lists
// ---- the Fock build (qc_fock.hip), the stream assignment (qc_assign.hip), dense linear algebra (qc_linalg.hip, qc_eig_*.hip)
// digestion modes
struct QcFockArgs {
    const double *Dj;     // density contracted into J (n*n)
    const double *Dk0;    // density contracted into K for spin 0
    const double *Dk1;    // spin 1 (UHF) or nullptr
    double *G0, *G1;      // accumulation targets (pre-zeroed), unsymmetrised
    double cK;            // K prefactor (0.5 RHF, 1.0 UHF)
    double *eri_out;      // if non-null: store the integrals into the n^4 tensor instead of digesting
    int nrep;             // accumulation replicas behind G0/G1
    size_t rep_stride;    // doubles between replicas
    const double *fxs;    // non-null: G0 / G1 accumulate 64-bit fixed-point integers (hi plane), scale 2^S at fxs[0], 2^-S at fxs[1] (device)
    size_t fx_lo;         // doubles from the hi plane to the lo plane
    double *schwarz_out;  // non-null: Schwarz pass over the (P|P) quartets, sqrt(max |(ab|cd)|) per pair (device), no digestion
};
int qc_launch_eri_full(qc_system *S, double *d_out);
// MP2 (qc_mp2.hip).  validate: host-side argument and denominator checks of qc_mp2 / qc_scf_mp2 (eps: nspin n-vectors on the host).
// device: the energies from orbitals in HBM (dC: nspin n x n blocks, dEps: nspin n-vectors), on the handle's stream; the AO tensor and
// the intermediates live for the duration of the call.
int qc_mp2_validate(int n, int nspin, const double *eps, const int32_t *nocc, int n_frozen);
int qc_mp2_device(qc_system *S, int nspin, const double *dC, const double *dEps, const int32_t *nocc, int n_frozen, qc_mp2_output *out);
// the batched strided f64 MFMA GEMM of the quarter transformations, C[b] = A[b] B[b]: A[m,k] = A[b a_bs + m a_ms + k a_ks] (any strides),
// B[k,j] = B[b b_bs + k ldb + j], C[m,j] = C[b c_bs + m ldc + j]; every edge is masked (M, N, K need not be multiples of the tile)
void qc_mp2_gemm(hipStream_t st, int batch, int M, int N, int K, const double *A, int64_t a_ms, int64_t a_ks, int64_t a_bs,
                 const double *B, int64_t ldb, int64_t b_bs, double *C, int64_t ldc, int64_t c_bs);
// the four contraction shapes of a quarter-transformation chain, one qc_mp2_gemm call each, against `m` columns of C (n x n, columns = MOs) from column c0; dense, slowest index
// first.  first: (mu x n^3) -> (m x n^3); second, batched over the first index: (batch x mu x n^2) -> (batch x m x n^2); third, over the first two: (batch x mu x n) -> (batch x m x n); last: (rows x mu) -> (rows x m)
void qc_quarter_first(hipStream_t st, int n, const double *C, int c0, int m, const double *In, double *Out);
void qc_quarter_second(hipStream_t st, int n, int batch, const double *C, int c0, int m, const double *In, double *Out);
void qc_quarter_third(hipStream_t st, int n, int batch, const double *C, int c0, int m, const double *In, double *Out);
void qc_quarter_last(hipStream_t st, int n, int rows, const double *C, int c0, int m, const double *In, double *Out);
// excited states (qc_excited.hip): CIS / TDHF of an RHF state from explicit A + B and A - B matrices built from MO integrals.  The
// caller has checked io's inputs.  matrices: the two d x d matrices of `kind` copied to the host (either nullable).
int qc_excitations_device(qc_system *S, int nocc, const double *dC, const double *dEps, qc_excitations *io, double *vectors);
int qc_excitation_matrices_device(qc_system *S, int nocc, const double *dC, const double *dEps, int kind, double *ApB, double *AmB);
// closed-shell CCSD of an RHF state (qc_ccsd.hip): io's inputs have been checked by the caller; t1 (o x v) and t2 (o^2 x v^2) nullable, host.
int qc_ccsd_device(qc_system *S, int nocc, const double *dC, const double *dEps, qc_ccsd *io, double *t1, double *t2);
// C = alpha A B + beta C (row-major) for few rows and a long k: (tiles of C) x (k slices) workgroups sum their slices in ascending k into
// `work` (qc_gemm_splitk_work doubles), a second launch adds the slices in slice order; a product of one slice writes C itself and
// needs no work.  The slice count is a function of (m, n, k) alone.
int qc_gemm_splitk_slices(int m, int n, int k, int *slice_len);
size_t qc_gemm_splitk_work(int m, int n, int k);
bool qc_gemm_splitk_pays(int m, int n, int k);          // qc_gemm would run under one wave per CU and k spans at least two slices
void qc_gemm_splitk(hipStream_t st, int m, int n, int k, double alpha, const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                    double *C, int64_t ldc, double *work);
// out = alpha perm(in) + beta out of a dense four-index tensor: axis x of `out` is axis p[x] of `in` (dimensions d)
void qc_permute4(hipStream_t st, const int d[4], const int p[4], double alpha, const double *in, double beta, double *out);
int qc_debug_gemm_device(int which, int m, int n, int k, double alpha, const double *A, const double *B, double beta, double *C, int reps, double *ms);
// nuclear gradient (qc_grad.hip): terms3 = [core | overlap | two-electron] x 3 natoms (host) from device densities dP (RHF D, UHF [Da; Db])
// and dW; ms[4] = phase times (transform, one-electron, two-electron, sum) or null.  w: W of an SCF state's orbitals (enqueued).
int qc_gradient_device(qc_system *S, int nspin, const double *dP, const double *dW, double *terms3, double *ms);
int qc_gradient_w_device(qc_system *S, int nspin, const double *dC, const double *dEps, const int *nocc, double *dW);
void qc_nuclear_gradient(const qc_system *S, double *g);
// stability analysis (qc_stability.hip).  dim: length of a vector.  device: the Davidson iteration for the lowest eigenpairs of (A + B) at the
// orbitals dC / energies dEps (nspin blocks, device); io's inputs are checked by the caller.  rotated_density: the determinant rotated along
// x (host) and its energy (dH: core Hamiltonian, device).  Both run direct Fock builds on the handle: the caller saves and restores what a
// prepared build of an SCF state left there (qc_scf.cpp, FockPrepSave).
int qc_stability_dim(int n, bool uhf, const int *nocc);
int qc_stability_device(qc_system *S, bool uhf, const int *nocc, const double *dC, const double *dEps, qc_stability *io, double *vectors);
int qc_rotated_density_device(qc_system *S, bool uhf, int kind, const int *nocc, const double *dC, const double *dH, const double *x, double angle,
                              double *hDa, double *hDb, double *energy);
int qc_schwarz_device(qc_system *S);     // fills pairQ / imax from the (P|P) quartets, then screens the work lists
// fixed-point scale of a build from its densities: out[0] = 2^S, out[1] = 2^-S, S = min(QC_FX_MAXBITS, 60 - ceil(log2(4 imax sum|D|)))
void qc_fx_scale(hipStream_t st, int n, const double *Da, const double *Db /*nullable*/, double imax, double *out);
int qc_one_electron_device(qc_system *S, int which /* 0 S, 1 T, 2 V */, double *d_out);
int qc_dipole_device(qc_system *S, const double *origin /* 3, host */, double *d_out /* 3 n*n: x, y, z */);   // (qc_one_electron.hip)
// properties of an SCF state (qc_response.hip).  dipole_trace: tr3[k] = tr((Pa + Pb) M_k) (dPb nullable; dM: 3 n*n; fixed-order sums).
// polarizability: the coupled-perturbed HF equations (A + B) U^q = r^q for the three dipole directions at the orbitals dC / energies
// dEps, by a reduced-space iteration on the Hessian-vector product of the stability analysis; io's inputs are checked by the caller,
// response (host, nullable): 3 x dim.  Runs direct Fock builds on the handle: the caller puts FockPrepSave around it.
int qc_dipole_trace_device(qc_system *S, const double *dPa, const double *dPb, const double *dM, double *tr3);
// Cartesian multipoles: the qc_nherm(order) matrices of order 0 .. 4 on the host (qc_system.cpp) and on the device
// (qc_one_electron.hip; origin: three doubles on the host), and tr[c] = tr((Pa + Pb) M_c) for `count` matrices (qc_response.hip)
void qc_host_multipole(const qc_system *S, int order, const double *origin /* 3 */, double *out /* qc_nherm(order) n*n */);
int qc_multipole_device(qc_system *S, int order, const double *origin, double *d_out);
int qc_multipole_trace_device(qc_system *S, int count, const double *dPa, const double *dPb, const double *dM, double *tr);
// ESP-fitted charges, host numerics (qc_espfit.cpp).  config: cfg's inputs with the defaults filled in (scales: 8 doubles), false = bad;
// grid: the points in the documented order; solve: the constrained fit, fills io's outputs (the caller has checked the pointers)
bool qc_espfit_config(const qc_esp_fit *cfg, int *nscales, double *scales, double *density);
void qc_espfit_grid(const qc_system *S, int nscales, const double *scales, double density, std::vector<double> &xyz);
int qc_espfit_solve(const qc_system *S, int64_t npts, const double *xyz, const double *v, double total_charge, qc_esp_fit *io, double *charges);
// population analysis (qc_population.hip): see the head of that file
int qc_population_x_device(qc_system *S, const double *dS, double *dX);
int qc_population_device(qc_system *S, int scheme, const double *dPa, const double *dPb, const double *dS, const double *dX, double *Nt, double *Ns,
                         double *orbital, double *bond_orders);
int qc_polarizability_device(qc_system *S, bool uhf, const int *nocc, const double *dC, const double *dEps, qc_polarizability *io, double *response);
// values on points (qc_points.hip): density / orbitals / electronic part of the electrostatic potential on npts > 0 host points from
// device matrices, in batches sized from the free device memory; the callers have checked the arguments.  orbitals: the m columns of dC
// (n rows, leading dimension ldc), out m x npts.  esp needs the handle's device side (pair data, Boys tables).  vnuc: host only.
int qc_points_density_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *rho);
int qc_points_orbitals_device(qc_system *S, int m, const double *dC, int ldc, int64_t npts, const double *xyz, double *out);
int qc_points_esp_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *v_elec);
// e_elec = -grad v_elec of the device density dD on npts > 0 host points, npts x 3 on the host; phase times into ms[4]
int qc_points_field_device(qc_system *S, const double *dD, int64_t npts, const double *xyz, double *e_elec, double *ms);
void qc_points_vnuc(const qc_system *S, int64_t npts, const double *xyz, double *v);
void qc_esp_record_counts(const qc_system *S, int64_t counts[QC_LPAIR + 1]);
int qc_launch_fock_classes(qc_system *S, const QcFockArgs &a, float *class_ms /*nullable*/, float *unit_ms = nullptr /*nullable, 14*/, bool nofork = false);
// hipEvent time of a build inside an SCF pass that ran under stream assignment `gen` (no-op once the choice is made)
void qc_fock_feedback(qc_system *S, float build_ms, unsigned gen);
void qc_assignment_freeze(qc_system *S);
// ---- queues, pipes and cross-stream waits (qc_streams.hip)
// The issue of a build - the only place where cross-stream dependencies are created - goes through a per-device gate (QcGate): the holder
// issues alone; `waits`: the issue under this hold put device-side waits in flight
struct QcGateHold { struct QcGate &g; qc_system *S; bool waits = false; explicit QcGateHold(qc_system *S_); ~QcGateHold(); };
void qc_gate_quiet(qc_system *S);                          // the host has seen the handle's stream drained: none of its waits is in flight
void qc_gate_forget(qc_system *S);                         // the handle goes away
// stream sets of handles that went away (the handle's own stream + its QcLanes).  take: into a handle without a stream; give: false = not pooled
bool qc_stream_pool_take(qc_system *S), qc_stream_pool_give(qc_system *S);
int qc_lane_probe(qc_system *S);                           // measures S->lanes (slot_side, nlanes, lane0_is_main)
int qc_join_probe(qc_system *S, bool *concurrent);         // do kernels of different streams run concurrently here?
// device-side join: a one-lane marker on `st` counts itself in `cnt`; a one-lane kernel on the handle's stream waits until `cnt` has reached
// `target` (gentle: the slow poll of waits that spin next to running kernels; tl: timeline slot or null), gives up after S->join.wait_limit
void qc_join_mark(hipStream_t st, unsigned *cnt);
int qc_join_wait(qc_system *S, unsigned *cnt, unsigned target, bool gentle, unsigned long long *tl);
long long qc_wait_limit(const qc_system *S);
// the beta step of a UHF pass on a side stream (another dispatch pipe than the handle's): fork = that stream, made to wait for what the
// handle's stream holds so far; join = the handle's stream waits for it (marker + waiting kernel, under the per-device gate)
hipStream_t qc_spin_fork(qc_system *S);
int qc_spin_join(qc_system *S);
int qc_spin_join_end(qc_system *S, int *ctl_all, int *ctl_out, unsigned *h_seq, unsigned seq);   // (... and ends the pass: control words, sequence word)
int qc_join_check(qc_system *S);                           // after a host wait: QC_ERR_HIP if a device-side wait of the handle gave up
// host-side time stamps of one SCF pass (QC_ISSUE_DEBUG: where the host's time goes between the end of a pass and the launches of the next
// build; printed as differences at the end of every pass).  No-ops unless the variable is set.
void qc_stamp(const char *what);
void qc_stamp_flush();
// ---- the Fock build again
// (scale_done: the fixed-point unit of these densities is already in d_fxs - written by the kernel that produced them)
int qc_fock_prepare_device(qc_system *S, const double *dDa, const double *dDb, bool uhf, const void *owner, bool scale_done = false);
// (dH with dFa / dFb: the Fock matrices H + G are written by the closing kernel as well; *f_done tells whether both were)
int qc_fock_build_device(qc_system *S, const double *dDa, const double *dDb, double *dGa, double *dGb, bool uhf, int *twin_cache = nullptr,
                         const double *dH = nullptr, double *dFa = nullptr, double *dFb = nullptr, bool *f_done = nullptr, const void *owner = nullptr);

// dense linear algebra on the handle's stream (all row-major n x n, device pointers)
void qc_gemm(hipStream_t st, int m, int n, int k, double alpha, const double *A, int lda, bool ta, const double *B,
             int ldb, bool tb, double beta, double *C, int ldc, const int *skip = nullptr /* device flag: non-zero = no-op */);
void qc_gemm_pair(hipStream_t st, int n, const double *A0, bool ta0, const double *B0, double *C0, const double *A1, bool ta1,
                  const double *B1, double *C1, const int *skip);
void qc_diis_solve(hipStream_t st, int m, int minlen, int maxlen, const int *slots, const double *dots, double *B, double *c, int *flag);
void qc_lincomb_dev(hipStream_t st, int n, const double *const *Fs, const double *c_dev, int m, double *out);

// ---- device control words of an SCF pass: QC_CTL_WORDS ints, cleared by the kernel that hands them to the host at the end of the pass
//   [QC_CTL_EIG + QC_CTL_EIG_STRIDE * spin + field]  the sync-free eigensolve of that spin
//   [QC_CTL_DIIS] the DIIS system was singular;  [QC_CTL_NOTCONV] Jacobi sweeps ran out before their criterion was met
//   [QC_CTL_SETUP + field]  the synchronous cold eigensolves (set-up, repeats): read back and cleared by qc_eig_cold_sync
// Fields of an eigensolve's four words (zero on entry; every kernel of the refinement returns at once unless STATE is RUNNING):
//   STATE  QC_EIG_RUNNING / QC_EIG_DONE (dV / dw hold the sorted eigenpairs) / QC_EIG_ROTATE (not perturbative, coupling inside a degenerate
//   cluster or passes exhausted: repeat with rotations);  LAST  one more update finishes;  CLEAN  no coupling left inside degenerate
//   pairs;  PASSES  refinement passes used.  The host reads a pass's scalars as QC_SYNC_WORDS 64-bit words: 4 doubles + the ints.
constexpr int QC_CTL_EIG = 0, QC_CTL_EIG_STRIDE = 4, QC_CTL_DIIS = 8, QC_CTL_NOTCONV = 9, QC_CTL_SETUP = 12, QC_CTL_WORDS = 16;
constexpr int QC_EIG_STATE = 0, QC_EIG_LAST = 1, QC_EIG_CLEAN = 2, QC_EIG_PASSES = 3;
constexpr int QC_EIG_RUNNING = 0, QC_EIG_DONE = 1, QC_EIG_ROTATE = 2;
constexpr int QC_SYNC_WORDS = 4 + QC_CTL_WORDS / 2;

// ---- shells, primitives, transforms and nuclei on the device: one blob per handle, uploaded at the first use (qc_one_electron.hip)
// coff: first Cartesian component of the shell in the Cartesian basis (nc components in all); poff / toff: offsets into exps, coefs / T
struct QcDevShell { double A[3]; int L, nprim, ncart, nfunc, off, coff, poff, toff, atom, pad; };
struct QcShellBlob {
    const QcDevShell *sh; const double *exps, *coefs, *T; const int *Z; const double *xyz;
    const int *cshell; int nc;              // shell of each Cartesian component
    const int *aoff, *flist;                // the basis functions of atom A, ascending: flist[aoff[A] .. aoff[A + 1])
    QcDev<unsigned char> mem;
};
int qc_shell_blob(qc_system *S, const QcShellBlob **out);

// ---- eigensolvers (qc_eig_jacobi.hip: rotations; qc_eig_refine.hip: refinement by the rule of qc_refine_rule.h; qc_eig_tridiag.hip:
// tridiagonal start).  dA: the symmetric matrix (left intact), dV0: start vectors, dV: sorted
// eigenvectors, dw: ascending eigenvalues; all on `st`.  QcEigWork: scratch of one eigensolve in flight, allocated once for a given n -
// work, t1..t4: n*n each (callers may use them between eigensolves); x0 / tri: start vectors and work array of the tridiagonal path;
// small: Rayleigh quotients, statistics, partner list, per-workgroup partials; ctl: four control words for callers without pass words.
inline size_t qc_eig_small_doubles(int n) { return (size_t)3 * n + 32 + 8; }
struct QcEigWork {
    DevBuf work, t1, t2, t3, t4, x0, tri, small;
    QcDev<int> ctl;
    int alloc(int n);
};
// Jacobi kernels: at most this many sweeps; they end after one that met no relative coupling above the tolerance (the sweep itself
// leaves ~tolerance^2 behind) - unless the spectrum has clusters of equal eigenvalues: a pair inside a cluster is turned by a large
// angle however small its coupling, which carries the couplings the sweep started with into pairs it has already been to, so that such a
// sweep leaves up to what it met.  The two-sided kernel therefore also looks at what is left (largest off-diagonal element <=
// QC_JACOBI_LEFT_TOL ||A||_F, 100 times its rounding floor at n = 100); the one-sided kernels, for which that look costs a sweep, end on
// a sweep that met nothing above QC_JACOBI_LEFT_TOL (their inner products carry ~sqrt(n) eps of rounding: 3e-15 at n = 512).
// notconv (device int, nullable): set to 1 when the sweeps ran out before the criterion was met.
constexpr int QC_JACOBI_MAX_SWEEPS = 40;
constexpr double QC_JACOBI_DONE_TOL = 1e-9, QC_JACOBI_LEFT_TOL = 1e-13;
bool qc_eig_force_jacobi();              // QC_EIG_JACOBI (A/B switch): no tridiagonal path, the single-workgroup Jacobi kernels only
int qc_eig_device(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *notconv = nullptr);
int qc_eig_device_warm(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *notconv = nullptr);
int qc_eig_device_refine(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *notconv = nullptr);
// sync-free refinement: `npass` passes enqueued, outcome in ctl (four words, zero on entry)
int qc_eig_refine_async(hipStream_t st, int n, double *dA, const double *dV0, double *dV, double *dw, QcEigWork &E, int *ctl, int npass);
// Tridiagonalisation-based start vectors (qc_eig_tridiag.hip, into E.x0) + refinement: the cold eigensolve.  On QC_EIG_ROTATE the start was
// not good enough - repeat with qc_eig_device.  Smaller matrices (n < QC_TRI_MIN_N) are for the single-workgroup Jacobi kernels.
constexpr int QC_TRI_MIN_N = 24, QC_TRI_MAX_N = 512;
inline bool qc_tri_ok(int n) { return n >= QC_TRI_MIN_N && n <= QC_TRI_MAX_N; }
size_t qc_eig_tridiag_work_doubles(int n);
int qc_eig_tridiag_start(hipStream_t st, int n, const double *dA, QcEigWork &E);
int qc_eig_cold_async(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *ctl, int npass = 3);
// synchronous: cold_async, then the Jacobi kernels if the control words ask for them (ctl: four ints of device scratch)
int qc_eig_cold_sync(hipStream_t st, int n, double *dA, double *dV, double *dw, QcEigWork &E, int *ctl, int *notconv = nullptr);
void qc_permute_tensor(hipStream_t st, int n, const double *I, double c_direct, double c_exch, double *T);
int qc_tensor_gemv(hipStream_t st, int n, const double *T1, const double *D1, const double *T2, const double *D2, double *G);   // QC_OK or QC_ERR_HIP
void qc_axpby(hipStream_t st, int n, double a, const double *x, double b, const double *y, double *out);
void qc_sub_transpose(hipStream_t st, int n, const double *M, double *out);              // out = M - M^T
// (fxs non-null: Gt = [hi | lo] planes of 64-bit fixed-point integers, lo_off doubles apart, units fxs[1] = 2^-S and 2^-(S+32))
void qc_symmetrize_add(hipStream_t st, int n, const double *Gt, size_t lo_off, double *G, const double *H, double *F, const double *fxs);   // G = Gt + Gt^T (and F = H + G)
// fixed-point builds on one rank: replica fold + symmetrisation (+ F = H + G) in one launch
// (the replicas are zeroed as they are read: the accumulator planes are clean again when it returns)
void qc_fold_symmetrize(hipStream_t st, int n, int nrep, size_t rep_stride, double *Gt, size_t lo_off, double *G, const double *H, double *F,
                        const double *fxs, unsigned long long *tl = nullptr);
// out[p * count + x] = sum_r Gt[p * plane_stride + r * stride + x], p < (fx ? 2 : 1)
void qc_reduce_replicas(hipStream_t st, size_t count, int nrep, size_t stride, const double *Gt, double *out, bool fx, size_t plane_stride);
void qc_count_diff(hipStream_t st, size_t count, const double *a, const double *b, int *flag);
void qc_sync_pack(hipStream_t st, unsigned long long *w, int nwords);     // w[nwords + i] = ~w[i]
int qc_lgc_for(int lab, int lcd, int ncd);
// owner of the i-th (cost-sorted) quartet of launch class `ci`: boustrophedon deal, start rank rotated per class
inline int qc_shard_owner(size_t i, int nranks, size_t ci) {
    const size_t round = i / nranks, pos = i % nranks;
    const size_t r = (round & 1) ? (nranks - 1 - pos) : pos;
    return (int)((r + ci) % nranks);
}
void qc_make_slots(const qc_system *S, const std::vector<QcTask> &tasks, int itmax, bool split_cols, std::vector<QcSlot> &out);
// group tasks by bra into bundles of <= 64 kets (sorted by primitive count); itmax > 0 also cuts the bra primitive range
// (unit > 0: lanes take chunks of at most `unit` primitives of a ket pair, packed into the ketlist entry; 0: whole pairs)
// Returns whether the ketlist entries are PACKED (pair | first primitive << 18 | length << 25, qc_pack_ket_entry) - only possible with
// unit > 0, fewer than 2^18 stored pairs and at most 127 primitives per ket pair - or plain pair indices.  Whoever decodes a list
// (qc_unpack_ket_entry) needs that flag: a plain index above 2^18 would otherwise be cut and its upper bits read as a chunk.
bool qc_make_bundles(const qc_system *S, const std::vector<QcTask> &tasks, int itmax, std::vector<QcBundle> &bundles, std::vector<int> &ketlist, int unit = 0);
constexpr int QC_KET_BITS = 18;
inline unsigned qc_pack_ket_entry(int ket, int kl0, int len) { return (unsigned)ket | ((unsigned)kl0 << QC_KET_BITS) | ((unsigned)len << (QC_KET_BITS + 7)); }
inline void qc_unpack_ket_entry(int entry, bool packed, int *ket, int *kl0, int *len) {
    const unsigned e = (unsigned)entry;
    if (!packed) { *ket = entry; *kl0 = 0; *len = 0; return; }          // (len 0: the whole pair)
    *ket = (int)(e & ((1u << QC_KET_BITS) - 1)); *kl0 = (int)((e >> QC_KET_BITS) & 0x7fu); *len = (int)(e >> (QC_KET_BITS + 7));
}
inline void qc_ensure_lists(qc_system *S) { if (S->lists_stale) qc_build_shards(S); }
inline int qc_unit_of(int LAB, int LCD, bool bm) { return bm ? 2 * (QC_LPAIR + 1) + 2 * LCD + (LAB >= 3 ? 1 : 0) : 2 * LAB + (LCD >= 4 ? 1 : 0); }
// the launch a class belongs to inside a build: with `merge_t1` (bases with f functions) the wide-ket buckets of the bra classes 0 and 1 ride
// in the launch of bra class 2, those of class 4 in the launch of class 3, those of class 6 in the launch of class 5 (qc_fock_tier1_low_kernel); the per-class launches of the profiling / set-up passes use qc_unit_of
inline int qc_build_unit_of(const qc_system *S, int LAB, int LCD, bool bm) {
    if (S->merge_t1 && !bm && LCD >= 4) return qc_unit_of(LAB <= 2 ? 2 : (LAB <= 4 ? 3 : 5), LCD, false);
    if (S->merge_bm && bm && LCD == 0 && LAB >= 3) return qc_unit_of(2, 1, true);       // ss kets / high bras ride with the ps kets / low bras (qc_fock_bm_kernel<3, 0>)
    return qc_unit_of(LAB, LCD, bm);
}
void qc_dots(hipStream_t st, int n, const double *x, const double *const *ys, int ny, double *out);  // device ptr list
void qc_lincomb(hipStream_t st, int n, const double *const *Fs, const double *c, int m, double *out);   // out = sum c_i Fs_i
void qc_scale_cols_invsqrt(hipStream_t st, int n, const double *U, const double *Lam, double *out);
int qc_device_reshard(qc_system *S);
void qc_energy_rms(hipStream_t st, int n, const double *Dnew, const double *Dold, const double *H, const double *G,
                   double *out2, int *ctl = nullptr, int *ctl_out = nullptr);  // out2[0] = 0.5 tr(Dnew (2H+G)), out2[1] = sum_i (Dnew-Dold)_ii^2

// ---- the whole Roothaan step of one spin in one workgroup, matrices in LDS (qc_scf_small.hip): n <= QC_SMALL_MAXN
constexpr int QC_SMALL_MAXN = 64;
struct QcSmallArgs {
    int n, phases;                 // phases: 1 pre, 2 refine, 4 post
    // ---- pre
    const double *F;               // this pass's Fock matrix (null: F = H + G is formed here and stored to F_out)
    double *F_out;                 // the pass's DIIS Fock slot
    const double *D, *S, *X, *H, *G;
    double *E_out;                 // the pass's DIIS error slot
    int m, minlen, maxlen;         // DIIS window length (newest first), Diis::new(minlen, maxlen)
    int dots_generic;              // the DIIS dot products in the summation order of qc_dots_kernel (open-shell runs: bit-identical trajectories)
    int slot[12];
    const double *errs[12], *focks[12];
    double *Bmat, *c_out;          // B (slot-indexed, maxlen x maxlen) and the coefficients, in HBM
    int *diis_flag;
    double *Fp;                    // F' = X^T F_diis X (written by pre, read by a refine / post launch of its own)
    // ---- refine
    const double *V0;              // start vectors
    int npass;
    int *ctl;                      // this spin's four eigensolve words (QC_EIG_* fields)
    // ---- post
    const double *Cp_in;           // eigenvectors of F' from another eigensolver (post without refine)
    double *Cp_out, *w_out, *C_out, *Dn;
    const double *Dold;
    int nocc; double dfac;
    double *scal_out;              // [0] 0.5 tr(Dn (2H + G)), [1] sum_i (Dn - Dold)_ii^2
    double *fxs_out; double imax;  // non-null (RHF): the fixed-point unit of the build that will digest Dn goes here (qc_fx_scale)
    int *ctl_all, *ctl_out;        // non-null: hand the QC_CTL_WORDS control words over to ctl_out and clear them
    unsigned *seq_out; unsigned seq; // non-null (pinned host memory): the pass's sequence number, stored after everything else the host reads
    unsigned long long *tl;        // non-null: [start, end] clock of this launch (QC_DEV_TIMELINE)
};
int qc_scf_small_launch(hipStream_t st, const QcSmallArgs &a);
constexpr int QC_TL_W = 34;   // (words per kernel slot: the launch's end is the maximum over 32 end words - plain stores, no atomics: 8000
                              // workgroups hammering ONE word with atomic min / max stretched an H2O/cc-pVTZ build from 172 to 231 us)
constexpr int QC_TL_PASSES = 64, QC_TL_SLOTS = QC_NUNITS + 4;       // launch units | join wait | fold | Roothaan kernel, first / second launch
int qc_tl_begin_pass(qc_system *S);                                 // (qc_streams.hip; no-op unless QC_DEV_TIMELINE is set)
void qc_tl_dump(qc_system *S);
size_t qc_scf_small_lds_bytes(int n);

// ---- RCCL, bound at run time (qc_rccl.cpp)
struct QcRccl {
    void *handle = nullptr;
    std::string path;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    bool ok = false;
};
QcRccl &qc_rccl();
void qc_system_free(qc_system *S);       // (qc_api.cpp; the last SCF state of a destroyed handle frees it)

#define QC_HIP_CHECK(expr)                                                                  \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            fprintf(stderr, "qchem_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return QC_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)
