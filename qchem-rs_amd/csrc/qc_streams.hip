// qc_streams.hip - what knows about queues, pipes and cross-stream waits: the per-device issue gate, the pool of stream sets, the dispatch-lane
// probe, the device-side join (marker and waiting kernels, their time-out), host time stamps and the device timeline.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "qc_fock_kernel.h"

// ---- One handle at a time may have device-side waits in flight on a device.  A waiting kernel sits at the head of its hardware queue
// until the kernel that releases it has run; the argument that this cannot deadlock - every wait is issued after everything it depends
// on, and a hardware queue runs in issue order - holds for ONE issuing sequence.  Two handles issuing from two threads (the header
// allows that) can park handle A's waiter in front of handle B's marker and B's waiter in front of A's: both then wait out their limit.
// So the issue of a build - the only place where cross-stream dependencies are created - goes through a per-device gate: the issuing
// thread holds the gate's mutex while it issues, and if ANOTHER handle still has waits in flight it first waits for that handle's
// stream (those waits finish without any help from the host: everything they depend on was issued before them).  Uncontended cost: one
// mutex per build.
struct QcGate { std::mutex mu; qc_system *owner = nullptr; };
static QcGate &qc_gate_of(int device) {
    static QcGate *gates = new QcGate[64];          // (never destroyed: handles may outlive the static destructors of the process)
    return gates[(device >= 0 && device < 64) ? device : 0];
}
QcGateHold::QcGateHold(qc_system *S_) : g(qc_gate_of(S_->device)), S(S_) {
    g.mu.lock();
    if (g.owner && g.owner != S) {
        if (g.owner->stream) (void)hipStreamSynchronize(g.owner->stream);      // (the join wait is the last thing of a build on it)
        g.owner->join.waits_in_flight = false;
        g.owner = nullptr;
    }
}
QcGateHold::~QcGateHold() {
    if (waits) { g.owner = S; S->join.waits_in_flight = true; }
    g.mu.unlock();
}
void qc_gate_forget(qc_system *S) {          // the handle goes away
    QcGate &g = qc_gate_of(S->device);
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.owner == S) g.owner = nullptr;
    S->join.waits_in_flight = false;
}
// the host has seen the handle's stream drained past its last build: nothing of this handle waits on the device any more
void qc_gate_quiet(qc_system *S) { if (S->join.waits_in_flight) qc_gate_forget(S); }

static std::vector<std::pair<const char *, double>> *qc_stamps = nullptr;
void qc_stamp(const char *what) {
    static const bool on = getenv("QC_ISSUE_DEBUG") != nullptr;
    if (!on) return;
    if (!qc_stamps) qc_stamps = new std::vector<std::pair<const char *, double>>();
    qc_stamps->emplace_back(what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count());
}
void qc_stamp_flush() {
    if (!qc_stamps || qc_stamps->size() < 2) return;
    fprintf(stderr, "[issue]");
    for (size_t i = 1; i < qc_stamps->size(); ++i) fprintf(stderr, " %s %.1f |", (*qc_stamps)[i].first, (*qc_stamps)[i].second - (*qc_stamps)[i - 1].second);
    fprintf(stderr, " total %.1f us\n", qc_stamps->back().second - qc_stamps->front().second);
    qc_stamps->clear();                         // (a fresh stamp behind the printing: the next pass's first difference is the caller's own time
    qc_stamp("printed");                        // between two passes)
}
// ---- device-side timeline (QC_DEV_TIMELINE): see qc_tl_stamp
constexpr size_t per_pass = (size_t)QC_TL_SLOTS * QC_TL_W, words = (size_t)QC_TL_PASSES * per_pass;
int qc_tl_begin_pass(qc_system *S) {
    if (getenv("QC_DEV_TIMELINE") == nullptr) { S->tl.cur = nullptr; return QC_OK; }      // (per pass: a harness switches it on after its warm-up)
    if (!S->tl.d_tl.p) {
        if (S->tl.d_tl.alloc(words) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemset(S->tl.d_tl.p, 0, words * sizeof(unsigned long long)));
        S->tl.pass = 0;
    }
    S->tl.cur = S->tl.pass < QC_TL_PASSES ? S->tl.d_tl.p + (size_t)S->tl.pass * per_pass : nullptr;
    ++S->tl.pass;
    return QC_OK;
}
void qc_tl_dump(qc_system *S) {
    if (!S->tl.d_tl.p || S->tl.pass == 0) return;
    const int np = std::min(S->tl.pass, QC_TL_PASSES);
    std::vector<unsigned long long> h(words);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), S->tl.d_tl.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long prev_end = 0;
    for (int p = 0; p < np; ++p) {
        const unsigned long long *t = h.data() + (size_t)p * per_pass;
        unsigned long long b[QC_TL_SLOTS], e[QC_TL_SLOTS], t0 = ~0ull, t1 = 0;
        for (int k = 0; k < QC_TL_SLOTS; ++k) {
            b[k] = t[(size_t)k * QC_TL_W]; e[k] = 0;
            for (int w = 1; w <= 32; ++w) e[k] = std::max(e[k], t[(size_t)k * QC_TL_W + w]);
            if (b[k]) { t0 = std::min(t0, b[k]); t1 = std::max(t1, e[k]); }
        }
        if (t1 == 0) continue;
        const unsigned long long base = prev_end ? prev_end : t0;
        fprintf(stderr, "[timeline] pass %d (us from the end of the previous pass; whole pass %.2f):", p, (double)(t1 - base) * 0.01);
        for (int k = 0; k < QC_TL_SLOTS; ++k) {
            if (!b[k]) continue;
            char name[32];
            if (k < QC_NUNITS) snprintf(name, sizeof(name), "unit%d", k);
            else snprintf(name, sizeof(name), "%s", k == QC_NUNITS ? "wait" : k == QC_NUNITS + 1 ? "fold" : k == QC_NUNITS + 2 ? "small" : "small2");
            fprintf(stderr, "  %s %.2f-%.2f", name, ((double)b[k] - (double)base) * 0.01, ((double)e[k] - (double)base) * 0.01);
        }
        fprintf(stderr, "\n");
        prev_end = t1;
    }
    qc_renew(S->tl);
}
// ---- Pool of stream sets (the handle's own stream, the side streams, their events, the dispatch lanes measured on them)
struct QcStreamSet { int device; hipStream_t main; QcLanes lanes; };
struct QcStreamPool { std::mutex mu; std::vector<QcStreamSet> sets; };
static QcStreamPool &qc_stream_pool() { static QcStreamPool *p = new QcStreamPool(); return *p; }     // (never destroyed: the runtime may be gone by then)
bool qc_stream_pool_take(qc_system *S) {
    if (getenv("QC_NO_STREAM_POOL") || getenv("QC_NO_LANES")) return false;
    QcStreamPool &P = qc_stream_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    for (size_t i = 0; i < P.sets.size(); ++i) {
        if (P.sets[i].device != S->device) continue;
        S->stream = P.sets[i].main; S->own_stream = true; S->lanes = P.sets[i].lanes;
        P.sets.erase(P.sets.begin() + i);
        return true;
    }
    return false;
}
// (only complete sets whose lanes were measured with the handle's OWN stream; everything on them has been waited for)
bool qc_stream_pool_give(qc_system *S) {
    const QcLanes &L = S->lanes;
    if (getenv("QC_NO_STREAM_POOL") || !S->own_stream || !S->stream || !L.lanes_probed || !L.ev_fork) return false;
    for (int k = 0; k < QC_NSTREAMS; ++k) if (!L.side[k] || !L.ev_join[k]) return false;
    if (hipStreamSynchronize(S->stream) != hipSuccess) return false;
    for (int k = 0; k < QC_NSTREAMS; ++k) if (hipStreamSynchronize(L.side[k]) != hipSuccess) return false;
    QcStreamPool &P = qc_stream_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    if (P.sets.size() >= 8) return false;
    P.sets.push_back(QcStreamSet{S->device, S->stream, L});
    return true;
}

// Device-side join of a build's side streams.  Joining through events costs the cross-queue signal path - event packet on the side
// queue, barrier packet on the handle's queue, ~20 us between the last class kernel and the fold on the H2O/cc-pVTZ trace.  Instead every
// side stream ends with a one-lane marker kernel that counts itself (in-queue dependency: a few us), and the handle's stream runs a
// one-lane kernel that waits for the count of this build (monotonic counter, signed comparison) before the fold.
//
// A wait gives up after S->join.wait_limit ticks of the constant 100 MHz clock (qc_wait_limit: 20 s, or fifty times the build's serial time if
// that is longer) - only possible when the launches it waits for never complete - and says so in pinned memory.  Every host wait that
// follows looks at that word (qc_join_check) and fails THAT call: a build whose join gave up has folded an incomplete matrix.
__global__ void qc_join_mark_kernel(unsigned *cnt) {
    if (threadIdx.x == 0) (void)__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// (the poll is a RELAXED agent-scope load - it goes past the non-coherent cache levels without invalidating anything; an acquire load
// in the loop invalidates the waiter's L2 every time round, and five waiters doing that every 100 ns through a whole Roothaan step cost
// the kernels running beside them 30 % - measured: iteration 0.33 -> 0.46 ms.  One acquire fence once the word is there.)
// (`gentle`: the join of the two spins' Roothaan steps and the concurrency probe - qc_spin_join, qc_join_probe - against the join of a build)
// What every waiter does between two looks at its counter: sleep SLEEP (x 64 clocks), look at the clock whenever the round counter passes
// CLOCK_MASK.  True: the wait has lasted longer than `limit` and gives up (said in *timeout_flag).  it, t0: the waiter's own, zero at first.
template <int SLEEP, unsigned CLOCK_MASK>
__device__ __forceinline__ bool qc_poll_round(unsigned &it, long long &t0, long long limit, int *timeout_flag) {
    __builtin_amdgcn_s_sleep(SLEEP);
    if ((++it & CLOCK_MASK) == 0) {
        const long long t = wall_clock64();
        if (t0 == 0) t0 = t;
        else if (t - t0 > limit) { __hip_atomic_store(timeout_flag, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); return true; }
    }
    return false;
}
// (the counter has not reached `target` yet: monotonic counter, signed comparison)
__device__ __forceinline__ bool qc_join_pending(unsigned *cnt, unsigned target) { return (int)(__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0; }
__global__ void qc_join_wait_kernel(unsigned *cnt, unsigned target, int *timeout_flag, long long limit, bool gentle, unsigned long long *tl = nullptr) {
    if (threadIdx.x != 0) return;
    qc_tl_stamp(tl, 0);
    long long t0 = 0;
    unsigned it = 0;
    if (!gentle) {
        // the join of a build: nothing runs next to this lane that its polling could disturb for long, and every 1.7 us step
        // of the gentle loop below is 0.85 us, on average, between the last marker and the fold - one load per ~0.2 us here
        while (qc_join_pending(cnt, target)) if (qc_poll_round<8, 127u>(it, t0, limit, timeout_flag)) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        qc_tl_stamp(tl, 1);
        return;
    }
    // (poll gently: one load per ~1.7 us, the clock only every 16th time round - this waiter spins through the other spin's whole Roothaan
    // step, and whatever it does to the memory system of its CU the workgroups of that step pay)
    while (qc_join_pending(cnt, target)) if (qc_poll_round<64, 15u>(it, t0, limit, timeout_flag)) break;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    qc_tl_stamp(tl, 1);
}

// twenty seconds of the 100 MHz clock, or fifty times the serial time of the build's launches when that is longer (a side chain of a
// very large system may legitimately end seconds after the handle's own); QC_WAIT_LIMIT_MS overrides (tests force a tiny limit)
long long qc_wait_limit(const qc_system *S) {
    const char *env = getenv("QC_WAIT_LIMIT_MS");          // (read per build: a test switches it on and off inside one process)
    const double env_ms = env ? atof(env) : 0.0;
    if (env_ms > 0.0) return std::max(1LL, (long long)(env_ms * 1e5));
    double serial_ms = 0.0;
    for (float x : S->assign.unit_ms) serial_ms += x;
    return (long long)(std::max(20000.0, 50.0 * serial_ms) * 1e5);
}
void qc_join_mark(hipStream_t st, unsigned *cnt) { hipLaunchKernelGGL(qc_join_mark_kernel, dim3(1), dim3(64), 0, st, cnt); }
int qc_join_wait(qc_system *S, unsigned *cnt, unsigned target, bool gentle, unsigned long long *tl) {
    hipLaunchKernelGGL(qc_join_wait_kernel, dim3(1), dim3(64), 0, S->stream, cnt, target, S->join.h_timeout, S->join.wait_limit, gentle, tl);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// ---- Dispatch lanes.  Measured on MI355X (tools/probes/pipe_probe.hip): with GPU_MAX_HW_QUEUES=8, eight HIP streams land on eight hardware
// queues that sit in PAIRS on four dispatch pipes, and a pipe works on one dispatch packet until every workgroup of that grid has been
// launched - a one-workgroup kernel on stream j completes in 12 us while a grid of 8192 workgroups dispatches on an unrelated stream, and
// only after 160 us (the grid's whole dispatch) when j's queue shares the pipe of that stream (pairs (i, i + 4) in creation order; with the
// runtime's default of four queues the pairs share a QUEUE).  So at most four kernels dispatch at a time, a launch on a fifth stream waits
// for its pipe neighbour, and which streams are neighbours is the runtime's business.  It is measured, once per handle: a busy grid on one
// stream, a marker on the other, the marker's latency against the grid's own duration.  The assignment of launch units then uses
// `nlanes` (<= 4) slots on distinct pipes instead of drawing among seven streams that are not what they seem (QC_NO_LANES: the old draw).
__global__ void qc_probe_busy_kernel(long long ticks) {
    extern __shared__ char probe_lds[];
    if (threadIdx.x == 0) probe_lds[0] = 1;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
int qc_lane_probe(qc_system *S) {
    for (int k = 0; k < QC_NSTREAMS; ++k) S->lanes.slot_side[k] = k;
    S->lanes.nlanes = QC_NSTREAMS; S->lanes.lane0_is_main = false;
    if (getenv("QC_NO_LANES")) return QC_OK;
    QcGateHold gate(S);                  // (one probe at a time per device; another handle's grids in flight can still make two lanes look like one - that costs time, never results)
    using clk = std::chrono::steady_clock;
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const int grid = 8192; const long long ticks = 500;                  // 8192 one-wave workgroups of 5 us, 40 KB of LDS each: four per CU
    auto busy = [&](hipStream_t st) { hipLaunchKernelGGL(qc_probe_busy_kernel, dim3(grid), dim3(64), 40 * 1024, st, ticks); };
    auto mark = [&](hipStream_t st) { qc_join_mark(st, S->dev.d_join.p + 3); };
    // warm-up (code upload, queue creation), then the grid alone
    busy(S->stream); mark(S->stream);
    for (int k = 0; k < QC_NSTREAMS; ++k) mark(S->lanes.side[k]);
    QC_HIP_CHECK(hipDeviceSynchronize());
    double d_alone = 1e30;
    {
        const auto t0 = clk::now();
        busy(S->stream);
        QC_HIP_CHECK(hipStreamSynchronize(S->stream));
        d_alone = us(t0, clk::now());
    }
    // coupled(x, y): a marker on y waits for the grid on x
    // (one measurement; a positive is measured again - a hiccup of the host must not merge two lanes)
    auto coupled = [&](hipStream_t x, hipStream_t y, bool *out) -> int {
        double lat = 1e30;
        for (int rep = 0; rep < 2; ++rep) {
            busy(x);
            const auto t1 = clk::now();
            mark(y);
            QC_HIP_CHECK(hipStreamSynchronize(y));
            lat = std::min(lat, us(t1, clk::now()));
            QC_HIP_CHECK(hipStreamSynchronize(x));
            if (lat <= 0.5 * d_alone) break;
        }
        *out = lat > 0.5 * d_alone;
        return QC_OK;
    };
    std::vector<std::vector<int>> lanes;      // side-stream indices per pipe; -1 stands for the handle's own stream
    lanes.push_back({-1});
    for (int k = 0; k < QC_NSTREAMS; ++k) {
        bool placed = false;
        for (auto &L : lanes) {
            bool c = false;
            int rc = coupled(L[0] < 0 ? S->stream : S->lanes.side[L[0]], S->lanes.side[k], &c);
            if (rc != QC_OK) return rc;
            if (c) { L.push_back(k); placed = true; break; }
        }
        if (!placed) lanes.push_back({k});
    }
    // slots: one side stream per pipe first (the pipe of the handle's own stream in front, if a side stream shares it), then the rest
    int n = 0;
    bool used[QC_NSTREAMS] = {};
    S->lanes.lane0_is_main = lanes[0].size() > 1;
    for (auto &L : lanes)
        for (int k : L) if (k >= 0) { S->lanes.slot_side[n++] = k; used[k] = true; break; }
    S->lanes.nlanes = n;
    for (int k = 0; k < QC_NSTREAMS; ++k) if (!used[k]) S->lanes.slot_side[n++] = k;
    if (getenv("QC_TUNE_DEBUG") || getenv("QC_SCF_DEBUG")) {
        fprintf(stderr, "[lanes] %d dispatch lanes (grid alone %.0f us):", S->lanes.nlanes, d_alone);
        for (auto &L : lanes) { fprintf(stderr, " {"); for (int k : L) fprintf(stderr, k < 0 ? " main" : " s%d", k); fprintf(stderr, " }"); }
        fprintf(stderr, "  slots:"); for (int k = 0; k < QC_NSTREAMS; ++k) fprintf(stderr, " %d", S->lanes.slot_side[k]); fprintf(stderr, "\n");
    }
    return QC_OK;
}

static hipStream_t spin_side(const qc_system *S) { return S->lanes.side[S->lanes.slot_side[S->lanes.lane0_is_main ? 1 : 0]]; }
hipStream_t qc_spin_fork(qc_system *S) {
    QcGateHold gate(S);
    hipStream_t side = spin_side(S);
    if (hipEventRecord(S->lanes.ev_fork, S->stream) != hipSuccess || hipStreamWaitEvent(side, S->lanes.ev_fork, 0) != hipSuccess) return nullptr;
    return side;
}
// what the two joins share: the beta stream's marker, the count and the limit of the wait that the caller launches under the same hold
static void spin_mark(qc_system *S, QcGateHold &gate) {
    S->join.spin_target += 1;
    S->join.wait_limit = qc_wait_limit(S);
    qc_join_mark(spin_side(S), S->dev.d_join.p + 4);
    gate.waits = true;
}
int qc_spin_join(qc_system *S) {
    QcGateHold gate(S);
    spin_mark(S, gate);
    return qc_join_wait(S, S->dev.d_join.p + 4, S->join.spin_target, true, nullptr);
}

// The join of the two spins' one-workgroup Roothaan kernels (scf_iterate: alpha on the handle's stream, beta on a side stream) that also
// ends the pass: once the beta stream's marker is in, the sixteen control words go to the host and are cleared, then the pass's sequence
// word - what the last spin's kernel does itself when the spins run one after the other (qc_scf_small.hip).
__global__ void qc_spin_join_end_kernel(unsigned *cnt, unsigned target, int *timeout_flag, long long limit, int *ctl_all, int *ctl_out,
                                        unsigned *h_seq, unsigned seq) {
    if (threadIdx.x == 0) {
        long long t0 = 0;
        unsigned it = 0;
        while (qc_join_pending(cnt, target)) if (qc_poll_round<16, 63u>(it, t0, limit, timeout_flag)) break;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (threadIdx.x < QC_CTL_WORDS) {
        int *p = ctl_all + threadIdx.x;
        ctl_out[threadIdx.x] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && h_seq) __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int qc_spin_join_end(qc_system *S, int *ctl_all, int *ctl_out, unsigned *h_seq, unsigned seq) {
    QcGateHold gate(S);
    spin_mark(S, gate);
    hipLaunchKernelGGL(qc_spin_join_end_kernel, dim3(1), dim3(64), 0, S->stream, S->dev.d_join.p + 4, S->join.spin_target, S->join.h_timeout, S->join.wait_limit, ctl_all, ctl_out, h_seq, seq);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

// After a host wait that follows a device-joined build: did one of its waits give up?  Then the matrix it folded was not complete: the
// call fails (last_error says why), the accumulator planes are no longer known to be clean, the counter and the host's target meet
// again, and this handle joins through events from now on.
int qc_join_check(qc_system *S) {
    if (!S->join.h_timeout || !__atomic_load_n(S->join.h_timeout, __ATOMIC_ACQUIRE)) return QC_OK;
    S->last_error = "a device-side wait of the Fock build gave up (QC_WAIT_LIMIT_MS): a launch it depended on never finished; "
                    "this handle joins its streams through events from now on";
    fprintf(stderr, "qchem_hip: %s\n", S->last_error.c_str());
    (void)hipDeviceSynchronize();
    unsigned c[5] = {0, 0, 0, 0, 0};
    if (hipMemcpy(c, S->dev.d_join.p, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "qchem_hip: join counter %u, the wait wanted %u; spin counter %u / %u\n", c[0], S->join.target, c[4], S->join.spin_target);
        S->join.target = c[0]; S->join.spin_target = c[4]; }
    __atomic_store_n(S->join.h_timeout, 0, __ATOMIC_RELEASE);
    S->join.by_events = true;
    S->prep.invalidate();
    return QC_ERR_HIP;
}

// The device-side join needs kernels of different streams to RUN concurrently: a waiting kernel whose marker cannot start would wait
// out its limit.  That is the case whenever something serialises dispatches - rocprofv3 counter collection (--pmc) does, so do the
// runtime's debugging switches.  Asked once per handle: a waiting kernel on one stream, then its marker on another; if the wait gives up
// after 2 ms, this handle joins through events (as QC_EVENT_JOIN does).
int qc_join_probe(qc_system *S, bool *concurrent) {
    QcGateHold hold(S);
    *S->join.h_timeout = 0;
    S->join.target += 1;
    hipLaunchKernelGGL(qc_join_wait_kernel, dim3(1), dim3(64), 0, S->stream, S->dev.d_join.p, S->join.target, S->join.h_timeout, 200000LL, true, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(qc_join_mark_kernel, dim3(1), dim3(64), 0, S->lanes.side[0], S->dev.d_join.p);
    if (hipGetLastError() != hipSuccess) return QC_ERR_HIP;
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->lanes.side[0]));
    *concurrent = *S->join.h_timeout == 0;
    *S->join.h_timeout = 0;
    return QC_OK;
}
