// qc_assign.hip - which launch unit of a Fock build runs on which dispatch lane: the first assignment (launches timed alone, placed longest
// first), its refinement in instalments, the process-wide cache of what the search found.  Reaches the build through qc_fock_build.h.
//
// ---- Refinement of the stream assignment, paid for by use.  A neighbouring assignment (one launch moved to another lane, two launches
// of different lanes swapped; first of all the proposals of the first build) is measured by two extra builds, back to back, and kept when
// the better of them beats the current best by 1.5 % - the local search of rounds 2-3.  What changed in round 4 is WHEN it runs: never in
// a handle's first builds (the offline tuner of rounds 1-3 spent 55 ms - ten times the 15-pass SCF of H2O/cc-pVTZ it served - to win 6 %
// of its builds), but in small instalments once the handle has shown that it lives long: from its 24th build on, a build may spend on
// trials as many extra builds as the handle has done useful ones so far, minus what was spent already.  A handle that does one SCF pays
// nothing; one that runs hundreds of builds (geometry loops, benchmarks) converges to the searched assignment at a bounded overhead
// and then stops (a whole sweep of the neighbourhood without a gain, or QC_SEARCH_TRIALS trials); the result goes to a process-wide cache keyed by
// the shape of the work lists.  The stream assignment does not change results (integer accumulation), only time.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "qc_fock_build.h"

constexpr int QC_SEARCH_FIRST_BUILD = 24, QC_SEARCH_CHUNK = 8, QC_SEARCH_TRIALS = 240, QC_SEARCH_KICKS = 3;

static void qc_online_reset(qc_system *S, bool frozen) {
    S->assign.on = QcOnline{};
    S->assign.on.frozen = frozen; S->assign.on.settled = frozen;
    S->assign.on.best = S->assign.unit_stream;
    S->assign.on.rng = 2463534242u;
}
static uint64_t qc_assign_key(const qc_system *S) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h ^= v; h *= 1099511628211ull; };
    mix((uint64_t)S->lanes.nlanes); mix((uint64_t)S->nbasis); mix((uint64_t)S->nranks); mix((uint64_t)S->rank); mix((uint64_t)S->accum_fx);
    for (const auto &c : S->classes) { mix(((uint64_t)c.LAB << 40) | ((uint64_t)c.LCD << 32) | (uint64_t)(c.bm ? 1 : 0)); mix((uint64_t)c.slots.size()); mix((uint64_t)c.bundles.size()); mix((uint64_t)c.prim_quartets); }
    return h;
}
struct QcAssignCache { std::mutex mu; std::vector<std::pair<uint64_t, std::pair<std::vector<int>, bool>>> e; };
static QcAssignCache &qc_assign_cache() { static QcAssignCache *c = new QcAssignCache(); return *c; }     // (never destroyed, as the gates)
static void qc_assign_cache_lookup(qc_system *S) {
    if (getenv("QC_NO_ASSIGN_CACHE")) return;
    const uint64_t key = qc_assign_key(S);
    QcAssignCache &C = qc_assign_cache();
    std::lock_guard<std::mutex> lk(C.mu);
    for (const auto &kv : C.e)
        if (kv.first == key && kv.second.first.size() == S->assign.unit_stream.size()) {
            S->assign.unit_stream = kv.second.first; S->assign.on.best = S->assign.unit_stream; S->assign.gen += 1;
            if (kv.second.second) { S->assign.on.frozen = true; S->assign.on.settled = true; }
            return;
        }
}
static void qc_assign_cache_store(const qc_system *S) {
    if (getenv("QC_NO_ASSIGN_CACHE")) return;
    const uint64_t key = qc_assign_key(S);
    QcAssignCache &C = qc_assign_cache();
    std::lock_guard<std::mutex> lk(C.mu);
    for (auto &kv : C.e) if (kv.first == key) { kv.second = {S->assign.on.best, S->assign.on.settled}; return; }
    if (C.e.size() < 64) C.e.push_back({key, {S->assign.on.best, S->assign.on.settled}});
}
// (the SCF passes report their build times: kept as the handle's running mean - the search itself measures its own builds)

// Launch units are independent (they only meet in the atomically accumulated Gt replicas); they go to the side streams of the dispatch
// lanes.  Kernels on one stream run in order, so the assignment matters: units are placed longest-first on the least loaded stream.
// (`head_start`, ms: stream 0 is given that much more work than the others.  The most loaded stream becomes the handle's own stream,
// and a build that ends on the handle's stream goes straight on to the fold, while one that ends on a side stream first pays the
// cross-queue signal - event packet, barrier packets, ~20 us on the H2O/cc-pVTZ trace.)
static void assign_longest_first(const QcBuild &b, const std::vector<float> &w, int nstreams, float head_start = 0.f) {
    qc_system *S = b.S;
    const std::vector<std::vector<int>> &units = b.plan.units;
    nstreams = std::min(nstreams, S->lanes.nlanes);              // (slots beyond the dispatch lanes share a pipe with an earlier one)
    std::vector<int> ord = b.plan.active();
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return w[x] > w[y]; });
    std::vector<float> load(nstreams, 0.f);
    load[0] = -head_start;
    S->assign.unit_stream.assign(units.size(), 0);
    for (int u : ord) {
        const int k = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        S->assign.unit_stream[u] = k;
        load[k] += w[u];
    }
    S->assign.unit_weight = w;
}

// First build of a shard.  No tuner run (round 4): the launches are timed alone once (two serial passes: the first pays the code
// upload), placed longest-first on the dispatch lanes, and the assignment is refined ONLINE from the build times the SCF passes
// report anyway (qc_fock_feedback) - a neighbouring assignment is tried for a few passes and kept when it is faster.  The offline
// tuner of rounds 1-3 (25 + up to 256 extra builds and a local search, 55 ms for H2O/cc-pVTZ) cost ten times the 15-pass SCF it
// served and won 6 % of its builds; a process that has seen the same work lists before starts from what it learned (qc_assign_cache).
int qc_first_build(const QcBuild &b) {
    qc_system *S = b.S;
    const std::vector<std::vector<int>> &units = b.plan.units;
    S->assign.unit_ms.assign(units.size(), 0.f);
    struct Untuned { qc_system *S; bool keep = false; ~Untuned() { if (!keep) { S->assign.unit_ms.clear(); S->assign.unit_stream.clear(); } } } untuned{S};
    // (the warm-up pass only where this process has not launched these units before: their first launches pay the code upload)
    static std::atomic<unsigned long long> units_warm{0};
    unsigned long long mine = 0;
    for (size_t u = 0; u < units.size() && u < 62; ++u) if (!units[u].empty()) mine |= 1ull << u;
    if (S->merge_bm) mine |= 1ull << 62;                 // (the merged launches are kernels of their own)
    if (S->merge_t1) mine |= 1ull << 63;
    int rc = QC_OK;
    if ((units_warm.load(std::memory_order_acquire) & mine) != mine) rc = qc_time_units_serial(b, nullptr, S->assign.unit_ms.data());
    if (rc == QC_OK) rc = qc_time_units_serial(b, nullptr, S->assign.unit_ms.data());   // serial, timed
    if (rc == QC_OK) units_warm.fetch_or(mine, std::memory_order_acq_rel);
    if (rc != QC_OK) return rc;
    static const int fixed_w = getenv("QC_TUNE_FIXED") ? atoi(getenv("QC_TUNE_FIXED")) : 0;      // (experiment switch: lanes used, no online search)
    assign_longest_first(b, S->assign.unit_ms, fixed_w >= 1 && fixed_w <= QC_NSTREAMS ? fixed_w : QC_NSTREAMS, 0.015f);
    S->assign.tune_count += 1; S->assign.gen += 1;
    const bool no_search = fixed_w >= 1 || getenv("QC_TUNE_OFF") != nullptr;
    qc_online_reset(S, no_search);
    qc_assign_cache_lookup(S);
    if (b.fa.G0) QC_HIP_CHECK(hipMemsetAsync(b.fa.G0, 0, b.accum_bytes(), S->stream));
    untuned.keep = true;
    return QC_OK;
}

// Kernels that overlap stretch each other by class-dependent factors (the bra-major launches 1.8x next to the one-wave-per-SIMD
// launches, those hardly at all), which the durations alone do not show: three concurrent builds with events around every launch,
// each proposing the longest-first assignment of the durations seen INSIDE it.  These proposals are the first trials of the online
// search and are made when it starts (its first instalment): a handle that runs one SCF does not pay for them.
static int seed_proposals(const QcBuild &b) {
    qc_system *S = b.S;
    const std::vector<std::vector<int>> &units = b.plan.units;
    const std::vector<int> keep = S->assign.unit_stream;
    EventList evl;
    if (evl.create(2 + 2 * units.size()) != QC_OK) return QC_ERR_HIP;
    std::vector<hipEvent_t> &ev = evl.ev;
    int rc = QC_OK;
    for (int round = 0; round < 3 && rc == QC_OK; ++round) {
        if (b.fa.G0) QC_HIP_CHECK(hipMemsetAsync(b.fa.G0, 0, b.accum_bytes(), S->stream));
        if ((rc = qc_issue_build(b, ev.data(), true, false)) != QC_OK) break;
        QC_HIP_CHECK(hipEventSynchronize(ev[1]));
        if ((rc = qc_join_check(S)) != QC_OK) break;
        std::vector<float> dur(units.size(), 0.f);
        for (size_t u = 0; u < units.size(); ++u)
            if (!units[u].empty()) { QC_HIP_CHECK(hipEventSynchronize(ev[3 + 2 * u])); QC_HIP_CHECK(hipEventElapsedTime(&dur[u], ev[2 + 2 * u], ev[3 + 2 * u])); }
        assign_longest_first(b, dur, QC_NSTREAMS, round == 1 ? 0.015f : 0.f);
        if (std::find(S->assign.on.cands.begin(), S->assign.on.cands.end(), S->assign.unit_stream) == S->assign.on.cands.end() && S->assign.unit_stream != keep) S->assign.on.cands.push_back(S->assign.unit_stream);
        S->assign.on.spent += 1;
    }
    S->assign.unit_stream = keep; S->assign.unit_weight = S->assign.unit_ms;
    return rc;
}

// the better of two back-to-back builds under `assign` (`ev`: two events, around the build)
static int measure_assignment(const QcBuild &b, hipEvent_t *ev, const std::vector<int> &assign, float &t) {
    qc_system *S = b.S;
    S->assign.unit_stream = assign;
    t = 1e30f;
    for (int rep = 0; rep < 2; ++rep) {
        QC_HIP_CHECK(hipMemsetAsync(b.fa.G0, 0, b.accum_bytes(), S->stream));
        int r = qc_issue_build(b, ev, false, false);
        if (r != QC_OK) return r;
        QC_HIP_CHECK(hipEventSynchronize(ev[1]));
        if ((r = qc_join_check(S)) != QC_OK) return r;
        float x = 0.f;
        QC_HIP_CHECK(hipEventElapsedTime(&x, ev[0], ev[1]));
        t = std::min(t, x);
        S->assign.on.spent += 1;
    }
    return QC_OK;
}

// The neighbourhood of the current best, in full and in a fixed order: every launch moved to every other lane, every pair of
// launches on different lanes swapped - launches of the most loaded lane first (they are the ones whose move can shorten the
// build).  The search ends when a whole sweep has found nothing (a local optimum of the FULL neighbourhood: ten random
// neighbours in a row, the rule before, left most of it unseen and ended anywhere between 0.172 and 0.192 ms on H2O/cc-pVTZ).
static void neighbours(const QcBuild &b) {
    qc_system *S = b.S;
    QcOnline &o = S->assign.on;
    o.nb.clear(); o.nb_pos = 0;
    std::vector<int> act = b.plan.active();
    const int nl = std::min(QC_NSTREAMS, S->lanes.nlanes);
    if (act.size() < 2 || nl < 2) return;
    float load[QC_NSTREAMS] = {};
    int cnt[QC_NSTREAMS] = {}, maxrank[QC_NSTREAMS] = {};
    for (int u : act) { const int k = o.best[u] & 7; load[k] += S->assign.unit_ms[u]; cnt[k] += 1; maxrank[k] = std::max(maxrank[k], o.best[u] >> 3); }
    std::stable_sort(act.begin(), act.end(), [&](int x, int y) { return load[o.best[x] & 7] > load[o.best[y] & 7]; });
    for (int u : act)
        for (int k = 0; k < nl; ++k)
            if (k != (o.best[u] & 7)) { std::vector<int> t = o.best; t[u] = k; o.nb.push_back(std::move(t)); }
    for (size_t i = 0; i < act.size(); ++i)
        for (size_t j = i + 1; j < act.size(); ++j)
            if ((o.best[act[i]] & 7) != (o.best[act[j]] & 7)) {
                std::vector<int> t = o.best;
                const int ki = t[act[i]] & 7, kj = t[act[j]] & 7;
                t[act[i]] = kj; t[act[j]] = ki;
                o.nb.push_back(std::move(t));
            }
    // order inside a lane: a launch sent to the back of its lane (the heavier-first rule is not always the better one: which kernel
    // of a chain meets which kernels of the other chains decides how far they stretch each other)
    for (int u : act) {
        const int k = o.best[u] & 7;
        if (cnt[k] >= 2 && maxrank[k] < 14) { std::vector<int> t = o.best; t[u] = k | ((maxrank[k] + 1) << 3); o.nb.push_back(std::move(t)); }
    }
}
// the next assignment to try, in o.trial: the proposals of the first build, then the neighbours not measured yet
static bool propose(const QcBuild &b) {
    QcOnline &o = b.S->assign.on;
    if (!o.cands.empty()) { o.trial = o.cands.back(); o.cands.pop_back(); return true; }
    if (o.nb.empty() && o.nb_pos == 0) neighbours(b);
    while (o.nb_pos < o.nb.size()) {
        o.trial = o.nb[o.nb_pos++];
        if (std::find(o.tried.begin(), o.tried.end(), o.trial) == o.tried.end()) { o.tried.push_back(o.trial); return true; }
    }
    return false;
}
// the three fastest assignments measured so far
static void note_top(QcOnline &o, const std::vector<int> &a, float t) {
    for (auto &e : o.top) if (e.second == a) { e.first = std::min(e.first, t); return; }
    o.top.push_back({t, a});
    std::sort(o.top.begin(), o.top.end(), [](const std::pair<float, std::vector<int>> &x, const std::pair<float, std::vector<int>> &y) { return x.first < y.first; });
    if (o.top.size() > 3) o.top.resize(3);
}
// A whole sweep without a gain is a local optimum of single moves and swaps - and those lie 0.166 to 0.195 ms apart on H2O/cc-pVTZ,
// process to process.  The search then starts again (QC_SEARCH_KICKS times) from the best assignment known with two random
// cross-lane swaps applied - a step no sweep can take - and descends from there; the best three of everything measured go to
// the finals as before.
static bool kick(const QcBuild &b) {
    QcOnline &o = b.S->assign.on;
    static const int max_kicks = getenv("QC_SEARCH_KICKS") ? atoi(getenv("QC_SEARCH_KICKS")) : QC_SEARCH_KICKS;
    if (o.kicks >= max_kicks || o.top.empty()) return false;
    std::vector<int> act = b.plan.active();
    if (act.size() < 4) return false;
    auto rnd = [&]() { o.rng ^= o.rng << 13; o.rng ^= o.rng >> 17; o.rng ^= o.rng << 5; return o.rng; };
    for (int attempt = 0; attempt < 32; ++attempt) {
        std::vector<int> t = o.top[0].second;
        for (int &x : t) x &= 7;
        for (int rep = 0; rep < 2; ++rep)
            for (int tries = 0; tries < 16; ++tries) {
                const int i = act[rnd() % act.size()], j = act[rnd() % act.size()];
                if (t[i] != t[j]) { std::swap(t[i], t[j]); break; }
            }
        if (std::find(o.tried.begin(), o.tried.end(), t) != o.tried.end()) continue;
        o.tried.push_back(t);
        o.best = t; o.nb.clear(); o.nb_pos = 0; o.kicks += 1;
        return true;
    }
    return false;
}
// the search is over: the finals inside SCF passes (qc_fock_feedback) - not for multi-rank handles, whose passes report nothing
static void search_ended(const QcBuild &b, bool dbg) {
    qc_system *S = b.S;
    QcOnline &o = S->assign.on;
    const std::vector<std::vector<int>> &units = b.plan.units;
    o.fin_sum.assign(o.top.size(), 0.0); o.fin_n.assign(o.top.size(), 0); o.fin_cur = 0;
    if (S->comm || o.top.size() < 2) o.settled = true;
    else { S->assign.unit_stream = o.top[0].second; S->assign.cand_skip = true; }
    qc_assign_cache_store(S);
    if (!dbg) return;
    if (!o.top.empty()) { o.best = o.top[0].second; o.base_ms = o.top[0].first; }
    fprintf(stderr, "[tune] search ends after %d trials, %d restarts (%ld extra builds): %.4f ms; lanes:", o.trials, o.kicks, (long)o.spent, o.base_ms);
    for (int k = 0; k < QC_NSTREAMS; ++k) {
        bool any = false;
        for (int rk = 0; rk < 16; ++rk)
            for (size_t u = 0; u < units.size(); ++u) if (!units[u].empty() && (o.best[u] & 7) == k && (o.best[u] >> 3) == rk) { fprintf(stderr, "%s u%zu(%.0f)%s", any ? "" : " [", u, S->assign.unit_ms[u] * 1e3, rk ? "'" : ""); any = true; }
        if (any) fprintf(stderr, " ]");
    }
    fprintf(stderr, "\n");
}
// an instalment is due: not in the builds of a profiling call (no G0), not before the handle has shown that it lives long
bool qc_search_due(const qc_system *S, const QcFockArgs &fa) {
    return !S->assign.on.frozen && fa.G0 && S->assign.on.builds >= QC_SEARCH_FIRST_BUILD && S->assign.on.spent + 2 * QC_SEARCH_CHUNK <= S->assign.on.builds;
}
// one instalment of the search: up to QC_SEARCH_CHUNK trials of two extra builds each
int qc_search_instalment(const QcBuild &b) {
    qc_system *S = b.S;
    QcOnline &o = S->assign.on;
    EventList evl;
    if (evl.create(2) != QC_OK) return QC_ERR_HIP;
    hipEvent_t *ev = evl.ev.data();
    static const bool dbg = getenv("QC_TUNE_DEBUG") != nullptr;
    int rc = QC_OK;
    if (o.best.empty()) o.best = S->assign.unit_stream;
    if (!o.seeded) { o.seeded = true; if ((rc = seed_proposals(b)) != QC_OK) return rc; }
    float tb = 0.f;
    if (o.base_ms <= 0.0) { if ((rc = measure_assignment(b, ev, o.best, tb)) != QC_OK) return rc; o.base_ms = tb; note_top(o, o.best, tb); }
    for (int k = 0; k < QC_SEARCH_CHUNK && !o.frozen; ++k) {
        if (!propose(b)) {
            if (!kick(b)) { o.frozen = true; break; }
            float tk = 0.f;
            if ((rc = measure_assignment(b, ev, o.best, tk)) != QC_OK) return rc;
            o.trials += 1; o.base_ms = tk;
            note_top(o, o.best, tk);
            if (dbg) fprintf(stderr, "[tune] trial %d: restart %d of the search from a perturbed best: %.4f ms (best known %.4f)\n", o.trials, o.kicks, tk, o.top[0].first);
            if (o.trials >= QC_SEARCH_TRIALS) o.frozen = true;
            continue;
        }
        const bool seeded = !o.cands.empty();
        float t = 0.f;
        if ((rc = measure_assignment(b, ev, o.trial, t)) != QC_OK) return rc;
        o.trials += 1;
        if (dbg) fprintf(stderr, "[tune] trial %d (build %ld of the handle): %.4f ms against %.4f ms - %s\n", o.trials, (long)o.builds, t, o.base_ms, t < 0.985 * o.base_ms ? "kept" : "dropped");
        if (t < 0.985 * o.base_ms) { o.best = o.trial; o.base_ms = t; o.rejects = 0; o.nb.clear(); o.nb_pos = 0; }     // (a new neighbourhood)
        else if (!seeded) o.rejects += 1;
        note_top(o, o.trial, t);
        if (o.trials >= QC_SEARCH_TRIALS) o.frozen = true;
    }
    S->assign.unit_stream = o.top.empty() ? o.best : o.top[0].second;       // (the best known - after a restart `best` is where the search stands)
    S->assign.gen += 1; S->assign.tune_count += 1;             // (this build carries extra builds: not a timing sample)
    if (o.frozen) search_ended(b, dbg);
    QC_HIP_CHECK(hipMemsetAsync(b.fa.G0, 0, b.accum_bytes(), S->stream));
    return QC_OK;
}

// (measurement hook: end the search here and now with what it has found - a harness that is about to time builds calls it so that no
// instalment falls into its timed region)
void qc_assignment_freeze(qc_system *S) {
    QcOnline &o = S->assign.on;
    if (o.settled) return;
    // (the best known: after a restart `best` is only where the search stands, and while the finals run the assignment in use is whichever
    // of the top three is being sampled)
    const std::vector<int> &keep = o.top.empty() ? o.best : o.top[0].second;
    if (!keep.empty() && S->assign.unit_stream != keep) { S->assign.unit_stream = keep; S->assign.gen += 1; }
    o.frozen = true; o.settled = true;
}
void qc_fock_feedback(qc_system *S, float build_ms, unsigned gen) {
    QcOnline &o = S->assign.on;
    if (gen != S->assign.gen) return;
    o.seen_sum += build_ms; o.seen_n += 1;
    if (!o.frozen || o.settled) return;
    if (o.top.size() < 2 || o.fin_cur >= (int)o.top.size()) { o.settled = true; return; }
    if (S->assign.cand_skip) { S->assign.cand_skip = false; return; }          // (first build under this finalist)
    o.fin_sum[o.fin_cur] += build_ms; o.fin_n[o.fin_cur] += 1;
    if (o.fin_n[o.fin_cur] < 3) return;
    auto switch_to = [&](const std::vector<int> &a) { if (S->assign.unit_stream != a) { S->assign.unit_stream = a; S->assign.gen += 1; S->assign.cand_skip = true; } };
    if (o.fin_cur + 1 < (int)o.top.size()) { o.fin_cur += 1; switch_to(o.top[o.fin_cur].second); return; }
    size_t b = 0;
    for (size_t i = 1; i < o.top.size(); ++i) if (o.fin_sum[i] / o.fin_n[i] < o.fin_sum[b] / o.fin_n[b]) b = i;
    static const bool dbg = getenv("QC_TUNE_DEBUG") != nullptr;
    if (dbg) { fprintf(stderr, "[tune] finals inside SCF passes:"); for (size_t i = 0; i < o.top.size(); ++i) fprintf(stderr, " %.4f (%.4f back to back)", o.fin_sum[i] / o.fin_n[i], o.top[i].first); fprintf(stderr, " -> %zu\n", b); }
    o.best = o.top[b].second;
    switch_to(o.best);
    o.settled = true;
    qc_assign_cache_store(S);
}
