// qc_plan.cpp - the work-list planner: from the host model's shell-pair table (qc_system.cpp) to what the Fock kernels are launched over.
// Host-only integer code; tests/host/plan_dump_main.cpp prints everything it decides.  In the order it runs:
//   qc_build_classes   every unique quartet (pair P >= pair Q) gets a launch class (classify), two kinds of short lists move
//                      (short_pp_list_to_columns, short_lgc5_lists_to_wave64), the classes are made and the launch merges decided;
//   qc_build_shards    per class: order, screen, deal to the ranks, cut (bundles with the chunk decision, or slots with the tile split),
//                      work model, sizes.  With meta_only: the sizes alone, over the whole task lists.
// The A/B switches of all of it: QcPlanSwitches (qc_internal.h; table in DESIGN.md 2).
#include <algorithm>
#include <cstdlib>

#include "qc_internal.h"

QcPlanSwitches QcPlanSwitches::from_env() {
    QcPlanSwitches w;
    auto flag = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; };
    w.no_bm_pp = flag("QC_NO_BM_PP"); w.no_bm_ps4 = flag("QC_NO_BM_PS4"); w.no_t1_merge = flag("QC_NO_T1_MERGE"); w.no_bm_merge = flag("QC_NO_BM_MERGE");
    w.bm_pp_min = num("QC_BM_PP_MIN", w.bm_pp_min); w.mfma4_max = num("QC_MFMA4_MAX", w.mfma4_max); w.bm_merge_max = num("QC_BM_MERGE_MAX", w.bm_merge_max);
    w.bm_pq = (int)num("QC_BM_PQ", w.bm_pq); w.bm_pp_pq = (int)num("QC_BM_PP_PQ", w.bm_pp_pq);
    w.bm_unit = (int)num("QC_BM_UNIT", w.bm_unit); w.bm_pp_unit = (int)num("QC_BM_PP_UNIT", w.bm_pp_unit);
    w.bm_gain = (int)num("QC_BM_GAIN", w.bm_gain);
    return w;
}

// Lane-group widths the kernels are instantiated for, per ket Hermite order (the switch in qc_fock_tier_kernel).  A group is
// made of whole 16-lane rows - the Hermite contractions broadcast inside rows (DPP) - so the 5..10 columns of a ds / fs ket
// leave lanes idle; as 8-lane groups with LDS-fed contractions those classes were 20 % slower.
int qc_lgc_for(int lab, int lcd, int ncd) {
    if (qc_mfma_always(lab, lcd)) return 6;         // matrix-core classes: one slot per wave, always the full wave
    static const int allowed[QC_LPAIR + 1][4] = {{4, -1, -1, -1}, {4, -1, -1, -1}, {4, -1, -1, -1}, {4, 5, -1, -1}, {5, 6, -1, -1}, {6, -1, -1, -1}, {6, -1, -1, -1}};
    for (int i = 0; i < 4 && allowed[lcd][i] >= 0; ++i)
        if ((1 << allowed[lcd][i]) >= ncd) return allowed[lcd][i];
    return 6;   // wider than a wave: the kernel makes several column passes
}

namespace {

// ---- launch classes
// A launch class (LAB, LCD, LGC, bm) and its place in the class order
struct BucketKey {
    int LAB, LCD, LGC; bool bm;
    static constexpr int count = (QC_LPAIR + 1) * (QC_LPAIR + 1) * 7 * 2;
    int index() const { return (((LAB * (QC_LPAIR + 1) + LCD) * 7) + LGC) * 2 + (bm ? 1 : 0); }
    static BucketKey of(int b) { return BucketKey{b / 14 / (QC_LPAIR + 1), (b / 14) % (QC_LPAIR + 1), (b / 2) % 7, (b & 1) != 0}; }
    static BucketKey bra_major(int LAB, int LCD) { return BucketKey{LAB, LCD, 0, true}; }
    static BucketKey column(int LAB, int LCD, int ncd) { return BucketKey{LAB, LCD, qc_lgc_for(LAB, LCD, ncd), false}; }
    static BucketKey pp() { return bra_major(2, 2); }                       // the p.p-ket bra-major class
    bool fket_column() const { return !bm && LCD >= 5; }                    // a column class with f.d / f.f kets
};
using Buckets = std::vector<std::vector<QcTask>>;
struct Placed { BucketKey key; QcTask task; };
void move_list(std::vector<QcTask> &from, std::vector<QcTask> &to) { to.insert(to.end(), from.begin(), from.end()); from.clear(); }

// Where the unique quartet (pair P | pair Q) goes, and which of the two is its bra.
//  * bra-major classes (bm): the narrower pair is an ss or ps pair and LAB + LCD <= QC_LREG.  It becomes the ket,
//    one lane per quartet: the per-primitive-quartet contraction costs ncd * HAB * HCD FMAs, so the pair with the
//    fewest functions belongs on the side that is contracted inside the primitive loop, and the bra side (shared
//    by the whole wave) is contracted once per bra primitive pair.
//  * all others: column kernels, the wider pair is the ket (one lane per ket function pair, R table shared in LDS).
// (the A/B switches of the classification are read once per system - a test switches them - and NOT per quartet: two getenv calls in this
// loop were 0.6 us each, a third of the time a handle took to create)
Placed classify(const qc_system *S, int P, int Q) {
    const QcPairDesc &dp = S->pairs[P], &dq = S->pairs[Q];
    const int np_ = dp.na * dp.nb, nq_ = dq.na * dq.nb;
    const bool p_is_wide = (np_ > nq_) || (np_ == nq_ && dp.L >= dq.L);
    const int wide = p_is_wide ? P : Q, narrow = p_is_wide ? Q : P;
    const QcPairDesc &dn = S->pairs[narrow], &dw = S->pairs[wide];
    // (round 3) p.p kets against p.p / d.s bras, total order 4: bra-major too - lane-per-quartet with the packed p.p records, three
    // bundles per ket group (one per Cartesian axis of the ket's first function, three columns each); the pair that would be the
    // ket of the column kernels (the wide one) stays the ket.  QC_NO_BM_PP: the column kernels keep them (A/B switch).
    const bool w_is_pp = S->shells[S->pairA[wide]].L == 1 && S->shells[S->pairB[wide]].L == 1;
    // (round 3: ps kets against d.d / f.p bras - total order 5: the table of 56 entries next to W[3][35] in a lane, one wave per SIMD
    // like the d.p / f.s bras of that launch - in the bra-major form too.  The column kernels ran (ps|dd) at 1.7 TFLOP/s; measured,
    // alternating runs on one box: H2O/cc-pVTZ iteration 0.3481 against 0.3529 ms (twelve runs each; the LCD = 4 bucket was 944 of the
    // 1444 waves of its tier<1, 1> launch), benzene/cc-pVDZ build 1.398 against 1.390 ms (four each: one launch fewer, no change).
    // QC_NO_BM_PS4 keeps them with the column kernels.)
    const bool ps4 = !S->plan.no_bm_ps4 && dn.L == 1 && dw.L == 4;
    if ((dn.L <= 1 && dn.L + dw.L <= QC_LREG) || ps4) return Placed{BucketKey::bra_major(dw.L, dn.L), QcTask{wide, narrow}};
    if (!S->plan.no_bm_pp && S->pp_ok && dn.L == 2 && dw.L == 2 && w_is_pp && dw.K <= 63 && QC_LREG >= 4) return Placed{BucketKey::pp(), QcTask{narrow, wide}};
    return Placed{BucketKey::column(dn.L, dw.L, dw.na * dw.nb), QcTask{narrow, wide}};
}

// The p.p-ket bra-major class pays where its list fills the chip (benzene/cc-pVDZ: 45 480 quartets, 0.148 ms against 0.186 ms in the
// column kernels, build -6 %); a small molecule's few hundred bundles are one more latency-bound launch (H2O/cc-pVTZ: 1526 quartets,
// no gain measured) - those stay with the column kernels.  QC_BM_PP_MIN overrides the threshold.
void short_pp_list_to_columns(const qc_system *S, Buckets &bucket) {
    auto &ppb = bucket[BucketKey::pp().index()];
    if (!ppb.empty() && (long)ppb.size() < S->plan.bm_pp_min) move_list(ppb, bucket[BucketKey::column(2, 2, 9).index()]);
}

// d.d / f.p kets against d.p ... f.f bras: a short list (a small molecule) goes to the 64-lane instance of its class, which runs the
// contractions as matrix-core tiles with one wave per 16-column tile; a long one keeps the 32-lane VALU form with two slots per wave
// (benzene/cc-pVDZ: the tile form cost the full chip 2.6 % in round 2).  QC_MFMA4_MAX: longest list that switches (0: never).
// (only where the wide-ket launches are the f-capable kernels - a basis with f functions; without them the launch is the variant
// that carries the d.d / f.p-ket bodies alone, in their VALU form, at two waves per SIMD: qc_fock_tier_kernel<LAB, 2>)
void short_lgc5_lists_to_wave64(qc_system *S, Buckets &bucket) {
    S->has_fkets = false;
    for (int b = 0; b < BucketKey::count; ++b) if (BucketKey::of(b).fket_column() && !bucket[b].empty()) S->has_fkets = true;
    for (int lab = 3; S->has_fkets && lab <= QC_LPAIR; ++lab) {
        auto &b5 = bucket[BucketKey{lab, 4, 5, false}.index()], &b6 = bucket[BucketKey{lab, 4, 6, false}.index()];
        if (!b5.empty() && (long)b5.size() <= S->plan.mfma4_max) move_list(b5, b6);
    }
}

// Which launches of a build ride together (qc_build_unit_of)
void decide_launch_merges(qc_system *S) {
    // one launch for the wide-ket buckets of the low bra classes (qc_fock_tier1_low_kernel) where there are f-ket buckets among them -
    // without f functions those launches are the two-waves-per-SIMD variants and stay apart.  QC_NO_T1_MERGE: off (A/B switch).
    int nseg[3] = {0, 0, 0}; bool fket = false;
    for (const auto &c : S->classes) if (!c.bm && c.LCD >= 4) { ++nseg[c.LAB <= 2 ? 0 : (c.LAB <= 4 ? 1 : 2)]; fket = fket || c.LCD >= 5; }
    S->merge_t1 = fket && std::max(nseg[0], std::max(nseg[1], nseg[2])) <= 12 && !S->plan.no_t1_merge;
    bool has01 = false, has10 = false;
    for (const auto &c : S->classes) if (c.bm) { has01 = has01 || (c.LCD == 0 && c.LAB >= 3); has10 = has10 || (c.LCD == 1 && c.LAB <= 2); }
    // (a matter of launch count, so only for small builds: one launch less is 5 % of an H2O/cc-pVTZ build (32 k quartets, 0.17 ms); in a long
    // build the merged launch is the longest chain by itself - benzene/cc-pVDZ, 1.1 M quartets: builds 1.379 ms apart against 1.405
    // merged, three alternating runs each.  QC_BM_MERGE_MAX: the limit in quartets)
    size_t q_all = 0;
    for (const auto &c : S->classes) q_all += c.tasks.size();
    S->merge_bm = has01 && has10 && (long)q_all <= S->plan.bm_merge_max && !S->plan.no_bm_merge;
}

// ---- sorting
// stable counting sort, ascending key in [0, nkeys): the list orders below have small integer keys, and a comparator merge sort over the
// two to four million entries of a large system's bra-major classes was 200 of the 250 ms its work lists took (this container's host)
template <class T, class KeyFn>
void counting_sort(std::vector<T> &v, size_t nkeys, KeyFn key) {
    if (v.size() < 2) return;
    std::vector<uint32_t> cnt(nkeys + 1, 0);
    for (const auto &x : v) ++cnt[(size_t)key(x) + 1];
    for (size_t i = 1; i < cnt.size(); ++i) cnt[i] += cnt[i - 1];
    std::vector<T> out(v.size());
    for (const auto &x : v) out[cnt[(size_t)key(x)]++] = x;
    v.swap(out);
}
// stable, descending by a non-negative integer key: the counting sort where every key is below `bound`, std::stable_sort above it
template <class T, class KeyFn>
void sort_descending(std::vector<T> &v, int64_t bound, KeyFn key) {
    int64_t kmax = 0;
    for (const auto &x : v) kmax = std::max(kmax, (int64_t)key(x));
    if (kmax < bound) counting_sort(v, (size_t)kmax + 1, [&](const T &x) { return kmax - (int64_t)key(x); });
    else std::stable_sort(v.begin(), v.end(), [&](const T &x, const T &y) { return (int64_t)key(x) > (int64_t)key(y); });
}
constexpr int64_t PRIM_KEYS = 1 << 20, COST_KEYS = 1 << 22;      // key bounds: primitive counts, bundle cost
// by bra, inside a bra the longest first, stable: the minor key first, then the major one
template <class T, class LenFn>
void sort_by_bra_longest_first(const qc_system *S, std::vector<T> &v, LenFn len) {
    sort_descending(v, PRIM_KEYS, len);
    counting_sort(v, S->pairs.size(), [](const T &x) { return x.bra; });
}
// long bundles first (stable): the tail of the launch is made of short ones.  cost = bra primitive pairs x longest ket
void long_bundles_first(std::vector<QcBundle> &bundles) {
    sort_descending(bundles, COST_KEYS, [](const QcBundle &x) { return (int64_t)(x.ij_hi - x.ij_lo) * x.maxK; });
}
const auto slot_length = [](const QcSlot &s) { return s.hi - s.lo; };
int64_t prim_quartets(const qc_system *S, const QcTask &t) { return (int64_t)S->pairs[t.bra].K * S->pairs[t.ket].K; }

}  // namespace

// Cut quartets into slots of at most `itmax` primitive quartets; longest first so the slots batched into one wave
// have (nearly) equal trip counts.  With `split_cols` (matrix-core classes that cannot fill the chip) a slot is further
// cut into the 16-column tiles of the ket block: the integrals of different ket columns are independent all the way into
// the digestion, so a single (ff|ff) quartet is then worked on by four waves (each repeats the R table, none waits).
void qc_make_slots(const qc_system *S, const std::vector<QcTask> &tasks, int itmax, bool split_cols, std::vector<QcSlot> &out) {
    out.clear();
    for (const auto &t : tasks) {
        const int npq = S->pairs[t.bra].K * S->pairs[t.ket].K, ncd = S->pairs[t.ket].na * S->pairs[t.ket].nb;
        const int step = itmax > 0 ? itmax : npq;
        const int nparts = (npq + step - 1) / step;
        const int ctile = split_cols ? 16 : ncd;
        for (int s = 0; s < nparts; ++s) {   // equal-length parts
            const int lo = (int)((int64_t)npq * s / nparts), hi = (int)((int64_t)npq * (s + 1) / nparts);
            for (int c0 = 0; c0 < ncd; c0 += ctile) out.push_back(QcSlot{t.bra, t.ket, lo, hi, c0, std::min(ncd, c0 + ctile)});
        }
    }
    sort_descending(out, PRIM_KEYS, slot_length);
}

// Bra-major work units: the tasks of one bra pair, kets sorted by primitive count (so the lanes of a wave run nearly
// equal trip counts), cut into bundles of at most 64 kets; with itmax > 0 a bundle is further cut along the bra primitive
// pairs so that a lane evaluates about itmax primitive quartets.
// `unit` > 0 (round 3): a lane's work unit is a CHUNK of at most `unit` primitives of a ket pair instead of the whole pair - the entry of
// `ketlist` then carries the chunk (ket | first primitive << 18 | length << 25, seven bits each; length 0 = the whole pair, as the set-up
// passes use it).  Integrals are linear in the ket primitives and the digestion is linear in the integrals, so every chunk is digested on its own.
// With whole pairs a wave runs as long as its most contracted ket (64 primitive pairs for a pair of contracted s shells) while the
// lanes of single-primitive kets idle, and a molecule with few shell pairs cannot fill 64 lanes per bra at all (H2O/cc-pVTZ: 55 ss
// pairs); chunks of equal length fill the lanes and bound the trip count.
bool qc_make_bundles(const qc_system *S, const std::vector<QcTask> &tasks, int itmax, std::vector<QcBundle> &bundles, std::vector<int> &ketlist, int unit) {
    bundles.clear(); ketlist.clear();
    if (S->pairs.size() >= (1u << QC_KET_BITS)) unit = 0;
    for (const auto &t : tasks) if (S->pairs[t.ket].K > 127) unit = 0;      // (does not fit the packed entry: whole pairs)
    const bool packed = unit > 0 && !tasks.empty();                         // (else the entries are plain pair indices)
    // a lane's unit: its bra and its ket-list entry - the packed chunk, or the plain index of the whole pair
    auto ket_of = [&](const QcTask &u) { int ket, kl0, len; qc_unpack_ket_entry(u.ket, packed, &ket, &kl0, &len); return ket; };
    auto len_of = [&](const QcTask &u) { return packed ? (int)((unsigned)u.ket >> (QC_KET_BITS + 7)) : S->pairs[u.ket].K; };
    std::vector<QcTask> us;
    if (packed) {
        us.reserve(tasks.size() * 2);
        for (const auto &t : tasks) {
            const int K = S->pairs[t.ket].K, nch = (K + unit - 1) / unit;
            for (int c = 0; c < nch; ++c) {      // equal-length chunks
                const int lo = (int)((int64_t)K * c / nch), hi = (int)((int64_t)K * (c + 1) / nch);
                us.push_back(QcTask{t.bra, (int)qc_pack_ket_entry(t.ket, lo, hi - lo)});
            }
        }
    } else us = tasks;
    sort_by_bra_longest_first(S, us, len_of);
    ketlist.reserve(us.size());
    for (size_t i = 0, j; i < us.size(); i = j) {
        for (j = i; j < us.size() && us[j].bra == us[i].bra && j - i < 64;) ++j;
        const int Kab = S->pairs[us[i].bra].K, maxK = len_of(us[i]);
        const int first = (int)ketlist.size();
        for (size_t k = i; k < j; ++k) ketlist.push_back(us[k].ket);
        int nparts = 1;
        if (packed) {
            // bra primitive pairs per bundle: about max(itmax, 32) primitive quartets per lane, so that the digestion of a partial block
            // (two to three primitive quartets' worth of instructions) stays a small share.  QC_BM_PQ / QC_BM_PP_PQ (A/B switches); the
            // p.p-ket class - large lists only - amortises its heavier digestion over three times the rows: 0.148 -> 0.131 ms alone on benzene
            const bool ket_pp = S->pairs[ket_of(us[i])].L == 2;
            const int rows = std::max(1, std::min(Kab, std::max(itmax, ket_pp ? S->plan.bm_pp_pq : S->plan.bm_pq) / std::max(maxK, 1)));
            nparts = (Kab + rows - 1) / rows;
        } else if (itmax > 0)
            nparts = (int)std::min<int64_t>(Kab, std::max<int64_t>(1, ((int64_t)Kab * maxK + itmax - 1) / itmax));
        for (int s = 0; s < nparts; ++s)
            bundles.push_back(QcBundle{us[i].bra, (int)((int64_t)Kab * s / nparts), (int)((int64_t)Kab * (s + 1) / nparts), first, (int)(j - i), maxK, 0, 0});
    }
    long_bundles_first(bundles);
    return packed;
}

namespace {

// ---- the steps of qc_build_shards, per class
// heaviest first: the primitive-quartet count is the dominant cost inside a class.  A stable counting sort on that count (a
// product of two primitive-pair counts: a few thousand at most) - the comparator sort with its four indirections per comparison
// was most of the 105 ms benzene/cc-pVDZ's lists took on the GPU box's host, twice per cold handle.
void order_tasks(const qc_system *S, std::vector<QcTask> &tasks) {
    sort_descending(tasks, PRIM_KEYS, [S](const QcTask &t) { return prim_quartets(S, t); });
}

// Schwarz screening (once the factors exist - they come from a device pass): |(ab|cd)| <= Q_ab Q_cd, quartets below
// schwarz_tau are not evaluated.  Density-independent, so the work lists stay static; the reference visits every quartet
// (its own TODO, uhf.rs:49-50), throughput figures keep counting the enumerated ones.
void screen_tasks(const qc_system *S, const std::vector<QcTask> &tasks, std::vector<QcTask> &kept) {
    const bool screen = !S->pairQ.empty() && S->schwarz_tau > 0.0;
    kept.clear();
    for (const auto &t : tasks)
        if (!screen || S->pairQ[t.bra] * S->pairQ[t.ket] >= S->schwarz_tau) kept.push_back(t);
}

// this rank's share of class `ci` (qc_shard_owner)
void deal_to_rank(const qc_system *S, size_t ci, bool bm, const std::vector<QcTask> &kept, std::vector<QcTask> &shard) {
    shard.clear();
    std::vector<QcBundle> pb; std::vector<int> kl;
    if (bm && S->nranks > 1) qc_make_bundles(S, kept, 0, pb, kl);
    if (pb.size() >= (size_t)8 * S->nranks) {
        // enough of them: deal whole 64-ket bundles, not single quartets, so a rank's waves stay full
        for (size_t i = 0; i < pb.size(); ++i)
            if (qc_shard_owner(i, S->nranks, ci) == S->rank)
                for (int k = 0; k < pb[i].nket; ++k) shard.push_back(QcTask{pb[i].bra, kl[pb[i].first + k]});
    } else {
        for (size_t i = 0; i < kept.size(); ++i)
            if (qc_shard_owner(i, S->nranks, ci) == S->rank) shard.push_back(kept[i]);
    }
}

// slot length: long enough to amortise the per-slot digestion, short enough that the class still fills the chip
int slot_itmax(const qc_system *S, const QcClass &c) {
    int64_t tot_pq = 0;
    for (const auto &t : c.shard) tot_pq += prim_quartets(S, t);
    const int64_t want_waves = 256 * 8, G = 64 >> c.LGC;
    // (at least 8 = one hoisted chunk: shorter slots only multiply the per-slot set-up and digestion; A/B on H2O/cc-pVTZ,
    // three runs each: 2 -> 0.346, 8 -> 0.327, 16 -> 0.342, 64 -> 0.465 ms per build)
    return (int)std::min<int64_t>(QC_SLOT_ITMAX, std::max<int64_t>(8, tot_pq / (want_waves * G)));
}

// ket-primitive chunks instead of whole ket pairs where they save instructions of the slowest lanes.  QC_BM_UNIT / QC_BM_PP_UNIT (the
// p.p-ket class): primitives per chunk, 0 = whole ket pairs; QC_BM_GAIN: percent of the old cost (A/B switches).
// Model of a list: sum over its bundles of (bra primitive pairs x longest chunk) + 6 for the digestion of the lanes' partial
// blocks.  Measured (four alternating runs each, H2O / benzene build in ms; whole pairs 0.269 / 1.642): chunks wherever this
// model gains 0.229 / 1.640; only in the launches of the low bras (LAB <= 2) 0.240 / 1.601; with a model that also prices
// step 3 - paid per bra primitive pair and LANE, 4116 FMAs for an (ff| bra, whatever the chunk length - 0.233 / 1.635.  So:
// the low-bra launches switch where the model gains (>= 20 % for lists that fill the chip, any modelled gain and up to a
// 20 % modelled loss for lists that cannot - there a launch is as long as its longest wave); the high-bra launches only when
// the list is tiny (H2O's 192 bundles).
void chunks_where_they_pay(const qc_system *S, QcClass &c, int itmax) {
    if (S->plan.bm_unit <= 0) return;
    auto cost = [](const std::vector<QcBundle> &bs) { int64_t t = 0; for (const auto &b : bs) t += (int64_t)(b.ij_hi - b.ij_lo) * b.maxK + 6; return t; };
    std::vector<QcBundle> ub; std::vector<int> uk;
    const bool upacked = qc_make_bundles(S, c.shard, itmax, ub, uk, c.LCD == 2 ? S->plan.bm_pp_unit : S->plan.bm_unit);
    const bool high_bra = c.LAB >= 3;
    const int gain = S->plan.bm_gain > 0 ? S->plan.bm_gain : (c.bundles.size() < 4096 ? 120 : 80);
    const bool allowed = !high_bra || c.bundles.size() < 512;
    if (!ub.empty() && allowed && cost(ub) * 100 < cost(c.bundles) * gain) { c.bundles.swap(ub); c.ketlist.swap(uk); c.ket_packed = upacked; }
}

void cut_bundles(const qc_system *S, QcClass &c, int itmax) {
    c.ket_packed = qc_make_bundles(S, c.shard, itmax, c.bundles, c.ketlist);
    chunks_where_they_pay(S, c, itmax);
    if (c.LCD == 2) {   // p.p kets: every bundle three times, once per Cartesian axis of the ket's first function (QcBundle::pad0)
        std::vector<QcBundle> b3;
        b3.reserve(3 * c.bundles.size());
        for (const auto &b : c.bundles)
            for (int ax = 0; ax < 3; ++ax) { QcBundle x = b; x.pad0 = ax; b3.push_back(x); }
        c.bundles.swap(b3);
    }
}

void cut_slots(const qc_system *S, QcClass &c, int itmax) {
    qc_make_slots(S, c.shard, itmax, false, c.slots);
    // a matrix-core class (one slot per wave) with fewer slots than the chip has SIMDs: one wave per 16-column tile
    if ((qc_mfma_always(c.LAB, c.LCD) || (S->has_fkets && qc_use_mfma(c.LAB, c.LCD))) && c.LGC == 6 && c.slots.size() * 4 <= 1024) qc_make_slots(S, c.shard, itmax, true, c.slots);
}

void work_model(const qc_system *S, QcClass &c) {
    c.prim_quartets = 0; c.bytes_alg = 0; c.flops_alg = 0;
    for (const auto &t : c.shard) {
        const QcPairDesc &b = S->pairs[t.bra], &k = S->pairs[t.ket];
        const QcShell &A = S->shells[S->pairA[t.bra]], &B = S->shells[S->pairB[t.bra]];
        const QcShell &C = S->shells[S->pairA[t.ket]], &D = S->shells[S->pairB[t.ket]];
        const double Kab = S->pairKfull[t.bra], Kcd = S->pairKfull[t.ket], L = b.L + k.L;   // model on enumerated primitives
        const double hab = qc_nherm(b.L), hcd = qc_nherm(k.L);
        const double na = b.na, nb = b.nb, nc = k.na, nd = k.nb;
        const double ca = A.ncart, cb = B.ncart, cc = C.ncart, cd = D.ncart;
        c.prim_quartets += (int64_t)b.K * k.K;          // evaluated (after the primitive-pair cut-off)
        // SURVEY.md 8(d) work model, verbatim
        c.bytes_alg += 8.0 * (5.0 * (Kab + Kcd) + 3.0 * (na * nb + nc * nd + na * nc + na * nd + nb * nc + nb * nd));
        // (the two Hermite -> Cartesian terms depend on which pair is transformed first; the model takes the cheaper order, so that the
        // figure is a function of the quartet and not of the orientation a launch class happens to store it in)
        const double tr_ab_first = 2.0 * ca * cb * hab * hcd + 2.0 * ca * cb * cc * cd * hcd;
        const double tr_cd_first = 2.0 * cc * cd * hcd * hab + 2.0 * cc * cd * ca * cb * hab;
        c.flops_alg += Kab * Kcd * (40.0 * (L + 1) + 3.0 * qc_rwork((int)L) + 2.0 * hab * hcd) + std::min(tr_ab_first, tr_cd_first) +
                       12.0 * na * nb * nc * nd;
    }
}

// LDS doubles one lane group of a column kernel with 2^lgc lanes needs for a quartet (layout in qc_fock_kernel.h): the head region, the
// I block, density tiles (the bra block is read straight from memory); with `accumulators` (64-lane groups) + those of the six target blocks
int column_slot_words(const qc_system *S, const QcTask &t, int lgc, bool accumulators) {
    const QcPairDesc &b = S->pairs[t.bra], &k = S->pairs[t.ket];
    const int ncd = k.na * k.nb, nab = b.na * b.nb, kt = b.na * k.na + b.na * k.nb + b.nb * k.na + b.nb * k.nb;
    return qc_region0(b.L + k.L, lgc) + nab * ncd + nab + ncd + 2 * kt + (accumulators ? ncd + 2 * kt : 0);
}
int column_lds_bytes(const QcClass &c, int words, int lgc) {
    return words * 8 * (64 >> lgc) + (qc_hoisted(c.LAB + c.LCD) ? 0 : qc_nplan(c.LAB + c.LCD) * 8);   // + the R recurrence plan
}
// Slot words / LDS bytes of the class over `list` - the whole task list (an upper bound of any shard's) or the shard -, of its
// column-kernel form (p.p-ket bra-major classes: what the column kernels need for this class, the set-up passes run it through them;
// over the whole task list either way), rows of the bra-major exchange buffer
void class_sizes(const qc_system *S, QcClass &c, const std::vector<QcTask> &list) {
    c.bm_rows = 0;
    if (!c.bm) {
        int words = 0;
        for (const auto &t : list) words = std::max(words, column_slot_words(S, t, c.LGC, c.LGC == 6));
        c.slot_words = words;
        c.lds_bytes = column_lds_bytes(c, words, c.LGC);
        return;
    }
    if (c.LCD == 2) {
        c.col_lgc = qc_lgc_for(c.LAB, c.LCD, 9);
        int cw = 0;
        for (const auto &t : c.tasks) cw = std::max(cw, column_slot_words(S, t, c.col_lgc, false));
        c.col_slot_words = cw;
        c.col_lds_bytes = column_lds_bytes(c, cw, c.col_lgc);
    }
    int mx = 0;          // I[nab * ncd][65]: one column per lane
    for (const auto &t : list) {
        const QcPairDesc &b = S->pairs[t.bra], &k = S->pairs[t.ket];
        mx = std::max(mx, qc_bm_wave_words(c.LAB, b.na * b.nb, c.LCD == 2 ? 3 : k.na * k.nb));
        c.bm_rows = std::max(c.bm_rows, b.na + b.nb);
    }
    c.slot_words = mx;
    c.lds_bytes = mx * 8;
}

}  // namespace

// unique quartets (pair P >= pair Q), bucketed by launch class; the classes in the order of their bucket index
void qc_build_classes(qc_system *S, QcLap &lap) {
    const int np = (int)S->pairs.size();
    Buckets bucket(BucketKey::count);
    for (int P = 0; P < np; ++P)
        for (int Q = 0; Q <= P; ++Q) {
            const Placed pl = classify(S, P, Q);
            bucket[pl.key.index()].push_back(pl.task);
        }
    short_pp_list_to_columns(S, bucket);
    short_lgc5_lists_to_wave64(S, bucket);
    lap("quartets into buckets");
    S->classes.clear();
    for (int b = 0; b < BucketKey::count; ++b) {
        if (bucket[b].empty()) continue;
        const BucketKey key = BucketKey::of(b);
        QcClass c;
        c.bm = key.bm; c.LGC = key.LGC; c.LCD = key.LCD; c.LAB = key.LAB;
        c.tasks = std::move(bucket[b]);
        S->classes.push_back(std::move(c));
    }
    decide_launch_merges(S);
    lap("classes");
}

// Static shard: inside every launch class the cost-sorted quartet list is dealt to the ranks in boustrophedon order
// (0..N-1, N-1..0, ...; start rank rotated per class), so each rank holds the same mix of classes and nearly the same
// modelled cost.  Data-only; no communication.
void qc_build_shards(qc_system *S, bool meta_only) {
    S->lists_stale = meta_only;
    static const bool sdbg = getenv("QC_SETUP_DEBUG") != nullptr;
    double tacc[5] = {0, 0, 0, 0, 0};
    double tlast = qc_now_ms();
    auto acc = [&](int k) { if (sdbg) { const double t = qc_now_ms(); tacc[k] += t - tlast; tlast = t; } };
    S->nscreened = 0;
    std::vector<QcTask> kept;
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        auto &c = S->classes[ci];
        c.shard.clear(); c.slots.clear(); c.bundles.clear(); c.ketlist.clear();
        if (meta_only) {
            c.prim_quartets = 0; c.bytes_alg = 0; c.flops_alg = 0;
            class_sizes(S, c, c.tasks);
            // (a column class in the passes that launch its WHOLE list - Schwarz pass, ERI tensor - needs these sizes, not the screened
            // shard's: kept where class_sizes(.., c.shard) does not touch them, next to those of the p.p-ket bra-major classes)
            if (!c.bm) { c.col_lgc = c.LGC; c.col_slot_words = c.slot_words; c.col_lds_bytes = c.lds_bytes; }
            continue;
        }
        order_tasks(S, c.tasks);
        acc(0);
        screen_tasks(S, c.tasks, kept);
        S->nscreened += (int64_t)(c.tasks.size() - kept.size());
        deal_to_rank(S, ci, c.bm, kept, c.shard);
        acc(1);
        const int itmax = slot_itmax(S, c);
        if (c.bm) cut_bundles(S, c, itmax);
        else cut_slots(S, c, itmax);
        acc(c.bm ? 2 : 3);
        work_model(S, c);
        class_sizes(S, c, c.shard);
        acc(4);
    }
    if (sdbg && !meta_only) fprintf(stderr, "[lists] order %.2f  screen + deal %.2f  bundles %.2f  slots %.2f  work model + sizes %.2f ms\n", tacc[0], tacc[1], tacc[2], tacc[3], tacc[4]);
}
