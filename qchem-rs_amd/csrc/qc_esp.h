// qc_esp.h - what the kernels of the potential and the field on points (qc_points.hip) and of the point-charge embedding (qc_embed.hip)
// share: the compile-time plan of the Hermite-Coulomb table R^0_tuv in registers, the dispatch of a run-time table order to its instance,
// the rescaling of the stored expansion blocks to the nuclear-attraction prefactor, the layout of records grouped by pair order, the
// Hermite records of a density, the ordered sum of tile sums, the phase clock of a call.
#pragma once
#include <type_traits>
#include <utility>
#include <vector>

#include "qc_fock_kernel.h"
#include "qc_md.h"

// The pair data holds E[h][ab] in basis functions with sqrt(2) pi^{5/4} / p folded in (the pair half of the ERI prefactor,
// qc_build_model); the nuclear-attraction integral carries 2 pi / p instead: the ratio is the constant below.
constexpr double ESP_RESCALE = 1.41421356237309504880 / 1.33133536380038971280;      // sqrt(2) / pi^{1/4}
struct EspGroups { long long off[QC_LPAIR + 1]; };       // first double of the records of order L in the record array

// ---- the Hermite-Coulomb table R^0_tuv, t + u + v <= L, in ONE array of nherm(L) registers: level n overwrites level n + 1 from the
// highest order down (an entry of order N reads orders N - 1 and N - 2 of the level above, which are still in place), the step is
// qc_md_r_step's.  The plan is a compile-time list, every index a constant: nothing is addressed dynamically.
struct EspRStep { short dst, s1, s2; signed char ax, cf, seed; };        // seed >= 0: R[0] = (-2p)^seed F_seed
template <int L> struct EspRPlan { EspRStep s[qc_rwork(L)]; };
template <int L> constexpr EspRPlan<L> esp_make_rplan() {
    EspRPlan<L> P{};
    int k = 0;
    P.s[k++] = EspRStep{0, 0, 0, 0, 0, (signed char)L};
    for (int n = L - 1; n >= 0; --n) {
        for (int N = L - n; N >= 1; --N)
            for (int t = N; t >= 0; --t)
                for (int u = N - t; u >= 0; --u) {
                    const int v = N - t - u;
                    EspRStep e{(short)qc_hidx(t, u, v), 0, 0, 0, 0, -1};
                    if (t) { e.ax = 0; e.s1 = (short)qc_hidx(t - 1, u, v); e.cf = (signed char)(t - 1); e.s2 = (short)(t > 1 ? qc_hidx(t - 2, u, v) : 0); }
                    else if (u) { e.ax = 1; e.s1 = (short)qc_hidx(t, u - 1, v); e.cf = (signed char)(u - 1); e.s2 = (short)(u > 1 ? qc_hidx(t, u - 2, v) : 0); }
                    else { e.ax = 2; e.s1 = (short)qc_hidx(t, u, v - 1); e.cf = (signed char)(v - 1); e.s2 = (short)(v > 1 ? qc_hidx(t, u, v - 2) : 0); }
                    P.s[k++] = e;
                }
        P.s[k++] = EspRStep{0, 0, 0, 0, 0, (signed char)n};
    }
    return P;
}
template <int L> inline constexpr EspRPlan<L> esp_rplan = esp_make_rplan<L>();

template <int L, int S>
__device__ __forceinline__ void esp_rstep(double (&R)[qc_nherm(L)], const double (&seed)[L + 1], const double (&X)[3]) {
    constexpr EspRStep e = esp_rplan<L>.s[S];
    if constexpr (e.seed >= 0) R[0] = seed[e.seed];
    else if constexpr (e.cf > 0) R[e.dst] = X[e.ax] * R[e.s1] + (double)e.cf * R[e.s2];
    else R[e.dst] = X[e.ax] * R[e.s1];
}
template <int L, int... S>
__device__ __forceinline__ void esp_rtable(double (&R)[qc_nherm(L)], const double (&seed)[L + 1], const double (&X)[3], std::integer_sequence<int, S...>) {
    (esp_rstep<L, S>(R, seed, X), ...);
}
// R^0_tuv(p, X), t + u + v <= L: Boys function from the handle's tables, the seeds (-2p)^n F_n as a running product, the plan above
template <int L>
__device__ __forceinline__ void esp_table(double p, const double (&X)[3], const double *__restrict__ boys, double (&R)[qc_nherm(L)]) {
    double F[L + 1], seed[L + 1];
    qc_boys<L>(p * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), boys, F);
    double f = 1.0;
#pragma unroll
    for (int m = 0; m <= L; ++m) { seed[m] = f * F[m]; f *= -2.0 * p; }
    esp_rtable<L>(R, seed, X, std::make_integer_sequence<int, qc_rwork(L)>{});
}

// A run-time order (of a table, a pair or a shell) as a compile-time one: f(std::integral_constant<int, L>) for order == L in
// 0 .. MAXL - 1; every other order takes the instance of MAXL (the orders the callers can reach end there).  Host launchers and kernels.
template <int MAXL, int L = 0, class F>
__host__ __device__ inline void esp_dispatch(int order, F &&f) {
    if constexpr (L == MAXL) f(std::integral_constant<int, MAXL>{});
    else if (order == L) f(std::integral_constant<int, L>{});
    else esp_dispatch<MAXL, L + 1>(order, f);
}

// Records grouped by the pair order L: add() them pair by pair, then close() with the doubles a record of order L takes.  cnt[L] records,
// group L begins at record first[L] of the list and at double g.off[L]; nrec / words in all.
struct EspLayout {
    int64_t cnt[QC_LPAIR + 1] = {};
    EspGroups g{};
    int first[QC_LPAIR + 1] = {}, nrec = 0;
    size_t words = 0;
    int add(int L, int K) { const int at = (int)cnt[L]; cnt[L] += K; return at; }      // K more records of order L -> index of the first in its group
    template <class W> void close(W record_words) {
        for (int L = 0; L <= QC_LPAIR; ++L) {
            g.off[L] = (long long)words; words += (size_t)cnt[L] * record_words(L);
            first[L] = nrec; nrec += (int)cnt[L];
        }
    }
    // the stored primitive pairs of a handle, in list order: -> the first record of every stored shell pair in its group
    template <class W> std::vector<int> stored_pairs(const qc_system *S, W record_words) {
        std::vector<int> recstart(S->pairs.size());
        for (size_t i = 0; i < S->pairs.size(); ++i) recstart[i] = add(S->pairs[i].L, S->pairs[i].K);
        close(record_words);
        return recstart;
    }
};

// out[i] = ((out[i] + t_0[i]) + t_1[i]) + ..., i < words: the sums of ntiles tiles, `words` doubles each, in ascending order (qc_points.hip)
void esp_tile_sum(hipStream_t st, size_t words, int ntiles, const double *partial, double *out);

// records of order L per LDS tile (16 KB at the most); a tile is also the unit of the fixed summation order of the potential
__host__ __device__ constexpr int esp_tile(int L) { return 2048 / (4 + qc_nherm(L)); }

// hipEvents of one call's phases, destroyed on every path out
struct PhaseClock {
    hipEvent_t e[5] = {};
    double *ms;
    explicit PhaseClock(double *ms_) : ms(ms_) { for (int i = 0; i < 4; ++i) ms[i] = 0.0; }
    int create() { for (auto &x : e) if (hipEventCreate(&x) != hipSuccess) return QC_ERR_HIP; return QC_OK; }
    void mark(int i, hipStream_t st) { (void)hipEventRecord(e[i], st); }
    void add(int first, int last) {                        // (after the stream has been waited for)
        for (int i = first; i < last; ++i) { float t = 0.f; if (hipEventElapsedTime(&t, e[i], e[i + 1]) == hipSuccess) ms[i] += t; }
    }
    ~PhaseClock() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
};

// The Hermite records of a density on the device (qc_points.hip): per stored primitive pair [p, P(3), -Lambda_h ...], grouped by the pair
// order L (lay); ntiles / tile0: LDS tiles and first tile of each group.  build: enqueued on the handle's stream and waited for;
// clk: phases 0 (upload) and 1 (the kernel).
struct EspRecords {
    DevBuf rec;
    EspLayout lay;
    int ntiles[QC_LPAIR + 1], tile0[QC_LPAIR + 1], tiles_all = 0;
    int build(qc_system *S, const double *dD, PhaseClock &clk);
};
