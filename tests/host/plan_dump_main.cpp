// plan_dump_main.cpp - a stand-alone dump of the host model's pair table and of the work-list planner's classes, slots and bundles, for
// tests/test_plan_host.py and for before/after comparisons of a planner change: built from this file, qc_system.cpp and qc_plan.cpp with the
// host compiler and its address and undefined-behaviour sanitizers.  No device is initialised and no HIP function is called (the HIP
// runtime is linked for the inline hipFree of the handle's empty device buffers only).
//   plan_dump_main <in> <rank> <nranks> <synthetic schwarz: 0|1>       the A/B switches of the planner come from the environment
// <in>, little endian: int32 natoms, nshells, nprim | int32 Z[natoms], shell_atom, shell_L, shell_pure, shell_nprim [nshells each] |
//   float64 xyz[3 natoms], exponents[nprim], coefficients[nprim]        (the arguments of qc_system_create)
// Output (stdout), one record per line, lists one entry per line behind their class:
//   const   QC_LREG QC_SLOT_ITMAX QC_KET_BITS QC_LPAIR
//   sys     nbasis nelec npairs rank nranks schwarz tau
//   pair    i | the ten QcPairDesc fields | pairA pairB pairKfull | hashes of its pairdata, pairdataT, pspack bytes | synthetic pairQ
//   flags   pp_ok has_fkets merge_t1 merge_bm nquartets nscreened
//   meta    ci LAB LCD LGC bm | slot_words lds_bytes col_slot_words col_lds_bytes col_lgc bm_rows | ntasks, hash of the task list
//           (the class as qc_build_model leaves it: sizes over the whole task list, tasks in bucket order)
//   class   ci LAB LCD LGC bm | slot_words lds_bytes col_slot_words col_lds_bytes col_lgc bm_rows ket_packed |
//           prim_quartets bytes_alg flops_alg (hex floats) | qc_lgc_for of the widest ket | ntasks nshard nslots nbundles nketlist
//   t / s   ci bra ket                                  tasks / shard
//   sl      ci bra ket lo hi c0 c1                      slots
//   b       ci bra ij_lo ij_hi first nket maxK pad0 pad1
//   k       ci entry                                    ketlist
// Synthetic Schwarz factors: pairQ[i] = 10^-(i mod 15), so that the screening branch runs without the device pass the real ones come from.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qc_internal.h"

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s <in> <rank> <nranks> <schwarz 0|1>\n", argv[0]); return 2; }
    const int rank = std::atoi(argv[2]), nranks = std::atoi(argv[3]), schwarz = std::atoi(argv[4]);
    if (nranks <= 0 || rank < 0 || rank >= nranks) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<int32_t> head, Z, sa, sl, sp, sn;
    std::vector<double> xyz, ex, co;
    if (!rd(f, head, 3) || head[0] <= 0 || head[1] <= 0 || head[2] <= 0) return 3;
    const int natoms = head[0], nshells = head[1], nprim = head[2];
    if (!rd(f, Z, natoms) || !rd(f, sa, nshells) || !rd(f, sl, nshells) || !rd(f, sp, nshells) || !rd(f, sn, nshells) ||
        !rd(f, xyz, 3 * (size_t)natoms) || !rd(f, ex, nprim) || !rd(f, co, nprim)) return 3;
    std::fclose(f);

    // the handle, as qc_system_create fills it
    qc_system *S = new qc_system();
    S->natoms = natoms; S->nshells = nshells;
    S->Z.assign(Z.begin(), Z.end());
    S->xyz = xyz;
    size_t po = 0;
    for (int s = 0; s < nshells; ++s) {
        QcShell sh{};
        sh.atom = sa[s]; sh.L = sl[s]; sh.nprim = sn[s];
        sh.pure = (sp[s] && sh.L >= 2) ? 1 : 0;
        if (sh.atom < 0 || sh.atom >= natoms || sh.nprim <= 0 || sh.L < 0 || sh.L > QC_LMAX || po + sh.nprim > (size_t)nprim) { delete S; return 3; }
        sh.exps.assign(ex.begin() + po, ex.begin() + po + sh.nprim);
        sh.coefs.assign(co.begin() + po, co.begin() + po + sh.nprim);
        po += sh.nprim;
        S->shells.push_back(std::move(sh));
    }
    qc_build_model(S);
    if (!S->last_error.empty()) { std::fprintf(stderr, "%s\n", S->last_error.c_str()); delete S; return 4; }

    static char obuf[1 << 20];
    std::setvbuf(stdout, obuf, _IOFBF, sizeof(obuf));
    const int np = (int)S->pairs.size();
    static const double decade[15] = {1e-0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12, 1e-13, 1e-14};
    std::printf("const %d %d %d %d\n", QC_LREG, QC_SLOT_ITMAX, QC_KET_BITS, QC_LPAIR);
    std::printf("sys %d %d %d %d %d %d %a\n", S->nbasis, S->nelec, np, rank, nranks, schwarz, S->schwarz_tau);
    for (int i = 0; i < np; ++i) {
        const QcPairDesc &d = S->pairs[i];
        const size_t blk = (size_t)d.K * qc_pair_stride(d.L, d.na * d.nb);
        size_t ps_end = S->pspack.size();                       // the packed records of a pair end where the next packed pair's begin
        for (int j = i + 1; j < np; ++j) if (S->pairs[j].psoff >= 0) { ps_end = (size_t)S->pairs[j].psoff; break; }
        std::printf("pair %d %d %d %d %d %d %d %d %d %d %d %d %d %d %016llx %016llx %016llx %a\n", i, d.doff, d.K, d.na, d.nb, d.offa, d.offb, d.L, d.shA_eq_shB,
                    d.psoff, d.psperm, S->pairA[i], S->pairB[i], S->pairKfull[i], (unsigned long long)fnv(S->pairdata.data() + d.doff, blk * 8),
                    (unsigned long long)fnv(S->pairdataT.data() + d.doff, blk * 8),
                    (unsigned long long)(d.psoff >= 0 ? fnv(S->pspack.data() + d.psoff, (ps_end - d.psoff) * 8) : 0), decade[i % 15]);
    }
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        const QcClass &c = S->classes[ci];
        std::printf("meta %zu %d %d %d %d %d %d %d %d %d %d %zu %016llx\n", ci, c.LAB, c.LCD, c.LGC, (int)c.bm, c.slot_words, c.lds_bytes, c.col_slot_words,
                    c.col_lds_bytes, c.col_lgc, c.bm_rows, c.tasks.size(), (unsigned long long)fnv(c.tasks.data(), c.tasks.size() * sizeof(QcTask)));
    }

    S->rank = rank; S->nranks = nranks;
    if (schwarz) { S->pairQ.resize(np); for (int i = 0; i < np; ++i) S->pairQ[i] = decade[i % 15]; }
    qc_build_shards(S);
    std::printf("flags %d %d %d %d %lld %lld\n", (int)S->pp_ok, (int)S->has_fkets, (int)S->merge_t1, (int)S->merge_bm, (long long)S->nquartets, (long long)S->nscreened);
    for (size_t ci = 0; ci < S->classes.size(); ++ci) {
        const QcClass &c = S->classes[ci];
        int widest = 0;
        for (const auto &t : c.tasks) widest = std::max(widest, S->pairs[t.ket].na * S->pairs[t.ket].nb);
        std::printf("class %zu %d %d %d %d %d %d %d %d %d %d %d %lld %a %a %d %zu %zu %zu %zu %zu\n", ci, c.LAB, c.LCD, c.LGC, (int)c.bm, c.slot_words, c.lds_bytes,
                    c.col_slot_words, c.col_lds_bytes, c.col_lgc, c.bm_rows, (int)c.ket_packed, (long long)c.prim_quartets, c.bytes_alg, c.flops_alg,
                    qc_lgc_for(c.LAB, c.LCD, widest), c.tasks.size(), c.shard.size(), c.slots.size(), c.bundles.size(), c.ketlist.size());
        for (const auto &t : c.tasks) std::printf("t %zu %d %d\n", ci, t.bra, t.ket);
        for (const auto &t : c.shard) std::printf("s %zu %d %d\n", ci, t.bra, t.ket);
        for (const auto &s : c.slots) std::printf("sl %zu %d %d %d %d %d %d\n", ci, s.bra, s.ket, s.lo, s.hi, s.c0, s.c1);
        for (const auto &b : c.bundles) std::printf("b %zu %d %d %d %d %d %d %d %d\n", ci, b.bra, b.ij_lo, b.ij_hi, b.first, b.nket, b.maxK, b.pad0, b.pad1);
        for (int e : c.ketlist) std::printf("k %zu %d\n", ci, e);
    }
    std::fflush(stdout);
    const bool bad = std::ferror(stdout) != 0;
    delete S;
    return bad ? 5 : 0;
}
