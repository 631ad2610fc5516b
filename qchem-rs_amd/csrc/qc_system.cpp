// qc_system.cpp - host model of a molecule + basis for the MI355X Hartree-Fock path.
//
// Replaces what the reference receives as `&MolecularSystem` from molint (main.rs:76-77; members read at
// rhf.rs:36-37) and precomputes, once per geometry, everything the HIP kernels stream: normalised shells, the
// shell-pair list with per-primitive-pair Hermite expansion matrices (spherical transform, contraction coefficients
// and the pair part of the ERI prefactor folded in); the class-sorted unique-quartet task lists and their
// per-rank shards are made from it by the planner (qc_plan.cpp).  Also holds the host implementation of molint::overlap/kinetic/nuclear (rhf.rs:41-43), which
// SURVEY.md 8f ranks as "next" for the GPU.  Integral formulas: McMurchie-Davidson.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include <cstdlib>

#include "qc_embed.h"
#include "qc_md.h"

namespace {

double dfact(int n) { double r = 1.0; for (; n > 1; n -= 2) r *= n; return r; }
double binom(int n, int k) { if (k < 0 || k > n) return 0.0; double r = 1.0; for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i; return r; }

// real solid harmonic S_lm in Cartesian monomials, Helgaker-Jorgensen-Olsen eq. 6.4.47 (scale fixed afterwards)
std::vector<double> solid_row(int l, int m) {
    std::vector<double> row(qc_ncart(l), 0.0);
    const int am = std::abs(m), neg = m < 0 ? 1 : 0;
    for (int t = 0; 2 * t <= l - am; ++t)
        for (int u = 0; u <= t; ++u)
            for (int k = 0; 2 * k + neg <= am; ++k) {          // 2v = 2k + neg
                const int tv = 2 * k + neg;
                double c = ((t + k) & 1 ? -1.0 : 1.0) * std::pow(0.25, t) * binom(l, t) * binom(l - t, am + t) * binom(t, u) * binom(am, tv);
                const int ex = 2 * t + am - 2 * u - tv, ey = 2 * u + tv, ez = l - 2 * t - am;
                if (ex < 0) continue;
                for (int i = 0; i < qc_ncart(l); ++i) {
                    const unsigned char *ci = qc_md_cart(l, i);
                    if (ci[0] == ex && ci[1] == ey && ci[2] == ez) row[i] += c;
                }
            }
    return row;
}

double mono_overlap_1d(int n, double p) { return (n & 1) ? 0.0 : dfact(n - 1) / std::pow(2.0 * p, n / 2) * std::sqrt(M_PI / p); }

// one axis' expansion table, i <= la, j <= lb + 2 (kinetic energy)
using E1 = QcMdE1<(QC_LMAX + 1) * (QC_LMAX + 3) * (2 * QC_LMAX + 3)>;

// Hermite Coulomb integrals R^0_tuv, t+u+v <= L (host, for the nuclear-attraction matrix)
void hermite_r_host(int L, double alpha, const double PC[3], std::vector<double> &R0) {
    std::vector<std::vector<double>> W(L + 1, std::vector<double>(qc_nherm(L), 0.0));
    std::vector<double> F(L + 1);
    qc_md_boys(L, alpha * (PC[0] * PC[0] + PC[1] * PC[1] + PC[2] * PC[2]), F.data());
    double f = 1.0;
    for (int n = 0; n <= L; ++n) { W[n][0] = f * F[n]; f *= -2.0 * alpha; }      // (the seeds: a running product here, see qc_md.h)
    for (int N = 1; N <= L; ++N)
        for (int n = 0; n + N <= L; ++n)
            for (int t = N; t >= 0; --t)
                for (int u = N - t; u >= 0; --u) W[n][qc_hidx(t, u, N - t - u)] = qc_md_r_step(W[n + 1].data(), t, u, N - t - u, PC);
    R0 = W[0];
}

}  // namespace

void qc_boys_host(int nmax, double x, double *F) { qc_md_boys(nmax, x, F); }

static void normalise_shell(QcShell &sh) {
    const int L = sh.L;
    sh.ncart = qc_ncart(L);
    sh.nfunc = sh.pure ? 2 * L + 1 : sh.ncart;
    for (int i = 0; i < sh.nprim; ++i) {
        const double a = sh.exps[i];
        sh.coefs[i] *= std::pow(2.0 * a / M_PI, 0.75) * std::pow(4.0 * a, 0.5 * L) / std::sqrt(dfact(2 * L - 1));
    }
    sh.T.assign((size_t)sh.nfunc * sh.ncart, 0.0);
    if (sh.pure) {
        for (int m = -L; m <= L; ++m) { auto r = solid_row(L, m); std::copy(r.begin(), r.end(), sh.T.begin() + (size_t)(m + L) * sh.ncart); }
    } else {
        for (int c = 0; c < sh.ncart; ++c) sh.T[(size_t)c * sh.ncart + c] = 1.0;
    }
    // contracted self-overlap of the monomials, then scale each function to unit norm
    std::vector<double> M((size_t)sh.ncart * sh.ncart, 0.0);
    for (int c1 = 0; c1 < sh.ncart; ++c1)
        for (int c2 = 0; c2 < sh.ncart; ++c2) {
            const unsigned char *l1 = qc_md_cart(L, c1), *l2 = qc_md_cart(L, c2);
            double s = 0.0;
            for (int i = 0; i < sh.nprim; ++i)
                for (int j = 0; j < sh.nprim; ++j) {
                    const double p = sh.exps[i] + sh.exps[j];
                    s += sh.coefs[i] * sh.coefs[j] * mono_overlap_1d(l1[0] + l2[0], p) * mono_overlap_1d(l1[1] + l2[1], p) * mono_overlap_1d(l1[2] + l2[2], p);
                }
            M[(size_t)c1 * sh.ncart + c2] = s;
        }
    for (int f = 0; f < sh.nfunc; ++f) {
        double *row = &sh.T[(size_t)f * sh.ncart];
        double s2 = 0.0;
        for (int c1 = 0; c1 < sh.ncart; ++c1) for (int c2 = 0; c2 < sh.ncart; ++c2) s2 += row[c1] * row[c2] * M[(size_t)c1 * sh.ncart + c2];
        const double sc = 1.0 / std::sqrt(s2);
        for (int c = 0; c < sh.ncart; ++c) row[c] *= sc;
    }
}

// Hermite expansion matrix of one primitive pair in basis functions: out[h * nab + (fa*nb+fb)], h < nherm(la+lb).
static void pair_hermite_matrix(const QcShell &A, const QcShell &B, int i, int j, double scale, double *out, double *p_out, double P[3]) {
    const int la = A.L, lb = B.L, nh = qc_nherm(la + lb), nab = A.nfunc * B.nfunc;
    const double a = A.exps[i], b = B.exps[j], p = a + b;
    for (int k = 0; k < 3; ++k) P[k] = (a * A.A[k] + b * B.A[k]) / p;
    *p_out = p;
    E1 E[3];
    for (int k = 0; k < 3; ++k) E[k].fill(la, lb, a, b, A.A[k] - B.A[k]);
    const size_t nca = A.ncart, ncb = B.ncart;
    const double cc = A.coefs[i] * B.coefs[j] * scale;
    std::vector<double> Ec(nca * ncb * nh, 0.0);
    for (size_t x = 0; x < nca; ++x)
        for (size_t y = 0; y < ncb; ++y) {
            const unsigned char *ca = qc_md_cart(la, (int)x), *cb = qc_md_cart(lb, (int)y);
            double *row = &Ec[(x * ncb + y) * nh];
            for (int t = 0; t <= ca[0] + cb[0]; ++t)
                for (int u = 0; u <= ca[1] + cb[1]; ++u)
                    for (int v = 0; v <= ca[2] + cb[2]; ++v)
                        row[qc_hidx(t, u, v)] = cc * E[0].g(ca[0], cb[0], t) * E[1].g(ca[1], cb[1], u) * E[2].g(ca[2], cb[2], v);
        }
    std::fill(out, out + (size_t)nh * nab, 0.0);
    for (int fa = 0; fa < A.nfunc; ++fa)
        for (size_t x = 0; x < nca; ++x) {
            const double ta = A.T[(size_t)fa * A.ncart + x];
            if (ta == 0.0) continue;
            for (int fb = 0; fb < B.nfunc; ++fb)
                for (size_t y = 0; y < ncb; ++y) {
                    const double tb = ta * B.T[(size_t)fb * B.ncart + y];
                    if (tb == 0.0) continue;
                    const double *row = &Ec[(x * ncb + y) * nh];
                    for (int h = 0; h < nh; ++h) out[(size_t)h * nab + fa * B.nfunc + fb] += tb * row[h];
                }
        }
}

// pp pairs: basis function of Cartesian axis x of a p shell: (perm >> 2x) & 3; false: the shell's functions are not the three axes
static bool p_axis_perm(const QcShell &sh, int &perm) {
    bool ok = sh.nfunc == 3 && sh.ncart == 3;
    perm = 0;
    int seen = 0;
    for (int ax = 0; ax < 3 && ok; ++ax) {
        int f = 0;
        for (int g = 1; g < 3; ++g) if (std::fabs(sh.T[(size_t)g * 3 + ax]) > std::fabs(sh.T[(size_t)f * 3 + ax])) f = g;
        for (int g = 0; g < 3; ++g) if (g != f && sh.T[(size_t)g * 3 + ax] != 0.0) ok = false;
        perm |= f << (2 * ax); seen |= 1 << f;
    }
    return ok && seen == 7;
}

// Packed record of a p.s primitive pair from its block blk = [p, P(3), E(4 x 3)], 8 doubles: [p, P | E_0[x, y, z], E_1].
// The 4 x 3 expansion block of a p.s product has 4 distinct numbers: row 0 (the s-type Hermite
// function) is dense, rows 1..3 are one value on a permutation (which p function is which axis).
// perm: that permutation; returns whether the block has this form.
static bool ps_packed_record(const double *blk, double rec[8], int &perm) {
    const double *E = blk + 4;             // E[h * 3 + col]
    perm = 0;
    double e1 = 0.0, e0[3] = {0, 0, 0};
    bool ok = true;
    for (int ax = 0; ax < 3; ++ax) {
        int col = 0;
        for (int c2 = 1; c2 < 3; ++c2) if (std::fabs(E[(1 + ax) * 3 + c2]) > std::fabs(E[(1 + ax) * 3 + col])) col = c2;
        for (int c2 = 0; c2 < 3; ++c2) if (c2 != col && std::fabs(E[(1 + ax) * 3 + c2]) > 1e-14 * std::fabs(E[(1 + ax) * 3 + col])) ok = false;
        if (ax == 0) e1 = E[3 + col];
        else if (std::fabs(E[(1 + ax) * 3 + col] - e1) > 1e-13 * std::fabs(e1)) ok = false;
        perm |= col << (2 * ax);
        e0[ax] = E[col];
    }
    if (((perm & 3) == ((perm >> 2) & 3)) || ((perm & 3) == ((perm >> 4) & 3)) || (((perm >> 2) & 3) == ((perm >> 4) & 3))) ok = false;
    const double r[8] = {blk[0], blk[1], blk[2], blk[3], e0[0], e0[1], e0[2], e1};
    std::copy(r, r + 8, rec);
    return ok;
}

// Packed record of a p.p primitive pair (ket side of qc_fock_bm_kernel<2, 0>) from its block blk = [p, P(3), E(10 x 9)], 16 doubles:
//   [q, Q | A_x, A_y, A_z, kh | D_x, D_y, D_z, khh | hA_x, hA_y, hA_z, 0],  A = K (Q - C), D = Q - D', hq = 1/(2q), kh = K hq,
//   khh = K hq^2, hA = hq A:  the expansion of the function pair (axis c of the first shell, axis d of the second) is
//   E_000 = A_c D_d + [c = d] kh,  E_{e_c} = kh D_d,  E_{e_d} = hA_c,  E_{e_c + e_d} = khh - everything else is zero.
// K is read off the block (second-order coefficient of the x.x pair), and the whole block is checked against the form: the return value.
static bool pp_packed_record(const double *blk, int nab, const QcShell &A, const QcShell &B, int ppermA, int ppermB, double rec[16]) {
    const double p = blk[0], *P = blk + 1;
    const double hq = 0.5 / p;
    const double PC[3] = {P[0] - A.A[0], P[1] - A.A[1], P[2] - A.A[2]}, PD[3] = {P[0] - B.A[0], P[1] - B.A[1], P[2] - B.A[2]};
    auto fn = [&](int perm, int ax) { return (perm >> (2 * ax)) & 3; };
    auto Eb = [&](int t, int u, int v, int c, int dd) { return blk[4 + (size_t)qc_hidx(t, u, v) * nab + fn(ppermA, c) * 3 + fn(ppermB, dd)]; };
    const double Kc = Eb(2, 0, 0, 0, 0) / (hq * hq);
    const double kh = Kc * hq, khh = Kc * hq * hq;
    double worst = 0.0, scale_e = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int dd = 0; dd < 3; ++dd)
            for (int t = 0; t <= 2; ++t)
                for (int u = 0; t + u <= 2; ++u)
                    for (int v = 0; t + u + v <= 2; ++v) {
                        const int tv[3] = {t, u, v};
                        int ec[3] = {0, 0, 0}, ed[3] = {0, 0, 0}, ecd[3] = {0, 0, 0};
                        ec[c] = 1; ed[dd] = 1; ecd[c] += 1; ecd[dd] += 1;
                        auto is = [&](const int *e) { return tv[0] == e[0] && tv[1] == e[1] && tv[2] == e[2]; };
                        double want = 0.0;
                        if (t + u + v == 0) want = Kc * PC[c] * PD[dd] + (c == dd ? kh : 0.0);
                        else if (t + u + v == 1) want = (is(ec) ? kh * PD[dd] : 0.0) + (is(ed) ? kh * PC[c] : 0.0);
                        else if (is(ecd)) want = khh;
                        worst = std::max(worst, std::fabs(want - Eb(t, u, v, c, dd)));
                        scale_e = std::max(scale_e, std::fabs(want));
                    }
    const double r[16] = {p, P[0], P[1], P[2], Kc * PC[0], Kc * PC[1], Kc * PC[2], kh, PD[0], PD[1], PD[2], khh,
                          hq * Kc * PC[0], hq * Kc * PC[1], hq * Kc * PC[2], 0.0};
    std::copy(r, r + 16, rec);
    return worst <= 1e-12 * std::max(scale_e, 1e-300);
}

// a primitive pair below QC_PRIM_CUTOFF still stays if it reaches this fraction of the largest block of its shell pair (qc_build_model)
static constexpr double QC_PRIM_REL = 1e-13;

void qc_build_model(qc_system *S) {
    static const bool sdbg = getenv("QC_SETUP_DEBUG") != nullptr;
    QcLap lap{"model", sdbg};
    S->plan = QcPlanSwitches::from_env();
    int off = 0;
    for (auto &sh : S->shells) {
        for (int k = 0; k < 3; ++k) sh.A[k] = S->xyz[3 * sh.atom + k];
        normalise_shell(sh);
        sh.off = off;
        off += sh.nfunc;
    }
    S->nbasis = off;
    S->nelec = std::accumulate(S->Z.begin(), S->Z.end(), 0);
    // shell pairs A >= B, with per-primitive-pair blocks [p, Px, Py, Pz, E(nherm x nab)].
    // The pair part of the ERI prefactor 2 pi^{5/2} / (p q sqrt(p+q)) is folded in as sqrt(2) pi^{5/4} / p.
    const double half_pref = std::sqrt(2.0) * std::pow(M_PI, 1.25);
    S->pairs.clear(); S->pairA.clear(); S->pairB.clear(); S->pairKfull.clear(); S->pairdata.clear(); S->pairdataT.clear(); S->pspack.clear();
    S->pp_ok = true;
    // Primitive pairs whose whole expansion block is below QC_PRIM_CUTOFF are not stored: with the Gaussian-product
    // factor exp(-mu R^2) and the coefficients folded into E, an integral is bounded by max|E_ab| max|E_cd| (times
    // O(10)), so a dropped primitive pair changes no integral by more than ~1e-16 - five orders below the 1e-10 parity
    // bar - while two-centre pairs of deeply contracted s/p shells lose a third to two thirds of their primitives.
    // (The reference evaluates them all; counts quoted as "enumerated" keep the full numbers.)
    // A WEAK pair - largest block below 1e-4, shells far apart - keeps every primitive pair down to QC_PRIM_REL times its largest
    // block: the absolute cut-off alone left such a pair's integrals, and its Schwarz factor sqrt(max (ab|ab)), with a RELATIVE
    // error of up to 1e-17 / (largest block) - 1e-9 for a factor of 8e-10 - and factors are compared with thresholds over thirty
    // orders of magnitude.  For every pair with a block of 1e-4 or more the rule drops what it dropped before; a pair whose
    // largest block is itself below QC_PRIM_CUTOFF is not stored, as before.
    int64_t npairs_all = 0;
    std::vector<double> blkbuf, allblk, blkmax;
    for (int a = 0; a < S->nshells; ++a)
        for (int b = 0; b <= a; ++b) {
            const QcShell &A = S->shells[a], &B = S->shells[b];
            ++npairs_all;
            QcPairDesc d;
            d.doff = (int)S->pairdata.size();
            d.K = 0;
            d.na = A.nfunc; d.nb = B.nfunc; d.offa = A.off; d.offb = B.off; d.L = A.L + B.L; d.shA_eq_shB = (a == b);
            d.psoff = -1; d.psperm = 0;
            const bool is_ps = (d.L == 1);
            const bool is_pp = (A.L == 1 && B.L == 1);
            if (is_ps || is_pp) d.psoff = (int)S->pspack.size();
            int ppermA = 0, ppermB = 0;
            if (is_pp) {
                if (!p_axis_perm(A, ppermA) || !p_axis_perm(B, ppermB)) S->pp_ok = false;
                d.psperm = ppermA | (ppermB << 6);
            }
            const int nab = d.na * d.nb, stride = qc_pair_stride(d.L, nab), ne = qc_nherm(d.L) * nab;
            // every primitive pair's block first (the cut-off of a weak pair follows the pair's largest block), then the ones that stay
            const int nij = A.nprim * B.nprim;
            allblk.assign((size_t)nij * stride, 0.0); blkmax.assign(nij, 0.0);
            double pairmax = 0.0;
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    double p, P[3];
                    const double pp = A.exps[i] + B.exps[j];
                    double *blk = allblk.data() + (size_t)(i * B.nprim + j) * stride;
                    pair_hermite_matrix(A, B, i, j, half_pref / pp, blk + 4, &p, P);
                    double mx = 0.0;
                    for (int k = 0; k < ne; ++k) mx = std::max(mx, std::fabs(blk[4 + k]));
                    blk[0] = p; blk[1] = P[0]; blk[2] = P[1]; blk[3] = P[2];
                    blkmax[i * B.nprim + j] = mx; pairmax = std::max(pairmax, mx);
                }
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    const double mx = blkmax[i * B.nprim + j];
                    if (mx < QC_PRIM_CUTOFF && (pairmax < QC_PRIM_CUTOFF || mx < QC_PRIM_REL * pairmax)) continue;
                    blkbuf.assign(allblk.begin() + (size_t)(i * B.nprim + j) * stride, allblk.begin() + (size_t)(i * B.nprim + j + 1) * stride);
                    S->pairdata.insert(S->pairdata.end(), blkbuf.begin(), blkbuf.end());
                    const int nh = qc_nherm(d.L);
                    if (is_ps) {
                        double rec[8];
                        int perm;
                        const bool ok = ps_packed_record(blkbuf.data(), rec, perm) && !(d.K > 0 && perm != d.psperm);
                        if (!ok) S->last_error = "p shell whose functions are not the Cartesian axes (in some order)";
                        d.psperm = perm;
                        S->pspack.insert(S->pspack.end(), rec, rec + 8);
                    }
                    if (is_pp && S->pp_ok) {
                        double rec[16];
                        if (!pp_packed_record(blkbuf.data(), nab, A, B, ppermA, ppermB, rec)) S->pp_ok = false;
                        S->pspack.insert(S->pspack.end(), rec, rec + 16);
                    }
                    const size_t t0 = S->pairdataT.size();
                    S->pairdataT.insert(S->pairdataT.end(), blkbuf.begin(), blkbuf.end());
                    for (int h = 0; h < nh; ++h)
                        for (int ab = 0; ab < nab; ++ab) S->pairdataT[t0 + 4 + (size_t)ab * nh + h] = blkbuf[4 + (size_t)h * nab + ab];
                    ++d.K;
                }
            if (d.K == 0) continue;                       // the whole shell pair is negligible
            S->pairs.push_back(d); S->pairA.push_back(a); S->pairB.push_back(b); S->pairKfull.push_back(A.nprim * B.nprim);
        }
    lap("shell pairs");
    S->nquartets = npairs_all * (npairs_all + 1) / 2;      // enumerated (unscreened) count, as the reference would visit
    qc_build_classes(S, lap);
    // (the lists themselves wait for the Schwarz factors of the device set-up - or for whoever asks first, qc_ensure_lists: building them
    // here as well was 1.6 ms of a 13.7 ms cold SCF of H2O/cc-pVTZ, 60 ms for benzene/cc-pVDZ)
    qc_build_shards(S, true);
    lap("class sizes");
}

// ---- one-electron matrices on the host (molint::overlap / kinetic / nuclear, rhf.rs:41-43); which: 0 S, 1 T, 2 V
void qc_host_one_electron(const qc_system *S, int which, double *out) {
    const int n = S->nbasis;
    std::fill(out, out + (size_t)n * n, 0.0);
    std::vector<double> R0;
    for (int a = 0; a < S->nshells; ++a)
        for (int b = 0; b <= a; ++b) {
            const QcShell &A = S->shells[a], &B = S->shells[b];
            const size_t nca = A.ncart, ncb = B.ncart;
            std::vector<double> cart(nca * ncb, 0.0);
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    const double ea = A.exps[i], eb = B.exps[j], p = ea + eb, cc = A.coefs[i] * B.coefs[j];
                    double P[3];
                    for (int k = 0; k < 3; ++k) P[k] = (ea * A.A[k] + eb * B.A[k]) / p;
                    E1 E[3];
                    for (int k = 0; k < 3; ++k) E[k].fill(A.L, B.L + 2, ea, eb, A.A[k] - B.A[k]);
                    const double s3 = std::pow(M_PI / p, 1.5);
                    for (size_t x = 0; x < nca; ++x)
                        for (size_t y = 0; y < ncb; ++y) {
                            const unsigned char *ca = qc_md_cart(A.L, (int)x), *cb = qc_md_cart(B.L, (int)y);
                            const int ai[3] = {ca[0], ca[1], ca[2]}, bi[3] = {cb[0], cb[1], cb[2]};
                            double val = 0.0;
                            if (which == 0) {
                                val = qc_md_ovl(E, ai, bi, s3);
                            } else if (which == 1) {
                                val = -0.5 * s3 * qc_md_kin(E, ai, bi, eb);
                            } else {
                                for (int c = 0; c < S->natoms; ++c) {
                                    const double PC[3] = {P[0] - S->xyz[3 * c], P[1] - S->xyz[3 * c + 1], P[2] - S->xyz[3 * c + 2]};
                                    hermite_r_host(A.L + B.L, p, PC, R0);
                                    val -= S->Z[c] * 2.0 * M_PI / p * qc_md_nuc(E, ai, bi, R0.data());
                                }
                            }
                            cart[x * ncb + y] += cc * val;
                        }
                }
            for (int fa = 0; fa < A.nfunc; ++fa)
                for (int fb = 0; fb < B.nfunc; ++fb) {
                    double v = 0.0;
                    for (size_t x = 0; x < nca; ++x)
                        for (size_t y = 0; y < ncb; ++y) v += A.T[(size_t)fa * A.ncart + x] * B.T[(size_t)fb * B.ncart + y] * cart[x * ncb + y];
                    out[(size_t)(A.off + fa) * n + B.off + fb] = v;
                    out[(size_t)(B.off + fb) * n + A.off + fa] = v;
                }
        }
}

// ---- dipole matrices on the host: out[k * n * n + ..] = <a| (r - O)_k |b>, k = x, y, z; normalisation and transform T as for the overlap
void qc_host_dipole(const qc_system *S, const double *origin, double *out) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    std::fill(out, out + 3 * nn, 0.0);
    for (int a = 0; a < S->nshells; ++a)
        for (int b = 0; b <= a; ++b) {
            const QcShell &A = S->shells[a], &B = S->shells[b];
            const size_t nca = A.ncart, ncb = B.ncart;
            std::vector<double> cart(3 * nca * ncb, 0.0);
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    const double ea = A.exps[i], eb = B.exps[j], p = ea + eb, cc = A.coefs[i] * B.coefs[j];
                    double PO[3];
                    for (int k = 0; k < 3; ++k) PO[k] = (ea * A.A[k] + eb * B.A[k]) / p - origin[k];
                    E1 E[3];
                    for (int k = 0; k < 3; ++k) E[k].fill(A.L, B.L, ea, eb, A.A[k] - B.A[k]);
                    const double s3 = std::pow(M_PI / p, 1.5);
                    for (size_t x = 0; x < nca; ++x)
                        for (size_t y = 0; y < ncb; ++y) {
                            const unsigned char *ca = qc_md_cart(A.L, (int)x), *cb = qc_md_cart(B.L, (int)y);
                            const int ai[3] = {ca[0], ca[1], ca[2]}, bi[3] = {cb[0], cb[1], cb[2]};
                            for (int k = 0; k < 3; ++k) cart[(k * nca + x) * ncb + y] += cc * qc_md_dip(E, ai, bi, k, PO[k], s3);
                        }
                }
            for (int k = 0; k < 3; ++k)
                for (int fa = 0; fa < A.nfunc; ++fa)
                    for (int fb = 0; fb < B.nfunc; ++fb) {
                        if (a == b && fb > fa) continue;               // diagonal blocks: one triangle, mirrored (exactly symmetric output)
                        double v = 0.0;
                        for (size_t x = 0; x < nca; ++x)
                            for (size_t y = 0; y < ncb; ++y) v += A.T[(size_t)fa * A.ncart + x] * B.T[(size_t)fb * B.ncart + y] * cart[(k * nca + x) * ncb + y];
                        out[k * nn + (size_t)(A.off + fa) * n + B.off + fb] = v;
                        out[k * nn + (size_t)(B.off + fb) * n + A.off + fa] = v;
                    }
        }
}

// ---- Cartesian multipole matrices on the host: out[c * n * n + ..] = <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b> for the qc_nherm(order)
// components c of qc_md_mom_comp; normalisation and transform T as for the overlap.  Per primitive pair the Hermite moments of the three
// axes (qc_md_mom_herm), per Cartesian pair the 1-D factors of every power (qc_md_mom_1d), per component their product.
void qc_host_multipole(const qc_system *S, int order, const double *origin, double *out) {
    constexpr int W = QC_MOM_MAX + 1;
    const int n = S->nbasis, count = qc_nherm(order);
    const size_t nn = (size_t)n * n;
    std::fill(out, out + count * nn, 0.0);
    for (int a = 0; a < S->nshells; ++a)
        for (int b = 0; b <= a; ++b) {
            const QcShell &A = S->shells[a], &B = S->shells[b];
            const size_t nca = A.ncart, ncb = B.ncart;
            std::vector<double> cart(count * nca * ncb, 0.0);
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    const double ea = A.exps[i], eb = B.exps[j], p = ea + eb, cc = A.coefs[i] * B.coefs[j];
                    E1 E[3];
                    double M[3][W * W];
                    for (int k = 0; k < 3; ++k) {
                        E[k].fill(A.L, B.L, ea, eb, A.A[k] - B.A[k]);
                        qc_md_mom_herm(order, (ea * A.A[k] + eb * B.A[k]) / p - origin[k], p, M[k]);
                    }
                    const double s3 = std::pow(M_PI / p, 1.5);
                    for (size_t x = 0; x < nca; ++x)
                        for (size_t y = 0; y < ncb; ++y) {
                            const unsigned char *ca = qc_md_cart(A.L, (int)x), *cb = qc_md_cart(B.L, (int)y);
                            double F[3][W];
                            for (int k = 0; k < 3; ++k) qc_md_mom_1d(E[k], ca[k], cb[k], order, M[k], F[k]);
                            for (int c = 0; c < count; ++c) {
                                const unsigned char *m = qc_md_mom_comp(c);
                                cart[(c * nca + x) * ncb + y] += cc * (s3 * F[0][m[0]] * F[1][m[1]] * F[2][m[2]]);
                            }
                        }
                }
            for (int c = 0; c < count; ++c)
                for (int fa = 0; fa < A.nfunc; ++fa)
                    for (int fb = 0; fb < B.nfunc; ++fb) {
                        if (a == b && fb > fa) continue;               // diagonal blocks: one triangle, mirrored (exactly symmetric output)
                        double v = 0.0;
                        for (size_t x = 0; x < nca; ++x)
                            for (size_t y = 0; y < ncb; ++y) v += A.T[(size_t)fa * A.ncart + x] * B.T[(size_t)fb * B.ncart + y] * cart[(c * nca + x) * ncb + y];
                        out[c * nn + (size_t)(A.off + fa) * n + B.off + fb] = v;
                        out[c * nn + (size_t)(B.off + fb) * n + A.off + fa] = v;
                    }
        }
}

// ---- basis functions on points, on the host: out[k * n + a] = phi_a(r_k).  Per shell the contracted radial part, the Cartesian
// monomials as running products (x^0 = 1 at a point on the centre), the rows of the shell's transform - normalisation as for the overlap.
void qc_host_basis_on_points(const qc_system *S, int64_t npts, const double *xyz, double *out) {
    const int n = S->nbasis;
    for (int64_t k = 0; k < npts; ++k)
        for (const QcShell &A : S->shells) {
            const double d[3] = {xyz[3 * k] - A.A[0], xyz[3 * k + 1] - A.A[1], xyz[3 * k + 2] - A.A[2]};
            const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            double radial = 0.0;
            for (int i = 0; i < A.nprim; ++i) radial += A.coefs[i] * std::exp(-A.exps[i] * r2);
            double pw[3][QC_LMAX + 1];
            for (int q = 0; q < 3; ++q) { pw[q][0] = 1.0; for (int i = 1; i <= A.L; ++i) pw[q][i] = pw[q][i - 1] * d[q]; }
            double mono[qc_ncart(QC_LMAX)];
            for (int x = 0; x < A.ncart; ++x) {
                const unsigned char *c = qc_md_cart(A.L, x);
                mono[x] = pw[0][c[0]] * pw[1][c[1]] * pw[2][c[2]] * radial;
            }
            for (int f = 0; f < A.nfunc; ++f) {
                double v = 0.0;
                for (int x = 0; x < A.ncart; ++x) v += A.T[(size_t)f * A.ncart + x] * mono[x];
                out[(size_t)k * n + A.off + f] = v;
            }
        }
}

// ---- matrices of Coulomb operators in the basis, one skeleton: NM matrices out[m] (n x n each) at once, element ab of matrix m
//   sign sum_prim c_a c_b 2 pi / p sum_tuv E^ab_tuv R^m_tuv,
// the nuclear-attraction sum of qc_host_one_electron with the tables R^m (order la + lb, indexed by qc_hidx) that `tables(L, p, P, R)` fills
// for the primitive pair of exponent p at P.  Per shell pair a >= b: the Cartesian block over the primitive pairs in list order, then the
// Cartesian -> pure transform; exactly symmetric (diagonal blocks: one triangle, mirrored).
template <int NM, class Tables>
static void host_coulomb_matrices(const qc_system *S, double sign, double *out, Tables tables) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    std::fill(out, out + NM * nn, 0.0);
    std::vector<double> R[NM];
    for (int a = 0; a < S->nshells; ++a)
        for (int b = 0; b <= a; ++b) {
            const QcShell &A = S->shells[a], &B = S->shells[b];
            const size_t nca = A.ncart, ncb = B.ncart;
            std::vector<double> cart(NM * nca * ncb, 0.0);
            for (int i = 0; i < A.nprim; ++i)
                for (int j = 0; j < B.nprim; ++j) {
                    const double ea = A.exps[i], eb = B.exps[j], p = ea + eb, cc = A.coefs[i] * B.coefs[j];
                    double P[3];
                    for (int k = 0; k < 3; ++k) P[k] = (ea * A.A[k] + eb * B.A[k]) / p;
                    E1 E[3];
                    for (int k = 0; k < 3; ++k) E[k].fill(A.L, B.L, ea, eb, A.A[k] - B.A[k]);
                    tables(A.L + B.L, p, P, R);
                    for (size_t x = 0; x < nca; ++x)
                        for (size_t y = 0; y < ncb; ++y) {
                            const unsigned char *ca = qc_md_cart(A.L, (int)x), *cb = qc_md_cart(B.L, (int)y);
                            const int ai[3] = {ca[0], ca[1], ca[2]}, bi[3] = {cb[0], cb[1], cb[2]};
                            for (int m = 0; m < NM; ++m) cart[(m * nca + x) * ncb + y] += sign * (cc * (2.0 * M_PI / p * qc_md_nuc(E, ai, bi, R[m].data())));
                        }
                }
            for (int m = 0; m < NM; ++m)
                for (int fa = 0; fa < A.nfunc; ++fa)
                    for (int fb = 0; fb < B.nfunc; ++fb) {
                        if (a == b && fb > fa) continue;
                        double v = 0.0;
                        for (size_t x = 0; x < nca; ++x)
                            for (size_t y = 0; y < ncb; ++y) v += A.T[(size_t)fa * A.ncart + x] * B.T[(size_t)fb * B.ncart + y] * cart[(m * nca + x) * ncb + y];
                        out[m * nn + (size_t)(A.off + fa) * n + B.off + fb] = v;
                        out[m * nn + (size_t)(B.off + fb) * n + A.off + fa] = v;
                    }
        }
}

// the potential of a unit point charge at r in the basis: out_ab = (a| 1/|r' - r| |b), positive - one centre without its -Z
void qc_host_potential_matrix(const qc_system *S, const double *r, double *out) {
    host_coulomb_matrices<1>(S, 1.0, out, [r](int L, double p, const double *P, std::vector<double> *R) {
        const double PC[3] = {P[0] - r[0], P[1] - r[1], P[2] - r[2]};
        hermite_r_host(L, p, PC, R[0]);
    });
}

// ---- point-charge embedding on the host (qc_embed.h): the reference statements of what qc_embed.hip computes
// E_nq = sum_A sum_c Z_A q_c / |R_A - R_c|, atoms outside, charges in list order
double qc_pc_nuclear_energy(const qc_system *S, const std::vector<double> &pc) {
    double e = 0.0;
    for (int a = 0; a < S->natoms; ++a)
        for (size_t c = 0; c < pc.size() / 4; ++c) {
            const double dx = S->xyz[3 * a] - pc[4 * c], dy = S->xyz[3 * a + 1] - pc[4 * c + 1], dz = S->xyz[3 * a + 2] - pc[4 * c + 2];
            e += (double)S->Z[a] * pc[4 * c + 3] / std::sqrt(dx * dx + dy * dy + dz * dz);
        }
    return e;
}

void qc_pc_nuclear_gradient(const qc_system *S, const std::vector<double> &pc, double *ga, double *gc) {
    const size_t npc = pc.size() / 4;
    if (ga) std::fill(ga, ga + 3 * S->natoms, 0.0);
    if (gc) std::fill(gc, gc + 3 * npc, 0.0);
    for (int a = 0; a < S->natoms; ++a)
        for (size_t c = 0; c < npc; ++c) {
            double d[3], r2 = 0.0;
            for (int k = 0; k < 3; ++k) { d[k] = S->xyz[3 * a + k] - pc[4 * c + k]; r2 += d[k] * d[k]; }
            const double f = -(double)S->Z[a] * pc[4 * c + 3] / (r2 * std::sqrt(r2));
            for (int k = 0; k < 3; ++k) { if (ga) ga[3 * a + k] += f * d[k]; if (gc) gc[3 * c + k] -= f * d[k]; }
        }
}

// V_pc = -sum_c q_c A(R_c): the charges as centres - per primitive pair the Hermite-Coulomb tables of all charges summed first, in list
// order, then one contraction
void qc_host_point_charge_matrix(const qc_system *S, const std::vector<double> &pc, double *out) {
    std::vector<double> R0;
    host_coulomb_matrices<1>(S, -1.0, out, [&](int L, double p, const double *P, std::vector<double> *R) {
        R[0].assign(qc_nherm(L), 0.0);
        for (size_t c = 0; c < pc.size() / 4; ++c) {
            const double PC[3] = {P[0] - pc[4 * c], P[1] - pc[4 * c + 1], P[2] - pc[4 * c + 2]};
            hermite_r_host(L, p, PC, R0);
            for (size_t h = 0; h < R[0].size(); ++h) R[0][h] += pc[4 * c + 3] * R0[h];
        }
    });
}

// B^k_ab = dA_ab(r)/dr_k, k = x, y, z: qc_host_potential_matrix with the table of order L + 1 shifted by one unit along k,
// d/dr_x R_tuv(P - r) = -R_{t+1,u,v}
void qc_host_field_matrix(const qc_system *S, const double *r, double *out) {
    std::vector<double> R0;
    host_coulomb_matrices<3>(S, 1.0, out, [&](int L, double p, const double *P, std::vector<double> *R) {
        const double PC[3] = {P[0] - r[0], P[1] - r[1], P[2] - r[2]};
        hermite_r_host(L + 1, p, PC, R0);
        for (int k = 0; k < 3; ++k) R[k].assign(qc_nherm(L), 0.0);
        for (int t = 0; t <= L; ++t)
            for (int u = 0; t + u <= L; ++u)
                for (int v = 0; t + u + v <= L; ++v) {
                    R[0][qc_hidx(t, u, v)] = -R0[qc_hidx(t + 1, u, v)];
                    R[1][qc_hidx(t, u, v)] = -R0[qc_hidx(t, u + 1, v)];
                    R[2][qc_hidx(t, u, v)] = -R0[qc_hidx(t, u, v + 1)];
                }
    });
}

void qc_points_enuc(const qc_system *S, int64_t npts, const double *xyz, double *e) {
    for (int64_t k = 0; k < npts; ++k) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int a = 0; a < S->natoms; ++a) {
            const double d[3] = {xyz[3 * k] - S->xyz[3 * a], xyz[3 * k + 1] - S->xyz[3 * a + 1], xyz[3 * k + 2] - S->xyz[3 * a + 2]};
            const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], r3 = r2 * std::sqrt(r2);
            for (int x = 0; x < 3; ++x) s[x] += (double)S->Z[a] * d[x] / r3;
        }
        for (int x = 0; x < 3; ++x) e[3 * k + x] = s[x];
    }
}
