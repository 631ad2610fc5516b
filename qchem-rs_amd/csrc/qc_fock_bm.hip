// qc_fock_bm.hip - "bra-major" ERI + Fock digestion kernels for the quartet classes whose narrower pair is an ss or a
// ps pair and whose total Hermite order is <= QC_LREG (all tables in registers; ps kets against d.d / f.p bras reach order 5), and for the
// p.p kets of large lists against p.p / d.s bras.  gfx950 / wave64.
//
// Same mathematics as qc_fock_kernel.h (molint::eri, rhf.rs:45, fused with compute_electronic_hamiltonian,
// rhf.rs:152-167 / uhf.rs:210-227), different mapping.  The contraction inside the primitive-quartet loop costs
// ncd * HAB * HCD FMAs, the one outside (once per bra primitive pair) nab * HAB * ncd: the pair with few functions
// belongs inside.  So here the narrow pair is the ket and
//   * one wave = one bundle: ONE bra pair (restricted to a range of its primitive pairs) against up to 64 ket pairs,
//     one ket - one whole shell quartet - per lane;
//   * everything of the bra is wave-uniform: its primitive headers and its expansion block E_ab (stored [ab][h] in
//     pairdataT) come through scalar loads, the step-3 contraction is FMAs with scalar operands, no LDS staging;
//   * a lane keeps W[ncd][HAB], the R table and the Boys values in registers and its block I[ab][cd] in a private LDS
//     column (row stride 65: conflict-free both ways); there is not a single barrier in the kernel;
//   * digestion: the J_ab block is common to the wave - it is reduced over the lanes through LDS and leaves as one
//     atomic per element; the ket-side J and the four K blocks are per-lane atomics into the replica of the wave.
#include "qc_fock_kernel.h"
#include "gen/qc_rtab.h"

#include "qc_fock_bm.h"

// The Boys table of the launch's Hermite order lives in LDS (QC_BM_TROW doubles per grid point: the 8 Taylor
// coefficients and exp(-x_k)): with one quartet per lane every table access is a 64-address gather, and the texture path
// - not the VALU - was what these kernels waited for when the rows came from global memory (rocprofv3: 60 % of the
// wave-cycles waiting to issue).  Same evaluation as qc_boys<L>.
// Wave-uniform reads of the bra's pair data go through the scalar unit: a pointer taken from the kernel's argument struct carries no
// no-alias information, so the compiler reads `pd[uniform]` with a 64-lane vector load per two values (10 loads and a full memory
// latency per row of step 3); the same address in the constant address space is an s_load.  (The pair data are written by the host
// before any launch.)
typedef const __attribute__((address_space(4))) double qc_cdouble;

constexpr int QC_BM_TROW = 9;
constexpr int QC_BM_TWORDS = QC_BOYS_NGRID * QC_BM_TROW;

template <int L>
__device__ __forceinline__ void qc_boys_lds(double x, const double *__restrict__ T, double (&F)[L + 1]) {
    if (x < QC_BOYS_XMAX) {
        const int k = (int)(x * (1.0 / QC_BOYS_DX) + 0.5);
        const double d = k * QC_BOYS_DX - x;
        const double *__restrict__ r = T + __umul24(k, QC_BM_TROW);   // (24-bit multiply: full rate, the 32-bit one a quarter)
        double f = r[7];
        f = fma(f, d, r[6]);
        f = fma(f, d, r[5]);
        f = fma(f, d, r[4]);
        f = fma(f, d, r[3]);
        f = fma(f, d, r[2]);
        f = fma(f, d, r[1]);
        f = fma(f, d, r[0]);
        F[L] = f;
        if constexpr (L > 0) {
            double ed = 1.0 / 40320.0;
            ed = fma(ed, d, 1.0 / 5040.0);
            ed = fma(ed, d, 1.0 / 720.0);
            ed = fma(ed, d, 1.0 / 120.0);
            ed = fma(ed, d, 1.0 / 24.0);
            ed = fma(ed, d, 1.0 / 6.0);
            ed = fma(ed, d, 0.5);
            ed = fma(ed, d, 1.0);
            ed = fma(ed, d, 1.0);
            const double ex = r[8] * ed, x2 = 2.0 * x;
#pragma unroll
            for (int n = L; n > 0; --n) F[n - 1] = fma(x2, F[n], ex) * (1.0 / (2 * n - 1));
        }
    } else {
        const double t = qc_rsqrt(x);
        F[0] = (0.5 * 1.7724538509055160273) * t;
        if constexpr (L > 0) {
            const double hr = 0.5 * (t * t);
#pragma unroll
            for (int n = 0; n < L; ++n) F[n + 1] = ((double)(2 * n + 1) * hr) * F[n];
        }
    }
}

// Step 2 against a ps ket in packed form: column c is the Cartesian axis c of the p function, its Hermite expansion is
// e0[c] on the s-type function plus e1 on the first-order function of that axis - 2 FMAs per (column, bra Hermite
// index) instead of the 4 of the dense 4 x 3 block.  `me1` = -e1 (odd ket order).
template <int LAB>
__device__ __forceinline__ void qc_step2_ps(double (&W)[3][qc_nherm(LAB)], const double (&e0)[3], const double me1,
                                            const double (&R)[qc_nherm(LAB + 1)]) {
    constexpr QcTuvTable T = qc_make_tuv();
#pragma unroll
    for (int h = 0; h < qc_nherm(LAB); ++h) {
        const int t = T.t[h], u = T.u[h], v = T.v[h];
        const double r0 = R[h];
        W[0][h] = fma(me1, R[qc_hidx(t + 1, u, v)], fma(e0[0], r0, W[0][h]));
        W[1][h] = fma(me1, R[qc_hidx(t, u + 1, v)], fma(e0[1], r0, W[1][h]));
        W[2][h] = fma(me1, R[qc_hidx(t, u, v + 1)], fma(e0[2], r0, W[2][h]));
    }
}

// Step 2 against a p.p ket in packed form (round 3), for the wave's Cartesian axis CAX of the ket's FIRST function: column d is the axis d of
// the second function, and its expansion has four terms - on the s-type Hermite function, on the first-order functions of the axes CAX
// and d, and on the second-order function of CAX + d (qc_system.cpp, packed record): 4 FMAs per (column, bra Hermite index) where the
// dense 10 x 9 block would take 10.  c0[d] = A_c D_d + [c = d] kh, cc[d] = -kh D_d, cd = -hq A_c, ccd = khh (signs: odd ket orders).
template <int LAB, int CAX>
__device__ __forceinline__ void qc_step2_pp(double (&W)[3][qc_nherm(LAB)], const double (&c0)[3], const double (&cc)[3], const double cd, const double ccd,
                                            const double (&R)[qc_nherm(LAB + 2)]) {
    constexpr QcTuvTable T = qc_make_tuv();
#pragma unroll
    for (int h = 0; h < qc_nherm(LAB); ++h) {
        const int t = T.t[h] + (CAX == 0), u = T.u[h] + (CAX == 1), v = T.v[h] + (CAX == 2);     // h + e_c
        const double r0 = R[h], rc = R[qc_hidx(t, u, v)];
        W[0][h] = fma(ccd, R[qc_hidx(t + 1, u, v)], fma(cd, R[qc_hidx(T.t[h] + 1, T.u[h], T.v[h])], fma(cc[0], rc, fma(c0[0], r0, W[0][h]))));
        W[1][h] = fma(ccd, R[qc_hidx(t, u + 1, v)], fma(cd, R[qc_hidx(T.t[h], T.u[h] + 1, T.v[h])], fma(cc[1], rc, fma(c0[1], r0, W[1][h]))));
        W[2][h] = fma(ccd, R[qc_hidx(t, u, v + 1)], fma(cd, R[qc_hidx(T.t[h], T.u[h], T.v[h] + 1)], fma(cc[2], rc, fma(c0[2], r0, W[2][h]))));
    }
}

// Device records of the work lists (built by qc_bm_device_lists, qc_fock.hip): the bundle carries what the kernel needs of its bra pair,
// the unit what it needs of the lane's ket pair - a wave used to start with three dependent trips to memory (bundle -> pair descriptors
// -> first ket record); now the bundle comes through the scalar unit and both records of the NEXT bundle are requested while the current
// one is being digested (qc_bm_segment).
typedef int qc_v4i __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) qc_v4i qc_cv4i;
struct QcBmBundleRegs { int bra, ij_lo, ij_hi, first, nket, maxK, bdoff, offa, offb, na, nb, eq, cax; };   // wave-uniform (cax: p.p kets, axis of the first function)
__device__ __forceinline__ QcBmBundleRegs qc_bm_load_bundle(const QcBundleDev *bundles, const int b) {
    const qc_cv4i *bp = (const qc_cv4i *)(bundles + b);
    const qc_v4i x = bp[0], y = bp[1], z = bp[2];
    return QcBmBundleRegs{x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, z.x, z.y & 0xff, (z.y >> 8) & 0xff, (z.y >> 16) & 1, z.z};
}

// ---- what the pieces of a bundle's body share
constexpr int QC_BM_LS = 65;                                  // row stride (doubles) of a wave's I block in LDS
constexpr int qc_bm_nc(int lcd) { return lcd == 0 ? 1 : 3; }  // ket columns of a lane: one (ss), or the three of an axis (ps, p.p)
// The wave's side of a bundle: its bra pair (wave-uniform) and its block I[ab * NC + col][lane]
struct QcBmView {
    const double *pd, *pdT, *Tb;                              // pair data, the same with the expansions stored [ab][h], the Boys table (LDS)
    int lane, n;
    int bdoff, strideB, ij_lo, ij_hi, maxK;                   // the bra's pair-data block, its primitive pairs [ij_lo, ij_hi), longest ket chunk
    int na, nb, nab, offa, offb;
    double *Iw, *I;                                           // the wave's block; this lane's column of it, I[x * QC_BM_LS]
};
// The lane's side: its ket pair, decoded from the unit (ket pair | offset of its (chunk of) primitive records | c0, d0 | primitives, shape)
template <int LCD>
struct QcBmKetView {
    const double *base;                                       // first primitive record of the chunk (ss: pair data; ps, p.p: packed records)
    int ket, K_cd, Kc1;                                       // ket pair; primitives of the chunk (0: idle lane) and the index of its last
    bool active, nd1, keq;                                    // (nc, nd) = (1,1), (3,1) [nd1] or (1,3); keq: one shell twice
    int c0, d0, kc[qc_bm_nc(LCD)], lc[qc_bm_nc(LCD)];         // column c of the lane is the function pair (c0 + kc[c], d0 + lc[c])
};
template <int LCD>
__device__ __forceinline__ QcBmKetView<LCD> qc_bm_ket_view(const QcBmView &v, const double *pspack, const QcBmBundleRegs &bd, const QcKetUnit ue) {
    QcBmKetView<LCD> k;
    k.active = v.lane < bd.nket;
    k.ket = ue.ket;
    k.K_cd = k.active ? (ue.info & 0xffff) : 0; k.Kc1 = max(k.K_cd - 1, 0);
    k.nd1 = (ue.info >> 16) & 1;
    k.keq = (ue.info >> 17) & 1;
    // (p.p kets: the lane's three columns share the function of the wave's axis in the first shell - it moves into the column base)
    k.c0 = (ue.cd & 0xffff) + (LCD == 2 ? ((ue.info >> (24 + 2 * bd.cax)) & 3) : 0); k.d0 = (int)((unsigned)ue.cd >> 16);
    k.base = ((LCD == 0) ? v.pd : pspack) + ue.koff;
#pragma unroll
    for (int c = 0; c < qc_bm_nc(LCD); ++c) {
        const int fc = (LCD == 0) ? 0 : (ue.info >> (18 + 2 * c)) & 3;   // ps kets: column c = axis c = p function fc
        k.kc[c] = k.nd1 ? fc : 0; k.lc[c] = k.nd1 ? 0 : fc;
    }
    return k;
}

// One ket primitive record.  ss kets: pair-data block [q, Q | E] (h, e); ps kets: packed record [q, Q | e0x, e0y, e0z, e1] (h, e4; stride
// 8); p.p kets: [q, Q | A_x, A_y, A_z, kh | D_x, D_y, D_z, khh | hq A_x, hq A_y, hq A_z, -] (h, e4, e4b, e4c; stride 16).
struct QcBmKetRec { double4 h; double e; double4 e4, e4b, e4c; };
template <int LCD>
__device__ __forceinline__ QcBmKetRec qc_bm_fetch(const double *__restrict__ kb) {
    QcBmKetRec r{};
    r.h = *reinterpret_cast<const double4 *>(kb);
    if constexpr (LCD == 0) r.e = kb[4];
    else r.e4 = *reinterpret_cast<const double4 *>(kb + 4);
    if constexpr (LCD == 2) { r.e4b = *reinterpret_cast<const double4 *>(kb + 8); r.e4c = *reinterpret_cast<const double4 *>(kb + 12); }
    return r;
}
// the headers (p, P) of the bra primitive pairs ij and ij + 1, clamped to the bundle's last
__device__ __forceinline__ void qc_bm_bra_headers(const QcBmView &v, const int ij, double (&hd)[2][4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        qc_cdouble *bh = (qc_cdouble *)(v.pd + v.bdoff + (size_t)min(ij + u, v.ij_hi - 1) * v.strideB);
        hd[u][0] = bh[0]; hd[u][1] = bh[1]; hd[u][2] = bh[2]; hd[u][3] = bh[3];
    }
}

// The primitive step: the primitive quartets of ket record `rc` with the NIJ bra primitive pairs of the pass (headers hd) - Boys values,
// R table, and step 2 in the form of the ket type: W[u][c][h] += sum_h' E_cd[c][h'] R_{h + h'} (`valid`: the record is one of the lane's)
template <int LAB, int LCD, int NIJ, int CAX>
__device__ __forceinline__ void qc_bm_prim(const QcBmKetRec &rc, const bool valid, const double (&hd)[2][4], const double *__restrict__ Tb,
                                           double (&W)[NIJ][qc_bm_nc(LCD)][qc_nherm(LAB)]) {
    constexpr int L = LAB + LCD;
    const double4 ck = rc.h;
    const double q = ck.x;
#pragma unroll
    for (int u = 0; u < NIJ; ++u) {
        const double p = hd[u][0], X = hd[u][1] - ck.y, Y = hd[u][2] - ck.z, Z = hd[u][3] - ck.w;
        const double pref = qc_rsqrt(p + q);
        const double alpha = p * q * (pref * pref);
        double F[L + 1], Rr[qc_nherm(L)];
        qc_boys_lds<L>(alpha * (X * X + Y * Y + Z * Z), Tb, F);
        qc_rtab<L>(alpha, X, Y, Z, F, Rr);
        const double sc = valid ? pref : 0.0;
        if constexpr (LCD == 0) {
            const double e = rc.e * sc;               // ss ket: a single Hermite function, W[h] += e R_h
#pragma unroll
            for (int h = 0; h < qc_nherm(LAB); ++h) W[u][0][h] = fma(e, Rr[h], W[u][0][h]);
        } else if constexpr (LCD == 1) {
            const double e0[3] = {rc.e4.x * sc, rc.e4.y * sc, rc.e4.z * sc};
            qc_step2_ps<LAB>(W[u], e0, -(rc.e4.w * sc), Rr);
        } else {
            const double Ac = (CAX == 0 ? rc.e4.x : (CAX == 1 ? rc.e4.y : rc.e4.z)) * sc, hAc = (CAX == 0 ? rc.e4c.x : (CAX == 1 ? rc.e4c.y : rc.e4c.z)) * sc;
            const double kh = rc.e4.w * sc;
            const double c0[3] = {fma(Ac, rc.e4b.x, CAX == 0 ? kh : 0.0), fma(Ac, rc.e4b.y, CAX == 1 ? kh : 0.0), fma(Ac, rc.e4b.z, CAX == 2 ? kh : 0.0)};
            const double cc[3] = {-(kh * rc.e4b.x), -(kh * rc.e4b.y), -(kh * rc.e4b.z)};
            qc_step2_pp<LAB, CAX>(W[u], c0, cc, -hAc, rc.e4b.w * sc, Rr);
        }
    }
}

// Step 3 of the high bras against ss kets (HAB = 20 / 35, up to 36 function pairs), I[ab] += sum_h E_ab,ij[ab][h] W[h]: a row is 2-4
// scalar pieces, and one piece ahead leaves the step bound by the scalar-load latency (17 us of a 36 us bundle for the (dd|ss) class).  The
// block is staged in the wave's LDS - coalesced loads, one latency - and read back as wave-uniform (broadcast) DS reads.
// (ps kets, three columns per lane: measured slower staged - 17 vs 10 us per bundle on H2O/cc-pVTZ)
constexpr bool qc_bm_staged(int lab, int lcd) { return lab >= 3 && lcd == 0; }
// LAB = 3: the block is requested BEFORE the primitive loop - NV values per lane held in registers through it (at most 18 function pairs
// x 20 = 6 per lane) - and stored to LDS after it.  LAB = 4 would need 20 - that costs the ss-ket launch its second wave per SIMD - and
// its bras are mostly single primitive pairs, one pass per bundle: staged after the loop, one exposed latency.
constexpr int qc_bm_nprestage(int lab) { return lab == 3 ? (18 * 20 + 63) / 64 : 1; }
template <int LAB>
__device__ __forceinline__ void qc_bm_prestage(const QcBmView &v, const int ij, double (&est)[qc_bm_nprestage(LAB)]) {
    if constexpr (LAB == 3) {
        const double *__restrict__ Eg = v.pdT + v.bdoff + (size_t)ij * v.strideB + 4;
        const int ne = v.nab * qc_nherm(LAB);
#pragma unroll
        for (int k = 0; k < qc_bm_nprestage(LAB); ++k) est[k] = (k * 64 < ne) ? Eg[min(v.lane + k * 64, ne - 1)] : 0.0;
    }
}
template <int LAB>
__device__ __forceinline__ void qc_bm_step3_staged(const QcBmView &v, const int ij, const double (&est)[qc_bm_nprestage(LAB)],
                                                   const double (&W)[1][1][qc_nherm(LAB)]) {
    constexpr int HAB = qc_nherm(LAB), NV = qc_bm_nprestage(LAB), LS = QC_BM_LS;
    constexpr bool PRE = LAB == 3;
    const int lane = v.lane, nab = v.nab, ne = nab * HAB;
    const double *__restrict__ Eg = v.pdT + v.bdoff + (size_t)ij * v.strideB + 4;
    double *const I = v.I;
    double *const Es = v.Iw + nab * LS;                       // behind the wave's I block (qc_bm_wave_words)
    if constexpr (PRE) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (k * 64 < ne) Es[min(lane + k * 64, ne - 1)] = est[k];   // (lanes past the end rewrite the last element with its own value)
    }
    for (int x0 = lane + (PRE ? NV * 64 : 0); x0 < ne; x0 += 4 * 64) {  // what the register stage does not hold
        double e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = Eg[min(x0 + k * 64, ne - 1)];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k * 64 < ne) Es[x0 + k * 64] = e[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int ab = 0; ab < nab; ++ab) {
        const double *row = Es + ab * HAB;
        double acc = 0.0;
#pragma unroll
        for (int h = 0; h < HAB; ++h) acc = fma(row[h], W[0][0][h], acc);   // (one chain in ascending h, as in the scalar form: same roundings)
        qc_ds_add(&I[ab * LS], acc);
    }
    // (the next pass overwrites Es only after these reads: DS operations of a wave execute in order)
}

// Step 3 with the bra blocks through the scalar unit, I[ab][c] += sum_u sum_h E_ab,ij+u[ab][h] W[u][c][h]: the rows come in pieces of
// QC_BM_PIECE scalars, each requested while the previous one is being used
constexpr int QC_BM_PIECE = 10;
template <int LAB, int LCD, int NIJ>
__device__ __forceinline__ void qc_bm_step3_scalar(const QcBmView &v, const int ij, const double (&W)[NIJ][qc_bm_nc(LCD)][qc_nherm(LAB)]) {
    constexpr int HAB = qc_nherm(LAB), NC = qc_bm_nc(LCD), LS = QC_BM_LS;
    constexpr int PL = QC_BM_PIECE, NPC = (HAB + PL - 1) / PL, NP = NIJ * NPC;
    const int nab = v.nab, strideB = v.strideB;
    double *const I = v.I;
    qc_cdouble *ET = (qc_cdouble *)(v.pdT + v.bdoff + (size_t)ij * strideB + 4);
    auto load_piece = [&](double (&e)[PL], const int ab, const int u, const int pc) {
        qc_cdouble *row = ET + (size_t)u * strideB + ab * HAB + pc * PL;
#pragma unroll
        for (int k = 0; k < PL; ++k)
            if (pc * PL + k < HAB) e[k] = row[k];
    };
    double cur[PL], nxt[PL];
#pragma unroll
    for (int k = 0; k < PL; ++k) cur[k] = nxt[k] = 0.0;
    load_piece(cur, 0, 0, 0);
    for (int ab = 0; ab < nab; ++ab) {
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        const int abn = min(ab + 1, nab - 1);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int u = j / NPC, pc = j % NPC;
            if (j + 1 < NP) load_piece(nxt, ab, (j + 1) / NPC, (j + 1) % NPC);
            else load_piece(nxt, abn, 0, 0);
#pragma unroll
            for (int k = 0; k < PL; ++k)
                if (pc * PL + k < HAB) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[c] = fma(cur[k], W[u][c][pc * PL + k], acc[c]);
                }
#pragma unroll
            for (int k = 0; k < PL; ++k) cur[k] = nxt[k];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) qc_ds_add(&I[(ab * NC + c) * LS], acc[c]);
    }
}

// One pass over the ket primitives for NIJ consecutive bra primitive pairs (NIJ = 2 shares every ket load between two
// primitive quartets), followed by step 3 with the wave-uniform bra blocks.
// Latencies a pass used to expose, and what hides them now (round 3; with ket chunks of <= 8 primitives a pass is only ~16 primitive
// quartets long, so they were a third to a half of a wave's life): the bra headers of the NEXT pass are requested before the
// primitive loop (`hd` carries them from pass to pass); the first ket record is loaded once per bundle (`first`); the expansion block
// of step 3 is pre-staged or comes in pieces, each requested while the previous one is being used.
template <int LAB, int LCD, int NIJ, int CAX = 0>
__device__ __forceinline__ void qc_bm_pass(const QcBmView &v, const QcBmKetView<LCD> &kv, const int ij, const QcBmKetRec &first, double (&hd)[2][4]) {
    constexpr int HAB = qc_nherm(LAB), NC = qc_bm_nc(LCD);
    constexpr int strideK = (LCD == 0) ? qc_pair_stride(0, 1) : (LCD == 1 ? 8 : 16);
    // headers of the bra primitive pairs after this pass (clamped: the last pass re-reads its own)
    double hn[2][4];
    qc_bm_bra_headers(v, ij + NIJ, hn);
    double W[NIJ][NC][HAB];
#pragma unroll
    for (int u = 0; u < NIJ; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int h = 0; h < HAB; ++h) W[u][c][h] = 0.0;
    double est[qc_bm_nprestage(LAB)];
    if constexpr (qc_bm_staged(LAB, LCD)) qc_bm_prestage<LAB>(v, ij, est);
    // The ket primitives' records are requested one iteration ahead.  An iteration takes 0.47-0.74 us in EVERY class, (ss|ss) with its 130
    // instructions as well as (pp|ps) with 217, against 0.15-0.3 us of issue - but two or three records ahead (round 4) gained nothing:
    // the loop takes turns with the SIMD's other waves, it does not wait for its record.
    QcBmKetRec next = first;
    for (int kl = 0; kl < v.maxK; ++kl) {
        const QcBmKetRec cur = next;
        next = qc_bm_fetch<LCD>(kv.base + (size_t)min(kl + 1, kv.Kc1) * strideK);
        qc_bm_prim<LAB, LCD, NIJ, CAX>(cur, kl < kv.K_cd, hd, v.Tb, W);
    }
    if constexpr (qc_bm_staged(LAB, LCD)) {
        static_assert(NIJ == 1, "high bras run one bra primitive pair per pass");
        qc_bm_step3_staged<LAB>(v, ij, est, W);
    } else qc_bm_step3_scalar<LAB, LCD, NIJ>(v, ij, W);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) hd[u][k] = hn[u][k];
}

// The passes of a bundle: two bra primitive pairs per pass while W[2][NC][HAB] fits the registers, then one; p.p kets: the instance of
// the wave's axis (wave-uniform)
template <int LAB, int LCD, int NIJ, int CAX = 0>
__device__ __forceinline__ void qc_bm_pass_run(const QcBmView &v, const QcBmKetView<LCD> &kv, int &ij, const QcBmKetRec &first, double (&hd)[2][4]) {
    for (; ij + NIJ <= v.ij_hi; ij += NIJ) qc_bm_pass<LAB, LCD, NIJ, CAX>(v, kv, ij, first, hd);
}
template <int LAB, int LCD>
__device__ __forceinline__ void qc_bm_passes(const QcBmView &v, const QcBmKetView<LCD> &kv, const int cax) {
    constexpr bool PAIRED = 2 * qc_bm_nc(LCD) * qc_nherm(LAB) <= 24;
    // first ket record of the lane's chunk (the same for every pass) and the headers of the first two bra primitive pairs
    const QcBmKetRec first = qc_bm_fetch<LCD>(kv.base);
    double hd[2][4];
    qc_bm_bra_headers(v, v.ij_lo, hd);
    int ij = v.ij_lo;
    if constexpr (LCD == 2) {
        if (cax == 0) qc_bm_pass_run<LAB, LCD, 1, 0>(v, kv, ij, first, hd);
        else if (cax == 1) qc_bm_pass_run<LAB, LCD, 1, 1>(v, kv, ij, first, hd);
        else qc_bm_pass_run<LAB, LCD, 1, 2>(v, kv, ij, first, hd);
    } else {
        if constexpr (PAIRED) qc_bm_pass_run<LAB, LCD, 2>(v, kv, ij, first, hd);
        qc_bm_pass_run<LAB, LCD, 1>(v, kv, ij, first, hd);
    }
}

// Output: Schwarz factors - the bundles are (P|P) quartets, one ket per bundle; the largest element of the block is on its diagonal
template <int LCD>
__device__ __forceinline__ void qc_bm_out_schwarz(const QcKernelArgs &a, const QcBmView &v, const QcBmKetView<LCD> &kv) {
    if (!kv.active) return;
    double m = 0.0;
    for (int x = 0; x < v.nab * qc_bm_nc(LCD); ++x) m = fmax(m, fabs(v.I[x * QC_BM_LS]));
    a.schwarz_out[kv.ket] = sqrt(m);
}
// Output: (ij|kl) materialised with its 8 symmetry images (qc_eri_full, MP2, stored-tensor mode; bundles are not cut along ij there)
template <int LCD>
__device__ __forceinline__ void qc_bm_out_tensor(const QcKernelArgs &a, const QcBmView &v, const QcBmKetView<LCD> &kv) {
    constexpr int NC = qc_bm_nc(LCD);
    if (!kv.active) return;
    const QcTensorOut out(a.eri_out, v.n);
    for (int ab = 0; ab < v.nab; ++ab)
        for (int c = 0; c < NC; ++c)
            out.store8(v.offa + ab / v.nb, v.offb + ab % v.nb, kv.c0 + kv.kc[c], kv.d0 + kv.lc[c], v.I[(ab * NC + c) * QC_BM_LS]);
}

// Where a bundle's Fock contributions go: the wave's replica of G (both spins) and, for the exchange rows of the bra's functions, the
// wave's row buffer in LDS (null: none - they go to G directly)
struct QcBmSink {
    double *G0, *G1, *rowbuf;
    int rowcap, n;
    double fxscale;                                           // 0: f64 atomics
    size_t fx_lo;
};
// Exchange contributions land in the rows of the bra's functions (r = i, or na + j; `grow` in G) at the columns of this lane's ket
// functions.  With a row buffer they are DS atomics and the rows leave as one global atomic per touched element after the bundle
// (qc_bm_flush_rows); without one they go to global memory directly.
__device__ __forceinline__ void qc_bm_kadd(const QcBmSink &g, int sp, int r, int grow, int col, double val) {
    if (g.rowbuf) qc_ds_add(&g.rowbuf[((size_t)sp * g.rowcap + r) * g.n + col], val);
    else qc_gadd(&(sp ? g.G1 : g.G0)[(size_t)grow * g.n + col], val, g.fxscale, g.fx_lo);
}
// the partial sums of one target row: G[target, c_k] (accK) and G[target, d_l] (accL) over the lane's columns
template <int LCD>
__device__ __forceinline__ void qc_bm_kadd3(const QcBmSink &g, const QcBmKetView<LCD> &kv, const double fk, int sp, int r, int grow,
                                            const double (&accK)[qc_bm_nc(LCD)], const double (&accL)[qc_bm_nc(LCD)]) {
    const int c0 = kv.c0, d0 = kv.d0;
    if constexpr (LCD == 0) {
        qc_bm_kadd(g, sp, r, grow, c0, fk * accK[0]);
        qc_bm_kadd(g, sp, r, grow, d0, fk * accL[0]);
    } else if (kv.nd1) {                                      // columns differ in k, share l
        qc_bm_kadd(g, sp, r, grow, c0 + kv.kc[0], fk * accK[0]); qc_bm_kadd(g, sp, r, grow, c0 + kv.kc[1], fk * accK[1]); qc_bm_kadd(g, sp, r, grow, c0 + kv.kc[2], fk * accK[2]);
        qc_bm_kadd(g, sp, r, grow, d0, fk * (accL[0] + accL[1] + accL[2]));
    } else {                                                  // columns differ in l, share k
        qc_bm_kadd(g, sp, r, grow, c0, fk * (accK[0] + accK[1] + accK[2]));
        qc_bm_kadd(g, sp, r, grow, d0 + kv.lc[0], fk * accL[0]); qc_bm_kadd(g, sp, r, grow, d0 + kv.lc[1], fk * accL[1]); qc_bm_kadd(g, sp, r, grow, d0 + kv.lc[2], fk * accL[2]);
    }
}
// One half of a spin's exchange blocks: the targets are the functions of one bra shell (on_a: a_i, with D[b_j, d_l] and D[b_j, c_k];
// else b_j, with D[a_i, .]).  The density rows of the functions of the OTHER bra shell are gathered first (one memory latency per half
// instead of one per target row: the elements do not depend on the target), then every target row is a loop over LDS reads.  RB covers
// a whole shell, so a target element is ONE sum over the other shell's functions in ascending order (the O2 triplet run of the tests
// sits on a saddle and follows these roundings).
// (Not force-inlined: inlined before the optimiser runs, both halves of the ss-ket instances compile to 40 % more register moves and
// another branch structure, and bm<0,1> ran 2 % longer on benzene/cc-pVDZ; inlined in its turn - it always is, the kernels have no
// calls and no scratch - it is the code of the lambda it replaces, profiles/r20_bm_body_kernel_resources.md.)
template <int LAB, int LCD>
__device__ inline void qc_bm_exchange_half(const QcBmView &v, const QcBmKetView<LCD> &kv, const QcBmSink &g, const double fk,
                                                    const double *__restrict__ Dk, const int s, const bool on_a) {
    constexpr int NC = qc_bm_nc(LCD), LS = QC_BM_LS, RB = (LAB <= 2) ? 6 : 10;
    const int na = v.na, nb = v.nb, n = v.n;
    const int nt = on_a ? na : nb, no = on_a ? nb : na;      // target shell / other shell (wave-uniform)
    const int offo = on_a ? v.offb : v.offa;
    const double *const I = v.I;
    for (int o0 = 0; o0 < no; o0 += RB) {
        double dK[RB][NC], dL[RB][NC];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll
            for (int c = 0; c < NC; ++c) dK[r][c] = dL[r][c] = 0.0;
            if (o0 + r < no) {
                const double *__restrict__ Drow = Dk + (size_t)(offo + o0 + r) * n;
#pragma unroll
                for (int c = 0; c < NC; ++c) { dK[r][c] = Drow[kv.d0 + kv.lc[c]]; dL[r][c] = Drow[kv.c0 + kv.kc[c]]; }
            }
        }
        for (int t = 0; t < nt; ++t) {
            double accK[NC], accL[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) accK[c] = accL[c] = 0.0;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (o0 + r < no) {
                    const int o = o0 + r;
                    const int ab = on_a ? t * nb + o : o * nb + t;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const double val = I[(ab * NC + c) * LS];
                        accK[c] = fma(val, dK[r][c], accK[c]);
                        accL[c] = fma(val, dL[r][c], accL[c]);
                    }
                }
            }
            qc_bm_kadd3<LCD>(g, kv, fk, s, on_a ? t : na + t, (on_a ? v.offa : v.offb) + t, accK, accL);
        }
    }
}
// Exchange blocks (they read I), per spin: Gt_ik -= cK f sum_jl I D_jl and the il / jk / jl images (fk = -cK f)
template <int LAB, int LCD>
__device__ __forceinline__ void qc_bm_exchange(const QcKernelArgs &a, const QcBmView &v, const QcBmKetView<LCD> &kv, const QcBmSink &g, const double fk) {
    if (!kv.active) return;
    for (int s = 0; s < (a.Dk1 != nullptr ? 2 : 1); ++s) {
        const double *__restrict__ Dk = s ? a.Dk1 : a.Dk0;
        qc_bm_exchange_half<LAB, LCD>(v, kv, g, fk, Dk, s, true);
        qc_bm_exchange_half<LAB, LCD>(v, kv, g, fk, Dk, s, false);
    }
}

// Coulomb blocks: Gt_cd += fj sum_ab I D_ab (per lane);  Gt_ab += fj sum_cd I D_cd (reduced over the wave); fj = 2f, dcd = the lane's
// ket-side density elements
template <int LCD>
__device__ __forceinline__ void qc_bm_coulomb(const QcKernelArgs &a, const QcBmView &v, const QcBmKetView<LCD> &kv, const QcBmSink &g, const double fj,
                                              const double (&dcd)[qc_bm_nc(LCD)]) {
    constexpr int NC = qc_bm_nc(LCD), LS = QC_BM_LS;
    const int n = v.n, na = v.na, nb = v.nb, nab = v.nab, offa = v.offa, offb = v.offb;
    const bool uhf = a.Dk1 != nullptr;
    double *const I = v.I;
    double jcd[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) jcd[c] = 0.0;
    {
        // D_ab is wave-uniform: scalar loads, one element ahead (the density is written by earlier launches only)
        qc_cdouble *Dj = (qc_cdouble *)a.Dj;
        int bi = 0, bj = 0;
        double dab = Dj[(size_t)offa * n + offb];
        for (int ab = 0; ab < nab; ++ab) {
            int bjn = bj + 1, bin = bi;
            if (bjn == nb) { bjn = 0; ++bin; }
            if (bin == na) { bin = na - 1; bjn = nb - 1; }
            const double dnx = Dj[(size_t)(offa + bin) * n + offb + bjn];
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double val = I[(ab * NC + c) * LS];
                jcd[c] = fma(val, dab, jcd[c]);
                t = fma(val, dcd[c], t);
            }
            I[(ab * NC) * LS] = fj * t;                       // own column: this lane's share of Gt_ab
            dab = dnx; bi = bin; bj = bjn;
        }
    }
    if (kv.active) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const size_t o = (size_t)(kv.c0 + kv.kc[c]) * n + kv.d0 + kv.lc[c];
            qc_gadd2(&g.G0[o], &g.G1[o], uhf, fj * jcd[c], g.fxscale, g.fx_lo);
        }
    }
    // same-wave LDS hand-off (DS operations of a wave execute in order): lane ab sums row ab over the 64 columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int ab = v.lane; ab < nab; ab += 64) {
        const double *row = v.Iw + (size_t)(ab * NC) * LS;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
        for (int j = 0; j < 64; j += 2) { s0 += row[j]; s1 += row[j + 1]; }
        const size_t o = (size_t)(offa + ab / nb) * n + offb + ab % nb;
        qc_gadd2(&g.G0[o], &g.G1[o], uhf, s0 + s1, g.fxscale, g.fx_lo);
    }
}

// One bundle: the lane's quartet block I through the passes, then one output - Schwarz factor, the materialised tensor, or digestion
template <int LAB, int LCD>
__device__ __forceinline__ void qc_bm_body(const QcKernelArgs &a, const double *__restrict__ pdT, const QcBmBundleRegs &bd, const QcKetUnit ue,
                                           const int blk, const double *__restrict__ Tb, double *const Iw,
                                           const double *__restrict__ pspack, double *const rowbuf, const int rowcap) {
    constexpr int NC = qc_bm_nc(LCD);
    const int lane = threadIdx.x & 63, nab = bd.na * bd.nb;
    const QcBmView v{a.pairdata, pdT, Tb, lane, a.n, bd.bdoff, qc_pair_stride(LAB, nab), bd.ij_lo, bd.ij_hi, bd.maxK,
                     bd.na, bd.nb, nab, bd.offa, bd.offb, Iw, Iw + lane};
    const QcBmKetView<LCD> kv = qc_bm_ket_view<LCD>(v, pspack, bd, ue);
    const double fxscale = a.fxs ? a.fxs[0] : 0.0;            // 0: f64 atomics
    for (int x = 0; x < nab * NC; ++x) v.I[x * QC_BM_LS] = 0.0;
    qc_bm_passes<LAB, LCD>(v, kv, bd.cax);

    if (a.schwarz_out != nullptr) { qc_bm_out_schwarz<LCD>(a, v, kv); return; }
    if (a.eri_out != nullptr) { qc_bm_out_tensor<LCD>(a, v, kv); return; }

    const size_t rep = (size_t)(blk % a.nrep) * a.rep_stride;
    const QcBmSink g{a.G0 + rep, a.G1 + rep, rowbuf, rowcap, a.n, fxscale, a.fx_lo};
    const double f = kv.active ? (bd.eq ? 0.5 : 1.0) * (kv.keq ? 0.5 : 1.0) * (bd.bra == kv.ket ? 0.5 : 1.0) : 0.0;
    // this lane's ket-side density elements (Coulomb part): requested here, used after the exchange blocks
    double dcd[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) dcd[c] = kv.active ? a.Dj[(size_t)(kv.c0 + kv.kc[c]) * a.n + kv.d0 + kv.lc[c]] : 0.0;
    qc_bm_exchange<LAB, LCD>(a, v, kv, g, -a.cK * f);
    qc_bm_coulomb<LCD>(a, v, kv, g, 2.0 * f, dcd);
}

// The Boys table of Hermite order L into the head of the workgroup's LDS, QC_BM_TROW words per grid point (every thread of the workgroup)
template <int L>
__device__ __forceinline__ void qc_bm_load_boys_table(const double *__restrict__ boys, double *const lds) {
    const double *__restrict__ rows = boys + (size_t)L * QC_BOYS_NGRID * 8;
    const double *__restrict__ exk = boys + (size_t)(QC_LTOT + 1) * QC_BOYS_NGRID * 8;
    // eight loads of a thread in flight together (an L2 round trip per batch, not per element)
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i0 = tid; i0 < QC_BM_TWORDS; i0 += 8 * nt) {
        double e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = min(i0 + j * nt, QC_BM_TWORDS - 1);
            const int k = i / QC_BM_TROW, r = i - k * QC_BM_TROW;
            e[j] = (r < 8) ? rows[k * 8 + r] : exk[k];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j * nt < QC_BM_TWORDS) lds[i0 + j * nt] = e[j];
    }
}
// The rows a wave has accumulated for the bundle `pb` leave as one global atomic per touched element (g: the wave's row buffer and its
// replica of G): the 64 kets of a bundle share most of their functions, so the lanes' contributions combine 2-5x in LDS first
__device__ __forceinline__ void qc_bm_flush_rows(const QcBmSink &g, const int nsp, const QcBmBundleRegs &pb, const int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int sp = 0; sp < nsp; ++sp) {
        double *G = sp ? g.G1 : g.G0;
        for (int r = 0; r < pb.na + pb.nb; ++r) {
            const int grow = r < pb.na ? pb.offa + r : pb.offb + r - pb.na;
            double *row = g.rowbuf + ((size_t)sp * g.rowcap + r) * g.n;
            for (int col = lane; col < g.n; col += 64) {
                const double val = row[col];
                if (val != 0.0) { qc_gadd(&G[(size_t)grow * g.n + col], val, g.fxscale, g.fx_lo); row[col] = 0.0; }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup = up to QC_BM_WAVES independent waves sharing the LDS Boys table of their segment's Hermite order; every wave
// walks the segment's bundle list with the stride of the launch (bundles are sorted longest first).
template <int LAB, int LCD>
__device__ __forceinline__ void qc_bm_segment(const QcBmArgs &a, const int s, const int wg, const int nwg) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, wave = tid >> 6;
    qc_bm_load_boys_table<LAB + LCD>(a.base.boys, lds);
    __syncthreads();
    const int nw = blockDim.x >> 6;                           // <= QC_BM_WAVES: fewer when the LDS blocks of that many waves would not fit
    const int n = a.base.n, lane = tid & 63;
    const int rowcap = a.seg_rows[s], nsp = a.base.Dk1 ? 2 : 1;
    const int rowwords = a.use_rowbuf ? nsp * rowcap * n : 0;
    double *const wbase = lds + ((QC_BM_TWORDS + 1) & ~1) + (size_t)wave * (a.seg_iwords[s] + rowwords);
    double *const Iw = wbase;
    double *const rowbuf = rowwords ? wbase + a.seg_iwords[s] : nullptr;
    for (int x = lane; x < rowwords; x += 64) rowbuf[x] = 0.0;
    const QcBundleDev *__restrict__ bundles = a.seg_bundles[s];
    const QcKetUnit *__restrict__ units = a.seg_ketlist[s];
    const size_t wrep = (size_t)((wg * nw + wave) % a.base.nrep) * a.base.rep_stride;
    const QcBmSink rows{a.base.G0 + wrep, a.base.G1 + wrep, rowbuf, rowcap, n, a.base.fxs ? a.base.fxs[0] : 0.0, a.base.fx_lo};
    const int nb = a.seg_nbundles[s];
    const int b0 = __builtin_amdgcn_readfirstlane(wg * nw + wave), bstep = nwg * nw;
    if (b0 >= nb) return;
    QcBmBundleRegs bd = qc_bm_load_bundle(bundles, b0);
    QcKetUnit ue = units[bd.first + min(lane, bd.nket - 1)];
    for (int b = b0; b < nb; b += bstep) {
        // records of the wave's next bundle: the bundle now (scalar), its unit while the rows of this one are flushed
        const QcBmBundleRegs bdn = qc_bm_load_bundle(bundles, min(b + bstep, nb - 1));
        qc_bm_body<LAB, LCD>(a.base, a.pairdataT, bd, ue, b, lds, Iw, a.pspack, rowbuf, rowcap);
        const QcKetUnit uen = units[bdn.first + min(lane, bdn.nket - 1)];
        if (rowbuf) qc_bm_flush_rows(rows, nsp, bd, lane);
        bd = bdn; ue = uen;
    }
}

template <int LCD, int HI>
__global__ __launch_bounds__(QC_BM_WAVES * 64) void qc_fock_bm_kernel(const QcBmArgs a) {
    qc_tl_stamp(a.base.tl, 0);
    const QcSegment sg = qc_find_segment(a);
    const int s = sg.s;
#define QC_BM_CASE(LAB) case LAB: qc_bm_segment<LAB, LCD>(a, s, sg.blk, sg.nblk); break;
    if constexpr (LCD == 0 && HI == 0) { switch (a.seg_lab[s]) { QC_BM_CASE(0) QC_BM_CASE(1) QC_BM_CASE(2) default: break; } }
    if constexpr (LCD == 0 && HI == 1) { switch (a.seg_lab[s]) { QC_BM_CASE(3) QC_BM_CASE(4) default: break; } }
    if constexpr (LCD == 1 && HI == 0) { switch (a.seg_lab[s]) { QC_BM_CASE(1) QC_BM_CASE(2) default: break; } }
    if constexpr (LCD == 1 && HI == 1) { switch (a.seg_lab[s]) { QC_BM_CASE(3) QC_BM_CASE(4) default: break; } }
    if constexpr (LCD == 2 && HI == 0) { switch (a.seg_lab[s]) { QC_BM_CASE(2) default: break; } }
#undef QC_BM_CASE
    // <3, 0>: ONE launch for the ss kets against the high bras and the ps kets against the low bras (round 3) - both run at two waves per
    // SIMD and one workgroup per CU (129 / 98 KB of LDS on H2O/cc-pVTZ), so sharing a launch costs neither; their bundles fill the
    // chip together instead of following each other on a stream (50 + 83 us in-build there)
    if constexpr (LCD == 3 && HI == 0) {
        switch ((a.seg_lcd[s] << 4) | a.seg_lab[s]) {
            case 0x03: qc_bm_segment<3, 0>(a, s, sg.blk, sg.nblk); break;
            case 0x04: qc_bm_segment<4, 0>(a, s, sg.blk, sg.nblk); break;
            case 0x11: qc_bm_segment<1, 1>(a, s, sg.blk, sg.nblk); break;
            case 0x12: qc_bm_segment<2, 1>(a, s, sg.blk, sg.nblk); break;
            default: break;
        }
    }
    qc_tl_stamp(a.base.tl, 1);
}

// The exchange rows of a bundle are summed in LDS with f64 DS atomics, several lanes of ONE instruction adding to one address (qc_ds_add):
// bitwise reproducible builds need the DS unit to serve such lanes in an order that does not depend on timing.  No manual says so; every
// device seen does it.  This probe asks the device at hand: 64 lanes add values of very different magnitudes (the sum depends on the
// order) to one word, 64 times over, with another wave of the workgroup hammering the same LDS bank meanwhile; all 64 sums must be the same
// bits.  A device that fails is served without the row buffer (direct fixed-point global atomics: order-independent by construction).
__global__ __launch_bounds__(128) void qc_ds_order_probe_kernel(double *out) {
    __shared__ double acc[64 + 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 1) {                                   // traffic on the same banks, other addresses
        for (int rep = 0; rep < 4096; ++rep) qc_ds_add(&acc[64 + ((lane * 7 + rep) & 63)], 1.0);
        return;
    }
    const double v = ldexp(1.0 + 0.001 * lane, (lane * 37) % 53 - 20) * ((lane & 1) ? -1.0 : 1.0);
    for (int rep = 0; rep < 64; ++rep) {
        double *word = &acc[rep & 1];
        if (lane == 0) *word = 0.0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if ((lane + rep) & 3) qc_ds_add(&acc[2 + (lane & 31)], 1.0);       // (an unrelated add with a partial mask in front)
        qc_ds_add(word, v);                            // the probed instruction: 64 lanes, one address
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) out[rep] = *word;
    }
}
int qc_ds_order_probe(hipStream_t st, double *d_out64) {
    hipLaunchKernelGGL(qc_ds_order_probe_kernel, dim3(1), dim3(128), 0, st, d_out64);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}

template <int LCD, int HI>
static int launch_bm(int grid, int nwaves, size_t lds, hipStream_t st, const QcBmArgs &a) {
    return qc_launch_column<qc_fock_bm_kernel<LCD, HI>>(grid, nwaves * 64, lds, st, a);
}
int qc_launch_bm(int lcd, int hi, int grid, int nwaves, size_t lds, hipStream_t st, const QcBmArgs &a) {
    if (lcd == 3) return hi ? QC_ERR_UNSUPPORTED : launch_bm<3, 0>(grid, nwaves, lds, st, a);
    if (lcd == 2) return hi ? QC_ERR_UNSUPPORTED : launch_bm<2, 0>(grid, nwaves, lds, st, a);
    if (lcd == 0) return hi ? launch_bm<0, 1>(grid, nwaves, lds, st, a) : launch_bm<0, 0>(grid, nwaves, lds, st, a);
    return hi ? launch_bm<1, 1>(grid, nwaves, lds, st, a) : launch_bm<1, 0>(grid, nwaves, lds, st, a);
}
