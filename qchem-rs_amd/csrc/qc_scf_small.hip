// qc_scf_small.hip - the Roothaan step of one spin for n <= 64 basis functions as ONE workgroup with every matrix in LDS.
//
// Replaces, for small molecules, the ~25-40 launches per SCF pass of the generic path (qc_api.cpp roothaan_enqueue + qc_linalg.hip, qc_eig_refine.hip):
// the body of the reference's loop between the Fock build and the convergence test (rhf.rs:70-88, uhf.rs:84-137), i.e.
//   pre    e = F D S - S D F (rhf.rs:71), DIIS over the sample window (diis.rs:28-59), F' = X^T F X (rhf.rs:74)
//   refine sorted_eigs(F') (rhf.rs:75, utils.rs:20-36) by Ogita-Aishima refinement from start vectors (previous pass / tridiagonal path)
//   post   C = X C' (rhf.rs:76), new density (rhf.rs:169-181), electronic energy and diagonal rms (rhf.rs:84-88)
// At n = 58 each of those launches is a 4-5 us latency kernel (16 tiles of 16 x 16, operands from L2) and the pass is bound by launch
// gaps.  Here four waves - one per SIMD of one CU, 512 registers each - own a 2 x 2 set of 16 x 16 tiles each.  A matrix is a 64 x 66
// block of LDS (34 KB; four of them in the CU's 160 KB) whose padding rows and columns are zeroed once and afterwards receive zeros only, so a
// product is 16 k-steps of four independent f64 MFMAs per wave fed by four ds_read_b64 with no bounds test anywhere (leading dimension
// 66 = 2 mod 4 doubles: the row-strided fragments hit distinct bank pairs), all operands requested before the first matrix
// instruction; phases are separated by s_barrier instead of kernel boundaries; whatever streams in from L2 (Fock / error matrices of the
// DIIS window, one-electron matrices) is requested sixteen elements per lane at a time.
// (Round 2's single-workgroup fusion lost because its tiles read their operands through the CU's L1 from global memory, DESIGN.md 3.3;
// a first LDS form with 16 waves of one tile each was no faster than the launches it replaced: 128 registers per lane serialise the
// loads; bounds tests as branches put a wait behind every load.)  All reductions have a fixed order: results are deterministic.
#include <atomic>
#include <cstddef>
#include <type_traits>

#include "qc_internal.h"
#include "qc_refine_rule.h"

typedef double qcs_d4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QCS_T = 256, QCS_W = QCS_T / 64, QCS_E = 16;           // threads, waves, matrix elements per thread (rows rr + 4 q)
constexpr int QCS_LD = 66, QCS_BUF = 64 * QCS_LD;                    // leading dimension and doubles of a matrix buffer
constexpr int QCS_SMALL_DOUBLES = 64 /*lam*/ + QCS_W * 12 /*red*/ + 12 /*dots*/ + 12 /*c*/ + 144 /*B*/ + 8 /*scalars*/ + 12 * 16 /*wave sums of the generic-order dots*/;
constexpr int QCS_SMALL_INTS = 64 /*partner*/ + 64 /*rank*/ + 16 /*flags*/;

__device__ __forceinline__ double qcs_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int qcs_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// A uniform / per-lane integer as a value the compiler knows nothing about.  Tests against n and the column index are loop invariants;
// hoisted out of the refinement loop and shared between products they are some hundred lane masks that do not fit the scalar registers
// and come back from the lanes of a vector register two v_readlane each.  A phase, a refinement pass and a product each start from a
// fresh copy, so their tests are formed where they are used (a scalar compare in front of a branch, a v_cmp in front of a select).
__device__ __forceinline__ int qcs_fresh(int v) { asm volatile("" : "+s"(v)); return v; }
__device__ __forceinline__ int qcs_fresh_v(int v) { asm volatile("" : "+v"(v)); return v; }

// A field of the launch's arguments, read from the kernarg segment where it is used.  QcSmallArgs is 128 dwords, more than a wave has
// scalar registers: taken as the kernel's parameter it is loaded whole at the top, and what of it stays live competes with the lane
// masks of the element loops for the scalar registers.  The offset goes through an empty asm statement, so the load cannot be hoisted
// to the top (nor merged with another read of the same field: a phase reads what it needs once, where it starts).
template <typename T>
__device__ __forceinline__ T qcs_karg(unsigned off) {
    asm volatile("" : "+s"(off));
    typedef const __attribute__((address_space(4))) char *kptr;
    return *(const __attribute__((address_space(4))) T *)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + off);
}
#define QCS_A(f) qcs_karg<decltype(QcSmallArgs::f)>((unsigned)offsetof(QcSmallArgs, f))
#define QCS_AI(f, i) qcs_karg<std::remove_extent_t<decltype(QcSmallArgs::f)>>((unsigned)(offsetof(QcSmallArgs, f) + sizeof(QcSmallArgs::f[0]) * (i)))
// element `off` bytes behind a uniform base: the scalar-base form of a global load / store, no 64-bit address per element.  The offset
// is made opaque HERE: its zero extension then stands in the block of the access, where instruction selection can fold it into the
// scalar-base form; extended where the offsets are formed (another block) every access got a v_lshl_add_u64 and a register pair.
__device__ __forceinline__ double qcs_ld(const double *base, unsigned off) { off = qcs_fresh_v(off); return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + off); }
__device__ __forceinline__ void qcs_st(double *base, unsigned off, double v) { off = qcs_fresh_v(off); *reinterpret_cast<double *>(reinterpret_cast<char *>(base) + off) = v; }

// C = alpha op(A) op(B) on the zero-padded 64 x 66 blocks.  QUAD (n > 32): wave w owns the tiles (w >> 1) + 2 a, (w & 1) + 2 b, a, b in
// {0, 1} - the partial edge tiles of a 58 x 58 matrix are spread evenly - and runs all 16 k-steps; otherwise (n <= 32) one tile per wave, 8
// k-steps.  `ks` limits the k-steps (density: only the occupied columns, KMASK).  Padding operands are zeros, padding results are stored as zeros.
// Lane maps of v_mfma_f64_16x16x4 as in qc_gemm_tile (qc_linalg.hip); the k-steps of a tile run in ascending order, so an element is the
// same chain of fused multiply-adds as there.  C must not alias A or B; the caller separates phases by barriers.
template <bool TA, bool TB, bool QUAD, bool KMASK>
__device__ __forceinline__ void qcs_gemm_t(const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ C, int n, int ks,
                                           int kdim, double alpha) {
    constexpr int NT = QUAD ? 2 : 1, NK = QUAD ? 16 : 8, ld = QCS_LD;
    n = qcs_fresh(n); ks = qcs_fresh(ks);
    if constexpr (!KMASK) __builtin_assume(QUAD ? (ks > NK / 2 && ks <= NK) : (ks >= 1 && ks <= NK));     // (kdim = n, and n > 32 with 2 x 2 tiles)
    const int wave = qcs_wave(), lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    const int r0 = (wave >> 1) * 16, c0 = (wave & 1) * 16;
    const int a_s = TA ? 1 : ld, a_k = TA ? ld : 1, b_s = TB ? ld : 1, b_k = TB ? 1 : ld;
    double av[NT][NK], bv[NT][NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const int kk = 4 * s + lk;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            av[t][s] = A[(r0 + 32 * t + li) * a_s + kk * a_k];
            bv[t][s] = B[(c0 + 32 * t + li) * b_s + kk * b_k];
            if constexpr (KMASK) { if (kk >= kdim) { av[t][s] = 0.0; bv[t][s] = 0.0; } }      // (inner range ends inside the matrix)
        }
    }
    qcs_d4 acc[NT][NT];
#pragma unroll
    for (int x = 0; x < NT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y) acc[x][y] = qcs_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        if (s < ks) {                                      // (uniform, scalar)
#pragma unroll
            for (int x = 0; x < NT; ++x)
#pragma unroll
                for (int y = 0; y < NT; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x][s], bv[y][s], acc[x][y], 0, 0, 0);
        }
    }
#pragma unroll
    for (int x = 0; x < NT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y) {
            const int col = c0 + 32 * y + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {                  // (the padding of C is zero and gets zeros: a select, no lane mask per store)
                const int row = r0 + 32 * x + lk + 4 * r;
                C[row * ld + col] = (row < n && col < n) ? alpha * acc[x][y][r] : 0.0;
            }
        }
}
// KMASK: kdim < n (the density, C_occ C_occ^T): operands past kdim are not padding and are masked
template <bool QUAD, bool TA, bool TB, bool KMASK = false>
__device__ __forceinline__ void qcs_gemm(const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ C, int n, int kdim,
                                         double alpha) {
    const int ks = (kdim + 3) >> 2;
    qcs_gemm_t<TA, TB, QUAD, KMASK>(A, B, C, n, ks, kdim, alpha);
}

// sum over the workgroup of NV values per thread, fixed order: lanes by shuffles, waves by thread j (nv <= NV of them are wanted)
template <int NV>
__device__ __forceinline__ void qcs_block_sums(const double (&v)[NV], int nv, double *red, double *out) {
    const int wave = qcs_wave(), lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (j < nv) {                                      // (uniform)
            double s = v[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) red[wave * 12 + j] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < QCS_W; ++k) t += red[k * 12 + threadIdx.x];
        out[threadIdx.x] = t;
    }
    __syncthreads();
}

// DIIS coefficients (diis.rs:40-51): the M x M system [B 1; 1 0] c = (0, ..., 0, 1), M = window + 1, by Householder QR in the order of
// operations of nalgebra's qr().solve() (qc_qr_solve_reg, qc_linalg.hip), by ONE wave with the matrix in registers: lane j holds column j
// (lane M the right-hand side), the pivot column travels by v_readlane.  Returns false when a pivot vanishes ("DIIS failed").
template <int M>
__device__ __forceinline__ bool qcs_qr_solve(double (&col)[13], int lane, double (&x)[13]) {
    bool fail = false;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if (!fail) {                                       // (uniform)
            double vk[M];
            double norm = 0.0;
#pragma unroll
            for (int i = k; i < M; ++i) { vk[i] = qcs_readlane(col[i], k); norm += vk[i] * vk[i]; }
            norm = sqrt(norm);
            if (norm == 0.0) fail = true;
            else {
                const double alpha = vk[k] > 0 ? -norm : norm;
                vk[k] -= alpha;
                double vn = 0.0;
#pragma unroll
                for (int i = k; i < M; ++i) vn += vk[i] * vk[i];
                if (vn > 0.0 && lane >= k) {               // columns k .. M-1 and the right-hand side
                    double d = 0.0;
#pragma unroll
                    for (int i = k; i < M; ++i) d += vk[i] * col[i];
                    d *= 2.0 / vn;
#pragma unroll
                    for (int i = k; i < M; ++i) col[i] -= d * vk[i];
                }
            }
        }
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        x[i] = 0.0;
        if (!fail) {                                       // (uniform)
            double s = qcs_readlane(col[i], M);
#pragma unroll
            for (int j = i + 1; j < M; ++j) s -= qcs_readlane(col[i], j) * x[j];
            const double piv = qcs_readlane(col[i], i);
            if (piv == 0.0) fail = true;
            else x[i] = s / piv;
        }
    }
    return !fail;
}

}  // namespace

// Block plan (a block is free once the barrier behind its last reader has passed):
//   pre     B0: F, (F D) S, F_diis, then V0    B1: D, F X    B2: S, then X = S^-1/2    B3: F D, (flat e), F' = X^T F_diis X
//   refine  B0 / B2: the vectors and their update in turn (X^T A X where the update will go)    B3: F'
//           B1: A X, X^T X, I + E, at the end X = S^-1/2 for post
//   post    B1: X = S^-1/2    C = X C' in whichever of B0 / B2 C' is not in    B3: the density
// One instance per shape (QUAD: n > 32, 2 x 2 tiles per wave) and per set of phases PH (1 pre, 2 refine, 4 post) that a launch runs: an
// instance holds only the products and branches of its launch.  The arguments are read through QCS_A / QCS_AI, never through `a`.
template <bool QUAD, int PH>
__global__ __launch_bounds__(QCS_T) void qc_scf_small_kernel(const QcSmallArgs a) {
    extern __shared__ double lds[];
    constexpr int ld = QCS_LD, BUF = QCS_BUF;
    {   // every cache line of the argument block is requested once, together, before the first field is read: the reads at the use sites
        // then hit the scalar cache instead of paying the block's memory latency one line after the other
        int t0, t1, t2, t3, t4, t5, t6, t7, t8;
        static_assert(sizeof(QcSmallArgs) == 512, "one request per 64-byte line of QcSmallArgs");
        asm volatile("s_load_dword %0, %9, 0x0\n\ts_load_dword %1, %9, 0x40\n\ts_load_dword %2, %9, 0x80\n\ts_load_dword %3, %9, 0xc0\n\t"
                     "s_load_dword %4, %9, 0x100\n\ts_load_dword %5, %9, 0x140\n\ts_load_dword %6, %9, 0x180\n\ts_load_dword %7, %9, 0x1c0\n\t"
                     "s_load_dword %8, %9, 0x1fc\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(t6), "=&s"(t7), "=&s"(t8)
                     : "s"(__builtin_amdgcn_kernarg_segment_ptr()));
    }
    const int n0 = QCS_A(n);
    double *B0 = lds, *B1 = lds + BUF, *B2 = lds + 2 * BUF, *B3 = lds + 3 * BUF;
    double *sm = lds + 4 * BUF;
    double *lam = sm, *red = lam + 64, *dots = red + QCS_W * 12, *cvec = dots + 12, *Bl = cvec + 12, *scal = Bl + 144, *gsh = scal + 8;
    int *partner = reinterpret_cast<int *>(gsh + 12 * 16), *rank_s = partner + 64, *flg = rank_s + 64;
    const int tid0 = threadIdx.x, rr0 = qcs_wave(), cc0 = tid0 & 63;     // this thread's elements: rows rr + 4 q (uniform in a wave), column cc
    // n, tid, rr, cc and the column test of a scope (qcs_fresh); the launcher guarantees the instance's range of n
#define QCS_FRESH() const int n = qcs_fresh(n0), tid = qcs_fresh_v(tid0), rr = qcs_fresh(rr0), cc = qcs_fresh_v(cc0); \
                    __builtin_assume(tid >= 0 && tid < QCS_T); \
                    __builtin_assume(QUAD ? (n > 32 && n <= 64) : (n >= 1 && n <= 32)); __builtin_assume(rr >= 0 && rr < QCS_W); \
                    __builtin_assume(cc >= 0 && cc < 64); const bool cok = cc < n; \
                    const int nq = qcs_fresh_v(cok ? (n - rr + QCS_W - 1) / QCS_W : 0); (void)nq   /* this thread's elements inside the matrix: q < nq */
    QCS_FRESH();
    { unsigned long long *const tl = QCS_A(tl); if (tl != nullptr && tid == 0) tl[0] = wall_clock64(); }
    bool ok = true;                                                      // (uniform) the eigenvectors for `post` exist
    double *Cpv = B0;                                                    // ... and the block they are in
#ifdef QC_SMALL_TIMING
    long long tph[40] = {}; int nph = 0;
#define QCS_STAMP() do { if (tid == 0 && nph < 40) tph[nph++] = wall_clock64(); } while (0)
    QCS_STAMP();
#else
#define QCS_STAMP() do {} while (0)
#endif
    // element loops: all of a thread's loads are requested before the first use; out-of-range elements read element 0 and are not stored
    // to global memory.  A row is in range for a whole wave or not at all (scalar branch), a column for a lane: global stores of a loop
    // stand under ONE lane mask (QCS_PUT), stores to the padded blocks of LDS under none - the padding is zero and gets zeros (QCS_PUTL).
#define QCS_EACH(q, i) _Pragma("unroll") for (int q = 0, i = rr; q < QCS_E; ++q, i += QCS_W)
#define QCS_IN(i) (q < nq)                                               // (inside QCS_EACH(q, i) only) cok && i < n as ONE vector compare
#define QCS_GX(i) (gx[q])                                                // (inside QCS_EACH(q, i) only: byte offset of element (i, cc))
#define QCS_GET(p) qcs_ld(p, gx[q])                                      // (likewise) element (i, cc) of the n x n matrix p in global memory
#define QCS_PUT(p, v) do { if (cok) QCS_EACH(q, i) if (i < n) qcs_st(p, gx[q], v); } while (0)
#define QCS_PUTL(B, v) QCS_EACH(q, i) (B)[i * ld + cc] = QCS_IN(i) ? (v) : 0.0
    // the sixteen byte offsets are formed once: re-formed at every load (two tests, a multiplication and a select each) they cost the phases
    // that stream matrices from L2 more than the loads themselves
    unsigned gx[QCS_E];
    QCS_EACH(q, i) gx[q] = QCS_IN(i) ? (unsigned)(i * n + cc) * 8u : 0u;

    // The padding of the four blocks (rows and columns >= n) and lam are zero for the whole kernel: products run over 64 x 64 without
    // bounds tests, and nothing stores anything but zeros there (but for the flat copy of the error matrix that the generic-order dots lay
    // over B3, which is zeroed whole behind them).  The interior is not zeroed: every element of it is written before it is read.  Runs
    // once, in whichever phase comes first, between that phase's requests to L2 and its stores to LDS (the barrier after those covers it).
    auto zero_padding = [&]() {
        for (int b = 0; b < 4; ++b) {
            double *Bk = lds + b * BUF;
            for (int x = n * ld + tid; x < BUF; x += QCS_T) Bk[x] = 0.0;                         // rows n .. 63
            if (cok) for (int c = n + rr; c < ld; c += QCS_W) Bk[cc * ld + c] = 0.0;             // columns n .. 65 of row cc < n
        }
        if (tid < 64) { lam[tid] = 0.0; partner[tid] = -1; }
    };

    if (PH & 1) {
        QCS_FRESH();
        const int m = QCS_A(m);                                          // (uniform) the DIIS window
        // ---- e = F D S - S D F
        {
            double f[QCS_E], d[QCS_E], s[QCS_E], g[QCS_E];
            const double *const aF = QCS_A(F);
            const bool haveF = aF != nullptr;                            // (uniform)
            {
                const double *__restrict__ fsrc = haveF ? aF : QCS_A(H), *__restrict__ aD = QCS_A(D), *__restrict__ aS = QCS_A(S), *__restrict__ aG = QCS_A(G);
                QCS_EACH(q, i) {
                    f[q] = QCS_GET(fsrc); d[q] = QCS_GET(aD); s[q] = QCS_GET(aS);
                    g[q] = haveF ? 0.0 : QCS_GET(aG);
                }
            }
            const int ML = QCS_A(maxlen);
            const bool hasB = tid < ML * ML;
            const double bl = QCS_A(Bmat)[hasB ? tid : 0];
            zero_padding();
            if (hasB) Bl[tid] = bl;
            if (!haveF) {
                QCS_EACH(q, i) f[q] = 1.0 * f[q] + 1.0 * g[q];           // the arithmetic of qc_axpby(1, H, 1, G)
                double *const aFo = QCS_A(F_out);
                QCS_PUT(aFo, f[q]);
            }
            QCS_PUTL(B0, f[q]); QCS_PUTL(B1, d[q]); QCS_PUTL(B2, s[q]);
        }
        __syncthreads();
        QCS_STAMP();
        qcs_gemm<QUAD, false, false>(B0, B1, B3, n, n, 1.0);                   // F D
        __syncthreads();
        QCS_STAMP();
        qcs_gemm<QUAD, false, false>(B3, B2, B0, n, n, 1.0);                   // (F D) S
        __syncthreads();
        QCS_STAMP();
        {
            double e[QCS_E], part[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) part[j] = 0.0;
            QCS_EACH(q, i) {
                const int ic = min(i, 63);
                e[q] = B0[ic * ld + cc] - B0[cc * ld + ic];              // FDS - (FDS)^T = FDS - SDF (zero in the padding)
                part[0] = fma(e[q], e[q], part[0]);
            }
            { double *const aE = QCS_A(E_out); QCS_PUT(aE, e[q]); }
            // <e_0, e_j>, diis.rs:43-45: the older error matrices three at a time (48 loads in flight)
#pragma unroll
            for (int j0 = 1; j0 < 12; j0 += 3) {
                if (j0 < m) {                                            // (uniform)
                    double o[3][QCS_E];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const double *__restrict__ src = QCS_AI(errs, j0 + u < m ? j0 + u : 0);  // (past the window: any valid matrix, weight 0)
                        QCS_EACH(q, i) o[u][q] = QCS_GET(src);
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        constexpr int JMAX = 11;
                        const int j = j0 + u < JMAX ? j0 + u : JMAX;
                        const double w = j0 + u < m ? 1.0 : 0.0;
                        QCS_EACH(q, i) part[j] = fma(e[q] * w, o[u][q], part[j]);                // (e is zero outside the matrix)
                    }
                }
            }
            qcs_block_sums<12>(part, m, red, dots);
            if (QCS_A(dots_generic)) {
                // Open-shell runs: the dot products in the summation order of the generic launch sequence (qc_dots_kernel, qc_linalg.hip: 1024
                // threads, thread t sums the elements t + 1024 u in ascending u, lanes by the shuffle tree, the sixteen wave sums in
                // order).  The trajectories of such runs - crawls along saddles of the UHF functional, DESIGN.md 1 - depend on the last bit
                // of these numbers, and the one that is pinned against the oracle is the generic sequence's.  The error matrix goes to a flat
                // copy in B3 (free between the two products around here), the 1024 virtual threads are served in four rounds.
                const int nn = n * n;
                QCS_EACH(q, i) if (QCS_IN(i)) B3[i * n + cc] = e[q];
                __syncthreads();
                const int wave = qcs_wave(), lane = tid & 63;
                for (int j = 0; j < m; ++j) {
                    const double *__restrict__ yj = QCS_AI(errs, j);
                    for (int r = 0; r < 4; ++r) {
                        const int t = r * QCS_T + tid;
                        double av[4], bv[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) { const int x = min(t + u * 1024, nn - 1); av[u] = B3[x]; bv[u] = j == 0 ? B3[x] : yj[x]; }
                        double sgen = 0.0;
#pragma unroll
                        for (int u = 0; u < 4; ++u) if (t + u * 1024 < nn) sgen = fma(av[u], bv[u], sgen);
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) sgen += __shfl_down(sgen, o, 64);
                        if (lane == 0) gsh[j * 16 + r * QCS_W + wave] = sgen;
                    }
                }
                __syncthreads();
                if (tid < m) {
                    double tsum = 0.0;
                    for (int k = 0; k < 16; ++k) tsum += gsh[tid * 16 + k];
                    dots[tid] = tsum;
                }
                for (int x = tid; x < BUF; x += QCS_T) B3[x] = 0.0;      // (the block's padding is zero for the rest of the kernel)
                __syncthreads();
            }
        }
        QCS_STAMP();
        // ---- DIIS coefficients by wave 0; the other three waves fetch X meanwhile.  The first three Fock matrices of the combination are
        // requested before the solve (they do not depend on it) and arrive while it runs.
        double fo0[3][QCS_E];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const double *__restrict__ src = QCS_AI(focks, u < m ? u : 0);
            QCS_EACH(q, i) fo0[u][q] = QCS_GET(src);
        }
        if (qcs_wave() == 0) {
            const int lane = tid, M = m + 1, ML = QCS_A(maxlen);
            int sl[12], myslot = 0;                                      // the window's slots, live in this block only; lane j's own
#pragma unroll
            for (int j = 0; j < 12; ++j) { sl[j] = QCS_AI(slot, j); myslot = lane == j ? sl[j] : myslot; }
            const int slot0 = sl[0];
            if (lane < m) {
                const double d = dots[lane];
                const int p = slot0 * ML + myslot, q = myslot * ML + slot0;
                double *const aB = QCS_A(Bmat);
                Bl[p] = d; Bl[q] = d; aB[p] = d; aB[q] = d;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double cj = lane == 0 ? 1.0 : 0.0;                           // diis.rs:33-38: the newest Fock matrix while the window is short
            if (m >= QCS_A(minlen)) {
                double col[13], x[13];
#pragma unroll
                for (int i = 0; i < 13; ++i) {
                    double v = 0.0;
                    if (i < M && lane <= M) {
                        if (lane == M) v = i == m ? 1.0 : 0.0;                                   // right-hand side
                        else if (i < m && lane < m) v = Bl[sl[i < 12 ? i : 0] * ML + myslot];
                        else v = (i == m && lane == m) ? 0.0 : 1.0;                              // border +1, corner 0
                    }
                    col[i] = v;
                    x[i] = 0.0;
                }
                bool solved = false;
                switch (M) {
#define QCS_QR(MM) case MM: solved = qcs_qr_solve<MM>(col, lane, x); break;
                    QCS_QR(2) QCS_QR(3) QCS_QR(4) QCS_QR(5) QCS_QR(6) QCS_QR(7) QCS_QR(8) QCS_QR(9) QCS_QR(10) QCS_QR(11) QCS_QR(12) QCS_QR(13)
#undef QCS_QR
                    default: break;
                }
                if (!solved) { if (lane == 0) *QCS_A(diis_flag) = 1; }        // "DIIS failed" (rhf.rs:73); c stays (1, 0, ...)
                else {
                    cj = 0.0;
#pragma unroll
                    for (int j = 0; j < 12; ++j) if (lane == j && j < m) cj = x[j];
                }
            }
            if (lane < 12) { cvec[lane] = cj; QCS_A(c_out)[lane] = cj; }
        } else {
            const int w3 = qcs_wave() - 1;                               // rows w3 + 3 q
            const double *__restrict__ aX = QCS_A(X);
            double xr[22];
#pragma unroll
            for (int q = 0; q < 22; ++q) { const int i = w3 + 3 * q; xr[q] = qcs_ld(aX, (cok && i < n) ? (unsigned)(i * n + cc) * 8u : 0u); }
#pragma unroll
            for (int q = 0; q < 22; ++q) { const int i = w3 + 3 * q; if (i < n) B2[i * ld + cc] = cok ? xr[q] : 0.0; }     // (uniform test; rows past 63 are outside the block)
        }
        __syncthreads();
        QCS_STAMP();
        // ---- F_diis = sum_j c_j F_j (diis.rs:52-58), three Fock matrices at a time; F' = X^T F_diis X
        {
            double acc[QCS_E];
            QCS_EACH(q, i) acc[q] = 0.0;
#pragma unroll
            for (int j0 = 0; j0 < 12; j0 += 3) {
                if (j0 < m) {                                            // (uniform)
                    double o[3][QCS_E];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        if (j0 == 0) { QCS_EACH(q, i) o[u][q] = fo0[u][q]; }
                        else {
                            const double *__restrict__ src = QCS_AI(focks, j0 + u < m ? j0 + u : 0);
                            QCS_EACH(q, i) o[u][q] = QCS_GET(src);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        if (j0 + u < m) {                                // (uniform)
                            const double c = cvec[j0 + u];
                            QCS_EACH(q, i) acc[q] = fma(c, o[u][q], acc[q]);
                        }
                    }
                }
            }
            QCS_PUTL(B0, acc[q]);
        }
        __syncthreads();
        QCS_STAMP();
        // the refinement's start vectors are requested ahead of the product that hides them and go to B0 once that product has read it
        constexpr bool refine = (PH & 2) != 0;
        double v0[QCS_E];
        if (refine) { const double *__restrict__ aV = QCS_A(V0); QCS_EACH(q, i) v0[q] = QCS_GET(aV); }
        qcs_gemm<QUAD, false, false>(B0, B2, B1, n, n, 1.0);                   // F X
        __syncthreads();
        QCS_STAMP();
        if (refine) {
            QCS_PUTL(B0, v0[q]);
            if (tid < QC_CTL_EIG_STRIDE) flg[tid] = 0;
        }
        qcs_gemm<QUAD, true, false>(B2, B1, B3, n, n, 1.0);                    // X^T (F X)
        __syncthreads();
        QCS_STAMP();
        { double *const aFp = QCS_A(Fp); QCS_PUT(aFp, B3[i * ld + cc]); }
    }

    if (PH & 2) {
        // ---- eigenvectors of F' (B3) by refinement from V0: the passes of qc_eig_refine_async (qc_eig_refine.hip) back to back
        // (after `pre` in the same launch everything is in place: V0 in B0, F' in B3, the flags cleared, and X = S^-1/2 still in B2)
        QCS_FRESH();
        constexpr bool post = (PH & 4) != 0;
        double xpost[QCS_E];                                             // X of this thread's elements for `post`, held across the refinement
        if (!(PH & 1)) {
            double v[QCS_E], f[QCS_E];
            const double *__restrict__ aV = QCS_A(V0), *__restrict__ aFp = QCS_A(Fp), *__restrict__ aX = QCS_A(X);
            QCS_EACH(q, i) { v[q] = QCS_GET(aV); f[q] = QCS_GET(aFp); xpost[q] = post ? QCS_GET(aX) : 0.0; }
            zero_padding();
            QCS_PUTL(B0, v[q]); QCS_PUTL(B3, f[q]);
            if (tid < QC_CTL_EIG_STRIDE) flg[tid] = 0;
            __syncthreads();
        } else QCS_EACH(q, i) xpost[q] = B2[min(i, 63) * ld + cc];
        QCS_STAMP();
        int state = QC_EIG_RUNNING, last = 0, clean = 0;                 // (uniform) the decisions of a pass: every thread takes them, thread 0 files them in flg
        double *X = B0, *Xn = B2;
        const int npass = QCS_A(npass);
        for (int pass = 0; pass < npass; ++pass) {
            QCS_FRESH();
            qcs_gemm<QUAD, false, false>(B3, X, B1, n, n, 1.0);                // A X
            __syncthreads();
            qcs_gemm<QUAD, true, false>(X, B1, Xn, n, n, 1.0);                 // S = X^T A X
            __syncthreads();
            qcs_gemm<QUAD, true, false>(X, X, B1, n, n, 1.0);                  // X^T X
            __syncthreads();
            QCS_STAMP();
            const double *Sm = Xn, *XtX = B1;
            // statistics and decisions by the rule of qc_refine_rule.h; everything reads the zero padding instead of testing bounds
            // Two barriers: wave results go to red (slot 1 ||R||^2, 2 max |lam|, 3 max coupling left in degenerate pairs) and every thread
            // combines them for itself, waves in ascending order - no thread waits for a single one.
            const int wave = qcs_wave(), lane = tid & 63;
            {
                double rsum = 0.0;
                QCS_EACH(q, i) {
                    const int ic = min(i, 63);
                    const double r = ((i < n ? i : -1) == cc ? 1.0 : 0.0) - XtX[ic * ld + cc];     // (the diagonal inside the matrix)
                    rsum = fma(r, r, rsum);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) rsum += __shfl_down(rsum, o, 64);
                if (lane == 0) red[wave * 12 + 1] = rsum;
                if (wave == 0) {                                         // the Rayleigh quotients: one division per lane (a maximum has no order)
                    double amax = 0.0;
                    if (cok) { const double l = qc_ref_quotient(Sm[cc * ld + cc], 1.0 - XtX[cc * ld + cc]); lam[cc] = l; amax = fmax(amax, fabs(l)); }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_down(amax, o, 64));
                    if (lane == 0) red[2] = amax;
                }
                if (tid == 0) { flg[4] = 0; flg[5] = 0; flg[6] = 0; flg[7] = 0; }      // multi, nstrong, big update, not the last update
                __syncthreads();
            }
            double rr2 = 0.0;                                            // ||R||^2
#pragma unroll
            for (int k = 0; k < QCS_W; ++k) rr2 += red[k * 12 + 1];
            const double scale = red[2];                                 // max |lam|
            const double tiny = QC_REF_TINY * scale, gfloor = QC_REF_GFLOOR * scale;
            {
                double cmax = 0.0;
                int big = 0, notlast = 0;                                // some regular pair has |a| > QC_REF_BIG g / > QC_REF_LAST g (update size, no division)
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) {                         // one row per team of 16 lanes
                    const int i = (tid >> 4) + 16 * ii;
                    int cnt = 0, who = -1;
                    const double li_ = lam[i];                           // (zero past n: such rows find av = 0 everywhere)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int j = (tid & 15) + 16 * jj;
                        const double lj = lam[j];
                        const double r = -XtX[i * ld + j];
                        const double sij = 0.5 * (Sm[i * ld + j] + Sm[j * ld + i]);
                        const double av = fabs(QC_REF_COUPLING(sij, li_, lj, r)), g = fabs(lj - li_);
                        const bool valid = j != i && qc_ref_coupled(av, tiny);       // the class tests as selects
                        const bool strong = valid && qc_ref_strong(av, g, gfloor);
                        cnt += strong ? 1 : 0;
                        who = strong ? j : who;
                        const bool weak = valid && !strong;
                        cmax = (weak && qc_ref_degenerate(g, gfloor)) ? fmax(cmax, av) : cmax;
                        const bool reg = weak && qc_ref_regular(g, gfloor);
                        big |= (reg && qc_ref_pair_big(av, g)) ? 1 : 0;
                        notlast |= (reg && qc_ref_pair_notlast(av, g)) ? 1 : 0;
                    }
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 16); who = max(who, __shfl_xor(who, o, 16)); }
                    if ((tid & 15) == 0 && i < n) {
                        partner[i] = qc_ref_partner(cnt, who);
                        if (cnt > 1) flg[4] = 1;
                        if (cnt == 1) atomicAdd(&flg[5], 1);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) cmax = fmax(cmax, __shfl_down(cmax, o, 64));
                if (big) flg[6] = 1;
                if (notlast) flg[7] = 1;
                if (lane == 0) red[wave * 12 + 3] = cmax;
                __syncthreads();
                // (n <= 64: the lanes of every wave cover the indices, so each wave finds the non-mutual pairs for itself)
                const bool notmutual = lane < n && qc_ref_not_mutual(partner, lane);
                const int multi = (flg[4] != 0 || __ballot(notmutual) != 0) ? 1 : 0;
                double ca = 0.0;
#pragma unroll
                for (int k = 0; k < QCS_W; ++k) ca = fmax(ca, red[k * 12 + 3]);
                const double orth = sqrt(rr2), scl = fmax(scale, QC_REF_SCALE_FLOOR);
                if (QC_REF_ROTATE(flg[6], orth, multi)) state = QC_EIG_ROTATE;
                else {
                    last = QC_REF_IS_LAST(flg[7], orth, flg[5]) ? 1 : 0;
                    clean = QC_REF_IS_CLEAN(ca, scl) ? 1 : 0;
                }
                if (tid == 0) {
                    if (state == QC_EIG_ROTATE) flg[QC_EIG_STATE] = QC_EIG_ROTATE;
                    else { flg[QC_EIG_LAST] = last; flg[QC_EIG_CLEAN] = clean; }
                }
                state = __builtin_amdgcn_readfirstlane(state); last = __builtin_amdgcn_readfirstlane(last); clean = __builtin_amdgcn_readfirstlane(clean);
            }
            QCS_STAMP();
            if (state != QC_EIG_RUNNING) break;
            // M = I + E with exact rotations on the strong pairs, into B1 in place of X^T X
            {
                QCS_FRESH();
                double mv[QCS_E];
                const double lj = lam[cc];
                QCS_EACH(q, i) {
                    const int ic = min(i, 63), j = cc;
                    const double li_ = lam[ic], xij = XtX[ic * ld + j];
                    const double sij = 0.5 * (Sm[ic * ld + j] + Sm[j * ld + ic]);
                    const double r = (ic == j ? 1.0 : 0.0) - xij;
                    const double av = QC_REF_COUPLING(sij, li_, lj, r), g = lj - li_;
                    const int pi_ = partner[ic];
                    double mm = QC_REF_M_WEAK(sij, r, lj, av, g, tiny, gfloor);
                    if (ic == j) mm = qc_ref_m_diag(r);
                    if (pi_ >= 0 && (pi_ == j || ic == j)) {             // this index rotates with its strong partner
                        const double avp = ic == j ? QC_REF_COUPLING(0.5 * (Sm[ic * ld + pi_] + Sm[pi_ * ld + ic]), li_, lam[pi_], -XtX[ic * ld + pi_]) : av;
                        const double gp = ic == j ? lam[pi_] - li_ : g;
                        mm = ic == j ? qc_ref_m_diag_rot(r, avp, gp) : qc_ref_m_rot(avp, gp);
                    }
                    mv[q] = mm;
                }
                __syncthreads();
                QCS_PUTL(B1, mv[q]);
            }
            __syncthreads();
            QCS_STAMP();
            qcs_gemm<QUAD, false, false>(X, B1, Xn, n, n, 1.0);                // X (I + E): error now ~ emax^2
            __syncthreads();
            QCS_STAMP();
            if (tid == 0) flg[QC_EIG_PASSES] += 1;                                   // passes used
            if (last && clean) {                                         // final vectors: ascending eigenvalues, columns alongside
                {   // the rank of index tid / 4 is a count: four threads take sixteen candidates each
                    const int idx = tid >> 2, j0 = 16 * (tid & 3);
                    const double wi = lam[idx];
                    int r = 0;
                    for (int j = j0; j < j0 + 16; ++j) r += (j < n && QC_REF_BEFORE(lam, j, wi, idx)) ? 1 : 0;
                    r += __shfl_xor(r, 1, 64);
                    r += __shfl_xor(r, 2, 64);
                    if ((tid & 3) == 0 && idx < n) { rank_s[idx] = r; QCS_A(w_out)[r] = wi; }
                }
                __syncthreads();
                const int rc = cok ? rank_s[cc] : 0;
                if (cok) QCS_EACH(q, i) if (i < n) X[i * ld + rc] = Xn[i * ld + cc];
                state = QC_EIG_DONE;
                break;
            }
            if (last || pass == npass - 1) { state = QC_EIG_ROTATE; break; }      // coupling inside a degenerate cluster, or passes exhausted
            double *t = X; X = Xn; Xn = t;
        }
        ok = state == QC_EIG_DONE;
        if (tid == 0) flg[QC_EIG_STATE] = state;
        __syncthreads();
        if (tid < QC_CTL_EIG_STRIDE) QCS_A(ctl)[tid] = flg[tid];
        if (ok) {
            { double *const aCp = QCS_A(Cp_out); QCS_PUT(aCp, X[i * ld + cc]); }
            Cpv = X;
            if (post) QCS_PUTL(B1, xpost[q]);                             // X = S^-1/2 for C = X C' (B1 is free once the last update is formed)
        }
        __syncthreads();
        QCS_STAMP();
    }

    if ((PH & 4) && ok) {
        QCS_FRESH();
        // ---- C = X C', D = dfac C_occ C_occ^T, energy, rms
        double h[QCS_E], g[QCS_E];                                       // H and G of this thread's elements: requested now, used at the end
        double dold = 0.0;
        const double *__restrict__ aH = QCS_A(H), *__restrict__ aG = QCS_A(G);
        if (!(PH & 2)) {                                                 // (after the refinement in the same launch X is in B1 already)
            double xv[QCS_E], cp[QCS_E];
            const double *__restrict__ aX = QCS_A(X), *__restrict__ aCi = QCS_A(Cp_in);
            QCS_EACH(q, i) { xv[q] = QCS_GET(aX); cp[q] = QCS_GET(aCi); }
            QCS_EACH(q, i) { h[q] = QCS_GET(aH); g[q] = QCS_GET(aG); }
            dold = QCS_A(Dold)[tid < n ? tid * n + tid : 0];
            zero_padding();
            QCS_PUTL(B1, xv[q]); QCS_PUTL(B0, cp[q]);
            __syncthreads();
        } else {
            QCS_EACH(q, i) { h[q] = QCS_GET(aH); g[q] = QCS_GET(aG); }
            dold = QCS_A(Dold)[tid < n ? tid * n + tid : 0];
        }
        QCS_STAMP();
        double *const Cm = Cpv == B2 ? B0 : B2;                          // (the block the eigenvectors are not in)
        qcs_gemm<QUAD, false, false>(B1, Cpv, Cm, n, n, 1.0);                  // C
        __syncthreads();
        const int nocc = QCS_A(nocc);
        if (nocc > 0) qcs_gemm<QUAD, false, true, true>(Cm, Cm, B3, n, nocc, QCS_A(dfac));        // C_occ C_occ^T
        else QCS_PUTL(B3, 0.0);
        { double *const aC = QCS_A(C_out); QCS_PUT(aC, Cm[i * ld + cc]); }
        __syncthreads();
        QCS_STAMP();
        double part[3] = {0.0, 0.0, 0.0};
        QCS_EACH(q, i) {
            const int ic = min(i, 63);
            const double dn = B3[ic * ld + cc];                                                  // (zero in the padding)
            part[0] = fma(QCS_IN(i) ? B3[cc * ld + ic] : 0.0, 2.0 * h[q] + g[q], part[0]);      // tr(Dn (2H + G)) = sum_ij Dn_ji (2H + G)_ij
            part[2] += fabs(dn);
        }
        { double *const aDn = QCS_A(Dn); QCS_PUT(aDn, B3[i * ld + cc]); }
        if (tid < n) { const double d = B3[tid * ld + tid] - dold; part[1] = d * d; }
        qcs_block_sums<3>(part, 3, red, scal);
        if (tid == 0) {
            double *const aso = QCS_A(scal_out), *const fxs = QCS_A(fxs_out);
            aso[0] = 0.5 * scal[0]; aso[1] = scal[1];
            if (fxs) {     // fixed-point unit of the build that will digest Dn (qc_fx_scale_kernel, qc_linalg.hip): 2^S (4 imax sum|D|) <= 2^60
                const double bound = 4.0 * QCS_A(imax) * scal[2];
                int e = 0;
                if (bound > 0.0 && bound < 1e300) (void)frexp(bound, &e);
                else if (!(bound < 1e300)) e = 1100;
                int S = 60 - e;
                S = S > QC_FX_MAXBITS ? QC_FX_MAXBITS : (S < -900 ? -900 : S);
                fxs[0] = ldexp(1.0, S); fxs[1] = (bound < 1e300) ? ldexp(1.0, -S) : __builtin_nan("");
            }
        }
        QCS_STAMP();
    }
    if (int *const ctl_all = QCS_A(ctl_all)) {
        __threadfence();
        __syncthreads();
        if (tid < QC_CTL_WORDS) {
            int *p = ctl_all + tid;
            QCS_A(ctl_out)[tid] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __threadfence_system();
    { unsigned long long *const tl = QCS_A(tl); if (tl != nullptr && tid == 0) tl[1] = wall_clock64(); }
    if (unsigned *const seq_out = QCS_A(seq_out)) {     // the host polls this word instead of the stream's event (which the packet processor signals some microseconds later)
        __syncthreads();
        if (tid == 0) __hip_atomic_store(seq_out, QCS_A(seq), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#ifdef QC_SMALL_TIMING
    if (tid == 0) {
        printf("[small n=%d phases %d m %d] stamps (10 ns):", n, PH, QCS_A(m));
        for (int k = 1; k < nph; ++k) printf(" %lld", tph[k] - tph[k - 1]);
        printf("\n");
    }
#endif
#undef QCS_EACH
#undef QCS_IN
#undef QCS_GX
#undef QCS_GET
#undef QCS_PUT
#undef QCS_PUTL
#undef QCS_FRESH
#undef QCS_STAMP
}

size_t qc_scf_small_lds_bytes(int) { return (size_t)(4 * QCS_BUF + QCS_SMALL_DOUBLES) * sizeof(double) + QCS_SMALL_INTS * sizeof(int); }

int qc_scf_small_launch(hipStream_t st, const QcSmallArgs &a) {
    if (a.n < 1 || a.n > QC_SMALL_MAXN || a.m < 1 || a.m > 12) return QC_ERR_INVALID;
    // the instance of the launch's shape and phases; each needs its dynamic LDS raised once
    typedef void (*kernel_t)(const QcSmallArgs);
    static const struct { int phases; kernel_t k[2]; } table[] = {
        {1, {qc_scf_small_kernel<false, 1>, qc_scf_small_kernel<true, 1>}},       // pre (before the tridiagonal start or a Jacobi kernel)
        {4, {qc_scf_small_kernel<false, 4>, qc_scf_small_kernel<true, 4>}},       // post (behind a Jacobi kernel)
        {6, {qc_scf_small_kernel<false, 6>, qc_scf_small_kernel<true, 6>}},       // refine + post (behind the tridiagonal start)
        {7, {qc_scf_small_kernel<false, 7>, qc_scf_small_kernel<true, 7>}},       // the whole step
    };
    constexpr int NI = sizeof(table) / sizeof(table[0]);
    static std::atomic<bool> raised[NI][2];
    int t = 0;
    while (t < NI && table[t].phases != a.phases) ++t;
    if (t == NI) return QC_ERR_INVALID;
    const int quad = a.n > 32 ? 1 : 0;
    const kernel_t kernel = table[t].k[quad];
    const size_t lds = qc_scf_small_lds_bytes(a.n);
    if (!raised[t][quad].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return QC_ERR_HIP;
        raised[t][quad].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(kernel, dim3(1), dim3(QCS_T), lds, st, a);
    return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
}
