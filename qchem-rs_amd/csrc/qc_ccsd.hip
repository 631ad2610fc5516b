// qc_ccsd.hip - closed-shell CCSD correlation energy of an RHF state on the GPU.
//
// Integrals: the AO tensor in HBM (qc_launch_eri_full), one first quarter (p nu|la si) over all active MOs, then the blocks
// (ij|kl), (ia|jk), (ij|ab), (ia|jb), (ia|bc) and (ab|cd) by the quarter chain of the MP2 code; every intermediate is freed as soon as
// nothing reads it.  Amplitudes: t1[i, a] and t2[i, j, a, b] with t_ij^ab = t_ji^ba, one vector [t1 | t2] of o v + o^2 v^2 doubles.
//
// Working equations (chemists' integrals, canonical orbitals: f_ia = 0 and the diagonal of f is in the denominators; L = 2 K - K^T):
//   tau_ij^ab = t_ij^ab + t_i^a t_j^b          x_il^da = 1/2 t_il^da + t_i^d t_l^a        L(kc|ld) = 2 (kc|ld) - (kd|lc)
//   Foo_ki = L(kc|ld) tau_il^cd                Fvv_ac = -L(kc|ld) tau_kl^ad               Fov_kc = L(kc|ld) t_l^d
//   Loo_ki = Foo_ki + [2 (lc|ki) - (kc|li)] t_l^c           Lvv_ac = Fvv_ac + [2 (kd|ac) - (kc|ad)] t_k^d
//   Woooo_klij = (ki|lj) + (lc|ki) t_j^c + (kc|lj) t_i^c + (kc|ld) tau_ij^cd
//   Wvoov_akic = (ia|kc) + (kc|ad) t_i^d - (kc|li) t_l^a - (ld|kc) x_il^da + 1/2 L(ld|kc) t_il^ad
//   Wvovo_akci = (ki|ac) + (kd|ac) t_i^d - (lc|ki) t_l^a - (lc|kd) x_il^da
//   Z_ijka = tau_ij^cd (kd|ac)                 (the t1 part of the particle-particle ladder, factorised: no v^4 work beyond the ladder)
//   D_i^a t_i^a = Fvv_ac t_i^c - Foo_ki t_k^a + Fov_kc (2 t_ki^ca - t_ik^ca + t_i^c t_k^a) + [2 (kc|ia) - (ki|ac)] t_k^c
//                 + [2 (kd|ac) - (kc|ad)] tau_ik^cd - [2 (lc|ki) - (kc|li)] tau_kl^ac
//   X_ij^ab = [(ia|cb) - (ki|bc) t_k^a] t_j^c - [(ia|jk) + (kc|ia) t_j^c] t_k^b - Z_ijka t_k^b + Lvv_ac t_ij^cb - Loo_ki t_kj^ab
//             + (2 Wvoov_akic - Wvovo_akci) t_kj^cb - Wvoov_akic t_kj^bc - Wvovo_bkci t_kj^ac
//   D_ij^ab t_ij^ab = (ia|jb) + X_ij^ab + X_ji^ba + Woooo_klij tau_kl^ab + tau_ij^cd (ac|bd)
//   E = sum L(ia|jb) tau_ij^ab
// Every contraction is one GEMM between two permuted operands (ein below): the ladder tau[ij, cd] (ac|bd)[cd, ab] and every product
// that would leave qc_gemm under one wave per CU over a long k go through qc_gemm_splitk, the rest through qc_gemm.
//
// Determinism: no atomics.  A GEMM tile sums k in ascending order; split-k partial sums are added in slice order and the slice count
// depends on (m, n, k) alone; the energy, the DIIS dot products and the maxima are fixed-order reductions; the DIIS system is solved on
// the host in a fixed order.  A call is bitwise reproducible.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "qc_subspace.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

// ---- C = alpha A B + beta C for few rows and a long k (row-major, A m x k, B k x n).  Grid (tiles of 64 columns, tiles of 32 rows,
// k slices); wave w of a workgroup owns columns 16 w .. 16 w + 15 of the tile and both 16-row halves, and sums its slice in ascending k
// into P[slice][m][n].  Operand lane maps of v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
// result register r holds C[row = (l >> 4) + 4 r][col = l & 15].  Operands come straight from memory: the 16 lanes of a k-row read 128
// contiguous bytes of B, and A (a few hundred rows) stays in L2.  No LDS, no barrier: a wave past the last column leaves at once.
constexpr int SK_BM = 32, SK_BN = 64, SK_KC = 32;
constexpr int SK_MIN_SLICE = 64;      // shortest k slice (a multiple of 16)
constexpr int SK_WORKGROUPS = 512;    // the slice count aims at this many workgroups (2048 waves on 256 CUs)

// direct (one slice): the tile goes straight to C = alpha A B + beta C (P = C, ldp = ldc) and no second launch follows
struct SplitK { int m, n, k, ks; const double *A; int64_t lda; const double *B; int64_t ldb; double *P; int64_t ldp; int direct; double alpha, beta; };

__global__ __launch_bounds__(256) void qc_gemm_splitk_kernel(const SplitK g) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int n0 = blockIdx.x * SK_BN + 16 * w, m0 = blockIdx.y * SK_BM, z = blockIdx.z;
    if (n0 >= g.n) return;                                            // (wave-uniform)
    const int kb = z * g.ks, ke = min(g.k, kb + g.ks);
    const int r0 = m0 + li, r1 = m0 + 16 + li, col = n0 + li;
    const bool ok0 = r0 < g.m, ok1 = r1 < g.m, okb = col < g.n, two = m0 + 16 < g.m;
    const double *__restrict__ A0 = g.A + (int64_t)r0 * g.lda;
    const double *__restrict__ A1 = g.A + (int64_t)r1 * g.lda;
    const double *__restrict__ Bc = g.B + col;
    double4_t acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = kb; k0 < ke; k0 += SK_KC) {
        double a0[SK_KC / 4], a1[SK_KC / 4], b[SK_KC / 4];           // all operands of the chunk are requested before its first MFMA
#pragma unroll
        for (int s = 0; s < SK_KC / 4; ++s) {
            const int kk = k0 + 4 * s + lk;
            const bool in = kk < ke;
            a0[s] = (ok0 && in) ? A0[kk] : 0.0;
            a1[s] = (ok1 && in) ? A1[kk] : 0.0;
            b[s] = (okb && in) ? Bc[(int64_t)kk * g.ldb] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < SK_KC / 4; ++s) {
            if (k0 + 4 * s >= ke) break;                              // (uniform)
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b[s], acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b[s], acc1, 0, 0, 0);
        }
    }
    if (!okb) return;
    double *P = g.P + (g.direct ? 0 : (int64_t)z * g.m * g.n);
    auto put = [&](int row, double x) {
        double *c = P + (int64_t)row * g.ldp + col;
        *c = !g.direct ? x : g.beta == 0.0 ? g.alpha * x : fma(g.alpha, x, g.beta * *c);
    };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = m0 + lk + 4 * r;
        if (row < g.m) put(row, acc0[r]);
        if (row + 16 < g.m) put(row + 16, acc1[r]);
    }
}

// C = alpha (P[0] + P[1] + ...) + beta C, the slices in ascending order
__global__ void qc_gemm_splitk_sum_kernel(int m, int n, int slices, const double *__restrict__ P, double alpha, double beta, double *__restrict__ C, int64_t ldc) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, mn = (int64_t)m * n;
    if (e >= mn) return;
    double s = 0.0;
    for (int z = 0; z < slices; ++z) s += P[z * mn + e];
    const int64_t row = e / n;
    double *c = C + row * ldc + (e - row * n);
    *c = beta == 0.0 ? alpha * s : fma(alpha, s, beta * *c);
}

// ---- out = alpha perm(in) + beta out for a four-index tensor.  `in` is dense row-major with dimensions d; os[x] is the stride of in-axis x
// in `out`.  Tiled: the fastest axis of `out` is in-axis Y != 3.  A workgroup turns one 32 x 32 tile of (Y, 3) through LDS rows of 33
// doubles (the 32 lanes that read a column stride 66 dwords: 32 distinct bank pairs), so both the loads and the stores run along rows.
struct Perm { int d[4]; int64_t os[4]; int Y, U, W, tx, ty; double alpha, beta; };

__global__ __launch_bounds__(256) void qc_permute_tiled_kernel(const Perm g, const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double tile[32][33];
    int64_t b = blockIdx.x;
    const int txi = (int)(b % g.tx); b /= g.tx;
    const int tyi = (int)(b % g.ty); b /= g.ty;
    const int u = (int)(b % g.d[g.U]), w = (int)(b / g.d[g.U]);
    int64_t is[4];
    is[3] = 1; is[2] = g.d[3]; is[1] = is[2] * g.d[2]; is[0] = is[1] * g.d[1];
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5, x0 = txi * 32, y0 = tyi * 32, dx = g.d[3], dy = g.d[g.Y];
    const int64_t ibase = u * is[g.U] + w * is[g.W], obase = u * g.os[g.U] + w * g.os[g.W];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + 8 * q, x = x0 + c, y = y0 + r;
        if (x < dx && y < dy) tile[r][c] = in[ibase + y * is[g.Y] + x];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + 8 * q, x = x0 + r, y = y0 + c;
        if (x < dx && y < dy) {
            double *o = out + obase + x * g.os[3] + y;
            *o = g.beta == 0.0 ? g.alpha * tile[c][r] : fma(g.alpha, tile[c][r], g.beta * *o);
        }
    }
}

// the same when the fastest axis stays the fastest: one element per thread, loads and stores both along rows
__global__ void qc_permute_rows_kernel(const Perm g, int64_t total, const double *__restrict__ in, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int64_t r = e;
    const int i3 = (int)(r % g.d[3]); r /= g.d[3];
    const int i2 = (int)(r % g.d[2]); r /= g.d[2];
    const int i1 = (int)(r % g.d[1]); const int i0 = (int)(r / g.d[1]);
    double *o = out + i0 * g.os[0] + i1 * g.os[1] + i2 * g.os[2] + i3 * g.os[3];
    *o = g.beta == 0.0 ? g.alpha * in[e] : fma(g.alpha, in[e], g.beta * *o);
}

// ---- element-wise kernels.  out[i,j,a,b] = c t2[i,j,a,b] + t1[i,a] t1[j,b]  (tau: c = 1; x: c = 1/2)
__global__ void qc_ccsd_tau_kernel(int o, int v, double c, const double *__restrict__ t2, const double *__restrict__ t1, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, total = (int64_t)o * o * v * v;
    if (e >= total) return;
    int64_t r = e;
    const int b = (int)(r % v); r /= v;
    const int a = (int)(r % v); r /= v;
    const int j = (int)(r % o), i = (int)(r / o);
    out[e] = fma(t1[i * v + a], t1[j * v + b], c * t2[e]);
}

// the update by the denominators: T = [R1 / (e_i - e_a) | R2 / (e_i + e_j - e_a - e_b)]  (R1 null: zeros)
__global__ void qc_ccsd_update_kernel(int o, int v, const double *__restrict__ eo, const double *__restrict__ ev, const double *__restrict__ R1,
                                      const double *__restrict__ R2, double *__restrict__ T) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ov = (int64_t)o * v, total = ov + ov * ov;
    if (e >= total) return;
    if (e < ov) { const int i = (int)(e / v), a = (int)(e % v); T[e] = R1 ? R1[e] / (eo[i] - ev[a]) : 0.0; return; }
    int64_t r = e - ov;
    const int b = (int)(r % v); r /= v;
    const int a = (int)(r % v); r /= v;
    const int j = (int)(r % o), i = (int)(r / o);
    T[e] = R2[e - ov] / (((eo[i] + eo[j]) - ev[a]) - ev[b]);
}

__global__ void qc_ccsd_axpby_kernel(int64_t n, double alpha, const double *__restrict__ x, double beta, const double *__restrict__ y, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = alpha * x[e] + beta * y[e];
}

struct Coef { double c[12]; };
__global__ void qc_ccsd_lincomb_kernel(int64_t dim, int m, const Coef c, const double *__restrict__ V, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= dim) return;
    double s = 0.0;
    for (int j = 0; j < m; ++j) s = fma(c.c[j], V[j * dim + e], s);
    out[e] = s;
}

// ---- fixed-order reductions in two launches.  MODE 0: sum x y; MODE 1: max |x|.  Stage one: workgroup b takes elements
// RED_CHUNK b .. RED_CHUNK (b + 1) - 1, thread t the elements t + 256 u in ascending u, then a fixed LDS tree.  Stage two: one workgroup
// over the partial results in the same way.
constexpr int RED_CHUNK = 8192;
template <int MODE> __device__ __forceinline__ double red_op(double s, double x, double y) { return MODE == 0 ? fma(x, y, s) : fmax(s, fabs(x)); }
template <int MODE> __device__ __forceinline__ double red_tree(double s, double *sh) {
    const int t = threadIdx.x;
    sh[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) sh[t] = MODE == 0 ? sh[t] + sh[t + h] : fmax(sh[t], sh[t + h]);
        __syncthreads();
    }
    return sh[0];
}
template <int MODE> __global__ __launch_bounds__(256) void qc_ccsd_reduce_kernel(int64_t n, const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ part) {
    __shared__ double sh[256];
    const int64_t e0 = (int64_t)blockIdx.x * RED_CHUNK, e1 = min(n, e0 + RED_CHUNK);
    double s = 0.0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) s = red_op<MODE>(s, x[e], MODE == 0 ? y[e] : 0.0);
    s = red_tree<MODE>(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
template <int MODE> __global__ __launch_bounds__(256) void qc_ccsd_reduce2_kernel(int np, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int e = threadIdx.x; e < np; e += 256) s = MODE == 0 ? s + part[e] : fmax(s, part[e]);
    s = red_tree<MODE>(s, sh);
    if (threadIdx.x == 0) out[0] = s;
}

inline unsigned blocks_of(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace

// ---- the split-k rule: a pure function of (m, n, k)
int qc_gemm_splitk_slices(int m, int n, int k, int *slice_len) {
    const int64_t wgs = (int64_t)((m + SK_BM - 1) / SK_BM) * ((n + SK_BN - 1) / SK_BN);
    const int64_t want = std::max<int64_t>(1, SK_WORKGROUPS / wgs);
    int64_t ks = (k + want - 1) / want;
    ks = std::max<int64_t>(SK_MIN_SLICE, (ks + 15) / 16 * 16);
    if (slice_len) *slice_len = (int)ks;
    return (int)((k + ks - 1) / ks);
}
size_t qc_gemm_splitk_work(int m, int n, int k) { const int sl = qc_gemm_splitk_slices(m, n, k, nullptr); return sl == 1 ? 0 : (size_t)sl * m * n; }   // (one slice writes C itself)
// qc_gemm leaves the chip under one wave per CU (one wave per 16 x 16 tile of C) and k is long enough for at least two slices
bool qc_gemm_splitk_pays(int m, int n, int k) { return (int64_t)((m + 15) / 16) * ((n + 15) / 16) < 256 && k >= 2 * SK_MIN_SLICE; }

void qc_gemm_splitk(hipStream_t st, int m, int n, int k, double alpha, const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                    double *C, int64_t ldc, double *work) {
    if (m <= 0 || n <= 0 || k <= 0) return;
    int ks = 0;
    const int slices = qc_gemm_splitk_slices(m, n, k, &ks);
    const bool direct = slices == 1;
    const SplitK g{m, n, k, ks, A, lda, B, ldb, direct ? C : work, direct ? ldc : (int64_t)n, direct ? 1 : 0, alpha, beta};
    hipLaunchKernelGGL(qc_gemm_splitk_kernel, dim3((n + SK_BN - 1) / SK_BN, (m + SK_BM - 1) / SK_BM, slices), dim3(256), 0, st, g);
    if (!direct) hipLaunchKernelGGL(qc_gemm_splitk_sum_kernel, dim3(blocks_of((int64_t)m * n)), dim3(256), 0, st, m, n, slices, work, alpha, beta, C, ldc);
}

// out[axes in the order p] = alpha in + beta out: axis x of `out` is axis p[x] of `in` (dimensions d, dense row-major both)
void qc_permute4(hipStream_t st, const int d[4], const int p[4], double alpha, const double *in, double beta, double *out) {
    Perm g;
    int64_t ostr[4];
    ostr[3] = 1;
    for (int x = 2; x >= 0; --x) ostr[x] = ostr[x + 1] * d[p[x + 1]];
    for (int x = 0; x < 4; ++x) { g.d[x] = d[x]; g.os[p[x]] = ostr[x]; }
    g.alpha = alpha; g.beta = beta;
    const int64_t total = (int64_t)d[0] * d[1] * d[2] * d[3];
    if (total == 0) return;
    g.Y = p[3]; g.U = g.W = 0; g.tx = g.ty = 1;
    if (g.Y == 3) {
        hipLaunchKernelGGL(qc_permute_rows_kernel, dim3(blocks_of(total)), dim3(256), 0, st, g, total, in, out);
        return;
    }
    int rest[2], nr = 0;
    for (int x = 0; x < 3; ++x) if (x != g.Y) rest[nr++] = x;
    g.U = rest[0]; g.W = rest[1];
    g.tx = (d[3] + 31) / 32; g.ty = (d[g.Y] + 31) / 32;
    const int64_t nblocks = (int64_t)g.tx * g.ty * d[g.U] * d[g.W];
    hipLaunchKernelGGL(qc_permute_tiled_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, g, in, out);
}

namespace {

// ---- contractions by label.  A tensor is a device pointer and its index labels, slowest first: i..n occupied, a..f virtual.
struct Ten { double *p; const char *lab; };

struct Ccsd {
    hipStream_t st = nullptr;
    int o = 0, v = 0;
    bool dry = false;                       // only record the workspace sizes
    size_t ws_max = 0, wk_max = 0;          // doubles: a permuted operand / result, the split-k partial sums
    DevBuf wsA, wsB, wsC, wsK;

    int dim(char c) const { return c <= 'f' ? v : o; }
    int64_t size(const std::string &l) const { int64_t s = 1; for (char c : l) s *= dim(c); return s; }

    // out[labels lo] = alpha in[labels li] + beta out
    void permute(double alpha, const double *in, const std::string &li, double beta, double *out, const std::string &lo) {
        if (dry) return;
        const int r = (int)li.size(), pad = 4 - r;
        int d[4] = {1, 1, 1, 1}, p[4] = {0, 1, 2, 3};
        for (int x = 0; x < r; ++x) { d[pad + x] = dim(li[x]); p[pad + x] = pad + (int)li.find(lo[x]); }
        qc_permute4(st, d, p, alpha, in, beta, out);
    }

    // C = alpha sum_(labels not in C) A B + beta C: both operands are brought to matrices (free, contracted) x (contracted, free) -
    // in place where their labels already are in one of the orders a GEMM reads, through a workspace otherwise - and the product is
    // written to C directly when its labels are (free of A, free of B), through a workspace and a permutation otherwise.
    void ein(double alpha, Ten A, Ten B, double beta, Ten C, bool ladder = false) {
        std::string a = A.lab, b = B.lab, c = C.lab, fa, fb, ct;
        for (char ch : c) (a.find(ch) != std::string::npos ? fa : fb) += ch;
        const std::string &big = size(b) >= size(a) ? b : a;
        for (char ch : big) if (c.find(ch) == std::string::npos) ct += ch;
        if (!fb.empty() && c != fa + fb && c.compare(0, fb.size(), fb) == 0) { std::swap(A, B); std::swap(a, b); std::swap(fa, fb); }
        const int m = (int)size(fa), n = (int)size(fb), k = (int)size(ct);
        const bool direct = c == fa + fb, sk = ladder || qc_gemm_splitk_pays(m, n, k);
        const bool a_rows = a == fa + ct, a_cols = !sk && a == ct + fa, b_rows = b == ct + fb, b_cols = !sk && b == fb + ct;
        if (dry) {
            if (!a_rows && !a_cols) ws_max = std::max(ws_max, (size_t)size(a));
            if (!b_rows && !b_cols) ws_max = std::max(ws_max, (size_t)size(b));
            if (!direct) ws_max = std::max(ws_max, (size_t)size(c));
            if (sk) wk_max = std::max(wk_max, qc_gemm_splitk_work(m, n, k));
            return;
        }
        const double *Ap = A.p, *Bp = B.p;
        if (!a_rows && !a_cols) { permute(1.0, A.p, a, 0.0, wsA.p, fa + ct); Ap = wsA.p; }
        if (!b_rows && !b_cols) { permute(1.0, B.p, b, 0.0, wsB.p, ct + fb); Bp = wsB.p; }
        double *Cp = direct ? C.p : wsC.p;
        const double bt = direct ? beta : 0.0;
        if (sk) { qc_gemm_splitk(st, m, n, k, alpha, Ap, k, Bp, n, bt, Cp, n, wsK.p); }
        else { qc_gemm(st, m, n, k, alpha, Ap, a_cols ? m : k, a_cols, Bp, b_cols ? k : n, b_cols, bt, Cp, n); }
        if (!direct) permute(1.0, wsC.p, fa + fb, beta, C.p, c);
    }
    void copy(const double *in, double *out, int64_t n) { if (!dry) (void)hipMemcpyAsync(out, in, n * sizeof(double), hipMemcpyDeviceToDevice, st); }
    void tau(double c, const double *t2, const double *t1, double *out) {
        if (!dry) hipLaunchKernelGGL(qc_ccsd_tau_kernel, dim3(blocks_of((int64_t)o * o * v * v)), dim3(256), 0, st, o, v, c, t2, t1, out);
    }
};

// the integral blocks and the intermediates of one iteration (device)
struct CcsdBufs {
    DevBuf ovov, oovv, ovvv, ovoo, oooo, vvvv;     // (ia|jb), (ij|ab), (ia|bc), (ia|jk), (ij|kl) as stored; vvvv[c,d,a,b] = (ac|bd)
    DevBuf Lovov, Lt, Kt;                          // 2 (kc|ld) - (kd|lc) as [k,c,l,d]; the same and (ia|jb) as [i,j,a,b]
    DevBuf tau, x, Foo, Fvv, Fov, Loo, Lvv, Woooo, Wvoov, Wvovo, Z, X, R1, R2, tA, tB, too;
    int alloc_intermediates(int64_t o, int64_t v) {
        const int64_t oovv_n = o * o * v * v;
        struct { DevBuf *b; int64_t n; } all[] = {{&tau, oovv_n}, {&x, oovv_n}, {&Foo, o * o}, {&Fvv, v * v}, {&Fov, o * v}, {&Loo, o * o}, {&Lvv, v * v},
            {&Woooo, o * o * o * o}, {&Wvoov, oovv_n}, {&Wvovo, oovv_n}, {&Z, o * o * o * v}, {&X, oovv_n}, {&R1, o * v}, {&R2, oovv_n},
            {&tA, o * v * v * v}, {&tB, o * o * o * v}, {&too, o * o}};
        for (auto &e : all) if (e.b->alloc((size_t)e.n) != QC_OK) return QC_ERR_HIP;
        return QC_OK;
    }
    static double intermediate_doubles(double o, double v) { return 6.0 * o * o * v * v + 3.0 * o * o + 2.0 * v * v + 2.0 * o * v + o * o * o * o + 2.0 * o * o * o * v + o * v * v * v; }
};

// one pass of the amplitude equations: Tn = [R1 / D1 | R2 / D2] from the amplitudes T = [t1 | t2]
void ccsd_pass(Ccsd &c, CcsdBufs &B, const double *eo, const double *ev, double *T, double *Tn) {
    const int o = c.o, v = c.v;
    const int64_t ov = (int64_t)o * v, oovv = ov * ov;
    double *t1p = T, *t2p = T ? T + ov : nullptr;                       // (the dry pass has no amplitudes)
    auto t1 = [&](const char *l) { return Ten{t1p, l}; };
    auto t2 = [&](const char *l) { return Ten{t2p, l}; };
    auto tau = [&](const char *l) { return Ten{B.tau.p, l}; };
    auto ovov = [&](const char *l) { return Ten{B.ovov.p, l}; };
    auto Lovov = [&](const char *l) { return Ten{B.Lovov.p, l}; };
    auto oovv_ = [&](const char *l) { return Ten{B.oovv.p, l}; };
    auto ovvv = [&](const char *l) { return Ten{B.ovvv.p, l}; };
    auto ovoo = [&](const char *l) { return Ten{B.ovoo.p, l}; };

    c.tau(1.0, t2p, t1p, B.tau.p);
    c.tau(0.5, t2p, t1p, B.x.p);
    // one-particle intermediates
    c.ein(1.0, Lovov("kcld"), tau("ilcd"), 0.0, {B.Foo.p, "ki"});
    c.ein(-1.0, Lovov("kcld"), tau("klad"), 0.0, {B.Fvv.p, "ac"});
    c.ein(1.0, Lovov("kcld"), t1("ld"), 0.0, {B.Fov.p, "kc"});
    c.copy(B.Foo.p, B.Loo.p, (int64_t)o * o);
    c.ein(2.0, ovoo("lcki"), t1("lc"), 1.0, {B.Loo.p, "ki"});
    c.ein(-1.0, ovoo("kcli"), t1("lc"), 1.0, {B.Loo.p, "ki"});
    c.copy(B.Fvv.p, B.Lvv.p, (int64_t)v * v);
    c.ein(2.0, ovvv("kdac"), t1("kd"), 1.0, {B.Lvv.p, "ac"});
    c.ein(-1.0, ovvv("kcad"), t1("kd"), 1.0, {B.Lvv.p, "ac"});
    // two-particle intermediates
    c.permute(1.0, B.oooo.p, "kilj", 0.0, B.Woooo.p, "klij");
    c.ein(1.0, ovoo("lcki"), t1("jc"), 1.0, {B.Woooo.p, "klij"});
    c.ein(1.0, ovoo("kclj"), t1("ic"), 1.0, {B.Woooo.p, "klij"});
    c.ein(1.0, ovov("kcld"), tau("ijcd"), 1.0, {B.Woooo.p, "klij"});
    c.ein(1.0, tau("ijcd"), ovvv("kdac"), 0.0, {B.Z.p, "ijka"});
    c.permute(1.0, B.ovov.p, "iakc", 0.0, B.Wvoov.p, "akic");
    c.ein(1.0, ovvv("kcad"), t1("id"), 1.0, {B.Wvoov.p, "akic"});
    c.ein(-1.0, ovoo("kcli"), t1("la"), 1.0, {B.Wvoov.p, "akic"});
    c.ein(-1.0, ovov("ldkc"), {B.x.p, "ilda"}, 1.0, {B.Wvoov.p, "akic"});
    c.ein(0.5, Lovov("ldkc"), t2("ilad"), 1.0, {B.Wvoov.p, "akic"});
    c.permute(1.0, B.oovv.p, "kiac", 0.0, B.Wvovo.p, "akci");
    c.ein(1.0, ovvv("kdac"), t1("id"), 1.0, {B.Wvovo.p, "akci"});
    c.ein(-1.0, ovoo("lcki"), t1("la"), 1.0, {B.Wvovo.p, "akci"});
    c.ein(-1.0, ovov("lckd"), {B.x.p, "ilda"}, 1.0, {B.Wvovo.p, "akci"});
    // singles
    const Ten R1{B.R1.p, "ia"};
    c.ein(1.0, {B.Fvv.p, "ac"}, t1("ic"), 0.0, R1);
    c.ein(-1.0, {B.Foo.p, "ki"}, t1("ka"), 1.0, R1);
    c.ein(2.0, {B.Fov.p, "kc"}, t2("kica"), 1.0, R1);
    c.ein(-1.0, {B.Fov.p, "kc"}, t2("ikca"), 1.0, R1);
    c.ein(1.0, {B.Fov.p, "kc"}, t1("ic"), 0.0, {B.too.p, "ki"});
    c.ein(1.0, {B.too.p, "ki"}, t1("ka"), 1.0, R1);
    c.ein(2.0, ovov("kcia"), t1("kc"), 1.0, R1);
    c.ein(-1.0, oovv_("kiac"), t1("kc"), 1.0, R1);
    c.ein(2.0, ovvv("kdac"), tau("ikcd"), 1.0, R1);
    c.ein(-1.0, ovvv("kcad"), tau("ikcd"), 1.0, R1);
    c.ein(-2.0, ovoo("lcki"), tau("klac"), 1.0, R1);
    c.ein(1.0, ovoo("kcli"), tau("klac"), 1.0, R1);
    // doubles: the part that is symmetrised, X
    const Ten X{B.X.p, "ijab"};
    c.permute(1.0, B.ovvv.p, "iacb", 0.0, B.tA.p, "abic");
    c.ein(-1.0, oovv_("kibc"), t1("ka"), 1.0, {B.tA.p, "abic"});
    c.ein(1.0, {B.tA.p, "abic"}, t1("jc"), 0.0, X);
    c.permute(1.0, B.ovoo.p, "iajk", 0.0, B.tB.p, "akij");
    c.ein(1.0, ovov("kcia"), t1("jc"), 1.0, {B.tB.p, "akij"});
    c.ein(-1.0, {B.tB.p, "akij"}, t1("kb"), 1.0, X);
    c.ein(-1.0, {B.Z.p, "ijka"}, t1("kb"), 1.0, X);
    c.ein(1.0, {B.Lvv.p, "ac"}, t2("ijcb"), 1.0, X);
    c.ein(-1.0, {B.Loo.p, "ki"}, t2("kjab"), 1.0, X);
    c.ein(2.0, {B.Wvoov.p, "akic"}, t2("kjcb"), 1.0, X);
    c.ein(-1.0, {B.Wvovo.p, "akci"}, t2("kjcb"), 1.0, X);
    c.ein(-1.0, {B.Wvoov.p, "akic"}, t2("kjbc"), 1.0, X);
    c.ein(-1.0, {B.Wvovo.p, "bkci"}, t2("kjac"), 1.0, X);
    // R2 = (ia|jb) + X + X^T + the two ladders
    c.copy(B.Kt.p, B.R2.p, oovv);
    c.permute(1.0, B.X.p, "ijab", 1.0, B.R2.p, "ijab");
    c.permute(1.0, B.X.p, "jiba", 1.0, B.R2.p, "ijab");
    c.ein(1.0, {B.Woooo.p, "klij"}, tau("klab"), 1.0, {B.R2.p, "ijab"});
    c.ein(1.0, tau("ijcd"), {B.vvvv.p, "cdab"}, 1.0, {B.R2.p, "ijab"}, true);
    if (!c.dry) hipLaunchKernelGGL(qc_ccsd_update_kernel, dim3(blocks_of(ov + oovv)), dim3(256), 0, c.st, o, v, eo, ev, B.R1.p, B.R2.p, Tn);
}

// sum x y (mode 0) or max |x| (mode 1) over n elements, to the host; part: ceil(n / RED_CHUNK) + 1 doubles on the device
int reduce_to_host(hipStream_t st, int mode, int64_t n, const double *x, const double *y, double *part, double *out) {
    const int np = (int)((n + RED_CHUNK - 1) / RED_CHUNK);
    if (mode == 0) {
        hipLaunchKernelGGL(qc_ccsd_reduce_kernel<0>, dim3(np), dim3(256), 0, st, n, x, y, part + 1);
        hipLaunchKernelGGL(qc_ccsd_reduce2_kernel<0>, dim3(1), dim3(256), 0, st, np, part + 1, part);
    } else {
        hipLaunchKernelGGL(qc_ccsd_reduce_kernel<1>, dim3(np), dim3(256), 0, st, n, x, y, part + 1);
        hipLaunchKernelGGL(qc_ccsd_reduce2_kernel<1>, dim3(1), dim3(256), 0, st, np, part + 1, part);
    }
    QC_HIP_CHECK(hipMemcpyAsync(out, part, sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    return QC_OK;
}

// DIIS coefficients: minimise |sum c_j e_j| with sum c_j = 1.  B (m x m, row-major) is scaled by its largest diagonal element, the bordered
// system is solved by Gaussian elimination with partial pivoting, rows and columns in a fixed order.  false: singular.
bool diis_coefficients(int m, const std::vector<double> &Bm, double *c) {
    const int d = m + 1;
    double scale = 0.0;
    for (int j = 0; j < m; ++j) scale = std::max(scale, Bm[(size_t)j * m + j]);
    if (!(scale > 0.0) || !std::isfinite(scale)) return false;
    std::vector<double> A((size_t)d * d, 0.0), y(d, 0.0);
    for (int r = 0; r < m; ++r) {
        for (int q = 0; q < m; ++q) A[(size_t)r * d + q] = Bm[(size_t)r * m + q] / scale;
        A[(size_t)r * d + m] = A[(size_t)m * d + r] = -1.0;
    }
    y[m] = -1.0;
    for (int p = 0; p < d; ++p) {
        int piv = p;
        for (int r = p + 1; r < d; ++r) if (std::fabs(A[(size_t)r * d + p]) > std::fabs(A[(size_t)piv * d + p])) piv = r;
        if (!(std::fabs(A[(size_t)piv * d + p]) > 1e-14)) return false;
        if (piv != p) { for (int q = 0; q < d; ++q) std::swap(A[(size_t)p * d + q], A[(size_t)piv * d + q]); std::swap(y[p], y[piv]); }
        for (int r = p + 1; r < d; ++r) {
            const double f = A[(size_t)r * d + p] / A[(size_t)p * d + p];
            for (int q = p; q < d; ++q) A[(size_t)r * d + q] -= f * A[(size_t)p * d + q];
            y[r] -= f * y[p];
        }
    }
    for (int p = d - 1; p >= 0; --p) {
        double s = y[p];
        for (int q = p + 1; q < d; ++q) s -= A[(size_t)p * d + q] * y[q];
        y[p] = s / A[(size_t)p * d + p];
    }
    for (int j = 0; j < m; ++j) { if (!std::isfinite(y[j])) return false; c[j] = y[j]; }
    return true;
}

// bytes the call holds at its peak: the phases of the integral chain, then the blocks with the solver's buffers
double ccsd_need_bytes(double n, double o, double v, double ndiis, double ws, double wk) {
    const double N = o + v, nn = n * n, dim = o * v + o * o * v * v;
    const double halves = (o * o + o * v + v * v) * nn;
    const double thirds = (o * o * o + o * o * v + o * v * o + o * v * v + v * v * v) * n;
    const double blocks = o * o * o * o + o * v * o * o + 2.0 * o * o * v * v + o * v * v * v + v * v * v * v;
    const double solver = 3.0 * o * o * v * v + CcsdBufs::intermediate_doubles(o, v) + (2.0 * ndiis + 2.0) * dim + 3.0 * ws + wk + dim / RED_CHUNK + 64.0;
    const double p1 = nn * nn + N * nn * n, p2 = N * nn * n + halves, p3 = halves + thirds + blocks, p4 = blocks + v * v * v * v + solver;
    return 8.0 * std::max(std::max(p1, p2), std::max(p3, p4));
}

}  // namespace

int qc_ccsd_device(qc_system *S, int nocc, const double *dC, const double *dEps, qc_ccsd *io, double *t1_out, double *t2_out) {
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const double t_begin = qc_now_ms();
    const int n = S->nbasis, nf = io->n_frozen, o = nocc - nf, v = n - nocc, N = o + v;
    const int maxit = io->max_iterations > 0 ? io->max_iterations : 100, ndiis = io->diis_size > 0 ? io->diis_size : 8;
    const double tol = io->tol > 0.0 ? io->tol : 1e-8;
    const int64_t nn = (int64_t)n * n, n3 = nn * n, n4 = nn * nn, ov = (int64_t)o * v, oovv = ov * ov, dim = ov + oovv;
    io->e_mp2 = io->e_ccsd = io->t1_diagnostic = io->t1_max = io->t2_max = io->residual = 0.0;
    io->iterations = io->converged = 0;
    io->ms_total = io->ms_tensor = io->ms_transform = io->ms_solve = 0.0;
    if (dim > 0x7fffffff || (int64_t)v * v * v > 0x7fffffff) return QC_ERR_UNSUPPORTED;          // (a GEMM dimension past int)
    hipStream_t st = S->stream;
    QC_HIP_CHECK(hipStreamSynchronize(st));

    Ccsd c;
    c.st = st; c.o = o; c.v = v;
    CcsdBufs B;
    c.dry = true;
    ccsd_pass(c, B, nullptr, nullptr, nullptr, nullptr);                                          // workspace sizes of one pass
    c.dry = false;
    size_t free_b = 0, total_b = 0;
    QC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (ccsd_need_bytes(n, o, v, ndiis, (double)c.ws_max, (double)c.wk_max) * 1.05 > (double)free_b) return QC_ERR_UNSUPPORTED;

    // 1. the AO tensor
    const double t0 = qc_now_ms();
    const double *eo = dEps + nf, *ev = dEps + nocc;
    {
        DevBuf I, Q1, Uoo, Uov, Uvv, Y;
        if (I.alloc(n4) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemsetAsync(I.p, 0, n4 * sizeof(double), st));
        int rc = qc_launch_eri_full(S, I.p);
        if (rc != QC_OK) return rc;
        QC_HIP_CHECK(hipStreamSynchronize(st));
        io->ms_tensor = qc_now_ms() - t0;
        // 2. quarter transformations: (p nu|la si) over the active MOs (occupied first), then the halves (ij|..), (ia|..), (ab|..)
        if (Q1.alloc(N * n3) != QC_OK) return QC_ERR_HIP;
        qc_quarter_first(st, n, dC, nf, N, I.p, Q1.p);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        I.reset();
        if (Uoo.alloc((int64_t)o * o * nn) != QC_OK || Uov.alloc(ov * nn) != QC_OK || Uvv.alloc((int64_t)v * v * nn) != QC_OK) return QC_ERR_HIP;
        qc_quarter_second(st, n, o, dC, nf, o, Q1.p, Uoo.p);
        qc_quarter_second(st, n, o, dC, nocc, v, Q1.p, Uov.p);
        qc_quarter_second(st, n, v, dC, nocc, v, Q1.p + (int64_t)o * n3, Uvv.p);
        QC_HIP_CHECK(hipStreamSynchronize(st));
        Q1.reset();
        // the blocks, one third quarter at a time through Y
        auto third = [&](const DevBuf &U, int rows, int c0, int m) -> int {
            Y.reset();
            if (Y.alloc((int64_t)rows * m * n) != QC_OK) return QC_ERR_HIP;
            qc_quarter_third(st, n, rows, dC, c0, m, U.p, Y.p);
            return QC_OK;
        };
        auto last = [&](int rows, int c0, int m, DevBuf &out) -> int {
            if (out.alloc((int64_t)rows * m) != QC_OK) return QC_ERR_HIP;
            qc_quarter_last(st, n, rows, dC, c0, m, Y.p, out.p);
            QC_HIP_CHECK(hipStreamSynchronize(st));
            return QC_OK;
        };
        DevBuf raw_vvvv;
        if (third(Uoo, o * o, nf, o) != QC_OK || last(o * o * o, nf, o, B.oooo) != QC_OK) return QC_ERR_HIP;
        if (third(Uoo, o * o, nocc, v) != QC_OK || last(o * o * v, nocc, v, B.oovv) != QC_OK) return QC_ERR_HIP;
        Uoo.reset();
        if (third(Uov, o * v, nf, o) != QC_OK || last(o * v * o, nocc, v, B.ovov) != QC_OK || last(o * v * o, nf, o, B.ovoo) != QC_OK) return QC_ERR_HIP;
        if (third(Uov, o * v, nocc, v) != QC_OK || last(o * v * v, nocc, v, B.ovvv) != QC_OK) return QC_ERR_HIP;
        Uov.reset();
        if (third(Uvv, v * v, nocc, v) != QC_OK || last(v * v * v, nocc, v, raw_vvvv) != QC_OK) return QC_ERR_HIP;
        Uvv.reset(); Y.reset();
        // (ab|cd) stored [a,b,c,d] -> [c,d,a,b] of (ac|bd): the ladder's right operand, read in place by every pass
        if (B.vvvv.alloc((int64_t)v * v * v * v) != QC_OK) return QC_ERR_HIP;
        c.permute(1.0, raw_vvvv.p, "acbd", 0.0, B.vvvv.p, "cdab");
        QC_HIP_CHECK(hipGetLastError());
        QC_HIP_CHECK(hipStreamSynchronize(st));
    }
    // L = 2 K - K^T as [k,c,l,d] and as [i,j,a,b]; K as [i,j,a,b]
    if (B.Lovov.alloc(oovv) != QC_OK || B.Lt.alloc(oovv) != QC_OK || B.Kt.alloc(oovv) != QC_OK) return QC_ERR_HIP;
    c.copy(B.ovov.p, B.Lovov.p, oovv);
    c.permute(-1.0, B.ovov.p, "kdlc", 2.0, B.Lovov.p, "kcld");
    c.permute(1.0, B.Lovov.p, "iajb", 0.0, B.Lt.p, "ijab");
    c.permute(1.0, B.ovov.p, "iajb", 0.0, B.Kt.p, "ijab");
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipStreamSynchronize(st));
    const double t_solve = qc_now_ms();
    io->ms_transform = t_solve - t0 - io->ms_tensor;

    // 3. the amplitude iteration
    DevBuf Tc, Tn, Th, Eh, part, dB;
    const int npart = (int)((dim + RED_CHUNK - 1) / RED_CHUNK) + 1;
    if (B.alloc_intermediates(o, v) != QC_OK || Tc.alloc(dim) != QC_OK || Tn.alloc(dim) != QC_OK || Th.alloc((size_t)ndiis * dim) != QC_OK ||
        Eh.alloc((size_t)ndiis * dim) != QC_OK || part.alloc(npart) != QC_OK || dB.alloc(12 * 12) != QC_OK || c.wsA.alloc(c.ws_max) != QC_OK ||
        c.wsB.alloc(c.ws_max) != QC_OK || c.wsC.alloc(c.ws_max) != QC_OK || c.wsK.alloc(c.wk_max) != QC_OK) return QC_ERR_HIP;
    hipLaunchKernelGGL(qc_ccsd_update_kernel, dim3(blocks_of(dim)), dim3(256), 0, st, o, v, eo, ev, (const double *)nullptr, B.Kt.p, Tc.p);   // t1 = 0, t2 = (ia|jb) / D
    int rc = reduce_to_host(st, 0, oovv, B.Lt.p, Tc.p + ov, part.p, &io->e_mp2);
    if (rc != QC_OK) return rc;

    std::vector<double> Bm(12 * 12, 0.0), Bw, row(12);
    int slots[12], nwin = 0, next = 0;                  // window, oldest first; the ring slot the next pair goes to
    bool converged = false;
    double change = 0.0;
    int it = 0;
    for (it = 1; it <= maxit; ++it) {
        ccsd_pass(c, B, eo, ev, Tc.p, Tn.p);
        const int s = next;
        next = (next + 1) % ndiis;
        double *Es = Eh.p + (size_t)s * dim, *Ts = Th.p + (size_t)s * dim;
        hipLaunchKernelGGL(qc_ccsd_axpby_kernel, dim3(blocks_of(dim)), dim3(256), 0, st, dim, 1.0, Tn.p, -1.0, Tc.p, Es);
        QC_HIP_CHECK(hipGetLastError());
        if ((rc = reduce_to_host(st, 1, dim, Es, nullptr, part.p, &change)) != QC_OK) return rc;
        if (!(change == change)) { change = INFINITY; break; }                       // (NaN: the iteration has diverged)
        if (change <= tol) { converged = true; break; }
        if (it == maxit) break;
        if (ndiis < 2) { std::swap(Tc.p, Tn.p); continue; }
        c.copy(Tn.p, Ts, dim);
        if (nwin == ndiis) { for (int j = 1; j < nwin; ++j) slots[j - 1] = slots[j]; --nwin; }   // (the oldest pair lived in slot s)
        slots[nwin++] = s;
        // row s of B by the fixed-order dots kernel: <e_j, e_s> for every ring slot j (slots not in the window are not read below)
        qc_stab_dots(st, (int)dim, Eh.p, std::min(it, ndiis), Eh.p, s, 1, 12, dB.p);
        QC_HIP_CHECK(hipMemcpyAsync(row.data(), dB.p + (size_t)s * 12, 12 * sizeof(double), hipMemcpyDeviceToHost, st));
        QC_HIP_CHECK(hipStreamSynchronize(st));
        for (int j = 0; j < std::min(it, ndiis); ++j) Bm[(size_t)s * 12 + j] = Bm[(size_t)j * 12 + s] = row[j];
        Bw.assign((size_t)nwin * nwin, 0.0);
        for (int p = 0; p < nwin; ++p) for (int q = 0; q < nwin; ++q) Bw[(size_t)p * nwin + q] = Bm[(size_t)slots[p] * 12 + slots[q]];
        Coef cf;
        for (double &x : cf.c) x = 0.0;
        double cw[12];
        if (nwin >= 2 && diis_coefficients(nwin, Bw, cw)) {
            for (int p = 0; p < nwin; ++p) cf.c[slots[p]] = cw[p];
            hipLaunchKernelGGL(qc_ccsd_lincomb_kernel, dim3(blocks_of(dim)), dim3(256), 0, st, dim, std::min(it, ndiis), cf, Th.p, Tc.p);
        } else {
            std::swap(Tc.p, Tn.p);
        }
    }
    if (it > maxit) it = maxit;
    QC_HIP_CHECK(hipGetLastError());
    // the energy and the diagnostics of the last amplitudes (Tn)
    c.tau(1.0, Tn.p + ov, Tn.p, B.tau.p);
    if ((rc = reduce_to_host(st, 0, oovv, B.Lt.p, B.tau.p, part.p, &io->e_ccsd)) != QC_OK) return rc;
    if ((rc = reduce_to_host(st, 1, oovv, Tn.p + ov, nullptr, part.p, &io->t2_max)) != QC_OK) return rc;
    std::vector<double> h1(ov);
    QC_HIP_CHECK(hipMemcpy(h1.data(), Tn.p, ov * sizeof(double), hipMemcpyDeviceToHost));
    double s2 = 0.0, m1 = 0.0;
    for (double x : h1) { s2 += x * x; m1 = std::max(m1, std::fabs(x)); }
    io->t1_diagnostic = std::sqrt(s2 / o); io->t1_max = m1;
    io->residual = change; io->iterations = it; io->converged = converged ? 1 : 0;
    if (t1_out) std::memcpy(t1_out, h1.data(), ov * sizeof(double));
    if (t2_out) QC_HIP_CHECK(hipMemcpy(t2_out, Tn.p + ov, oovv * sizeof(double), hipMemcpyDeviceToHost));
    io->ms_solve = qc_now_ms() - t_solve;
    io->ms_total = qc_now_ms() - t_begin;
    return converged ? QC_OK : QC_NOT_CONVERGED;
}

// C = alpha A B + beta C of host matrices (row-major, dense) on the default device: which 0 through qc_gemm, 1 through qc_gemm_splitk.
// reps > 0 repeats the product on the same buffers (beta applies every time) and ms (nullable, reps doubles) takes each launch's time.
int qc_debug_gemm_device(int which, int m, int n, int k, double alpha, const double *A, const double *B, double beta, double *C, int reps, double *ms) {
    DevBuf dA, dB, dC, dW;
    const size_t sa = (size_t)m * k, sb = (size_t)k * n, sc = (size_t)m * n;
    if (dA.alloc(sa) != QC_OK || dB.alloc(sb) != QC_OK || dC.alloc(sc) != QC_OK || dW.alloc(qc_gemm_splitk_work(m, n, k)) != QC_OK) return QC_ERR_HIP;
    hipStream_t st = nullptr;
    QC_HIP_CHECK(hipMemcpy(dA.p, A, sa * sizeof(double), hipMemcpyHostToDevice));
    QC_HIP_CHECK(hipMemcpy(dB.p, B, sb * sizeof(double), hipMemcpyHostToDevice));
    QC_HIP_CHECK(hipMemcpy(dC.p, C, sc * sizeof(double), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    QC_HIP_CHECK(hipEventCreate(&e0));
    QC_HIP_CHECK(hipEventCreate(&e1));
    struct EvDel { hipEvent_t a, b; ~EvDel() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } del{e0, e1};
    for (int r = 0; r < std::max(reps, 1); ++r) {
        QC_HIP_CHECK(hipEventRecord(e0, st));
        if (which == 1) qc_gemm_splitk(st, m, n, k, alpha, dA.p, k, dB.p, n, beta, dC.p, n, dW.p);
        else qc_gemm(st, m, n, k, alpha, dA.p, k, false, dB.p, n, false, beta, dC.p, n);
        QC_HIP_CHECK(hipEventRecord(e1, st));
        QC_HIP_CHECK(hipEventSynchronize(e1));
        float t = 0.f;
        QC_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        if (ms) ms[r] = t;
    }
    QC_HIP_CHECK(hipGetLastError());
    QC_HIP_CHECK(hipMemcpy(C, dC.p, sc * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}
