// qc_scf.cpp - the host-side SCF drivers and the step API (qc_scf_* of include/qchem_hip.h).
//
// qc_scf_rhf / qc_scf_uhf restate the control flow of restricted_hartree_fock (core/src/hf/rhf.rs:32-108) and
// unrestricted_hartree_fock (uhf.rs:36-167) - guess, DIIS windows, update order, energy expression, diagonal-only
// convergence test - with every matrix resident in HBM and every step a HIP kernel, the DIIS (<= 9 x 9) QR solve
// included; the host takes the convergence decision from two scalars it reads back once per pass.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <new>

#include "qc_embed.h"
#include "qc_solvent.h"

namespace {

// Diis (diis.rs:6-60) with the sample window, the B matrix and the QR solve in HBM / on the device: nothing of it
// synchronises with the host.  Samples live in ring slots; `slots` lists them newest first.  A singular system
// ("DIIS failed", rhf.rs:73) raises *d_flag, which the SCF step reads back together with the energy.
struct DeviceDiis {
    int minlen, maxlen, n;
    std::deque<int> slots;
    std::vector<DevBuf> pool;              // err of slot s = pool[2s], fock = pool[2s + 1]
    DevBuf d_dots, d_B, d_c;
    DeviceDiis(int mn, int mx, int n_) : minlen(mn), maxlen(mx), n(n_) {}
    int init() {
        if (maxlen > 11) return QC_ERR_INVALID;
        pool = std::vector<DevBuf>(2 * maxlen);
        for (auto &b : pool) if (b.alloc((size_t)n * n) != QC_OK) return QC_ERR_HIP;
        if (d_dots.alloc(16) != QC_OK || d_c.alloc(16) != QC_OK || d_B.alloc((size_t)maxlen * maxlen) != QC_OK) return QC_ERR_HIP;
        return hipMemset(d_B.p, 0, sizeof(double) * maxlen * maxlen) == hipSuccess ? QC_OK : QC_ERR_HIP;
    }
    // claim the slot of the next sample (push_front + truncate, diis.rs:29-30: the oldest slot is recycled); the caller
    // writes the error and Fock matrices straight into the returned buffers
    void next_sample(double **d_err, double **d_fock) {
        int s;
        if ((int)slots.size() == maxlen) { s = slots.back(); slots.pop_back(); } else s = (int)slots.size();
        slots.push_front(s);
        *d_err = pool[2 * s].p; *d_fock = pool[2 * s + 1].p;
    }
    // enqueues: new row of B, coefficient solve, extrapolated Fock matrix into d_out
    int extrapolate(hipStream_t st, double *d_out, int *d_flag) {
        const int m = (int)slots.size();
        const double *ys[12], *fs[12];
        int sl[12];
        for (int j = 0; j < m; ++j) { sl[j] = slots[j]; ys[j] = pool[2 * slots[j]].p; fs[j] = pool[2 * slots[j] + 1].p; }
        qc_dots(st, n, ys[0], ys, m, d_dots.p);                                        // <e_0, e_j>, diis.rs:43-45
        // (sensitivity probe, QC_DIIS_PERTURB: one dot product moved by one unit in the last place - what a different summation
        // order does - to see how far a run's trajectory depends on such bits)
        static const bool perturb = getenv("QC_DIIS_PERTURB") != nullptr;
        if (perturb && m > 1) qc_axpby(st, 1, 1.0 + 0x1p-52, d_dots.p + 1, 0.0, nullptr, d_dots.p + 1);
        qc_diis_solve(st, m, minlen, maxlen, sl, d_dots.p, d_B.p, d_c.p, d_flag);         // (1, 0, ...) while m < minlen
        qc_lincomb_dev(st, n, fs, d_c.p, m, d_out);                               // diis.rs:52-58
        return hipGetLastError() == hipSuccess ? QC_OK : QC_ERR_HIP;
    }
};

struct ScfWork {
    int n;
    // (work buffers of a Roothaan step come in two sets: the two spins of a UHF pass run at the same time on two streams, set b = spin;
    // eig[b].t1 .. t4 double as the step's GEMM scratch)
    DevBuf H, S, X, Fp[2], Cp, C, w, Fd[2], scal, CpPrev[2], CpNew[2], Fps[2];
    QcEigWork eig[2];
    bool have_prev[2] = {false, false};
    // Open-shell runs (n_alpha != n_beta) use the rotation-based eigensolvers only.  Their SCF solutions of interest include
    // saddles of the UHF functional that are kept by spatial symmetry alone (O2 triplet, BASELINE config 4): Jacobi rotations
    // never mix functions that are not coupled, so symmetry-equivalent blocks of F' get bit-identical treatment and the
    // iteration stays on the symmetric determinant exactly like the reference's fixed sequence of operations; Householder
    // reflectors mix everything and seed the unstable direction with rounding noise (measured: the run then leaves the saddle
    // for the 0.024 Eh lower broken-symmetry determinant after ~60 passes).
    bool rotations_only = false;
    bool small_fused = false;              // n <= QC_SMALL_MAXN: the Roothaan step runs as one workgroup with its matrices in LDS (qc_scf_small.hip)
    int64_t small_steps[3] = {0, 0, 0}; // Roothaan steps through the one-workgroup kernel by route: Refine, Tridiag, the Jacobi routes (qc_scf_counters)
    bool cold[2] = {false, false};         // this pass's eigensolve of the spin started from the tridiagonal path (no previous vectors involved)
    int npass[2] = {3, 3};                 // refinement passes enqueued per eigensolve (follows what the last one needed)
    int mode[2] = {2, 2};                  // eigensolve of the next pass: 0 refinement, 1 two Jacobi sweeps + refinement, 2 Jacobi
    QcDev<int> ctl;                        // the pass's QC_CTL_WORDS device control words
    double *h_scal = nullptr;              // pinned read-back: the QC_SYNC_WORDS words of pass scalars, then (multi-rank) their complements
    QcDev<unsigned long long> d_sync;      // multi-rank runs: the same words + their bitwise complements, all-reduced (max) across the ranks
    ~ScfWork() { if (h_scal) (void)hipHostFree(h_scal); }
    int init(int n_, int nsets) {
        n = n_;
        const size_t nn = (size_t)n * n;
        DevBuf *all[] = {&H, &S, &X, &Cp, &C, &CpPrev[0], &CpPrev[1], &CpNew[0], &CpNew[1], &Fps[0], &Fps[1]};
        for (auto b : all) if (b->alloc(nn) != QC_OK) return QC_ERR_HIP;
        for (int b = 0; b < nsets; ++b)
            if (eig[b].alloc(n) != QC_OK || Fp[b].alloc(nn) != QC_OK || Fd[b].alloc(nn) != QC_OK) return QC_ERR_HIP;
        if (w.alloc(n) != QC_OK || scal.alloc(16) != QC_OK) return QC_ERR_HIP;
        if (ctl.alloc(QC_CTL_WORDS) != QC_OK || hipMemset(ctl.p, 0, QC_CTL_WORDS * sizeof(int)) != hipSuccess) return QC_ERR_HIP;
        if (hipHostMalloc(&h_scal, (2 * QC_SYNC_WORDS + 1) * sizeof(double)) != hipSuccess) return QC_ERR_HIP;
        std::memset(h_scal, 0, (2 * QC_SYNC_WORDS + 1) * sizeof(double));     // (the last word: sequence number of the pass, see scf_iterate)
        return d_sync.alloc(2 * QC_SYNC_WORDS);
    }
};

// sorted_eigs on device (utils.rs:20-36): Fp -> (Cp, w)
int device_sorted_eigs(qc_system *S, ScfWork &W, double *dA, double *dV, double *dw) {
    // (set-up eigensolves: synchronous)
    if (W.rotations_only) return qc_eig_device(S->stream, W.n, dA, dV, dw, W.eig[0], W.ctl.p + QC_CTL_NOTCONV);
    return qc_eig_cold_sync(S->stream, W.n, dA, dV, dw, W.eig[0], W.ctl.p + QC_CTL_SETUP, W.ctl.p + QC_CTL_NOTCONV);
}

// start-up shared by both drivers: H = T + V, X = S^-1/2 (rhf.rs:124-131), Hückel matrix (rhf.rs:141-143)
int scf_setup(qc_system *S, ScfWork &W, std::vector<double> &h_eht) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    // S, T, V on the device (molint::overlap / kinetic / nuclear, rhf.rs:41-43); H = T + V (rhf.rs:48)
    hipStream_t st = S->stream;
    int rc1 = qc_one_electron_device(S, 0, W.S.p);
    if (rc1 == QC_OK) rc1 = qc_one_electron_device(S, 1, W.eig[0].t1.p);
    if (rc1 == QC_OK) rc1 = qc_one_electron_device(S, 2, W.eig[0].t2.p);
    if (rc1 != QC_OK) return rc1;
    qc_axpby(st, n, 1.0, W.eig[0].t1.p, 1.0, W.eig[0].t2.p, W.H.p);
    if (!S->pc.empty()) {                                   // point-charge embedding: H = T + V + V_pc (whole on every rank, like T and V)
        if ((rc1 = qc_pc_matrix_device(S, S->pc, W.eig[0].t1.p)) != QC_OK) return rc1;
        qc_axpby(st, n, 1.0, W.H.p, 1.0, W.eig[0].t1.p, W.H.p);
    }
    std::vector<double> s(nn), h(nn);
    QC_HIP_CHECK(hipMemcpyAsync(s.data(), W.S.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipMemcpyAsync(h.data(), W.H.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    h_eht.assign(nn, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j)
            h_eht[(size_t)i * n + j] = h_eht[(size_t)j * n + i] = 1.75 * s[(size_t)i * n + j] * (h[(size_t)i * n + i] + h[(size_t)j * n + j]) / 2.0;
    // X = U (diag((U^T S U)_ii^-1/2) U^T): note the diagonal of the product, not the returned eigenvalues
    int rc = device_sorted_eigs(S, W, W.S.p, W.Cp.p, W.w.p);          // U (column order is immaterial for X)
    if (rc != QC_OK) return rc;
    qc_gemm(st, n, n, n, 1.0, W.S.p, n, false, W.Cp.p, n, false, 0.0, W.eig[0].t1.p, n);      // S U
    qc_gemm(st, n, n, n, 1.0, W.Cp.p, n, true, W.eig[0].t1.p, n, false, 0.0, W.eig[0].t2.p, n);      // U^T (S U)
    qc_scale_cols_invsqrt(st, n, W.Cp.p, W.eig[0].t2.p, W.eig[0].t1.p);                               // U diag^-1/2
    qc_gemm(st, n, n, n, 1.0, W.eig[0].t1.p, n, false, W.Cp.p, n, true, 0.0, W.X.p, n);       // (.) U^T
    return QC_OK;
}

// compute_hückel_density (rhf.rs:133-150): D = factor * C_occ C_occ^T with C = X eigvecs(X^T H_eht X)
int huckel_density(qc_system *S, ScfWork &W, const std::vector<double> &h_eht, int nocc, double factor, double *dD) {
    const int n = S->nbasis;
    hipStream_t st = S->stream;
    QC_HIP_CHECK(hipMemcpyAsync(W.Fd[0].p, h_eht.data(), h_eht.size() * sizeof(double), hipMemcpyHostToDevice, st));
    qc_gemm(st, n, n, n, 1.0, W.Fd[0].p, n, false, W.X.p, n, false, 0.0, W.eig[0].t1.p, n);
    qc_gemm(st, n, n, n, 1.0, W.X.p, n, true, W.eig[0].t1.p, n, false, 0.0, W.Fp[0].p, n);
    int rc = device_sorted_eigs(S, W, W.Fp[0].p, W.Cp.p, W.w.p);
    if (rc != QC_OK) return rc;
    qc_gemm(st, n, n, n, 1.0, W.X.p, n, false, W.Cp.p, n, false, 0.0, W.C.p, n);
    if (nocc > 0) qc_gemm(st, n, n, nocc, factor, W.C.p, n, false, W.C.p, n, true, 0.0, dD, n);
    else QC_HIP_CHECK(hipMemsetAsync(dD, 0, sizeof(double) * n * n, st));
    return QC_OK;
}

// The eigensolve of a spin's Roothaan step.  Near convergence (mode 0): GEMM refinement from this spin's previous vectors.  Otherwise -
// first pass, or the density still moves by more than the warm threshold per element - the tridiagonal path (start vectors from
// qc_eig_tridiag.hip + the same refinement); matrices below QC_TRI_MIN_N, open-shell runs and QC_EIG_JACOBI go to the single-workgroup
// Jacobi kernels, in the basis of the previous vectors once they exist.  Refine and Tridiag report through the spin's control words.
enum class EigRoute { Refine, Tridiag, JacobiWarm, JacobiCold };
EigRoute eig_route(const ScfWork &W, int spin, int n) {
    if (W.have_prev[spin] && W.mode[spin] == 0) return EigRoute::Refine;
    if (qc_tri_ok(n) && !qc_eig_force_jacobi() && !W.rotations_only) return EigRoute::Tridiag;
    return W.have_prev[spin] ? EigRoute::JacobiWarm : EigRoute::JacobiCold;
}

// Times of the passes.  Events of a pass (start | build done | pass done), two sets used alternately: a pass whose end the host saw through
// the pinned sequence word reads none of them before it returns - the last event may still be in flight, and asking costs host time
// between two passes.  The next pass asks (flush), after its own build has been issued.
struct PassTiming {
    struct Build { bool tuned; unsigned gen; };   // the build contained a tuner run; it ran under this stream assignment (qc_system::assign_gen)
    hipEvent_t evs[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int cur = 0, pending_set = 0;
    bool pending = false;                      // the pass of set `pending_set` has ended and its event times have not been read yet
    Build cur_build = {false, 0}, pend_build = {false, 0};
    double ms_fock = 0, ms_linalg = 0, ms_tuner = 0;
    int64_t builds_timed = 0;
    ~PassTiming() { for (auto &set : evs) for (hipEvent_t e : set) if (e) (void)hipEventDestroy(e); }
    int create() {
        for (auto &set : evs) for (hipEvent_t &e : set) QC_HIP_CHECK(hipEventCreate(&e));
        return QC_OK;
    }
    hipEvent_t *begin_pass() { cur ^= 1; return evs[cur]; }
    // (`t_start`: the host's clock before the build was issued - the time of a build with a tuner run in it is the tuner's)
    void build_issued(bool tuned, double t_start, unsigned gen) { cur_build = {tuned, gen}; if (tuned) ms_tuner += qc_now_ms() - t_start; }
    void pass_seen() { pending = true; pending_set = cur; pend_build = cur_build; }
    void repeat_seen() { float ms = 0; (void)hipEventElapsedTime(&ms, evs[cur][1], evs[cur][2]); ms_linalg += ms; }
    // (`tuner`: the handle whose stream tuner takes the build time as a sample, null for builds it does not assign)
    void flush(qc_system *tuner) {
        if (!pending) return;
        pending = false;
        hipEvent_t *e = evs[pending_set];
        float ms_f = 0, ms_l = 0;
        if (hipEventSynchronize(e[2]) != hipSuccess) return;
        const bool have_f = hipEventElapsedTime(&ms_f, e[0], e[1]) == hipSuccess;
        if (hipEventElapsedTime(&ms_l, e[1], e[2]) == hipSuccess) ms_linalg += ms_l;
        // (a build that contained a tuner run is not a sample of the build time: neither for the totals nor for the tuner's online choice)
        if (!have_f || pend_build.tuned) return;
        ms_fock += ms_f; builds_timed += 1;
        if (tuner) qc_fock_feedback(tuner, ms_f, pend_build.gen);
    }
};

}  // namespace

// ---- step-wise drivers: the host (the Rust `core` crate in the north-star design) owns the convergence loop and
// calls one FFI entry per loop-body pass; qc_scf_rhf / qc_scf_uhf below are that loop written in C++.
struct qc_scf_state {
    qc_system *S = nullptr;
    bool uhf = false;
    int nocc[2] = {0, 0};
    ScfWork W;
    DevBuf D[2], Dn[2], G, Cs, ws;             // densities are double-buffered per spin: D <-> Dn swap when a pass is accepted
    int64_t passes = 0, redos = 0;
    bool spin_parallel = getenv("QC_NO_SPIN_PARALLEL") == nullptr;      // (A/B switch, read per SCF state)
    double warm_rms_env = getenv("QC_EIG_WARM_RMS") ? atof(getenv("QC_EIG_WARM_RMS")) : 0.0;   // (read per SCF state: tests reach the repeat branch with it)
    DevBuf T4, TK, Dtot;                       // stored mode: RHF T = I - I^x / 2; UHF I and its exchange-permuted copy
    bool stored = false;
    int twin = -1;                             // UHF spin-twin decision, taken at the first build
    double ms_tensor = 0, ms_setup = 0;
    DeviceDiis *diis[2] = {nullptr, nullptr};
    PassTiming tm;
    unsigned pass_seq = 0;                     // sequence number of the last pass whose end the host saw through the pinned word
    bool event_wait = getenv("QC_EVENT_WAIT") != nullptr;      // (A/B switch, read per SCF state: the stream's event instead)
    std::vector<double> pc;                    // the handle's point charges when the state began ([x, y, z, q] each): what its H contains
    // continuum solvation: the handle's cavity when the state began.  W.H is then H_eff = Hvac + V_R(q) of the state's current
    // density, renewed behind every pass (solvent_update); solv_q / solv_out: the charges and {1/2 q.v_nuc, 1/2 q.v_elec, sum q} that go with it
    std::shared_ptr<QcSolvent> solv;
    DevBuf Hvac, VR, Dsum;                     // (Dsum: the total density of a UHF state, formed per pass)
    std::vector<double> solv_q, solv_ve;
    double solv_out[3] = {0.0, 0.0, 0.0};
    ~qc_scf_state() {
        if (S && S->prep.owner == this) { S->prep.prepared = false; S->prep.owner = nullptr; }
        delete diis[0]; delete diis[1];
        if (S && S->stream) { (void)hipStreamSynchronize(S->stream); qc_gate_quiet(S); qc_tl_dump(S); }
    }
    qc_system *tuner() const { return !stored && !S->comm ? S : nullptr; }   // (for PassTiming::flush)
};
static void scf_state_delete(qc_scf_state *st) {
    if (!st) return;
    qc_system *S = st->S;
    delete st;
    if (S && --S->live_states == 0 && S->zombie) qc_system_free(S);
}

namespace {

// The shape of a pass, decided once before anything is enqueued.
struct PassPlan {
    bool fused;                // the one-workgroup kernels (qc_scf_small.hip) instead of the generic launch sequence
    // UHF: the two spins' steps are independent (uhf.rs:84-135 runs them one after the other) - the beta step goes to a side stream on
    // another dispatch pipe, with the second set of work buffers, behind an event of the build's closing kernel, and meets the handle's
    // stream again before the scalars (device-side join).  Same kernels, same arithmetic, per spin: results are bit for bit those of the
    // serial order (QC_NO_SPIN_PARALLEL).  On the one-workgroup path the kernel that joins the streams on the device also hands the control
    // words over and stores the sequence word (qc_spin_join_end); not with a communicator.
    bool side_by_side;
    // Multi-rank runs take every decision (convergence, DIIS failure, eigensolve mode, repeat) from the SAME numbers on every
    // rank: the pass scalars go to device memory, are all-reduced as bit patterns (max) together with their complements - so a
    // rank whose copy differs is noticed (max(x) != ~max(~x)) - and only then reach the host.  The replicated linear algebra is
    // deterministic and starts from bit-identical G (integer all-reduce), so the copies agree; this makes a divergence an
    // error on all ranks in the same pass instead of a hang in the next all-reduce.
    bool multi;
    bool clear_sync_slot;      // multi-rank RHF: the unused spin slot of d_sync is cleared in every pass
    // Single-rank runs on the one-workgroup path: the kernel that ends the pass stores the pass's sequence number into pinned memory
    // after the scalars and control words, and the host polls THAT instead of the event behind it (a few microseconds earlier per pass).
    bool seq_wait;
    unsigned *h_seq; unsigned seq;
    // (RHF, direct fixed-point builds on the one-workgroup path: the kernel that forms the new density also leaves the next build's fixed-point unit)
    bool scale_in_kernel;
    double *scal_out;          // where the kernels put energy and rms: pinned host memory, or (multi-rank) d_sync
    int *ctl_out, *h_ctl;      // ... and the control words; where the host reads them
};
PassPlan plan_pass(const qc_scf_state *st) {
    const qc_system *S = st->S;
    const ScfWork &W = st->W;
    PassPlan p{};
    p.fused = W.small_fused;
    p.multi = S->comm != nullptr;
    p.side_by_side = st->uhf && st->spin_parallel && S->lanes.nlanes >= 2 && !S->join.by_events && !(p.fused && p.multi);
    p.clear_sync_slot = p.multi && !st->uhf;
    p.seq_wait = p.fused && !p.multi && !st->event_wait;
    p.h_seq = reinterpret_cast<unsigned *>(W.h_scal + 2 * QC_SYNC_WORDS); p.seq = st->pass_seq + 1;
    p.scale_in_kernel = p.fused && !st->uhf && !st->stored && S->accum_fx;
    p.h_ctl = reinterpret_cast<int *>(W.h_scal + 4);
    p.scal_out = p.multi ? reinterpret_cast<double *>(W.d_sync.p) : W.h_scal;
    p.ctl_out = p.multi ? reinterpret_cast<int *>(W.d_sync.p + 4) : p.h_ctl;
    return p;
}

// What one spin's part of a pass works on, built once per pass.
struct SpinStep {
    int spin;
    hipStream_t st; int b;     // the stream the step is enqueued on and its set of work buffers (side by side: beta on the side stream, set 1)
    int nocc; double dfac;     // D = dfac * C_occ C_occ^T
    const double *G, *D;       // this pass's G and the density it was built from
    double *Dn, *w, *C;        // new density, orbital energies, C
    double *E, *F;             // this pass's DIIS sample buffers (error, Fock matrix)
    DeviceDiis *diis;
    bool dens_done;            // Dn was formed on the side stream already (generic sequence, side by side)
    double *scal_out;          // the spin's two pass scalars
};
// (claims the spin's DIIS sample slot of the pass)
SpinStep spin_step(qc_scf_state *st, const PassPlan &plan, int s) {
    const size_t n = st->S->nbasis, nn = n * n;
    SpinStep p{};
    p.spin = s; p.st = st->S->stream; p.b = 0;
    p.nocc = st->nocc[s]; p.dfac = st->uhf ? 1.0 : 2.0;
    p.G = st->G.p + s * nn; p.D = st->D[s].p; p.Dn = st->Dn[s].p; p.w = st->ws.p + s * n; p.C = st->Cs.p + s * nn;
    p.diis = st->diis[s]; p.scal_out = plan.scal_out + 2 * s;
    p.diis->next_sample(&p.E, &p.F);
    return p;
}

// enqueues the eigensolve of the spin's F' (W.Fps) by `route`: vectors to W.CpNew, eigenvalues to p.w.  (`again`: the repeat of a
// pass's eigensolve - Refine and Tridiag in their synchronous forms, which report through QC_CTL_NOTCONV like the Jacobi routes)
int eig_enqueue(ScfWork &W, const SpinStep &p, EigRoute route, bool again) {
    const int n = W.n;
    QcEigWork &E = W.eig[p.b];
    double *const Fps = W.Fps[p.spin].p, *const CpPrev = W.CpPrev[p.spin].p, *const CpNew = W.CpNew[p.spin].p;
    int *const ctl = W.ctl.p + QC_CTL_EIG + QC_CTL_EIG_STRIDE * p.spin, *const notconv = W.ctl.p + QC_CTL_NOTCONV;
    switch (route) {
    case EigRoute::Refine:
        return again ? qc_eig_device_refine(p.st, n, Fps, CpPrev, CpNew, p.w, E, notconv)
                     : qc_eig_refine_async(p.st, n, Fps, CpPrev, CpNew, p.w, E, ctl, W.npass[p.spin]);
    // (three refinement passes are enqueued: two finish most starts - the third is then five empty launches - but near-degenerate
    // clusters of a nearly converged benzene need it, and running out of passes costs a Jacobi eigensolve)
    case EigRoute::Tridiag:
        return again ? qc_eig_cold_sync(p.st, n, Fps, CpNew, p.w, E, W.ctl.p + QC_CTL_SETUP, notconv)
                     : qc_eig_cold_async(p.st, n, Fps, CpNew, p.w, E, ctl, 3);
    case EigRoute::JacobiWarm: return qc_eig_device_warm(p.st, n, Fps, CpPrev, CpNew, p.w, E, notconv);
    case EigRoute::JacobiCold: return qc_eig_device(p.st, n, Fps, CpNew, p.w, E, notconv);     // sorted_eigs (rhf.rs:75)
    }
    return QC_ERR_INVALID;
}
// ... followed by C = X C'
int eig_and_coefficients(ScfWork &W, const SpinStep &p, EigRoute route, bool again) {
    const int n = W.n;
    const int rc = eig_enqueue(W, p, route, again);
    if (rc != QC_OK) return rc;
    qc_gemm(p.st, n, n, n, 1.0, W.X.p, n, false, W.CpNew[p.spin].p, n, false, 0.0, p.C, n);   // C = X C'
    return QC_OK;
}

// One spin's Roothaan step, enqueued without any host synchronisation: F = H + G; e = FDS - SDF; DIIS; F' = X^T F X;
// eigenvectors (eig_route); C = X C'   (rhf.rs:70-76).  New vectors go to CpNew[spin], C to p.C.
int roothaan_enqueue(ScfWork &W, const SpinStep &p, bool have_F) {
    const int n = W.n, b = p.b;
    hipStream_t st = p.st;
    QcEigWork &E = W.eig[b];
    if (!have_F) qc_axpby(st, n, 1.0, W.H.p, 1.0, p.G, p.F);                                // F (else written by the build's closing kernel)
    qc_gemm(st, n, n, n, 1.0, p.F, n, false, p.D, n, false, 0.0, E.t2.p, n);                // F D
    qc_gemm(st, n, n, n, 1.0, E.t2.p, n, false, W.S.p, n, false, 0.0, W.Fp[b].p, n);        // F D S
    qc_sub_transpose(st, n, W.Fp[b].p, p.E);                                                // e = FDS - (FDS)^T = FDS - SDF
    const int rc = p.diis->extrapolate(st, W.Fd[b].p, W.ctl.p + QC_CTL_DIIS);
    if (rc != QC_OK) return rc;
    qc_gemm(st, n, n, n, 1.0, W.Fd[b].p, n, false, W.X.p, n, false, 0.0, E.t1.p, n);        // F X
    qc_gemm(st, n, n, n, 1.0, W.X.p, n, true, E.t1.p, n, false, 0.0, W.Fps[p.spin].p, n);   // X^T (F X)
    const EigRoute route = eig_route(W, p.spin, n);
    W.cold[p.spin] = route == EigRoute::Tridiag;
    return eig_and_coefficients(W, p, route, false);
}

// The same step for n <= QC_SMALL_MAXN, density / energy / rms of rhf.rs:78-88 included: one launch when the eigensolve is a refinement from
// the previous vectors, pre | tridiagonal start | refine + post when it starts cold, pre | Jacobi kernel | post for the rotation-only runs.
// (`ends_pass`: this spin's last launch also hands the control words over, clears them and - plan.seq_wait - stores the sequence word)
int roothaan_small(qc_system *S, ScfWork &W, const PassPlan &plan, const SpinStep &p, bool have_F, bool ends_pass) {
    const int n = W.n;
    const DeviceDiis &diis = *p.diis;
    QcSmallArgs a{};
    a.n = n;
    a.F = have_F ? p.F : nullptr; a.F_out = p.F;
    a.D = p.D; a.S = W.S.p; a.X = W.X.p; a.H = W.H.p; a.G = p.G;
    a.E_out = p.E;
    a.m = (int)diis.slots.size(); a.minlen = diis.minlen; a.maxlen = diis.maxlen;
    a.dots_generic = W.rotations_only ? 1 : 0;
    for (int j = 0; j < a.m; ++j) { a.slot[j] = diis.slots[j]; a.errs[j] = diis.pool[2 * diis.slots[j]].p; a.focks[j] = diis.pool[2 * diis.slots[j] + 1].p; }
    a.Bmat = diis.d_B.p; a.c_out = diis.d_c.p; a.diis_flag = W.ctl.p + QC_CTL_DIIS;
    a.Fp = W.Fps[p.spin].p;
    a.ctl = W.ctl.p + QC_CTL_EIG + QC_CTL_EIG_STRIDE * p.spin;
    a.Cp_out = W.CpNew[p.spin].p; a.w_out = p.w; a.C_out = p.C; a.Dn = p.Dn; a.Dold = p.D; a.nocc = p.nocc; a.dfac = p.dfac;
    a.scal_out = p.scal_out; a.ctl_all = ends_pass ? W.ctl.p : nullptr; a.ctl_out = plan.ctl_out; a.imax = S->imax;
    a.fxs_out = plan.scale_in_kernel ? S->dev.d_fxs.p : nullptr;
    if (ends_pass && plan.seq_wait) { a.seq_out = plan.h_seq; a.seq = plan.seq; }
    a.tl = S->tl.cur ? S->tl.cur + QC_TL_W * (QC_NUNITS + 2) : nullptr;
    const EigRoute route = eig_route(W, p.spin, n);
    W.cold[p.spin] = route == EigRoute::Tridiag;
    W.small_steps[route == EigRoute::Refine ? 0 : route == EigRoute::Tridiag ? 1 : 2] += 1;
    int rc = QC_OK;
    if (route != EigRoute::Refine) {
        QcSmallArgs pre = a;
        pre.phases = 1; pre.ctl_all = nullptr; pre.seq_out = nullptr;
        if (a.tl) a.tl += QC_TL_W;                              // (the second launch of the pass has its own slot)
        if ((rc = qc_scf_small_launch(p.st, pre)) != QC_OK) return rc;
    }
    switch (route) {
    case EigRoute::Refine: a.phases = 7; a.V0 = W.CpPrev[p.spin].p; a.npass = W.npass[p.spin]; break;
    case EigRoute::Tridiag: rc = qc_eig_tridiag_start(p.st, n, a.Fp, W.eig[p.b]); a.phases = 6; a.V0 = W.eig[p.b].x0.p; a.npass = 3; break;
    case EigRoute::JacobiWarm:
    case EigRoute::JacobiCold: rc = eig_enqueue(W, p, route, false); a.phases = 4; a.Cp_in = a.Cp_out; break;
    }
    if (rc != QC_OK) return rc;
    return qc_scf_small_launch(p.st, a);
}

// The rare repeat of a spin's eigensolve when the route that reports through the control words asked for rotations (QC_EIG_ROTATE).
// After Tridiag (the start was not good enough): the Jacobi routes.  After Refine (not perturbative after all): the synchronous forms
// of Tridiag (its own fallback: the Jacobi kernels) or, for the rotation-only runs, of Refine (rotations in the basis of the previous vectors).
// On the handle's stream with the first set of work buffers, whichever the spin's step used.
int roothaan_redo_eig(qc_system *S, ScfWork &W, const SpinStep &p) {
    SpinStep r = p;
    r.st = S->stream; r.b = 0;
    const EigRoute again = W.cold[p.spin] ? (W.have_prev[p.spin] ? EigRoute::JacobiWarm : EigRoute::JacobiCold)
                                          : (W.rotations_only ? EigRoute::Refine : EigRoute::Tridiag);
    return eig_and_coefficients(W, r, again, true);
}

// enqueues, on the handle's stream: the spin's new density - unless the side stream formed it, once: a repeat of the eigensolve forms it
// again, here - and its energy and rms straight into the plan's scalars; `hand_over`: the kernel also hands over and clears the control words
int density_and_scalars(qc_system *S, ScfWork &W, const PassPlan &plan, SpinStep &p, bool hand_over) {
    const int n = W.n;
    hipStream_t sm = S->stream;
    if (p.dens_done) p.dens_done = false;
    else if (p.nocc > 0) qc_gemm(sm, n, n, p.nocc, p.dfac, p.C, n, false, p.C, n, true, 0.0, p.Dn, n);
    else QC_HIP_CHECK(hipMemsetAsync(p.Dn, 0, (size_t)n * n * sizeof(double), sm));
    qc_energy_rms(sm, n, p.Dn, p.D, W.H.p, p.G, p.scal_out, hand_over ? W.ctl.p : nullptr, plan.ctl_out);
    return QC_OK;
}

}  // namespace

// A solvated state's reaction field for its current density D: v_elec(D) -> q = K v -> V_R(q) -> W.H = Hvac + V_R, so that the next pass's
// F = H + G and its energy 1/2 tr[D_new (2 H + G)] contain V_R(D).  That energy counts V_R twice - the definition is
// 1/2 tr[D_new (2 Hvac + G + V_R)] - and tr(D_new V_R(q_old)) = q_old . v_elec(D_new): *correction = -1/2 q_old . v_elec(D), summed on the
// host in element order, with q_old the charges in force before this call (`correction` null: the first call, from scf_begin).
// Synchronous: the handle's stream is drained when it returns.
static int solvent_update(qc_scf_state *st, double *correction) {
    qc_system *S = st->S;
    QcSolvent &Q = *st->solv;
    const int n = S->nbasis;
    const double *P = st->D[0].p;
    if (st->uhf) {
        qc_axpby(S->stream, n, 1.0, st->D[0].p, 1.0, st->D[1].p, st->Dsum.p);
        P = st->Dsum.p;
    }
    std::vector<double> q(Q.M);
    st->solv_ve.resize(Q.M);
    const int rc = qc_solvent_response_device(S, Q, P, q.data(), st->solv_ve.data(), st->VR.p, st->solv_out);
    if (rc != QC_OK) return rc;
    if (correction) {
        double dot = 0.0;
        for (int64_t i = 0; i < Q.M; ++i) dot += st->solv_q[i] * st->solv_ve[i];
        *correction = -0.5 * dot;
    }
    st->solv_q.swap(q);
    qc_axpby(S->stream, n, 1.0, st->Hvac.p, 1.0, st->VR.p, st->W.H.p);
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

// (hDa / hDb non-null: the caller's densities, host, in place of the Hueckel guess - qc_scf_begin_*_from)
static int scf_begin(qc_system *S, bool uhf, int n_alpha, int n_beta, qc_scf_state **out, const double *hDa = nullptr, const double *hDb = nullptr) {
    if (!S || !out) return QC_ERR_INVALID;
    const double t0 = qc_now_ms();
    static const bool sdbg = getenv("QC_SETUP_DEBUG") != nullptr;
    QcLap lap{"setup", sdbg, t0};
    // a continuum goes with one whole direct build in vacuum: no shards, no stored tensor, no point charges (checked before the device is touched)
    if (S->solvent && (S->comm || S->nranks != 1 || S->fock_mode == 1 || !S->pc.empty())) return QC_ERR_UNSUPPORTED;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    lap("qc_device_init (total)");
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    qc_scf_state *st = new (std::nothrow) qc_scf_state();
    if (!st) return QC_ERR_INVALID;
    struct Del { void operator()(qc_scf_state *p) const { scf_state_delete(p); } };
    std::unique_ptr<qc_scf_state, Del> guard(st);
    st->S = S; st->uhf = uhf;
    ++S->live_states;
    st->nocc[0] = st->nocc[1] = S->nelec / 2;                             // rhf.rs:176 / uhf.rs:43-45
    if (uhf && (n_alpha > 0 || n_beta > 0)) { st->nocc[0] = n_alpha; st->nocc[1] = n_beta; }
    if (st->nocc[0] < 0 || st->nocc[1] < 0 || st->nocc[0] > n || st->nocc[1] > n) return QC_ERR_INVALID;
    const int nspin = uhf ? 2 : 1;
    st->W.rotations_only = uhf && st->nocc[0] != st->nocc[1];
    // (QC_NO_SMALL_FUSED: A/B switch, the generic launch sequence.  Open-shell runs take the one-workgroup kernels too since the two spins'
    // kernels run side by side - pre | Jacobi kernel | post per spin, O2 triplet/cc-pVDZ 0.130 ms of linear algebra per pass against 0.148
    // for the generic sequence, 0.198 with the spins one after the other - with the DIIS dot products in the generic sequence's summation
    // order, QcSmallArgs::dots_generic.  Their saddle-point trajectories depend on every last bit - DESIGN.md 1 - and the two paths differ
    // in the last bit of the first pass's energy: O2 triplet reaches 1e-10 in 118 passes on this path and in 450 on the generic one, 15
    // and 15 at the CLI's 1e-6, energies 8e-6 Eh apart there.  QC_NO_OPEN_SHELL_FUSED: A/B switch.)
    static const bool open_fused = getenv("QC_NO_OPEN_SHELL_FUSED") == nullptr;
    st->W.small_fused = n <= QC_SMALL_MAXN && (!st->W.rotations_only || open_fused) && getenv("QC_NO_SMALL_FUSED") == nullptr;
    if ((rc = st->W.init(n, uhf ? 2 : 1)) != QC_OK) return rc;
    for (int s = 0; s < nspin; ++s) if (st->D[s].alloc(nn) != QC_OK || st->Dn[s].alloc(nn) != QC_OK) return QC_ERR_HIP;
    if (st->G.alloc(nspin * nn) != QC_OK || st->Cs.alloc(nspin * nn) != QC_OK || st->ws.alloc(nspin * n) != QC_OK) return QC_ERR_HIP;
    std::vector<double> h_eht;
    lap("state buffers");
    st->pc = S->pc;
    if ((rc = scf_setup(S, st->W, h_eht)) != QC_OK) return rc;           // rhf.rs:41-49
    lap("S, T, V, X = S^-1/2");
    for (int s = 0; s < nspin; ++s) {                                     // rhf.rs:50 / uhf.rs:60-63
        const double *given = s == 0 ? hDa : hDb;
        if (given) QC_HIP_CHECK(hipMemcpyAsync(st->D[s].p, given, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
        else if ((rc = huckel_density(S, st->W, h_eht, st->nocc[s], uhf ? 1.0 : 2.0, st->D[s].p)) != QC_OK) return rc;
    }
    lap("Hueckel guess");
    if (S->solvent) {                                                    // the reaction field of the starting density (the guess itself is the vacuum one)
        st->solv = S->solvent;
        if (st->Hvac.alloc(nn) != QC_OK || st->VR.alloc(nn) != QC_OK || (uhf && st->Dsum.alloc(nn) != QC_OK)) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemcpyAsync(st->Hvac.p, st->W.H.p, nn * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        if ((rc = solvent_update(st, nullptr)) != QC_OK) return rc;
        lap("solvent: K, first reaction field");
    }
    if (S->fock_mode == 1) {
        // the reference's conventional SCF: ERI tensor once (rhf.rs:45), antisymmetrised copy (rhf.rs:58-62), dense
        // contraction per pass.  8 n^4 bytes per tensor; two of them live during the build.
        if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;        // sharded builds are direct-mode only
        const size_t n4 = nn * nn;
        size_t free_b = 0, total_b = 0;
        QC_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if ((double)n4 * 8.0 * 2.2 > (double)free_b) return QC_ERR_UNSUPPORTED;
        const double tt0 = qc_now_ms();
        DevBuf I;
        if (I.alloc(n4) != QC_OK || st->T4.alloc(n4) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipMemsetAsync(I.p, 0, n4 * sizeof(double), S->stream));
        if ((rc = qc_launch_eri_full(S, I.p)) != QC_OK) return rc;
        if (uhf) {
            qc_permute_tensor(S->stream, n, I.p, 0.0, 1.0, st->T4.p);      // TK[i,j,k,l] = I[i,k,j,l]
            st->TK.p = st->T4.p; st->T4.p = I.p; I.p = nullptr;            // keep I (as T4) and TK
            if (st->Dtot.alloc(nn) != QC_OK) return QC_ERR_HIP;
        } else {
            qc_permute_tensor(S->stream, n, I.p, 1.0, -0.5, st->T4.p);     // electron_terms, rhf.rs:58-62
        }
        QC_HIP_CHECK(hipStreamSynchronize(S->stream));
        st->stored = true;
        st->ms_tensor = qc_now_ms() - tt0;
    }
    for (int s = 0; s < nspin; ++s) {                                     // Diis::new(4,6) rhf.rs:65 / (2,8) uhf.rs:76-78
        st->diis[s] = uhf ? new DeviceDiis(2, 8, n) : new DeviceDiis(4, 6, n);
        if ((rc = st->diis[s]->init()) != QC_OK) return rc;
    }
    if ((rc = st->tm.create()) != QC_OK) return rc;
    int eig_flag = 0;                                                     // the eigensolves of X and of the Hueckel guess
    QC_HIP_CHECK(hipMemcpyAsync(&eig_flag, st->W.ctl.p + QC_CTL_NOTCONV, sizeof(int), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    if (eig_flag) return QC_EIG_NOT_CONVERGED;
    st->ms_setup = qc_now_ms() - t0;
    *out = guard.release();
    return QC_OK;
}

// Wait for the end of a pass by polling (what hipStreamSynchronize does too): a parked thread's wake-up latency is longer than a whole
// SCF pass of a small molecule.  `h_seq` non-null: for the pass's sequence word `want` in pinned memory, with the event behind the pass
// as the witness of a failure (a failed launch or a fault never stores the word: the event knows); null: for the event alone.
// Not for ever: a kernel that never finishes is an error of the call, not a host core pinned for good (QC_HOST_WAIT_LIMIT_S, default
// 120 s; the device-side waits give up earlier and say why).
static int wait_pass(hipEvent_t ev, const unsigned *h_seq = nullptr, unsigned want = 0) {
    static const double limit_ms = getenv("QC_HOST_WAIT_LIMIT_S") ? atof(getenv("QC_HOST_WAIT_LIMIT_S")) * 1e3 : 120e3;
    unsigned spins = 0;
    double t0 = 0.0;
    for (;;) {
        if (h_seq && __atomic_load_n(h_seq, __ATOMIC_ACQUIRE) == want) return QC_OK;
        const bool look = (++spins & 0xfff) == 0;               // (now and then: the clock, and next to the word the event)
        if (h_seq && !look) continue;
        const hipError_t e = hipEventQuery(ev);
        if (e == hipErrorNotReady) {
            if (!look) continue;
            const double t = qc_now_ms();
            if (t0 == 0.0) t0 = t;
            else if (t - t0 > limit_ms) { fprintf(stderr, "qchem_hip: an SCF pass did not finish within %.0f s\n", limit_ms * 1e-3); return QC_ERR_HIP; }
            continue;
        }
        if (!h_seq && e == hipSuccess) return QC_OK;
        if (!h_seq) { fprintf(stderr, "qchem_hip: the wait for the end of an SCF pass failed: %s\n", hipGetErrorString(e)); return QC_ERR_HIP; }
        if (e != hipSuccess || __atomic_load_n(h_seq, __ATOMIC_ACQUIRE) != want) { fprintf(stderr, "qchem_hip: the pass ended without its sequence word (%s)\n", hipGetErrorString(e)); return QC_ERR_HIP; }
    }
}

// ---- one pass of the loop body, step by step (scf_iterate)

// enqueues G of every spin from the *old* densities, behind the pass's first event; direct builds also write F = H + G where they can (*have_F)
static int build_G(qc_scf_state *st, hipEvent_t ev0, const SpinStep *sp, bool *have_F) {
    qc_system *S = st->S;
    ScfWork &W = st->W;
    const int n = S->nbasis;
    hipStream_t sm = S->stream;
    double *const dG = st->G.p, *const dGb = dG + (size_t)n * n;
    int rc;
    QC_HIP_CHECK(hipEventRecord(ev0, sm));
    if (st->stored) {
        if (st->uhf) {   // uhf.rs:216-226: G_s = <I, D_s + D_s'> - <I^x, D_s>
            qc_axpby(sm, n, 1.0, st->D[0].p, 1.0, st->D[1].p, st->Dtot.p);
            qc_axpby(sm, n, -1.0, st->D[0].p, 0.0, nullptr, W.eig[0].t1.p);
            if ((rc = qc_tensor_gemv(sm, n, st->T4.p, st->Dtot.p, st->TK.p, W.eig[0].t1.p, dG)) != QC_OK) return rc;
            qc_axpby(sm, n, -1.0, st->D[1].p, 0.0, nullptr, W.eig[0].t1.p);
            if ((rc = qc_tensor_gemv(sm, n, st->T4.p, st->Dtot.p, st->TK.p, W.eig[0].t1.p, dGb)) != QC_OK) return rc;
        } else {
            if ((rc = qc_tensor_gemv(sm, n, st->T4.p, st->D[0].p, nullptr, nullptr, dG)) != QC_OK) return rc;   // rhf.rs:152-167
        }
        st->tm.build_issued(false, 0.0, S->assign.gen);
        return QC_OK;
    }
    qc_stamp("ev0");
    const int tunes0 = S->assign.tune_count;
    const double tt0 = qc_now_ms();
    if ((rc = qc_fock_build_device(S, st->D[0].p, st->uhf ? st->D[1].p : nullptr, dG, st->uhf ? dGb : nullptr, st->uhf,
                                   &st->twin, W.H.p, sp[0].F, st->uhf ? sp[1].F : nullptr, have_F, st)) != QC_OK) return rc;
    st->tm.build_issued(S->assign.tune_count != tunes0, tt0, S->assign.gen);
    return QC_OK;
}

// enqueues every spin's Roothaan step - on the stream and with the work buffers the plan gives it - and the join the plan names; on
// the generic sequence then the densities and scalars, which the one-workgroup kernels form themselves
static int issue_spins(qc_scf_state *st, const PassPlan &plan, SpinStep *sp, bool have_F) {
    qc_system *S = st->S;
    ScfWork &W = st->W;
    const int n = S->nbasis, nspin = st->uhf ? 2 : 1;
    int rc;
    if (plan.clear_sync_slot && plan.fused) QC_HIP_CHECK(hipMemsetAsync(W.d_sync.p + 2, 0, 2 * sizeof(double), S->stream));       // unused spin slot
    hipStream_t side = plan.side_by_side ? qc_spin_fork(S) : nullptr;
    if (plan.side_by_side && !side) return QC_ERR_HIP;
    for (int s = 0; s < nspin; ++s) {                                     // (the control words were cleared by the previous pass)
        SpinStep &p = sp[s];
        const bool on_side = plan.side_by_side && s == 1;
        if (on_side) { p.st = side; p.b = 1; }
        // (the kernel that hands over and clears the control words: the last spin's kernel when the spins run one after the other)
        if (plan.fused) rc = roothaan_small(S, W, plan, p, have_F, !plan.side_by_side && s == nspin - 1);
        else rc = roothaan_enqueue(W, p, have_F);
        if (rc != QC_OK) return rc;
        if (on_side && !plan.fused) {    // the beta density on the side stream as well; then the streams meet
            if (p.nocc > 0) qc_gemm(side, n, n, p.nocc, 1.0, p.C, n, false, p.C, n, true, 0.0, p.Dn, n);
            else QC_HIP_CHECK(hipMemsetAsync(p.Dn, 0, (size_t)n * n * sizeof(double), side));
            p.dens_done = true;                                           // (the density step below skips it, once)
        }
    }
    if (plan.side_by_side && (rc = plan.fused ? qc_spin_join_end(S, W.ctl.p, plan.ctl_out, plan.seq_wait ? plan.h_seq : nullptr, plan.seq)
                                              : qc_spin_join(S)) != QC_OK) return rc;
    if (plan.fused) return QC_OK;
    if (plan.clear_sync_slot) QC_HIP_CHECK(hipMemsetAsync(W.d_sync.p + 2, 0, 2 * sizeof(double), S->stream));                     // unused spin slot
    // energy and rms straight into pinned host memory; the last spin's kernel also hands over and clears the control words
    for (int s = 0; s < nspin; ++s) if ((rc = density_and_scalars(S, W, plan, sp[s], s == nspin - 1)) != QC_OK) return rc;
    return QC_OK;
}

// enqueues (multi-rank) the scalars' way to the host: complements, all-reduce, copy; then what the next pass's build can do with the new
// densities alone - it starts from Dn, and its density-only preliminaries run while the host turns around
// (`scale_done`: the kernel that formed the density left the build's fixed-point unit as well)
static int publish_and_prepare(qc_scf_state *st, const PassPlan &plan, bool scale_done) {
    qc_system *S = st->S;
    ScfWork &W = st->W;
    if (plan.multi) {
        qc_sync_pack(S->stream, W.d_sync.p, QC_SYNC_WORDS);
        if (qc_rccl().AllReduce(W.d_sync.p, W.d_sync.p, 2 * QC_SYNC_WORDS, ncclUint64, ncclMax, (ncclComm_t)S->comm, S->stream) != ncclSuccess) return QC_ERR_RCCL;
        QC_HIP_CHECK(hipMemcpyAsync(W.h_scal, W.d_sync.p, 2 * QC_SYNC_WORDS * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    }
    return st->stored ? QC_OK : qc_fock_prepare_device(S, st->Dn[0].p, st->uhf ? st->Dn[1].p : nullptr, st->uhf, st, scale_done);
}

// the host's wait for the end of the pass: the sequence word or the event `ev2`, as the plan says
static int wait_pass_end(qc_scf_state *st, const PassPlan &plan, hipEvent_t ev2) {
    if (!plan.seq_wait) return wait_pass(ev2);
    const int rc = wait_pass(ev2, plan.h_seq, plan.seq);
    if (rc != QC_OK) return rc;
    st->pass_seq = plan.seq;
    // The word says that the pass's last kernel is through.  If the preliminaries of the next build were put behind it (UHF: density
    // sum and fixed-point unit; a memset after a mode change), the next build's side streams - which start without a fork event -
    // must not overtake them: then the event behind them is waited for as well.  (RHF on this path has nothing there: the kernel
    // leaves the fixed-point unit itself and the fold left the planes clean.)
    return !st->stored && st->S->prep.enqueued ? wait_pass(ev2) : QC_OK;
}

// what the host makes of a pass, or of its repeat, once it has waited for it; enqueues nothing
// (`first`: the DIIS word is looked at after the pass itself only - a repeat runs no DIIS)
static int pass_verdict(qc_scf_state *st, const PassPlan &plan, bool first) {
    qc_system *S = st->S;
    int rc;
    if ((rc = qc_join_check(S)) != QC_OK) return rc;                     // (the join of this pass's build is in front of everything waited for)
    qc_gate_quiet(S);                                                    // (nothing of this handle waits on the device any more)
    const unsigned long long *w = reinterpret_cast<const unsigned long long *>(st->W.h_scal);
    for (int i = 0; plan.multi && i < QC_SYNC_WORDS; ++i)
        if (w[QC_SYNC_WORDS + i] != ~w[i]) { fprintf(stderr, "qchem_hip: rank %d: the ranks' SCF scalars differ - replicated state diverged\n", S->rank); return QC_ERR_RCCL; }
    if (first && plan.h_ctl[QC_CTL_DIIS] != 0) return QC_DIIS_SINGULAR;            // "DIIS failed", rhf.rs:73
    if (plan.h_ctl[QC_CTL_NOTCONV] != 0) return QC_EIG_NOT_CONVERGED;              // (a repeat: it ran out of sweeps, no vectors to go on with)
    return QC_OK;
}

// QC_SCF_DEBUG: the pass's control words and host times, and its DIIS coefficients (diis.rs:50-51), newest sample first
static void debug_pass(const qc_scf_state *st, const PassPlan &plan, double us_enqueue, double us_waited) {
    const ScfWork &W = st->W;
    const int *const ea = plan.h_ctl + QC_CTL_EIG, *const eb = ea + QC_CTL_EIG_STRIDE;
    fprintf(stderr, "[scf] ctl a: %d %d %d %d  b: %d %d %d %d  npass %d %d have_prev %d mode %d cold %d | host enqueue %.0f us, then waited %.0f us\n", ea[QC_EIG_STATE], ea[QC_EIG_LAST], ea[QC_EIG_CLEAN], ea[QC_EIG_PASSES], eb[QC_EIG_STATE], eb[QC_EIG_LAST], eb[QC_EIG_CLEAN], eb[QC_EIG_PASSES], W.npass[0], W.npass[1], (int)W.have_prev[0], W.mode[0], (int)W.cold[0], us_enqueue, us_waited);
    double c[12] = {0};
    const int m = (int)st->diis[0]->slots.size();
    (void)hipMemcpy(c, st->diis[0]->d_c.p, m * sizeof(double), hipMemcpyDeviceToHost);
    fprintf(stderr, "[scf] diis c:");
    for (int j = 0; j < m; ++j) fprintf(stderr, " %.3e", c[j]);
    fprintf(stderr, "\n");
}

// The refinement passes of the next eigensolve follow what this one needed; a spin whose refinement wanted rotations (large step, or a
// degenerate cluster) has its eigensolve repeated the careful way: enqueues, per such spin, the eigensolve and the density and scalars
// again, then the hand-over, the scalars' way to the host and the next build's preliminaries once more, and waits.  *redo: it happened.
static int repeat_eigensolves(qc_scf_state *st, const PassPlan &plan, SpinStep *sp, hipEvent_t *ev, bool *redo) {
    qc_system *S = st->S;
    ScfWork &W = st->W;
    hipStream_t sm = S->stream;
    int rc;
    for (int s = 0; s < (st->uhf ? 2 : 1); ++s) {
        const bool refined = W.cold[s] || (W.have_prev[s] && W.mode[s] == 0);       // the eigensolve reported through the control word
        if (!refined) continue;
        const int *const eig = plan.h_ctl + QC_CTL_EIG + QC_CTL_EIG_STRIDE * s;
        if (eig[QC_EIG_STATE] == QC_EIG_DONE) { W.npass[s] = W.cold[s] ? 3 : std::max(1, std::min(3, eig[QC_EIG_PASSES])); continue; }
        W.npass[s] = 3;
        // (this pass's times are read first, once, and its second event is recorded again: the repeat counts as linear algebra)
        if (!*redo) { st->tm.flush(st->tuner()); QC_HIP_CHECK(hipEventRecord(ev[1], sm)); }
        if ((rc = roothaan_redo_eig(S, W, sp[s])) != QC_OK) return rc;
        if ((rc = density_and_scalars(S, W, plan, sp[s], false)) != QC_OK) return rc;
        *redo = true;
    }
    if (!*redo) return QC_OK;
    st->redos += 1;
    // the repeated eigensolves report through the same control words (Jacobi sweeps exhausted: QC_CTL_NOTCONV): hand them over again,
    // whichever spin was repeated, and clear them for the next pass
    QC_HIP_CHECK(hipMemcpyAsync(plan.ctl_out, W.ctl.p, QC_CTL_WORDS * sizeof(int), hipMemcpyDefault, sm));
    QC_HIP_CHECK(hipMemsetAsync(W.ctl.p, 0, QC_CTL_WORDS * sizeof(int), sm));
    if ((rc = publish_and_prepare(st, plan, false)) != QC_OK) return rc;  // (the density changed)
    QC_HIP_CHECK(hipEventRecord(ev[2], sm));
    if ((rc = wait_pass(ev[2])) != QC_OK) return rc;
    if ((rc = pass_verdict(st, plan, false)) != QC_OK) return rc;
    st->tm.repeat_seen();
    return QC_OK;
}

// accepts the pass: energy and rms from the scalars, the eigensolve of the next pass, new density and vectors become the current ones
static void accept_pass(qc_scf_state *st, bool redo, double *energy, double *rms_out) {
    ScfWork &W = st->W;
    const int nspin = st->uhf ? 2 : 1;
    double rms_sum = 0.0, e_sum = 0.0;
    for (int s = 0; s < nspin; ++s) {
        const double rms_s = std::sqrt(W.h_scal[2 * s + 1] / W.n);
        e_sum += W.h_scal[2 * s]; rms_sum += rms_s;
        // the refinement is perturbative: on its own once the density has nearly stopped moving, behind two Jacobi sweeps
        // while it still moves, not at all in the first wild passes
        // (the one-workgroup path of small matrices pays 150 us for a cold start and nothing extra for a refinement pass that turns out to
        // be needed: it refines from the previous vectors one decade earlier - H2O/cc-pVTZ: one cold pass less per run, no repeats;
        // benzene at 1e-2: two repeated eigensolves per run, slower than 1e-3)
        const double warm_rms = st->warm_rms_env > 0.0 ? st->warm_rms_env : (W.small_fused ? 1e-2 : 1e-3);
        W.mode[s] = rms_s >= 1.0 ? 2 : (rms_s >= warm_rms || redo) ? 1 : 0;
        std::swap(st->D[s].p, st->Dn[s].p);                              // D += 1.0 * dD
        std::swap(W.CpPrev[s].p, W.CpNew[s].p);
        W.have_prev[s] = true;
    }
    st->passes += 1;
    if (energy) *energy = e_sum;
    if (rms_out) *rms_out = st->uhf ? rms_sum / 2.0 : rms_sum;
}

// one pass of the loop body.  RHF: rhf.rs:67-88.  UHF: uhf.rs:81-137 (returns the reference's `density_rms`,
// i.e. (rms_a + rms_b) / 2, and the energy expression of uhf.rs:145-153 evaluated every pass).
// The whole pass is enqueued without looking at the device; one synchronisation at its end returns the energy, the rms
// and the control words (DIIS failure, eigen-refinement outcome).  Launch latency of ~50 small kernels then overlaps with
// their execution instead of adding to it.
static int scf_iterate(qc_scf_state *st, double *energy, double *rms_out) {
    qc_system *S = st->S;
    hipStream_t sm = S->stream;
    int rc;
    const double th0 = qc_now_ms();
    qc_stamp("enter pass");
    if ((rc = qc_tl_begin_pass(S)) != QC_OK) return rc;
    hipEvent_t *const ev = st->tm.begin_pass();                           // start | build done | pass done
    const PassPlan plan = plan_pass(st);
    SpinStep sp[2] = {spin_step(st, plan, 0), st->uhf ? spin_step(st, plan, 1) : SpinStep{}};
    bool have_F = false, redo = false;
    if ((rc = build_G(st, ev[0], sp, &have_F)) != QC_OK) return rc;
    qc_stamp("build out");
    st->tm.flush(st->tuner());                                            // (the previous pass's times, now that this pass's build is out)
    QC_HIP_CHECK(hipEventRecord(ev[1], sm));
    qc_stamp("flush timing, ev1");
    if ((rc = issue_spins(st, plan, sp, have_F)) != QC_OK) return rc;
    if ((rc = publish_and_prepare(st, plan, plan.scale_in_kernel)) != QC_OK) return rc;
    qc_stamp("roothaan out");
    QC_HIP_CHECK(hipEventRecord(ev[2], sm));
    qc_stamp("ev2");
    const double th1 = qc_now_ms();
    if ((rc = wait_pass_end(st, plan, ev[2])) != QC_OK) return rc;
    const double th2 = qc_now_ms();
    qc_stamp("pass seen");
    if ((rc = pass_verdict(st, plan, true)) != QC_OK) return rc;
    static const bool dbg = getenv("QC_SCF_DEBUG") != nullptr;
    if (dbg) debug_pass(st, plan, (th1 - th0) * 1e3, (th2 - th1) * 1e3);
    st->tm.pass_seen();
    if ((rc = repeat_eigensolves(st, plan, sp, ev, &redo)) != QC_OK) return rc;
    accept_pass(st, redo, energy, rms_out);
    if (st->solv) {                                                       // the reaction field of the new density, and this pass's energy by its definition
        double corr = 0.0;
        if ((rc = solvent_update(st, &corr)) != QC_OK) return rc;
        if (energy) *energy += corr;
    }
    qc_stamp("pass end");
    qc_stamp_flush();
    return QC_OK;
}

static int scf_run(qc_system *S, const qc_hf_config *cfg, qc_hf_output *out, bool uhf) {
    if (!S || !cfg || !out || !out->orbital_energies || (uhf && !out->orbital_energies_beta)) return QC_ERR_INVALID;
    const double t_begin = qc_now_ms();
    qc_scf_state *st = nullptr;
    int rc = scf_begin(S, uhf, cfg->n_alpha, cfg->n_beta, &st);
    if (rc != QC_OK) return rc;
    struct Del { void operator()(qc_scf_state *p) const { scf_state_delete(p); } };
    std::unique_ptr<qc_scf_state, Del> guard(st);
    const int n = S->nbasis;
    out->nuclear_repulsion = qc_nuclear_repulsion(S);                    // rhf.rs:39
    out->electronic_energy = 0.0; out->iterations = 0;
    int status = QC_NOT_CONVERGED;
    for (size_t it = 0; it <= cfg->max_iterations; ++it) {               // inclusive range, rhf.rs:66 / uhf.rs:80
        double e = 0.0, rms = 0.0;
        rc = scf_iterate(st, &e, &rms);
        if (rc != QC_OK) { status = rc; break; }
        // the reference's per-iteration log line (rhf.rs:90-92, uhf.rs:138; `log::info!`, silent unless a logger is installed): QC_LOG=1
        static const bool log_info = getenv("QC_LOG") != nullptr;
        if (log_info) fprintf(stderr, "iteration %-4zu - electronic energy %1.4f. density rms %1.4e\n", it, e, rms);
        const bool conv = uhf ? (rms / 2.0 < cfg->epsilon) : (rms < cfg->epsilon);   // uhf.rs:139 / rhf.rs:94
        if (conv) {
            out->electronic_energy = e; out->iterations = it;
            QC_HIP_CHECK(hipMemcpy(out->orbital_energies, st->ws.p, n * sizeof(double), hipMemcpyDeviceToHost));
            if (uhf) QC_HIP_CHECK(hipMemcpy(out->orbital_energies_beta, st->ws.p + n, n * sizeof(double), hipMemcpyDeviceToHost));
            if (st->solv) { st->solv->last = {st->solv_out[0], st->solv_out[1], st->solv_out[2], st->solv->M}; st->solv->have_last = true; }
            status = QC_OK;
            break;
        }
    }
    st->tm.flush(st->tuner());
    out->ms_setup = st->ms_setup; out->ms_fock_total = st->tm.ms_fock; out->ms_linalg_total = st->tm.ms_linalg;
    out->ms_total = qc_now_ms() - t_begin;
    out->ms_tuner = st->tm.ms_tuner;
    return status;
}

// What a direct Fock build outside the SCF loop overwrites on the handle, saved and put back around it: the fixed-point unit (the
// one-workgroup Roothaan path leaves the unit of the NEXT pass's build there, PassPlan::scale_in_kernel), the UHF density sum of a prepared
// build, and the flags that let the next pass's build skip its preliminaries.  (The accumulator planes need nothing: every build's
// closing fold leaves them zero, whatever its layout.)  With this a later qc_scf_iterate is bit for bit what it would have been.
namespace {
struct FockPrepSave {
    qc_system *S;
    DevBuf fxs, Dj;
    const QcPrepared prep;
    explicit FockPrepSave(qc_system *S_) : S(S_), prep(S_->prep) {}
    int save() {
        const size_t nn = (size_t)S->nbasis * S->nbasis;
        if (fxs.alloc(2) != QC_OK || Dj.alloc(nn) != QC_OK) return QC_ERR_HIP;
        QC_HIP_CHECK(hipStreamSynchronize(S->stream));
        QC_HIP_CHECK(hipMemcpyAsync(fxs.p, S->dev.d_fxs.p, 2 * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        QC_HIP_CHECK(hipMemcpyAsync(Dj.p, S->dev.d_Dj.p, nn * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        return QC_OK;
    }
    int restore() {
        const size_t nn = (size_t)S->nbasis * S->nbasis;
        QC_HIP_CHECK(hipMemcpyAsync(S->dev.d_fxs.p, fxs.p, 2 * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        QC_HIP_CHECK(hipMemcpyAsync(S->dev.d_Dj.p, Dj.p, nn * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
        QC_HIP_CHECK(hipStreamSynchronize(S->stream));
        // (a build that ran in between left the planes clean for ITS layout; the saved flags speak of the state's layout, which is zero too)
        const bool clean = prep.gt_clean && S->prep.gt_clean; S->prep = prep; S->prep.gt_clean = clean;
        return QC_OK;
    }
};
// runs `call` between save and restore.  A failed restore counts unless the call failed (rc < 0) or, `status_first`, returned any status
template <class F> int with_fock_prep_saved(qc_system *S, bool status_first, F call) {
    FockPrepSave keep(S);
    int rc = keep.save();
    if (rc != QC_OK) return rc;
    rc = call();
    const int rc2 = keep.restore();
    return status_first ? (rc != QC_OK ? rc : rc2) : (rc < 0 ? rc : (rc2 != QC_OK ? rc2 : rc));
}
// the guard of the post-SCF entry points that work from a pass's C and orbital energies on one rank
int ran_on_one_rank(const qc_scf_state *st) {
    if (st->passes == 0) return QC_ERR_INVALID;
    return st->S->comm || st->S->nranks != 1 ? QC_ERR_UNSUPPORTED : QC_OK;
}
}  // namespace

extern "C" {

int qc_scf_begin_rhf(qc_system *S, qc_scf_state **out) { return scf_begin(S, false, 0, 0, out); }
int qc_scf_begin_uhf(qc_system *S, int n_alpha, int n_beta, qc_scf_state **out) { return scf_begin(S, true, n_alpha, n_beta, out); }
int qc_scf_iterate(qc_scf_state *st, double *electronic_energy, double *density_rms) {
    if (!st) return QC_ERR_INVALID;
    return scf_iterate(st, electronic_energy, density_rms);
}
int qc_scf_orbital_energies(qc_scf_state *st, int spin, double *out) {
    if (!st || !out || spin < 0 || spin > (st->uhf ? 1 : 0)) return QC_ERR_INVALID;
    QC_HIP_CHECK(hipMemcpy(out, st->ws.p + (size_t)spin * st->S->nbasis, st->S->nbasis * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}
int qc_scf_density(qc_scf_state *st, int spin, double *out) {
    if (!st || !out || spin < 0 || spin > (st->uhf ? 1 : 0)) return QC_ERR_INVALID;
    const size_t nn = (size_t)st->S->nbasis * st->S->nbasis;
    QC_HIP_CHECK(hipMemcpy(out, st->D[spin].p, nn * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}
int qc_scf_coefficients(qc_scf_state *st, int spin, double *out) {
    if (!st || !out || spin < 0 || spin > (st->uhf ? 1 : 0) || st->passes == 0) return QC_ERR_INVALID;
    const size_t nn = (size_t)st->S->nbasis * st->S->nbasis;
    QC_HIP_CHECK(hipStreamSynchronize(st->S->stream));
    QC_HIP_CHECK(hipMemcpy(out, st->Cs.p + spin * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}
int qc_scf_mp2(qc_scf_state *st, int32_t n_frozen, qc_mp2_output *out) {
    if (!st || !out || st->passes == 0) return QC_ERR_INVALID;
    qc_system *S = st->S;
    const int n = S->nbasis, nspin = st->uhf ? 2 : 1;
    std::vector<double> eps((size_t)nspin * n);
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    QC_HIP_CHECK(hipMemcpy(eps.data(), st->ws.p, eps.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int32_t nocc[2] = {st->nocc[0], st->nocc[1]};
    int rc = qc_mp2_validate(n, nspin, eps.data(), nocc, n_frozen);
    if (rc != QC_OK) return rc;
    return qc_mp2_device(S, nspin, st->Cs.p, st->ws.p, nocc, n_frozen, out);   // (reads Cs / ws, writes nothing of the state)
}
int qc_scf_gradient(qc_scf_state *st, double *grad) {
    if (!st || !grad) return QC_ERR_INVALID;
    if (st->solv) return QC_ERR_UNSUPPORTED;                             // (no cavity derivative)
    int rc = ran_on_one_rank(st);
    if (rc != QC_OK) return rc;
    qc_system *S = st->S;
    const int n = S->nbasis, nspin = st->uhf ? 2 : 1, na3 = 3 * S->natoms;
    const size_t nn = (size_t)n * n;
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    DevBuf dP, dW;
    if (dP.alloc(nspin * nn) != QC_OK || dW.alloc(nn) != QC_OK) return QC_ERR_HIP;
    hipEvent_t ev[2];
    for (auto &e : ev) QC_HIP_CHECK(hipEventCreate(&e));
    struct EvDel { hipEvent_t *e; ~EvDel() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } evdel{ev};
    // P: the state's own density, exactly what qc_scf_density returns; W from the C and orbital energies the state reports
    QC_HIP_CHECK(hipEventRecord(ev[0], S->stream));
    for (int s = 0; s < nspin; ++s) QC_HIP_CHECK(hipMemcpyAsync(dP.p + s * nn, st->D[s].p, nn * sizeof(double), hipMemcpyDeviceToDevice, S->stream));
    const int nocc[2] = {st->nocc[0], st->nocc[1]};
    if ((rc = qc_gradient_w_device(S, nspin, st->Cs.p, st->ws.p, nocc, dW.p)) != QC_OK) return rc;   // (reads Cs / ws, writes nothing of the state)
    QC_HIP_CHECK(hipEventRecord(ev[1], S->stream));
    std::vector<double> t((size_t)4 * na3);
    qc_nuclear_gradient(S, t.data());
    if ((rc = qc_gradient_device(S, nspin, dP.p, dW.p, t.data() + na3, S->grad_ms)) != QC_OK) return rc;
    float pw = 0.f;
    QC_HIP_CHECK(hipEventElapsedTime(&pw, ev[0], ev[1]));
    S->grad_ms[0] += pw;                                                    // (phase 0: P/W build + Cartesian transform)
    for (int k = 0; k < na3; ++k) grad[k] = ((t[k] + t[na3 + k]) + t[2 * na3 + k]) + t[3 * na3 + k];
    if (st->pc.empty()) return QC_OK;
    // an embedded state: + dE_nq/dR_A + the basis-function derivatives of tr(P_t V_pc), for the charges the state began with
    std::vector<double> gn(na3), ge(na3);
    if (nspin == 2) qc_axpby(S->stream, n, 1.0, dP.p, 1.0, dP.p + nn, dP.p);
    if ((rc = qc_pc_atom_gradient_device(S, st->pc, dP.p, ge.data())) != QC_OK) return rc;
    qc_pc_nuclear_gradient(S, st->pc, gn.data(), nullptr);
    for (int k = 0; k < na3; ++k) grad[k] += gn[k] + ge[k];
    return QC_OK;
}

int qc_scf_stability_dim(qc_scf_state *st, int kind) {
    if (!st || kind < 0 || kind > (st->uhf ? 0 : 1)) return QC_ERR_INVALID;
    return qc_stability_dim(st->S->nbasis, st->uhf, st->nocc);
}
int qc_scf_stability(qc_scf_state *st, qc_stability *io, double *vectors) {
    if (!st || !io) return QC_ERR_INVALID;
    if (st->solv) return QC_ERR_UNSUPPORTED;                             // (the Hessian lacks the solvent's response term; so do the four below)
    if (io->kind < 0 || io->kind > (st->uhf ? 0 : 1) || io->nroots < 1 || io->nroots > 8 || io->max_iterations < 0 || !(io->tol >= 0.0)) return QC_ERR_INVALID;
    qc_system *S = st->S;
    const int dim = qc_stability_dim(S->nbasis, st->uhf, st->nocc);
    if (dim <= 0 || io->nroots > dim) return QC_ERR_INVALID;
    const int rc = ran_on_one_rank(st);
    if (rc != QC_OK) return rc;
    // (reads Cs / ws, writes nothing of the state)
    return with_fock_prep_saved(S, false, [&] { return qc_stability_device(S, st->uhf, st->nocc, st->Cs.p, st->ws.p, io, vectors); });
}
int qc_scf_rotated_density(qc_scf_state *st, int kind, const double *x, double angle, double *Da, double *Db, double *energy) {
    if (!st || !x || !Da || !Db || kind < 0 || kind > (st->uhf ? 0 : 1) || angle != angle) return QC_ERR_INVALID;
    if (st->solv) return QC_ERR_UNSUPPORTED;
    qc_system *S = st->S;
    if (qc_stability_dim(S->nbasis, st->uhf, st->nocc) <= 0) return QC_ERR_INVALID;
    const int rc = ran_on_one_rank(st);
    if (rc != QC_OK) return rc;
    return with_fock_prep_saved(S, true, [&] { return qc_rotated_density_device(S, st->uhf, kind, st->nocc, st->Cs.p, st->W.H.p, x, angle, Da, Db, energy); });
}
// mu_k = sum_A Z_A (R_A - O)_k - tr(P_t M_k): the nuclear part on the host, the trace by a fixed-order reduction on the device
int qc_scf_dipole(qc_scf_state *st, const double *origin, double mu[3], double mu_nuclear[3]) {
    if (!st || !mu) return QC_ERR_INVALID;
    qc_system *S = st->S;
    const double zero[3] = {0.0, 0.0, 0.0};
    const double *O = origin ? origin : zero;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    double nuc[3] = {0.0, 0.0, 0.0}, tr[3];
    for (int a = 0; a < S->natoms; ++a) for (int k = 0; k < 3; ++k) nuc[k] += S->Z[a] * (S->xyz[3 * a + k] - O[k]);
    DevBuf M;
    if (M.alloc(3 * nn) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    int rc = qc_dipole_device(S, O, M.p);
    if (rc != QC_OK) return rc;
    if ((rc = qc_dipole_trace_device(S, st->D[0].p, st->uhf ? st->D[1].p : nullptr, M.p, tr)) != QC_OK) return rc;
    for (int k = 0; k < 3; ++k) { mu[k] = nuc[k] - tr[k]; if (mu_nuclear) mu_nuclear[k] = nuc[k]; }
    return QC_OK;
}
// total Cartesian moments up to io->order: the nuclear sums on the host, tr(P_t M_c) by the fixed-order trace on the device
int qc_scf_multipoles(qc_scf_state *st, qc_multipoles *io) {
    if (!st || !io || qc_multipole_count(io->order) < 0) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const int count = qc_multipole_count(io->order);
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    const double *O = io->origin;
    double tr[35];
    for (int c = 0; c < 35; ++c) io->total[c] = io->nuclear[c] = io->electronic[c] = 0.0;
    for (double &q : io->quadrupole_traceless) q = 0.0;
    for (int a = 0; a < S->natoms; ++a) {
        double pw[3][QC_MULTIPOLE_MAX_ORDER + 1];
        for (int k = 0; k < 3; ++k) { pw[k][0] = 1.0; for (int m = 1; m <= io->order; ++m) pw[k][m] = pw[k][m - 1] * (S->xyz[3 * a + k] - O[k]); }
        for (int c = 0, l = 0; l <= io->order; ++l)
            for (int i = l; i >= 0; --i)
                for (int j = l - i; j >= 0; --j, ++c) io->nuclear[c] += S->Z[a] * (pw[0][i] * pw[1][j] * pw[2][l - i - j]);
    }
    DevBuf M;
    if (M.alloc(count * nn) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    int rc = qc_multipole_device(S, io->order, O, M.p);
    if (rc != QC_OK) return rc;
    if ((rc = qc_multipole_trace_device(S, count, st->D[0].p, st->uhf ? st->D[1].p : nullptr, M.p, tr)) != QC_OK) return rc;
    for (int c = 0; c < count; ++c) { io->electronic[c] = -tr[c]; io->total[c] = io->nuclear[c] - tr[c]; }
    if (io->order >= 2) {
        const double *Q = io->total + 4, t = Q[0] + Q[3] + Q[5];           // xx xy xz yy yz zz
        for (int k = 0; k < 6; ++k) io->quadrupole_traceless[k] = 0.5 * (3.0 * Q[k] - ((k == 0 || k == 3 || k == 5) ? t : 0.0));
    }
    return QC_OK;
}
// populations of the state's densities with its own S and X, where they lie on the device (qc_population.hip)
int qc_scf_populations(qc_scf_state *st, int scheme, double *charges, double *spin, double *orbital, double *bond_orders) {
    if (!st || !charges || scheme < 0 || scheme > 1) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    std::vector<double> Nt(S->natoms), Ns(S->natoms);
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    const int rc = qc_population_device(S, scheme, st->D[0].p, st->uhf ? st->D[1].p : nullptr, st->W.S.p, st->W.X.p, Nt.data(), Ns.data(), orbital, bond_orders);
    if (rc != QC_OK) return rc;
    for (int a = 0; a < S->natoms; ++a) { charges[a] = S->Z[a] - Nt[a]; if (spin) spin[a] = Ns[a]; }
    return QC_OK;
}
// charges fitted to the state's potential on the library's grid or the caller's points: the V of qc_scf_esp_on_points, then the host fit
int qc_scf_esp_charges(qc_scf_state *st, qc_esp_fit *io, int64_t npts, const double *xyz, double *charges, double *v_out) {
    int nscales; double scales[8], density;
    if (!st || !io || !charges || (xyz && npts < 0) || !qc_espfit_config(io, &nscales, scales, &density)) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (xyz && npts < S->natoms) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const double t0 = qc_now_ms();
    std::vector<double> grid;
    if (!xyz) {
        qc_espfit_grid(S, nscales, scales, density, grid);
        xyz = grid.data(); npts = (int64_t)(grid.size() / 3);
        if (npts < S->natoms) return QC_ERR_INVALID;
    }
    std::vector<double> v(npts);
    int rc = qc_scf_esp_on_points(st, npts, xyz, v.data(), nullptr);
    if (rc != QC_OK) return rc;
    const double t1 = qc_now_ms();
    int nz = 0;
    for (int a = 0; a < S->natoms; ++a) nz += S->Z[a];
    if ((rc = qc_espfit_solve(S, npts, xyz, v.data(), (double)(nz - st->nocc[0] - st->nocc[1]), io, charges)) != QC_OK) return rc;
    if (v_out) std::copy(v.begin(), v.end(), v_out);
    io->ms_potential = t1 - t0; io->ms_total = qc_now_ms() - t0;
    return QC_OK;
}
// ---- values on points from the state's own densities and orbitals (qc_points.hip): they are read where they lie on the device; no Fock
// build runs and nothing of the state or of a prepared build is written, so a following qc_scf_iterate is unchanged.
// The state's density P_alpha + w P_beta on the device: the RHF pointer where it lies (its density is the total one), or the UHF sum,
// enqueued on the handle's stream, in `sum`.  Null: the allocation failed.
static const double *state_density(qc_scf_state *st, double w, DevBuf &sum) {
    if (!st->uhf) return st->D[0].p;
    qc_system *S = st->S;
    if (sum.alloc((size_t)S->nbasis * S->nbasis) != QC_OK) return nullptr;
    qc_axpby(S->stream, S->nbasis, 1.0, st->D[0].p, w, st->D[1].p, sum.p);
    return sum.p;
}
// which 0: P_alpha + P_beta, 1: P_alpha - P_beta (an RHF state: exactly zero, nothing is launched)
int qc_scf_density_on_points(qc_scf_state *st, int which, int64_t npts, const double *xyz, double *rho) {
    if (!st || !xyz || !rho || npts < 0 || which < 0 || which > 1) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (npts == 0) return QC_OK;
    if (!st->uhf && which == 1) { std::fill(rho, rho + npts, 0.0); return QC_OK; }
    DevBuf sum;
    const double *P = state_density(st, which ? -1.0 : 1.0, sum);
    return P ? qc_points_density_device(S, P, npts, xyz, rho) : QC_ERR_HIP;
}
// v_total = v_nuc + v_elec of P_alpha + P_beta; the nuclear part on the host, as in qc_scf_dipole
int qc_scf_esp_on_points(qc_scf_state *st, int64_t npts, const double *xyz, double *v_total, double *v_elec) {
    if (!st || !xyz || !v_total || npts < 0) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (npts == 0) return QC_OK;
    DevBuf sum;
    const double *P = state_density(st, 1.0, sum);
    if (!P) return QC_ERR_HIP;
    std::vector<double> ve(npts);
    const int rc = qc_points_esp_device(S, P, npts, xyz, ve.data());
    if (rc != QC_OK) return rc;
    qc_points_vnuc(S, npts, xyz, v_total);
    for (int64_t k = 0; k < npts; ++k) { v_total[k] += ve[k]; if (v_elec) v_elec[k] = ve[k]; }
    return QC_OK;
}
// the field of the molecule alone, E = -grad V of qc_scf_esp_on_points: e_total = e_nuc + e_elec, npts x 3 each
int qc_scf_field_on_points(qc_scf_state *st, int64_t npts, const double *xyz, double *e_total, double *e_elec) {
    if (!st || !xyz || !e_total || npts < 0) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (npts == 0) return QC_OK;
    DevBuf sum;
    const double *P = state_density(st, 1.0, sum);
    if (!P) return QC_ERR_HIP;
    std::vector<double> ee(3 * (size_t)npts);
    const int rc = qc_points_field_device(S, P, npts, xyz, ee.data(), S->points_ms);
    if (rc != QC_OK) return rc;
    qc_points_enuc(S, npts, xyz, e_total);
    for (int64_t k = 0; k < 3 * npts; ++k) { e_total[k] += ee[k]; if (e_elec) e_elec[k] = ee[k]; }
    return QC_OK;
}
// dE/dR_c = -q_c E_total(R_c) for the charges the state began with, npc x 3
int qc_scf_point_charge_gradient(qc_scf_state *st, double *grad) {
    if (!st || !grad) return QC_ERR_INVALID;
    qc_system *S = st->S;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    const int64_t npc = (int64_t)(st->pc.size() / 4);
    if (npc == 0) return QC_OK;
    std::vector<double> xyz(3 * (size_t)npc);
    for (int64_t c = 0; c < npc; ++c) for (int k = 0; k < 3; ++k) xyz[3 * c + k] = st->pc[4 * c + k];
    const int rc = qc_scf_field_on_points(st, npc, xyz.data(), grad, nullptr);
    if (rc != QC_OK) return rc;
    for (int64_t c = 0; c < npc; ++c) for (int k = 0; k < 3; ++k) grad[3 * c + k] *= -st->pc[4 * c + 3];
    return QC_OK;
}
// the reaction field that goes with the state's current density (solvent_update)
int qc_scf_solvent(qc_scf_state *st, qc_solvent_energy *out, double *q) {
    if (!st || !out || !st->solv) return QC_ERR_INVALID;
    *out = {st->solv_out[0], st->solv_out[1], st->solv_out[2], st->solv->M};
    if (q) std::copy(st->solv_q.begin(), st->solv_q.end(), q);
    return QC_OK;
}
int64_t qc_scf_point_charge_count(const qc_scf_state *st) { return st ? (int64_t)(st->pc.size() / 4) : QC_ERR_INVALID; }
double qc_scf_point_charge_nuclear_energy(const qc_scf_state *st) { return st ? qc_pc_nuclear_energy(st->S, st->pc) : 0.0; }
// orbitals first .. first + count - 1 of `spin`, counted from 0 in the order of qc_scf_orbital_energies; out: count x npts
int qc_scf_orbitals_on_points(qc_scf_state *st, int spin, int first, int count, int64_t npts, const double *xyz, double *out) {
    if (!st || !xyz || !out || npts < 0 || spin < 0 || spin > (st->uhf ? 1 : 0)) return QC_ERR_INVALID;
    qc_system *S = st->S;
    const int n = S->nbasis;
    if (first < 0 || count <= 0 || first >= n || count > n - first || st->passes == 0) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (npts == 0) return QC_OK;
    return qc_points_orbitals_device(S, count, st->Cs.p + (size_t)spin * n * n + first, n, npts, xyz, out);
}

int qc_scf_polarizability(qc_scf_state *st, qc_polarizability *io, double *response) {
    if (!st || !io || io->max_iterations < 0 || !(io->tol >= 0.0)) return QC_ERR_INVALID;
    if (st->solv) return QC_ERR_UNSUPPORTED;
    qc_system *S = st->S;
    const int rc = ran_on_one_rank(st);
    if (rc != QC_OK) return rc;
    // (reads Cs / ws, writes nothing of the state)
    return with_fock_prep_saved(S, false, [&] { return qc_polarizability_device(S, st->uhf, st->nocc, st->Cs.p, st->ws.p, io, response); });
}
// CIS / TDHF from MO integrals: like qc_scf_mp2 the calls read Cs / ws and run no Fock build, so nothing of the handle needs saving
int qc_scf_excitations(qc_scf_state *st, qc_excitations *io, double *vectors) {
    if (!st || !io || st->passes == 0) return QC_ERR_INVALID;
    if (io->method < 0 || io->method > 1 || io->kind < 0 || io->kind > 1 || io->nroots < 1 || io->nroots > 8 || io->max_iterations < 0 || !(io->tol >= 0.0))
        return QC_ERR_INVALID;
    if (st->uhf || st->solv) return QC_ERR_UNSUPPORTED;
    qc_system *S = st->S;
    const int dim = qc_stability_dim(S->nbasis, false, st->nocc);
    if (dim <= 0 || io->nroots > dim) return QC_ERR_INVALID;
    if (const int rc = ran_on_one_rank(st)) return rc;                  // (a pass has run, see above: the number of ranks)
    return qc_excitations_device(S, st->nocc[0], st->Cs.p, st->ws.p, io, vectors);
}
int qc_scf_excitation_matrices(qc_scf_state *st, int kind, double *ApB, double *AmB) {
    if (!st || st->passes == 0 || kind < 0 || kind > 1) return QC_ERR_INVALID;
    if (st->uhf || st->solv) return QC_ERR_UNSUPPORTED;
    qc_system *S = st->S;
    if (qc_stability_dim(S->nbasis, false, st->nocc) <= 0) return QC_ERR_INVALID;
    if (const int rc = ran_on_one_rank(st)) return rc;                  // (a pass has run, see above: the number of ranks)
    return qc_excitation_matrices_device(S, st->nocc[0], st->Cs.p, st->ws.p, kind, ApB, AmB);
}
// closed-shell CCSD from MO integrals: like qc_scf_mp2 the call reads Cs / ws and runs no Fock build
int qc_scf_ccsd(qc_scf_state *st, qc_ccsd *io, double *t1, double *t2) {
    if (!st || !io || st->passes == 0) return QC_ERR_INVALID;
    const int n = st->S->nbasis, nocc = st->nocc[0];
    if (io->n_frozen < 0 || io->n_frozen >= nocc || n - nocc <= 0 || io->max_iterations < 0 || io->diis_size < 0 || io->diis_size > 12 || !(io->tol >= 0.0))
        return QC_ERR_INVALID;
    if (st->uhf || st->solv) return QC_ERR_UNSUPPORTED;
    if (const int rc = ran_on_one_rank(st)) return rc;
    qc_system *S = st->S;
    std::vector<double> eps(n);
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    QC_HIP_CHECK(hipMemcpy(eps.data(), st->ws.p, eps.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int32_t no[2] = {nocc, 0};
    if (const int rc = qc_mp2_validate(n, 1, eps.data(), no, io->n_frozen)) return rc;       // (a denominator >= 0)
    return qc_ccsd_device(S, nocc, st->Cs.p, st->ws.p, io, t1, t2);
}
int qc_debug_gemm(int which, int m, int n, int k, double alpha, const double *A, const double *B, double beta, double *C, int reps, double *ms) {
    if (which < 0 || which > 1 || m < 1 || n < 1 || k < 1 || !A || !B || !C || reps < 0) return QC_ERR_INVALID;
    if (qc_device_ready() != QC_OK) return QC_ERR_NO_DEVICE;
    return qc_debug_gemm_device(which, m, n, k, alpha, A, B, beta, C, reps, ms);
}
int qc_scf_begin_rhf_from(qc_system *S, const double *D, qc_scf_state **out) {
    if (!S || !D || !out) return QC_ERR_INVALID;
    return scf_begin(S, false, 0, 0, out, D, nullptr);
}
int qc_scf_begin_uhf_from(qc_system *S, int n_alpha, int n_beta, const double *Da, const double *Db, qc_scf_state **out) {
    if (!S || !Da || !Db || !out) return QC_ERR_INVALID;
    return scf_begin(S, true, n_alpha, n_beta, out, Da, Db);
}
int qc_scf_matrix(qc_scf_state *st, int which, double *out) {
    if (!st || !out || which < 0 || which > 2) return QC_ERR_INVALID;
    const size_t nn = (size_t)st->S->nbasis * st->S->nbasis;
    const double *src = which == 0 ? st->W.S.p : which == 1 ? (st->solv ? st->Hvac.p : st->W.H.p) : st->W.X.p;   // (a solvated state: the vacuum H)
    QC_HIP_CHECK(hipMemcpy(out, src, nn * sizeof(double), hipMemcpyDeviceToHost));
    return QC_OK;
}
int qc_scf_spin_square(qc_scf_state *st, double *s2) {
    if (!st || !s2) return QC_ERR_INVALID;
    *s2 = 0.0;
    if (!st->uhf) return QC_OK;
    qc_system *S = st->S;
    ScfWork &W = st->W;
    const int n = S->nbasis;
    hipStream_t sm = S->stream;
    qc_gemm(sm, n, n, n, 1.0, st->D[0].p, n, false, W.S.p, n, false, 0.0, W.eig[0].t1.p, n);      // D_alpha S
    qc_gemm(sm, n, n, n, 1.0, st->D[1].p, n, false, W.S.p, n, false, 0.0, W.eig[0].t2.p, n);      // D_beta S
    // tr(A B) = sum_ij A_ij B_ji: one dot product of A with B^T - reuse the DIIS dot kernel on (A, B^T)
    qc_sub_transpose(sm, n, W.eig[0].t2.p, W.eig[0].t3.p);                                                // t3 = B - B^T
    qc_axpby(sm, n, 1.0, W.eig[0].t2.p, -1.0, W.eig[0].t3.p, W.eig[0].t4.p);                                    // t4 = B^T
    const double *ys[1] = {W.eig[0].t4.p};
    qc_dots(sm, n, W.eig[0].t1.p, ys, 1, W.scal.p);
    double tr = 0.0;
    QC_HIP_CHECK(hipMemcpyAsync(&tr, W.scal.p, sizeof(double), hipMemcpyDeviceToHost, sm));
    QC_HIP_CHECK(hipStreamSynchronize(sm));
    const double sz = 0.5 * (st->nocc[0] - st->nocc[1]);
    *s2 = sz * (sz + 1.0) + st->nocc[1] - tr;
    return QC_OK;
}
double qc_scf_tensor_ms(qc_scf_state *st) { return st ? st->ms_tensor : 0.0; }
int qc_scf_timings(qc_scf_state *st, double *ms_setup, double *ms_fock, double *ms_linalg) {
    if (!st) return QC_ERR_INVALID;
    st->tm.flush(st->tuner());
    if (ms_setup) *ms_setup = st->ms_setup;
    if (ms_fock) *ms_fock = st->tm.ms_fock;
    if (ms_linalg) *ms_linalg = st->tm.ms_linalg;
    return QC_OK;
}
void qc_scf_end(qc_scf_state *st) { scf_state_delete(st); }
int qc_scf_set_stop_rule(qc_scf_state *st, double epsilon) {
    if (!st || !(epsilon >= 0.0)) return QC_ERR_INVALID;
    return QC_OK;                                                        // (nothing acts on the rule: see the header)
}
int qc_scf_counters(qc_scf_state *st, double *out, int n) {
    if (!st || !out || n < 0) return QC_ERR_INVALID;
    st->tm.flush(st->tuner());
    const double v[QC_SCF_NCOUNTERS] = {st->ms_setup, st->tm.ms_fock, st->tm.ms_linalg, (double)st->tm.builds_timed, st->tm.ms_tuner, (double)st->passes,
                                        0.0, 0.0 /* reserved */, (double)st->redos,
                                        (double)st->S->assign.on.trials, st->S->assign.on.settled ? 1.0 : 0.0,
                                        (double)st->W.small_steps[0], (double)st->W.small_steps[1], (double)st->W.small_steps[2]};
    for (int i = 0; i < n && i < QC_SCF_NCOUNTERS; ++i) out[i] = v[i];
    return QC_OK;
}

// restricted_hartree_fock (rhf.rs:32-108) / unrestricted_hartree_fock (uhf.rs:36-167)
int qc_scf_rhf(qc_system *S, const qc_hf_config *cfg, qc_hf_output *out) { return scf_run(S, cfg, out, false); }
int qc_scf_uhf(qc_system *S, const qc_hf_config *cfg, qc_hf_output *out) { return scf_run(S, cfg, out, true); }

}  // extern "C"
