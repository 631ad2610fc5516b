// qc_api.cpp - the C ABI (include/qchem_hip.h) and nothing else: system creation, the Fock-build and eigensolver entry points, sharding /
// communicator and profiling entry points.  The SCF drivers and the step API: qc_scf.cpp; the build itself: qc_fock.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qc_embed.h"

namespace {

// hipEvent that is destroyed on every path out of its scope
struct Event {
    hipEvent_t e = nullptr;
    int create() { return hipEventCreate(&e) == hipSuccess ? QC_OK : QC_ERR_HIP; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

// `reps` instrumented passes over the class kernels (launches timed one by one: per class, or per launch unit, summed into `acc`), each
// followed by an un-instrumented whole build whose times are summed into *tot
int profile_builds(qc_system *S, const double *dD, double *dG, int reps, bool per_unit, std::vector<float> &acc, float *tot) {
    const int n = S->nbasis;
    const size_t nn = (size_t)n * n;
    std::vector<float> one(acc.size(), 0.f);
    S->prep.invalidate();
    if (S->accum_fx) qc_fx_scale(S->stream, n, dD, nullptr, S->imax, S->dev.d_fxs.p);
    Event ev0, ev1;
    if (ev0.create() != QC_OK || ev1.create() != QC_OK) return QC_ERR_HIP;
    hipEvent_t e0 = ev0.e, e1 = ev1.e;
    for (int r = 0; r < reps; ++r) {
        QC_HIP_CHECK(hipMemsetAsync(S->dev.d_Gtmp.p, 0, (size_t)2 * QC_NREP * nn * sizeof(double), S->stream));
        QcFockArgs a{};
        a.nrep = QC_NREP; a.rep_stride = nn; a.fxs = S->accum_fx ? S->dev.d_fxs.p : nullptr; a.fx_lo = (size_t)QC_NREP * nn;
        a.Dj = dD; a.Dk0 = dD; a.Dk1 = nullptr; a.cK = 0.5; a.G0 = S->dev.d_Gtmp.p; a.G1 = S->dev.d_Gtmp.p + nn;
        int rc = qc_launch_fock_classes(S, a, per_unit ? nullptr : one.data(), per_unit ? one.data() : nullptr);
        if (rc != QC_OK) return rc;
        for (size_t i = 0; i < acc.size(); ++i) acc[i] += one[i];
        QC_HIP_CHECK(hipEventRecord(e0, S->stream));
        if ((rc = qc_fock_build_device(S, dD, nullptr, dG, nullptr, false)) != QC_OK) return rc;
        QC_HIP_CHECK(hipEventRecord(e1, S->stream));
        QC_HIP_CHECK(hipEventSynchronize(e1));
        float ms; (void)hipEventElapsedTime(&ms, e0, e1); *tot += ms;
    }
    return QC_OK;
}

// Eigenpairs of a host matrix, sorted: the cold eigensolve, or (V0: eigenvectors of a nearby matrix) the refinement from them.
// d_flag[0]: Jacobi sweeps ran out.
int sym_eig_host(qc_system *S, int n, const double *A, const double *V0, double *V, double *w) {
    if (!S || n <= 0 || !w) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)n * n;
    hipStream_t st = S->stream;
    DevBuf dA, dV0, dV, dw;
    QcEigWork E;
    if (dA.alloc(nn) != QC_OK || (V0 && dV0.alloc(nn) != QC_OK) || dV.alloc(nn) != QC_OK || dw.alloc(n) != QC_OK || E.alloc(n) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dA.p, A, nn * sizeof(double), hipMemcpyHostToDevice, st));
    if (V0) QC_HIP_CHECK(hipMemcpyAsync(dV0.p, V0, nn * sizeof(double), hipMemcpyHostToDevice, st));
    int flag = 0;
    QC_HIP_CHECK(hipMemsetAsync(S->dev.d_flag.p, 0, (V0 ? 1 : 4) * sizeof(int), st));
    rc = V0 ? qc_eig_device_refine(st, n, dA.p, dV0.p, dV.p, dw.p, E, S->dev.d_flag.p) : qc_eig_cold_sync(st, n, dA.p, dV.p, dw.p, E, E.ctl.p, S->dev.d_flag.p);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(V, dV.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipMemcpyAsync(w, dw.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipMemcpyAsync(&flag, S->dev.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    QC_HIP_CHECK(hipStreamSynchronize(st));
    return flag ? QC_EIG_NOT_CONVERGED : QC_OK;
}

// the handle's work lists as those of shard (rank, nranks) for the life of this object; its own shard's lists are back when it ends
struct ShardScope {
    qc_system *S; int rank0, nranks0;
    ShardScope(qc_system *S_, int rank, int nranks) : S(S_), rank0(S_->rank), nranks0(S_->nranks) { set(rank, nranks); }
    ~ShardScope() { set(rank0, nranks0); }
    void set(int rank, int nranks) { S->rank = rank; S->nranks = nranks; qc_build_shards(S); }
};

}  // namespace

void qc_system_free(qc_system *S) {
    if (S->comm) { qc_rccl().CommDestroy((ncclComm_t)S->comm); S->comm = nullptr; }
    S->solvent.reset();                      // (its device buffers go before the device side does)
    qc_device_free(S);
    delete S;
}

// =============================================================================================== C ABI
extern "C" {

int qc_system_create(int natoms, const int32_t *Z, const double *xyz, int nshells, const int32_t *shell_atom, const int32_t *shell_L,
                     const int32_t *shell_pure, const int32_t *shell_nprim, const double *exponents, const double *coefficients,
                     qc_system **out) {
    if (!out || natoms <= 0 || nshells <= 0 || !Z || !xyz || !shell_atom || !shell_L || !shell_nprim || !exponents || !coefficients) return QC_ERR_INVALID;
    qc_system *S = new (std::nothrow) qc_system();
    if (!S) return QC_ERR_INVALID;
    S->natoms = natoms; S->nshells = nshells;
    S->Z.assign(Z, Z + natoms);
    S->xyz.assign(xyz, xyz + 3 * natoms);
    size_t po = 0;
    for (int s = 0; s < nshells; ++s) {
        QcShell sh{};
        sh.atom = shell_atom[s]; sh.L = shell_L[s]; sh.nprim = shell_nprim[s];
        sh.pure = (shell_pure && shell_pure[s] && sh.L >= 2) ? 1 : 0;
        if (sh.atom < 0 || sh.atom >= natoms || sh.nprim <= 0 || sh.L < 0) { delete S; return QC_ERR_INVALID; }
        if (sh.L > QC_LMAX) { delete S; return QC_ERR_UNSUPPORTED; }
        sh.exps.assign(exponents + po, exponents + po + sh.nprim);
        sh.coefs.assign(coefficients + po, coefficients + po + sh.nprim);
        po += sh.nprim;
        S->shells.push_back(std::move(sh));
    }
    if (const char *e = getenv("QC_ACCUM")) S->accum_fx = std::strcmp(e, "f64") == 0 ? 0 : 1;     // A/B switch: QC_ACCUM=f64
    qc_build_model(S);
    if (!S->last_error.empty()) { fprintf(stderr, "qchem_hip: %s\n", S->last_error.c_str()); delete S; return QC_ERR_UNSUPPORTED; }
    *out = S;
    return QC_OK;
}

// A handle with live qc_scf_state objects is kept until the last of them ends (their buffers and destructors use its stream).
void qc_system_destroy(qc_system *S) {
    if (!S) return;
    if (S->live_states > 0) { S->zombie = true; return; }
    qc_system_free(S);
}

int qc_nbasis(const qc_system *S) { return S ? S->nbasis : QC_ERR_INVALID; }
int qc_nelectrons(const qc_system *S) { return S ? S->nelec : QC_ERR_INVALID; }
int qc_nshells(const qc_system *S) { return S ? S->nshells : QC_ERR_INVALID; }
int64_t qc_nquartets(const qc_system *S) { return S ? S->nquartets : QC_ERR_INVALID; }

double qc_nuclear_repulsion(const qc_system *S) {
    double e = 0.0;
    for (int a = 0; a < S->natoms; ++a)
        for (int b = a + 1; b < S->natoms; ++b) {
            double d2 = 0.0;
            for (int k = 0; k < 3; ++k) { const double x = S->xyz[3 * b + k] - S->xyz[3 * a + k]; d2 += x * x; }
            e += (double)(S->Z[a] * S->Z[b]) / std::sqrt(d2);
        }
    return e;
}

int qc_overlap(const qc_system *S, double *out) { if (!S || !out) return QC_ERR_INVALID; qc_host_one_electron(S, 0, out); return QC_OK; }
int qc_kinetic(const qc_system *S, double *out) { if (!S || !out) return QC_ERR_INVALID; qc_host_one_electron(S, 1, out); return QC_OK; }
int qc_nuclear(const qc_system *S, double *out) { if (!S || !out) return QC_ERR_INVALID; qc_host_one_electron(S, 2, out); return QC_OK; }

int qc_one_electron_gpu(qc_system *S, int which, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    DevBuf M;
    if (M.alloc(nn) != QC_OK) return QC_ERR_HIP;
    if ((rc = qc_one_electron_device(S, which, M.p)) != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(out, M.p, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

int qc_dipole_matrices(const qc_system *S, const double *origin, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    const double zero[3] = {0.0, 0.0, 0.0};
    qc_host_dipole(S, origin ? origin : zero, out);
    return QC_OK;
}
int qc_dipole_matrices_gpu(qc_system *S, const double *origin, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    const double zero[3] = {0.0, 0.0, 0.0};
    DevBuf M;
    if (M.alloc(3 * nn) != QC_OK) return QC_ERR_HIP;
    if ((rc = qc_dipole_device(S, origin ? origin : zero, M.p)) != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(out, M.p, 3 * nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

int qc_multipole_count(int order) { return order < 0 || order > QC_MULTIPOLE_MAX_ORDER ? -1 : qc_nherm(order); }
int qc_multipole_matrices(const qc_system *S, int order, const double *origin, double *out) {
    if (!S || !out || qc_multipole_count(order) < 0) return QC_ERR_INVALID;
    const double zero[3] = {0.0, 0.0, 0.0};
    qc_host_multipole(S, order, origin ? origin : zero, out);
    return QC_OK;
}
int qc_multipole_matrices_gpu(qc_system *S, int order, const double *origin, double *out) {
    if (!S || !out || qc_multipole_count(order) < 0) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t all = (size_t)qc_nherm(order) * S->nbasis * S->nbasis;
    const double zero[3] = {0.0, 0.0, 0.0};
    DevBuf M;
    if (M.alloc(all) != QC_OK) return QC_ERR_HIP;
    if ((rc = qc_multipole_device(S, order, origin ? origin : zero, M.p)) != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(out, M.p, all * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

// populations from host densities: S by the one-electron kernel, X as the SCF set-up forms it (Loewdin only)
int qc_populations(qc_system *S, int scheme, int nspin, const double *D, double *charges, double *spin, double *orbital, double *bond_orders) {
    if (!S || !D || !charges || scheme < 0 || scheme > 1 || nspin < 1 || nspin > 2) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    DevBuf dD, dS, dX;
    if (dD.alloc(nspin * nn) != QC_OK || dS.alloc(nn) != QC_OK || (scheme == 1 && dX.alloc(nn) != QC_OK)) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dD.p, D, nspin * nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    if ((rc = qc_one_electron_device(S, 0, dS.p)) != QC_OK) return rc;
    if (scheme == 1 && (rc = qc_population_x_device(S, dS.p, dX.p)) != QC_OK) return rc;
    std::vector<double> Nt(S->natoms), Ns(S->natoms);
    if ((rc = qc_population_device(S, scheme, dD.p, nspin == 2 ? dD.p + nn : nullptr, dS.p, dX.p, Nt.data(), Ns.data(), orbital, bond_orders)) != QC_OK) return rc;
    for (int a = 0; a < S->natoms; ++a) { charges[a] = S->Z[a] - Nt[a]; if (spin) spin[a] = Ns[a]; }
    return QC_OK;
}

int qc_esp_fit_points(const qc_system *S, const qc_esp_fit *cfg, int64_t capacity, double *xyz, int64_t *npts) {
    int nscales; double scales[8], density;
    if (!S || !npts || capacity < 0 || (capacity > 0 && !xyz) || !qc_espfit_config(cfg, &nscales, scales, &density)) return QC_ERR_INVALID;
    std::vector<double> pts;
    qc_espfit_grid(S, nscales, scales, density, pts);
    *npts = (int64_t)(pts.size() / 3);
    if (capacity < *npts) return QC_ERR_INVALID;
    std::copy(pts.begin(), pts.end(), xyz);
    return QC_OK;
}
int qc_esp_fit_solve(const qc_system *S, int64_t npts, const double *xyz, const double *v, double total_charge, qc_esp_fit *io, double *charges) {
    if (!S || !xyz || !v || !io || !charges || npts < 0 || !std::isfinite(total_charge)) return QC_ERR_INVALID;
    return qc_espfit_solve(S, npts, xyz, v, total_charge, io, charges);
}

int qc_set_stream(qc_system *S, void *hip_stream) {
    if (!S) return QC_ERR_INVALID;
    if (S->own_stream && S->stream) { (void)hipStreamDestroy(S->stream); S->own_stream = false; }
    S->lanes.lanes_probed = false;                                     // (which side stream shares the pipe of the caller's stream was not measured)
    S->prep.invalidate();                    // (the preliminaries of a prepared build were enqueued on the old stream)
    S->stream = (hipStream_t)hip_stream;
    if (!S->stream && S->device_ready) { QC_HIP_CHECK(hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking)); S->own_stream = true; }
    return QC_OK;
}

int qc_eri_full(qc_system *S, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    if (S->nranks != 1) return QC_ERR_INVALID;
    const size_t n = S->nbasis, n4 = n * n * n * n;
    DevBuf T;
    if (T.alloc(n4) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemsetAsync(T.p, 0, n4 * sizeof(double), S->stream));
    rc = qc_launch_eri_full(S, T.p);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(out, T.p, n4 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    return QC_OK;
}

int qc_fock_rhf_device(qc_system *S, const double *dD, double *dG) {
    if (!S || !dD || !dG) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    return qc_fock_build_device(S, dD, nullptr, dG, nullptr, false);
}
int qc_fock_uhf_device(qc_system *S, const double *dDa, const double *dDb, double *dGa, double *dGb) {
    if (!S || !dDa || !dDb || !dGa || !dGb) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    return qc_fock_build_device(S, dDa, dDb, dGa, dGb, true);
}

int qc_fock_rhf(qc_system *S, const double *D, double *G) {
    if (!S || !D || !G) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    QC_HIP_CHECK(hipMemcpyAsync(S->dev.d_D.p, D, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    rc = qc_fock_build_device(S, S->dev.d_D.p, nullptr, S->dev.d_G.p, nullptr, false);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(G, S->dev.d_G.p, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    if ((rc = qc_join_check(S)) != QC_OK) return rc;        // (a join that gave up folded an incomplete matrix: this call fails)
    qc_gate_quiet(S);
    return QC_OK;
}

int qc_fock_uhf(qc_system *S, const double *Da, const double *Db, double *Ga, double *Gb) {
    if (!S || !Da || !Db || !Ga || !Gb) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    QC_HIP_CHECK(hipMemcpyAsync(S->dev.d_D.p, Da, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    QC_HIP_CHECK(hipMemcpyAsync(S->dev.d_D.p + nn, Db, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    rc = qc_fock_build_device(S, S->dev.d_D.p, S->dev.d_D.p + nn, S->dev.d_G.p, S->dev.d_G.p + nn, true);
    if (rc != QC_OK) return rc;
    QC_HIP_CHECK(hipMemcpyAsync(Ga, S->dev.d_G.p, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipMemcpyAsync(Gb, S->dev.d_G.p + nn, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    if ((rc = qc_join_check(S)) != QC_OK) return rc;
    qc_gate_quiet(S);
    return QC_OK;
}

int qc_sym_eig(qc_system *S, int n, const double *A, double *V, double *w) { return A && V ? sym_eig_host(S, n, A, nullptr, V, w) : QC_ERR_INVALID; }
// sorted_eigs with a starting guess: V0 = eigenvectors of a nearby matrix (what the SCF loop uses from its second pass on)
int qc_sym_eig_warm(qc_system *S, int n, const double *A, const double *V0, double *V, double *w) {
    return A && V0 && V ? sym_eig_host(S, n, A, V0, V, w) : QC_ERR_INVALID;
}

int qc_mp2(qc_system *S, int nspin, const double *C, const double *eps, const int32_t *nocc, int32_t n_frozen, qc_mp2_output *out) {
    if (!S || !C || !eps || !nocc || !out || (nspin != 1 && nspin != 2)) return QC_ERR_INVALID;
    const int n = S->nbasis;
    int rc = qc_mp2_validate(n, nspin, eps, nocc, n_frozen);
    if (rc != QC_OK) return rc;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if ((rc = qc_device_init(S)) != QC_OK) return rc;
    const size_t nn = (size_t)n * n;
    DevBuf dC, dE;
    if (dC.alloc(nspin * nn) != QC_OK || dE.alloc((size_t)nspin * n) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dC.p, C, nspin * nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    QC_HIP_CHECK(hipMemcpyAsync(dE.p, eps, nspin * n * sizeof(double), hipMemcpyHostToDevice, S->stream));
    return qc_mp2_device(S, nspin, dC.p, dE.p, nocc, n_frozen, out);
}
int qc_gradient(qc_system *S, int nspin, const double *D, const double *W, double *terms) {
    if (!S || !D || !W || !terms || (nspin != 1 && nspin != 2)) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const int na3 = 3 * S->natoms;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    DevBuf dP, dW;
    if (dP.alloc(nspin * nn) != QC_OK || dW.alloc(nn) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dP.p, D, nspin * nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    QC_HIP_CHECK(hipMemcpyAsync(dW.p, W, nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    qc_nuclear_gradient(S, terms);
    if ((rc = qc_gradient_device(S, nspin, dP.p, dW.p, terms + na3, S->grad_ms)) != QC_OK || S->pc.empty()) return rc;
    // point charges on the handle: term 0 gains dE_nq/dR_A, term 1 the basis-function derivatives of tr(P_t V_pc)
    std::vector<double> gn(na3), ge(na3);
    if (nspin == 2) qc_axpby(S->stream, S->nbasis, 1.0, dP.p, 1.0, dP.p + nn, dP.p);
    if ((rc = qc_pc_atom_gradient_device(S, S->pc, dP.p, ge.data())) != QC_OK) return rc;
    qc_pc_nuclear_gradient(S, S->pc, gn.data(), nullptr);
    for (int k = 0; k < na3; ++k) { terms[k] += gn[k]; terms[na3 + k] += ge[k]; }
    return QC_OK;
}
int qc_gradient_timings(const qc_system *S, double *ms) {
    if (!S || !ms) return QC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = S->grad_ms[i];
    return QC_OK;
}

// ---- values on points: the host-only pair, then the GPU entries from host matrices.  Order of the checks: arguments, sharding, an
// empty call (QC_OK, nothing launched or written), the device.
// Those checks and the density: D (nspin blocks of n x n on the host) -> the total density at the head of dD, on the handle's stream.
// args_ok: the caller's own argument checks; empty: nothing to compute - QC_OK with dD left empty.
static int density_to_device(qc_system *S, bool args_ok, bool empty, int nspin, const double *D, DevBuf &dD) {
    if (!S || !D || !args_ok || (nspin != 1 && nspin != 2)) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (empty) return QC_OK;
    const int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    if (dD.alloc(nspin * nn) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dD.p, D, nspin * nn * sizeof(double), hipMemcpyHostToDevice, S->stream));
    if (nspin == 2) qc_axpby(S->stream, S->nbasis, 1.0, dD.p, 1.0, dD.p + nn, dD.p);
    return QC_OK;
}
int qc_basis_on_points(const qc_system *S, int64_t npts, const double *xyz, double *out) {
    if (!S || !xyz || !out || npts < 0) return QC_ERR_INVALID;
    qc_host_basis_on_points(S, npts, xyz, out);
    return QC_OK;
}
int qc_potential_matrix(const qc_system *S, const double r[3], double *out) {
    if (!S || !r || !out) return QC_ERR_INVALID;
    qc_host_potential_matrix(S, r, out);
    return QC_OK;
}
int qc_esp_records(const qc_system *S, int64_t counts[7]) {
    if (!S || !counts) return QC_ERR_INVALID;
    qc_esp_record_counts(S, counts);
    return QC_OK;
}
int qc_density_on_points(qc_system *S, const double *D, int64_t npts, const double *xyz, double *rho) {
    DevBuf dD;
    const int rc = density_to_device(S, xyz && rho && npts >= 0, npts == 0, 1, D, dD);
    return rc != QC_OK || !dD.p ? rc : qc_points_density_device(S, dD.p, npts, xyz, rho);
}
int qc_esp_on_points(qc_system *S, const double *D, int64_t npts, const double *xyz, double *v_elec, double *v_nuc) {
    DevBuf dD;
    int rc = density_to_device(S, xyz && v_elec && npts >= 0, npts == 0, 1, D, dD);
    if (rc != QC_OK || !dD.p) return rc;
    if ((rc = qc_points_esp_device(S, dD.p, npts, xyz, v_elec)) != QC_OK) return rc;
    if (v_nuc) qc_points_vnuc(S, npts, xyz, v_nuc);
    return QC_OK;
}
int qc_orbitals_on_points(qc_system *S, int m, const double *C, int64_t npts, const double *xyz, double *out) {
    if (!S || !C || !xyz || !out || npts < 0 || m <= 0) return QC_ERR_INVALID;
    if (S->comm || S->nranks != 1) return QC_ERR_UNSUPPORTED;
    if (npts == 0) return QC_OK;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nm = (size_t)S->nbasis * m;
    DevBuf dC;
    if (dC.alloc(nm) != QC_OK) return QC_ERR_HIP;
    QC_HIP_CHECK(hipMemcpyAsync(dC.p, C, nm * sizeof(double), hipMemcpyHostToDevice, S->stream));
    return qc_points_orbitals_device(S, m, dC.p, m, npts, xyz, out);
}
int qc_points_timings(const qc_system *S, double ms[4]) {
    if (!S || !ms) return QC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = S->points_ms[i];
    return QC_OK;
}

// ---- point-charge embedding (qc_embed.h).  The set lives on the handle as [x, y, z, q] per charge; an SCF state copies it when it begins.
int qc_set_point_charges(qc_system *S, int64_t npc, const double *xyz, const double *q) {
    if (!S || npc < 0 || (npc > 0 && (!xyz || !q))) return QC_ERR_INVALID;
    std::vector<double> pc(4 * (size_t)npc);
    for (int64_t c = 0; c < npc; ++c) {
        for (int k = 0; k < 3; ++k) pc[4 * c + k] = xyz[3 * c + k];
        pc[4 * c + 3] = q[c];
        for (int k = 0; k < 4; ++k) if (!std::isfinite(pc[4 * c + k])) return QC_ERR_INVALID;
        for (int a = 0; a < S->natoms; ++a) {
            const double dx = xyz[3 * c] - S->xyz[3 * a], dy = xyz[3 * c + 1] - S->xyz[3 * a + 1], dz = xyz[3 * c + 2] - S->xyz[3 * a + 2];
            if (dx * dx + dy * dy + dz * dz == 0.0) return QC_ERR_INVALID;
        }
    }
    S->pc.swap(pc);
    return QC_OK;
}
int64_t qc_point_charge_count(const qc_system *S) { return S ? (int64_t)(S->pc.size() / 4) : QC_ERR_INVALID; }
double qc_point_charge_nuclear_energy(const qc_system *S) { return S ? qc_pc_nuclear_energy(S, S->pc) : 0.0; }
int qc_point_charge_matrix(const qc_system *S, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    qc_host_point_charge_matrix(S, S->pc, out);
    return QC_OK;
}
int qc_point_charge_matrix_gpu(qc_system *S, double *out) {
    if (!S || !out) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const size_t nn = (size_t)S->nbasis * S->nbasis;
    DevBuf M;
    if (M.alloc(nn) != QC_OK) return QC_ERR_HIP;
    if ((rc = qc_pc_matrix_device(S, S->pc, M.p)) != QC_OK) return rc;
    const double t0 = qc_now_ms();
    QC_HIP_CHECK(hipMemcpyAsync(out, M.p, nn * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    QC_HIP_CHECK(hipStreamSynchronize(S->stream));
    S->pc_ms[3] = qc_now_ms() - t0;
    return QC_OK;
}
int qc_point_charge_timings(const qc_system *S, double ms[4]) {
    if (!S || !ms) return QC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = S->pc_ms[i];
    return QC_OK;
}
int qc_field_matrix(const qc_system *S, const double r[3], double *out) {
    if (!S || !r || !out) return QC_ERR_INVALID;
    qc_host_field_matrix(S, r, out);
    return QC_OK;
}
int qc_field_on_points(qc_system *S, const double *D, int64_t npts, const double *xyz, double *e_elec, double *e_nuc) {
    DevBuf dD;
    int rc = density_to_device(S, xyz && e_elec && npts >= 0, npts == 0, 1, D, dD);
    if (rc != QC_OK || !dD.p) return rc;
    if ((rc = qc_points_field_device(S, dD.p, npts, xyz, e_elec, S->points_ms)) != QC_OK) return rc;
    if (e_nuc) qc_points_enuc(S, npts, xyz, e_nuc);
    return QC_OK;
}
// terms = [dE_nq/dR_c | d tr(P_t V_pc)/dR_c], the second -q_c E_elec(R_c) by the field kernels at the charges
int qc_point_charge_gradient(qc_system *S, int nspin, const double *D, double *terms) {
    const int64_t npc = S ? (int64_t)(S->pc.size() / 4) : 0;
    DevBuf dD;
    int rc = density_to_device(S, terms != nullptr, npc == 0, nspin, D, dD);
    if (rc != QC_OK || !dD.p) return rc;
    std::vector<double> xyz(3 * (size_t)npc);
    for (int64_t c = 0; c < npc; ++c) for (int k = 0; k < 3; ++k) xyz[3 * c + k] = S->pc[4 * c + k];
    if ((rc = qc_points_field_device(S, dD.p, npc, xyz.data(), terms + 3 * npc, S->pc_ms)) != QC_OK) return rc;
    for (int64_t c = 0; c < npc; ++c) for (int k = 0; k < 3; ++k) terms[3 * (npc + c) + k] *= -S->pc[4 * c + 3];
    qc_pc_nuclear_gradient(S, S->pc, nullptr, terms);
    return QC_OK;
}

int qc_set_accumulation(qc_system *S, int fixed_point) {
    if (!S || (fixed_point != 0 && fixed_point != 1)) return QC_ERR_INVALID;
    S->accum_fx = fixed_point;
    S->prep.invalidate();                    // (a prepared build zeroed the planes of the other mode)
    return QC_OK;
}

int qc_set_schwarz(qc_system *S, double tau) {
    if (!S || !(tau >= 0.0)) return QC_ERR_INVALID;
    S->schwarz_tau = tau;
    return qc_device_reshard(S);
}
// the factors the screening rule reads (pairQ comes from the device pass of the set-up), with the shells of their pairs
int qc_schwarz_factors(qc_system *S, int32_t *shell_ab /* 2 * npairs or NULL */, double *Q /* npairs or NULL */, int64_t capacity) {
    if (!S) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const int64_t np = (int64_t)S->pairQ.size();
    if (!Q) return (int)np;
    if (!shell_ab || capacity < np) return QC_ERR_INVALID;
    for (int64_t i = 0; i < np; ++i) { shell_ab[2 * i] = S->pairA[i]; shell_ab[2 * i + 1] = S->pairB[i]; Q[i] = S->pairQ[i]; }
    return (int)np;
}

int qc_set_fock_mode(qc_system *S, int mode) {
    if (!S || (mode != 0 && mode != 1)) return QC_ERR_INVALID;
    S->fock_mode = mode;
    return QC_OK;
}
// (test hook, host only: what the bra-major work lists store for one lane and what the device-record builder reads back from it)
int qc_debug_ket_entry(int ket, int first_primitive, int length, int packed, int32_t out[3]) {
    if (!out || ket < 0) return QC_ERR_INVALID;
    if (packed && (ket >= (1 << QC_KET_BITS) || first_primitive < 0 || first_primitive > 127 || length < 0 || length > 127)) return QC_ERR_INVALID;
    const int entry = packed ? (int)qc_pack_ket_entry(ket, first_primitive, length) : ket;
    int k, f, l;
    qc_unpack_ket_entry(entry, packed != 0, &k, &f, &l);
    out[0] = k; out[1] = f; out[2] = l;
    return QC_OK;
}
int qc_freeze_assignment(qc_system *S) {
    if (!S) return QC_ERR_INVALID;
    qc_assignment_freeze(S);
    return QC_OK;
}
int qc_dispatch_lanes(qc_system *S, int32_t *nlanes, int32_t slot_stream[8]) {
    if (!S || !nlanes) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    *nlanes = S->lanes.nlanes;
    if (slot_stream) { for (int k = 0; k < QC_NSTREAMS; ++k) slot_stream[k] = S->lanes.slot_side[k]; slot_stream[QC_NSTREAMS] = S->lanes.lane0_is_main ? 1 : 0; }
    return QC_OK;
}

// ---- multi-GPU
int qc_comm_unique_id(uint8_t id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    if (!qc_rccl().ok || qc_rccl().GetUniqueId(&u) != ncclSuccess) return QC_ERR_RCCL;
    std::memcpy(id, &u, 128);
    return QC_OK;
}

int qc_set_shard(qc_system *S, int rank, int nranks) {
    if (!S || nranks <= 0 || rank < 0 || rank >= nranks) return QC_ERR_INVALID;
    S->rank = rank; S->nranks = nranks;
    return qc_device_reshard(S);
}

int qc_comm_init(qc_system *S, const uint8_t id[128], int rank, int nranks) {
    if (!S || !id) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    if ((rc = qc_set_shard(S, rank, nranks)) != QC_OK) return rc;
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    ncclComm_t comm;
    if (!qc_rccl().ok) return QC_ERR_RCCL;
    if (S->comm) { qc_rccl().CommDestroy((ncclComm_t)S->comm); S->comm = nullptr; }      // a second init replaces the communicator
    if (qc_rccl().CommInitRank(&comm, nranks, u, rank) != ncclSuccess) return QC_ERR_RCCL;
    S->comm = comm;
    return QC_OK;
}

int qc_rccl_info(char *buf, size_t len) {
    if (!buf || len == 0) return QC_ERR_INVALID;
    QcRccl &r = qc_rccl();
    int v = 0;
    if (r.ok && r.GetVersion) (void)r.GetVersion(&v);
    snprintf(buf, len, "%s version %d", r.ok ? r.path.c_str() : "unavailable", v);
    return r.ok ? QC_OK : QC_ERR_RCCL;
}

int qc_plan_shard(qc_system *S, int rank, int nranks, int64_t *nquartets, double *flops) {
    if (!S || nranks <= 0 || rank < 0 || rank >= nranks) return QC_ERR_INVALID;
    ShardScope as(S, rank, nranks);
    int64_t nq = 0; double fl = 0.0;
    for (const auto &c : S->classes) { nq += (int64_t)c.shard.size(); fl += c.flops_alg; }
    if (nquartets) *nquartets = nq;
    if (flops) *flops = fl;
    return QC_OK;
}

// list the quartets of a shard as (shell A, B, C, D) so a host-side checker can digest exactly the same units
int qc_plan_shard_quartets(qc_system *S, int rank, int nranks, int32_t *abcd /* 4 * nquartets or NULL */, int64_t capacity) {
    if (!S || nranks <= 0 || rank < 0 || rank >= nranks) return QC_ERR_INVALID;
    ShardScope as(S, rank, nranks);                       // exactly the lists the device would be given
    int64_t k = 0;
    for (const auto &c : S->classes)
        for (const auto &t : c.shard) {
            if (abcd) {
                if (k >= capacity) return QC_ERR_INVALID;
                abcd[4 * k + 0] = S->pairA[t.bra]; abcd[4 * k + 1] = S->pairB[t.bra];
                abcd[4 * k + 2] = S->pairA[t.ket]; abcd[4 * k + 3] = S->pairB[t.ket];
            }
            ++k;
        }
    return (int)k;
}

int qc_work_stats_get(qc_system *S, qc_work_stats *out) {
    if (!S || !out) return QC_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    qc_ensure_lists(S);
    for (const auto &c : S->classes) {
        if (c.shard.empty()) continue;
        out->quartets += (int64_t)c.shard.size(); out->prim_quartets += c.prim_quartets;
        out->bytes_alg += c.bytes_alg; out->flops_alg += c.flops_alg; out->nclasses += 1;
    }
    out->quartets_enumerated = S->nquartets;
    out->quartets_screened_out = S->nscreened;
    out->schwarz_tau = S->pairQ.empty() ? 0.0 : S->schwarz_tau;
    return QC_OK;
}

int qc_fock_profile(qc_system *S, const double *dD, double *dG, int reps, float *class_ms, int32_t *class_id, int64_t *class_quartets,
                    double *class_bytes, double *class_flops, float *total_ms) {
    if (!S || !dD || !dG || reps <= 0) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    std::vector<float> acc(S->classes.size(), 0.f);
    float tot = 0.f;
    if ((rc = profile_builds(S, dD, dG, reps, false, acc, &tot)) != QC_OK) return rc;
    int k = 0;
    for (size_t i = 0; i < S->classes.size(); ++i) {
        const QcClass &c = S->classes[i];
        if (c.shard.empty()) continue;
        if (class_ms) class_ms[k] = acc[i] / reps;
        if (class_id) class_id[k] = (c.bm ? 1 << 12 : 0) | (c.LAB << 8) | (c.LCD << 4) | c.LGC;
        if (class_quartets) class_quartets[k] = (int64_t)c.shard.size();
        if (class_bytes) class_bytes[k] = c.bytes_alg;
        if (class_flops) class_flops[k] = c.flops_alg;
        ++k;
    }
    if (total_ms) *total_ms = tot / reps;
    return QC_OK;
}

int qc_unit_quartets(qc_system *S, int64_t *unit_quartets) {
    if (!S || !unit_quartets) return QC_ERR_INVALID;
    for (int u = 0; u < QC_NUNITS; ++u) unit_quartets[u] = 0;
    qc_ensure_lists(S);
    for (const auto &c : S->classes) unit_quartets[qc_build_unit_of(S, c.LAB, c.LCD, c.bm)] += (int64_t)c.shard.size();
    return QC_OK;
}

// Per launch unit ("tier" = (LAB, LCD <= 3 | LCD >= 4), the kernels an un-instrumented build really launches), timed
// serially with hipEvents on the handle's stream.  Arrays have 14 entries, unit u = 2 * LAB + tier; empty units are 0.
int qc_fock_profile_tiers(qc_system *S, const double *dD, double *dG, int reps, float *unit_ms, int64_t *unit_quartets,
                          double *unit_bytes, double *unit_flops, float *total_ms) {
    if (!S || !dD || !dG || reps <= 0 || !unit_ms) return QC_ERR_INVALID;
    int rc = qc_device_init(S);
    if (rc != QC_OK) return rc;
    const int NU = QC_NUNITS;
    std::vector<float> acc(NU, 0.f);
    float tot = 0.f;
    if ((rc = profile_builds(S, dD, dG, reps, true, acc, &tot)) != QC_OK) return rc;
    for (int u = 0; u < NU; ++u) {
        unit_ms[u] = acc[u] / reps;
        if (unit_quartets) unit_quartets[u] = 0;
        if (unit_bytes) unit_bytes[u] = 0;
        if (unit_flops) unit_flops[u] = 0;
    }
    for (const auto &c : S->classes) {
        if (c.shard.empty()) continue;
        const int u = qc_build_unit_of(S, c.LAB, c.LCD, c.bm);
        if (unit_quartets) unit_quartets[u] += (int64_t)c.shard.size();
        if (unit_bytes) unit_bytes[u] += c.bytes_alg;
        if (unit_flops) unit_flops[u] += c.flops_alg;
    }
    if (total_ms) *total_ms = tot / reps;
    return QC_OK;
}

}  // extern "C"
