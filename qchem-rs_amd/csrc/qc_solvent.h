// qc_solvent.h - conductor-like continuum solvation (the model: include/qchem_hip.h).  A QcSolvent is the cavity of one
// qc_set_solvent call - surface, configuration, and once it has been used on the device K = -f S^-1 and v_nuc - shared by the handle and
// the SCF states that began with it.
#pragma once
#include <memory>
#include <vector>

#include "qc_internal.h"

constexpr int64_t QC_SOLVENT_MAX_POINTS = 16384;
constexpr int QC_CHOL_NB = 64;          // diagonal block of the device Cholesky factorisation (qc_chol.hip)

struct QcSolvent {
    qc_solvent cfg{};                     // defaults filled in
    double f = 0.0;                       // (eps - 1) / (eps + x)
    int64_t M = 0;
    std::vector<double> xyz, area, zeta, vnuc;   // M x 3, M, M, M
    std::vector<int32_t> atom;
    // device side, built at the first use (qc_solvent_prepare)
    bool ready = false;
    DevBuf dK, dv, dq, dout, dpart;       // K (M x M) | [v_nuc, v_elec] (2 M) | q (M) | the three sums | per-workgroup partial sums
    QcDev<unsigned> dcnt;                 // arrival counter of the reaction kernel's workgroups
    hipEvent_t ev[2] = {nullptr, nullptr};  // around the reaction kernel (ms[2])
    double ms[4] = {0, 0, 0, 0};          // qc_solvent_timings
    qc_solvent_energy last{};             // of the last one-shot run (qc_solvent_last)
    bool have_last = false;
    QcSolvent() = default;
    QcSolvent(const QcSolvent &) = delete; QcSolvent &operator=(const QcSolvent &) = delete;
    ~QcSolvent() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// ---- host (qc_solvent.cpp; the sphere rule itself: qc_espfit.cpp)
// Radius table (bohr) and the golden-angle points of spheres of radii R (bohr, one per atom) around the atoms, a point kept iff its
// distance to every other centre B is >= R[B]; order atom, k.  atom / area (nullable) receive each kept point's owner and 4 pi R^2 / N.
double qc_vdw_radius_bohr(int Z);
void qc_sphere_points(const qc_system *S, const double *R, double density, std::vector<double> &xyz, std::vector<int32_t> *atom, std::vector<double> *area);
void qc_solvent_host_matrix(const QcSolvent &Q, double *Smat);

// ---- device (qc_chol.hip, qc_solvent.hip)
// dAinv = scale * A^-1 for the SPD matrix dA (n x n, device, left intact), exactly symmetric; QC_ERR_INVALID: a pivot <= 0 or not finite
int qc_spd_inverse_device(qc_system *S, int n, const double *dA, double scale, double *dAinv);
// S of the cavity into dS (M x M, device)
int qc_solvent_matrix_device(qc_system *S, const QcSolvent &Q, double *dS);
// K and v_nuc on the device, once per cavity
int qc_solvent_prepare(qc_system *S, QcSolvent &Q);
// the response at the device density dD (total, n x n): q and v_elec to the host (M each, nullable), V_R into dV (n x n, device, nullable),
// out3 = {1/2 q.v_nuc, 1/2 q.v_elec, sum q}.  Synchronous: the handle's stream is drained when it returns.
int qc_solvent_response_device(qc_system *S, QcSolvent &Q, const double *dD, double *q, double *v_elec, double *dV, double out3[3]);
