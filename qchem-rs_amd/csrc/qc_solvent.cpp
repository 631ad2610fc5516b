// qc_solvent.cpp - the host side of the conductor-like continuum (the model: include/qchem_hip.h): the cavity surface, the
// host statement of its matrix S, and the entry points that need no device.  The device side: qc_solvent.hip, qc_chol.hip.
#include <cmath>

#include "qc_solvent.h"

// S of the cavity, M x M, serially: the reference statement of the assembly kernel
void qc_solvent_host_matrix(const QcSolvent &Q, double *Smat) {
    const int64_t M = Q.M;
    for (int64_t i = 0; i < M; ++i) {
        Smat[i * M + i] = Q.zeta[i] * std::sqrt(2.0 / M_PI);
        for (int64_t j = 0; j < i; ++j) {
            const double dx = Q.xyz[3 * i] - Q.xyz[3 * j], dy = Q.xyz[3 * i + 1] - Q.xyz[3 * j + 1], dz = Q.xyz[3 * i + 2] - Q.xyz[3 * j + 2];
            const double r = std::sqrt(dx * dx + dy * dy + dz * dz);
            const double zij = Q.zeta[i] * Q.zeta[j] / std::sqrt(Q.zeta[i] * Q.zeta[i] + Q.zeta[j] * Q.zeta[j]);
            Smat[i * M + j] = Smat[j * M + i] = std::erf(zij * r) / r;
        }
    }
}

extern "C" {

int qc_set_solvent(qc_system *S, const qc_solvent *cfg, const double *radii) {
    if (!S) return QC_ERR_INVALID;
    if (!cfg) { S->solvent.reset(); return QC_OK; }
    if (!std::isfinite(cfg->epsilon) || !(cfg->epsilon > 1.0) || !std::isfinite(cfg->x) || !(cfg->x >= 0.0)) return QC_ERR_INVALID;
    if (!std::isfinite(cfg->scale) || !(cfg->scale >= 0.0) || !std::isfinite(cfg->density) || !(cfg->density >= 0.0)) return QC_ERR_INVALID;
    auto Q = std::make_shared<QcSolvent>();
    Q->cfg = *cfg;
    if (Q->cfg.scale == 0.0) Q->cfg.scale = 1.2;
    if (Q->cfg.density == 0.0) Q->cfg.density = 5.0;
    Q->f = (cfg->epsilon - 1.0) / (cfg->epsilon + cfg->x);
    std::vector<double> R(S->natoms);
    for (int A = 0; A < S->natoms; ++A) {
        const double r = radii ? radii[A] : qc_vdw_radius_bohr(S->Z[A]);
        if (!std::isfinite(r) || !(r > 0.0)) return QC_ERR_INVALID;
        R[A] = Q->cfg.scale * r;
    }
    qc_sphere_points(S, R.data(), Q->cfg.density * (QC_BOHR_ANGSTROM * QC_BOHR_ANGSTROM), Q->xyz, &Q->atom, &Q->area);
    Q->M = (int64_t)Q->area.size();
    if (Q->M == 0) return QC_ERR_INVALID;
    if (Q->M > QC_SOLVENT_MAX_POINTS) return QC_ERR_UNSUPPORTED;
    const double c = 1.0694 * M_PI * std::sqrt(2.0);
    Q->zeta.resize(Q->M);
    for (int64_t i = 0; i < Q->M; ++i) Q->zeta[i] = c / std::sqrt(Q->area[i]);
    Q->vnuc.resize(Q->M);
    qc_points_vnuc(S, Q->M, Q->xyz.data(), Q->vnuc.data());
    S->solvent = std::move(Q);
    return QC_OK;
}

int64_t qc_solvent_surface(const qc_system *S, int64_t capacity, double *xyz, double *area, int32_t *atom) {
    if (!S || !S->solvent) return QC_ERR_INVALID;
    const QcSolvent &Q = *S->solvent;
    if (capacity >= Q.M) {
        if (xyz) std::copy(Q.xyz.begin(), Q.xyz.end(), xyz);
        if (area) std::copy(Q.area.begin(), Q.area.end(), area);
        if (atom) std::copy(Q.atom.begin(), Q.atom.end(), atom);
    }
    return Q.M;
}

int qc_solvent_matrix(const qc_system *S, double *Smat) {
    if (!S || !S->solvent || !Smat) return QC_ERR_INVALID;
    qc_solvent_host_matrix(*S->solvent, Smat);
    return QC_OK;
}

int qc_solvent_last(const qc_system *S, qc_solvent_energy *out) {
    if (!S || !out || !S->solvent || !S->solvent->have_last) return QC_ERR_INVALID;
    *out = S->solvent->last;
    return QC_OK;
}

int qc_solvent_timings(const qc_system *S, double ms[4]) {
    if (!S || !ms || !S->solvent) return QC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = S->solvent->ms[i];
    return QC_OK;
}

}  // extern "C"
