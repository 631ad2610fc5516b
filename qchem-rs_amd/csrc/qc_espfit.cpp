// qc_espfit.cpp - the host numerics of the ESP-fitted (Merz-Kollman) charges: the grid of points on scaled van der
// Waals spheres and the constrained least-squares fit.  The potential itself is the point code's (qc_points.hip).
#include <cmath>

#include "qc_solvent.h"
#include "qc_subspace_host.h"

namespace {

// van der Waals radius in Angstrom
double vdw_radius(int Z) {
    switch (Z) {
        case 1: return 1.20;  case 2: return 1.40;  case 6: return 1.70;  case 7: return 1.55;  case 8: return 1.52;  case 9: return 1.47;
        case 10: return 1.54; case 14: return 2.10; case 15: return 1.80; case 16: return 1.80; case 17: return 1.75; case 18: return 1.88;
        default: return 2.00;
    }
}

}  // namespace

// the inputs of cfg with the defaults filled in; false: a bad configuration
bool qc_espfit_config(const qc_esp_fit *cfg, int *nscales, double *scales, double *density) {
    static const double def[4] = {1.4, 1.6, 1.8, 2.0};
    *nscales = 4; *density = QC_BOHR_ANGSTROM * QC_BOHR_ANGSTROM;      // 1 per Angstrom^2, in points per bohr^2
    for (int k = 0; k < 4; ++k) scales[k] = def[k];
    if (!cfg) return true;
    if (cfg->nscales < 0 || cfg->nscales > 8 || !(cfg->density >= 0.0) || !std::isfinite(cfg->density)) return false;
    if (cfg->nscales > 0) {
        *nscales = cfg->nscales;
        for (int k = 0; k < cfg->nscales; ++k) { if (!(cfg->scales[k] > 0.0) || !std::isfinite(cfg->scales[k])) return false; scales[k] = cfg->scales[k]; }
    }
    if (cfg->density > 0.0) *density = cfg->density;
    return true;
}

// van der Waals radius in bohr (the table of qchem_hip.h)
double qc_vdw_radius_bohr(int Z) { return vdw_radius(Z) / QC_BOHR_ANGSTROM; }

// The sphere-point rule, stated once for the ESP-fit grid and the solvent cavity (qc_solvent.h): on the sphere of radius R[A] around atom A
// the N = ceil(density 4 pi R^2) golden-angle points k = 0 .. N - 1; a point is kept iff its distance to every other atom B is >= R[B].
// Appends to xyz (and to atom / area) in the order atom, k.
void qc_sphere_points(const qc_system *S, const double *Rs, double density, std::vector<double> &xyz, std::vector<int32_t> *atom, std::vector<double> *area) {
    const double golden = M_PI * (3.0 - std::sqrt(5.0));
    for (int A = 0; A < S->natoms; ++A) {
        const double R = Rs[A];
        const long N = (long)std::ceil(density * 4.0 * M_PI * R * R);
        for (long k = 0; k < N; ++k) {
            const double z = 1.0 - (2.0 * k + 1.0) / N, rho = std::sqrt(1.0 - z * z), phi = k * golden;
            const double r[3] = {S->xyz[3 * A] + R * (rho * std::cos(phi)), S->xyz[3 * A + 1] + R * (rho * std::sin(phi)), S->xyz[3 * A + 2] + R * z};
            bool keep = true;
            for (int B = 0; B < S->natoms && keep; ++B) {
                if (B == A) continue;
                const double d[3] = {r[0] - S->xyz[3 * B], r[1] - S->xyz[3 * B + 1], r[2] - S->xyz[3 * B + 2]};
                keep = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) >= Rs[B];
            }
            if (!keep) continue;
            xyz.insert(xyz.end(), r, r + 3);
            if (atom) atom->push_back(A);
            if (area) area->push_back(4.0 * M_PI * R * R / (double)N);
        }
    }
}

// the grid, in the order scale, atom, k (qchem_hip.h)
void qc_espfit_grid(const qc_system *S, int nscales, const double *scales, double density, std::vector<double> &xyz) {
    xyz.clear();
    std::vector<double> R(S->natoms);
    for (int s = 0; s < nscales; ++s) {
        for (int A = 0; A < S->natoms; ++A) R[A] = scales[s] * qc_vdw_radius_bohr(S->Z[A]);
        qc_sphere_points(S, R.data(), density, xyz, nullptr, nullptr);
    }
}

// the fit: KKT system [A^T A, 1; 1^T, 0] (q; lambda) = (A^T v; total_charge), A_pA = 1 / |r_p - R_A|, sums in point order
int qc_espfit_solve(const qc_system *S, int64_t npts, const double *xyz, const double *v, double total_charge, qc_esp_fit *io, double *charges) {
    const int na = S->natoms, m = na + 1;
    if (npts < na) return QC_ERR_INVALID;
    std::vector<double> K((size_t)m * m, 0.0), rhs(m, 0.0), row(na), sol(m);
    auto fill_row = [&](int64_t p) {
        for (int A = 0; A < na; ++A) {
            const double d[3] = {xyz[3 * p] - S->xyz[3 * A], xyz[3 * p + 1] - S->xyz[3 * A + 1], xyz[3 * p + 2] - S->xyz[3 * A + 2]};
            row[A] = 1.0 / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        }
    };
    for (int64_t p = 0; p < npts; ++p) {
        if (!std::isfinite(v[p])) return QC_ERR_INVALID;
        fill_row(p);
        for (int A = 0; A < na; ++A) {
            if (!std::isfinite(row[A])) return QC_ERR_INVALID;         // a point on a nucleus
            for (int B = 0; B <= A; ++B) K[(size_t)A * m + B] += row[A] * row[B];
            rhs[A] += row[A] * v[p];
        }
    }
    for (int A = 0; A < na; ++A) {
        for (int B = 0; B < A; ++B) K[(size_t)B * m + A] = K[(size_t)A * m + B];
        K[(size_t)A * m + na] = K[(size_t)na * m + A] = 1.0;
    }
    rhs[na] = total_charge;
    if (!host_lu_solve(m, K, 1, rhs.data(), sol.data())) return QC_ERR_INVALID;
    for (int A = 0; A < na; ++A) if (!std::isfinite(sol[A])) return QC_ERR_INVALID;
    double r2 = 0.0, v2 = 0.0;
    for (int64_t p = 0; p < npts; ++p) {
        fill_row(p);
        double fit = 0.0;
        for (int A = 0; A < na; ++A) fit += sol[A] * row[A];
        r2 += (v[p] - fit) * (v[p] - fit);
        v2 += v[p] * v[p];
    }
    io->npts = npts; io->total_charge = total_charge;
    io->rms = npts ? std::sqrt(r2 / (double)npts) : 0.0;
    io->rrms = v2 > 0.0 ? std::sqrt(r2 / v2) : 0.0;
    for (int k = 0; k < 3; ++k) { io->dipole[k] = 0.0; for (int A = 0; A < na; ++A) io->dipole[k] += sol[A] * S->xyz[3 * A + k]; }
    for (int A = 0; A < na; ++A) charges[A] = sol[A];
    return QC_OK;
}
