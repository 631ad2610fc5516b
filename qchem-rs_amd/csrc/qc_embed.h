// qc_embed.h - point-charge embedding: a set of external charges q_c at R_c enters the core Hamiltonian as
//   V_pc = -sum_c q_c A(R_c),  A_ab(r) = (a| 1/|r' - r| |b),   and the energy as   E_nq = sum_A sum_c Z_A q_c / |R_A - R_c|.
// A charge set is a vector of [x, y, z, q] per charge (qc_system::pc, or the snapshot an SCF state took of it).
#pragma once
#include <vector>

#include "qc_internal.h"

constexpr int QC_PC_TILE = 256;     // charges of a tile: the unit of the fixed summation order of the Hermite sums (qc_embed.hip)

// ---- host (qc_system.cpp)
double qc_pc_nuclear_energy(const qc_system *S, const std::vector<double> &pc);
// dE_nq/dR_A into ga (3 natoms) and dE_nq/dR_c into gc (3 per charge), either nullable
void qc_pc_nuclear_gradient(const qc_system *S, const std::vector<double> &pc, double *ga, double *gc);
void qc_host_point_charge_matrix(const qc_system *S, const std::vector<double> &pc, double *out /* n*n */);
void qc_host_field_matrix(const qc_system *S, const double *r /* 3 */, double *out /* 3 n*n: dA_ab(r)/dr_k */);
// E_nuc(r) = sum_A Z_A (r - R_A) / |r - R_A|^3 on npts points, npts x 3 (plain IEEE: a point on a nucleus is not finite)
void qc_points_enuc(const qc_system *S, int64_t npts, const double *xyz, double *e);

// ---- device (qc_embed.hip); the handle's device side is initialised
// V_pc of `pc` (not empty) into d_out (n*n, device), enqueued on the handle's stream and waited for; phase times 0..2 into S->pc_ms
int qc_pc_matrix_device(qc_system *S, const std::vector<double> &pc, double *d_out);
// d tr(P_t V_pc)/dR_A at fixed charges from the device density dPt (n*n, P_alpha + P_beta), 3 natoms doubles on the host (basis-function
// derivatives only); phase times into S->pc_ms
int qc_pc_atom_gradient_device(qc_system *S, const std::vector<double> &pc, const double *dPt, double *grad);
