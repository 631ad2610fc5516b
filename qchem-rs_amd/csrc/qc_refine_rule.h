// qc_refine_rule.h - the rule of the eigenvector refinement, stated once for its three forms: one workgroup + host loop and the chip-wide
// A / B kernels (qc_eig_refine.hip), the LDS form of the small-molecule Roothaan kernel (qc_scf_small.hip).  Open-shell trajectories depend
// on every bit of an eigensolve: a threshold or the handling of a cluster is changed here and nowhere else.
//
// Eigenvector refinement (Ogita & Aishima, Japan J. Indust. Appl. Math. 35 (2018) 1007): with X an approximate
// eigenvector matrix of symmetric A,  R = I - X^T X,  S = X^T A X,  lam_i = S_ii / (1 - R_ii),
//   E_ij = (S_ij + lam_j R_ij) / (lam_j - lam_i)   (|lam_i - lam_j| > delta),   E_ij = R_ij / 2   (otherwise, and i = j),
//   X <- X (I + E)   converges quadratically; everything O(n^3) is an f64 MFMA GEMM.
// Pair (i,j) classes, with  a_ij = S_ij + (lam_i + lam_j)/2 R_ij  (coupling),  g = |lam_j - lam_i|,  scale = max|lam|:
//   negligible : |a_ij| <= 1e-13 scale                       -> E_ij = R_ij / 2        (orthogonality only)
//   strong     : |a_ij| / max(g, 1e-8 scale) > 1e-3          -> exact 2x2 Jacobi rotation, provided every index has at
//                most one strong partner (near-degenerate pairs: their eigenvectors turn by finite angles under tiny
//                changes of A; the first-order formula would need many passes); otherwise the caller goes to Jacobi
//   degenerate : g <= 1e-8 scale, weak coupling              -> E_ij = R_ij / 2, coupling recorded in stats[4]
//   regular    :                                             -> E_ij = (S_ij + lam_j R_ij) / (lam_j - lam_i)
// stats: [0] ||offdiag(S)||_F  [1] ||R||_F  [2] scale  [3] #strong pairs  [4] max coupling left in degenerate pairs
//        [5] max |a_ij| / g over regular pairs (size of the first-order update; the A / B kernels test |a| <= tau g without the division
//        and report the threshold exceeded: the two round differently)  [6] 1 if some index has > 1 strong partner
// S is symmetric only to rounding: `sij` is always (S_ij + S_ji) / 2.  Loops, bounds handling, control flow (branches in global memory,
// selects in LDS) and what is accumulated stay with the kernels.  Macros where a function changed a kernel's code: lazily evaluated
// operands (the LDS kernel reads its flags behind the tests that guard them), the coupling and weak-pair expressions of the M loops, the
// comparison inside the sorting loops.
#pragma once
#include <hip/hip_runtime.h>

#define QC_RULE __host__ __device__ __forceinline__
// class scale factors (times scale, floored; TAU is relative to the gap) and decision thresholds: update too big to be perturbative,
// orthogonality lost, update and orthogonality small enough for one last update, coupling left in degenerate pairs (times scale)
constexpr double QC_REF_TAU = 1e-3, QC_REF_TINY = 1e-13, QC_REF_GFLOOR = 1e-8, QC_REF_SCALE_FLOOR = 1e-300;
constexpr double QC_REF_BIG = 0.1, QC_REF_ORTH_LOST = 1e-3, QC_REF_LAST = 1e-7, QC_REF_CLEAN = 1e-12;

QC_RULE double qc_ref_quotient(double sii, double rii) { return sii / (1.0 - rii); }                          // lam_i
#define QC_REF_COUPLING(sij, li, lj, r) ((sij) + 0.5 * ((li) + (lj)) * (r))                                   // a_ij, signed
// pair classes from av = |a_ij|, g = |lam_j - lam_i|: a pair is the first class whose test it meets, in this order
QC_RULE bool qc_ref_coupled(double av, double tiny) { return av > tiny; }                                     // else negligible
QC_RULE bool qc_ref_strong(double av, double g, double gfloor) { return av > QC_REF_TAU * fmax(g, gfloor); }
QC_RULE bool qc_ref_degenerate(double g, double gfloor) { return g <= gfloor; }                               // else regular:
QC_RULE bool qc_ref_regular(double g, double gfloor) { return g > gfloor; }     // (for the select form; g is a number wherever av is finite)
// size of the first-order update of a regular pair, division-free
QC_RULE bool qc_ref_pair_big(double av, double g) { return !(av <= QC_REF_BIG * g); }
QC_RULE bool qc_ref_pair_notlast(double av, double g) { return !(av <= QC_REF_LAST * g); }
// partner[i]: -1 no strong partner, j its only one, -2 more than one.  A strong pair must be mutual; anything else is "multi".
QC_RULE int qc_ref_partner(int cnt, int who) { return cnt == 0 ? -1 : (cnt == 1 ? who : -2); }
QC_RULE bool qc_ref_not_mutual(const int *partner, int i) { const int pj = partner[i]; return pj >= 0 && partner[pj] != i; }
// the decisions of a pass.  QC_EIG_STATE <- QC_EIG_ROTATE (not perturbative: rotations needed) if ROTATE; otherwise QC_EIG_LAST (one more
// update finishes) and QC_EIG_CLEAN (no coupling left inside degenerate pairs; scl: the floored scale)
#define QC_REF_ROTATE(big, orth, multi) ((big) || !((orth) <= QC_REF_ORTH_LOST) || (multi))
#define QC_REF_IS_LAST(notlast, orth, nstrong) (!(notlast) && (orth) <= QC_REF_LAST && !(nstrong))
#define QC_REF_IS_CLEAN(cmax, scl) ((cmax) <= QC_REF_CLEAN * (scl))
// elements of M = I + E (a, g: signed coupling and gap lam_j - lam_i).  Tangent of the exact 2x2 rotation, also the Jacobi kernels':
QC_RULE double qc_ref_tangent(double a, double g) {
    const double theta = g / (2.0 * a);
    return (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
}
QC_RULE double qc_ref_m_diag(double r) { return 1.0 + 0.5 * r; }                                              // no strong partner
QC_RULE double qc_ref_m_diag_rot(double r, double a, double g) { const double t = qc_ref_tangent(a, g); return 1.0 / sqrt(fma(t, t, 1.0)) + 0.5 * r; }   // cosine
QC_RULE double qc_ref_m_rot(double a, double g) { const double t = qc_ref_tangent(a, g); return t / sqrt(fma(t, t, 1.0)); }   // (i, partner[i]): sine
// every other pair: R_ij / 2 for negligible and degenerate ones, the first-order quotient for regular ones
#define QC_REF_M_WEAK(sij, r, lj, a, g, tiny, gfloor) ((fabs(a) <= (tiny) || fabs(g) <= (gfloor)) ? 0.5 * (r) : ((sij) + (lj) * (r)) / (g))
// ascending order, ties by index (stable; utils.rs:28): lam[j] < wi || (lam[j] == wi && j < i) puts j before i; the rank of i counts such j.
// (The two-sided Jacobi kernel sorts the diagonal it holds by the same comparison, written out there.)
#define QC_REF_BEFORE(lam, j, wi, i) ((lam)[j] < (wi) || ((lam)[j] == (wi) && (j) < (i)))
#undef QC_RULE
