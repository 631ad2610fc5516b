/*
 * qchem_hip.h - C ABI of libqchem_hip.so, the MI355X (gfx950) Hartree-Fock hot path that sits behind the public API
 * of qchem-rs's `core` crate.
 *
 * The reference has no FFI of its own; its boundary is the Rust API
 *     core::hf::restricted_hartree_fock(&MolecularSystem, &HartreeFockConfig) -> Option<RestrictedHartreeFockOutput>
 *     core::hf::unrestricted_hartree_fock(...)                                 (core/src/hf/rhf.rs:32, uhf.rs:36)
 * plus the `molint` free functions those drivers call (rhf.rs:41-45, uhf.rs:52-55).  Every entry point below names
 * the reference interface it replaces; INTEGRATION.md shows the `extern "C"` block and the safe wrapper a maintainer
 * would add to `core/src/hf/` to route the two drivers through this library.
 *
 * Conventions
 *   - plain pointers and sizes only; all matrices are n x n, f64, row-major (the ones crossing the boundary are
 *     symmetric, so nalgebra's column-major DMatrix reads them unchanged); coordinates in bohr.
 *   - every call returns a status: QC_OK, QC_NOT_CONVERGED (the reference's `None`), QC_DIIS_SINGULAR (the
 *     reference's `expect("DIIS failed")` panic), or a negative error.  Nothing throws across the boundary.
 *   - a qc_system handle owns its HIP stream and device buffers; it is not thread-safe; distinct handles may be used
 *     from distinct threads.  No global mutable state.
 *   - nothing is printed unless QC_LOG is set: then the drivers write the reference's per-iteration log line (rhf.rs:90-92) to stderr.
 *   - there is NO CPU fallback: any call that needs the GPU returns QC_ERR_NO_DEVICE when no gfx950 device is visible.
 *     Creating a handle, querying sizes, the one-electron matrices and the work plan are host-only and work anywhere.
 */
#ifndef QCHEM_HIP_H
#define QCHEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    QC_OK = 0,
    QC_NOT_CONVERGED = 1,   /* rhf.rs:106-107 / uhf.rs:165-166 return None */
    QC_DIIS_SINGULAR = 2,   /* rhf.rs:73 expect("DIIS failed") / uhf.rs:95-97 panic */
    QC_EIG_NOT_CONVERGED = 3, /* the Jacobi sweeps of an eigensolve ran out (no counterpart: nalgebra's SymmetricEigen, utils.rs:16,
                               * iterates until it converges; reported instead of continuing on unconverged vectors) */
    QC_ERR_INVALID = -1,
    QC_ERR_NO_DEVICE = -2,
    QC_ERR_HIP = -3,
    QC_ERR_RCCL = -4,
    QC_ERR_UNSUPPORTED = -5
};

typedef struct qc_system qc_system;

/* ---- system model: replaces `&MolecularSystem` (molint::system, main.rs:76-77; members read at rhf.rs:36-37).
 * Atoms: atomic numbers + xyz (bohr).  Shells are *segmented* contracted shells: centre atom index, angular momentum
 * (0..3), pure (1 = real solid harmonics, 0 = Cartesian; ignored for L < 2), primitive count, then the primitives of
 * all shells concatenated in `exponents` / `coefficients` (raw contraction coefficients as in the basis-set file;
 * normalisation is done here).  Inputs are copied. */
int qc_system_create(int natoms, const int32_t *atomic_numbers, const double *xyz,
                     int nshells, const int32_t *shell_atom, const int32_t *shell_L, const int32_t *shell_pure,
                     const int32_t *shell_nprim, const double *exponents, const double *coefficients,
                     qc_system **out);
void qc_system_destroy(qc_system *sys);

int qc_nbasis(const qc_system *sys);              /* system.n_basis(), rhf.rs:37 */
int qc_nelectrons(const qc_system *sys);          /* sum of atom.ordinal, rhf.rs:36 */
int qc_nshells(const qc_system *sys);
int64_t qc_nquartets(const qc_system *sys);       /* unique shell quartets (A>=B, C>=D, AB>=CD), before screening */
double qc_nuclear_repulsion(const qc_system *sys);/* compute_nuclear_repulsion, rhf.rs:110-122 */

/* ---- one-electron matrices: replace molint::overlap / kinetic / nuclear (rhf.rs:41-43).  Host code (round 1);
 * out = caller-allocated n*n doubles. */
int qc_overlap(const qc_system *sys, double *out);
int qc_kinetic(const qc_system *sys, double *out);
int qc_nuclear(const qc_system *sys, double *out);
/* The same three matrices computed on the GPU (qc_one_electron.hip; what the SCF drivers use): which = 0 overlap,
 * 1 kinetic, 2 nuclear attraction; out: n*n doubles on the host.  The three entry points above run on the host and need
 * no device. */
int qc_one_electron_gpu(qc_system *sys, int which, double *out);

/* ---- two-electron integrals: replaces molint::eri (rhf.rs:45, uhf.rs:55).  GPU.  out = n^4 doubles on the host,
 * row-major (i,j,k,l), chemists' notation (ij|kl) - the index order rhf.rs:60-61 reads.  The same device tensor feeds
 * every MP2 energy (qc_mp2, qc_scf_mp2) and the stored Fock mode (qc_set_fock_mode); the direct SCF drivers never
 * materialise it. */
int qc_eri_full(qc_system *sys, double *out);

/* ---- Fock build: replaces compute_electronic_hamiltonian (rhf.rs:152-167 incl. the tensor of rhf.rs:58-62;
 * uhf.rs:210-227).  GPU, direct: ERI shell quartets are evaluated and digested on the fly.
 *   RHF:  G = J[D] - 1/2 K[D]          (D carries the factor 2 of rhf.rs:179)
 *   UHF:  Ga = J[Da+Db] - K[Da],  Gb = J[Da+Db] - K[Db]
 * Host pointers, n*n each.  With a communicator attached (qc_comm_init) each rank digests its shard of the quartet
 * list and the partial matrices are summed with one RCCL all-reduce. */
int qc_fock_rhf(qc_system *sys, const double *D, double *G);
int qc_fock_uhf(qc_system *sys, const double *Da, const double *Db, double *Ga, double *Gb);
/* Same with device pointers (inputs/outputs resident in HBM); asynchronous on the handle's stream. */
int qc_fock_rhf_device(qc_system *sys, const double *dD, double *dG);
int qc_fock_uhf_device(qc_system *sys, const double *dDa, const double *dDb, double *dGa, double *dGb);

/* ---- symmetric eigensolver: replaces utils::sorted_eigs (hf/utils.rs:20-36).  GPU.  A: n*n symmetric;
 * V: eigenvectors as columns (V[i*n+k] = component i of vector k); w ascending. */
int qc_sym_eig(qc_system *sys, int n, const double *A, double *V, double *w);
/* Same, started from the eigenvectors V0 of a nearby matrix (the SCF loop's case from its second pass on): GEMM-based
 * eigenvector refinement with a Jacobi fallback.  Result identical to qc_sym_eig up to rounding and rotations inside
 * degenerate subspaces. */
int qc_sym_eig_warm(qc_system *sys, int n, const double *A, const double *V0, double *V, double *w);

/* ---- SCF drivers: replace restricted_hartree_fock (rhf.rs:32-108) / unrestricted_hartree_fock (uhf.rs:36-167). */
typedef struct {
    size_t max_iterations;   /* HartreeFockConfig.max_iterations, hf/mod.rs:11 */
    double epsilon;          /* HartreeFockConfig.epsilon, hf/mod.rs:14 */
    /* extension block - zero-initialise for reference behaviour */
    int32_t n_alpha;         /* UHF only; <= 0 with n_beta <= 0: the reference's rule N/2 each (uhf.rs:43-45) */
    int32_t n_beta;
    int32_t reserved[6];
} qc_hf_config;

typedef struct {
    double *orbital_energies;        /* caller buffer, n doubles (RHF) - RestrictedHartreeFockOutput, rhf.rs:14-24 */
    double *orbital_energies_beta;   /* caller buffer, n doubles (UHF beta; alpha goes to orbital_energies), uhf.rs:15-28 */
    double electronic_energy;
    double nuclear_repulsion;
    size_t iterations;               /* 0-based index of the converging iteration (rhf.rs:101) */
    /* timings of the run, milliseconds (not in the reference; the CLI prints its own wall-clock, main.rs:79-101) */
    double ms_setup, ms_fock_total, ms_linalg_total, ms_total;
    double ms_tuner;                 /* of ms_total: host time of the builds that tuned the stream assignment (first build of a geometry) */
} qc_hf_output;

int qc_scf_rhf(qc_system *sys, const qc_hf_config *cfg, qc_hf_output *out);
int qc_scf_uhf(qc_system *sys, const qc_hf_config *cfg, qc_hf_output *out);

/* ---- the same drivers one loop-body pass at a time, for a host that owns the convergence loop itself (the Rust
 * `core` crate in the north-star design; bench.py times exactly K passes through these).
 *   begin   = everything before the loop: integrals, S^-1/2, Hueckel guess, DIIS windows  (rhf.rs:36-65, uhf.rs:40-78)
 *   iterate = one pass of the body: G, F, error, DIIS, eigensolve, new density, energy, rms (rhf.rs:67-88, uhf.rs:81-137);
 *             returns the electronic energy of rhf.rs:84-85 (uhf.rs:145-153) and the density rms the reference
 *             compares with epsilon (for UHF the averaged value of uhf.rs:137, to be tested as rms/2 < epsilon). */
typedef struct qc_scf_state qc_scf_state;
int qc_scf_begin_rhf(qc_system *sys, qc_scf_state **out);
int qc_scf_begin_uhf(qc_system *sys, int n_alpha, int n_beta, qc_scf_state **out);
int qc_scf_iterate(qc_scf_state *st, double *electronic_energy, double *density_rms);
int qc_scf_orbital_energies(qc_scf_state *st, int spin, double *out_n);
int qc_scf_density(qc_scf_state *st, int spin, double *out_nxn);
/* Set-up matrices of the state, n*n doubles to the host: which = 0 overlap S (rhf.rs:41), 1 core Hamiltonian H = T + V
 * (rhf.rs:48), 2 transformation matrix X = S^-1/2 (compute_transformation_matrix, rhf.rs:124-131). */
int qc_scf_matrix(qc_scf_state *st, int which, double *out_nxn);
/* <S^2> of the current UHF determinant: Sz (Sz + 1) + N_beta - tr(D_alpha S D_beta S), Sz = (N_alpha - N_beta) / 2.
 * The reference leaves open shells as a TODO (uhf.rs:42, main.rs:111); this is the diagnostic that goes with the
 * n_alpha / n_beta extension.  RHF states return 0. */
int qc_scf_spin_square(qc_scf_state *st, double *s2);
int qc_scf_timings(qc_scf_state *st, double *ms_setup, double *ms_fock, double *ms_linalg);
/* The stopping rule of the host's loop, told to the library: "I stop calling qc_scf_iterate once rms < epsilon (RHF, rhf.rs:94) /
 * rms / 2 < epsilon (UHF, uhf.rs:139)".  Kept for hosts that call it: a null state or a negative / NaN epsilon is QC_ERR_INVALID,
 * anything else is accepted and ignored (nothing in the library acts on the rule any more). */
int qc_scf_set_stop_rule(qc_scf_state *st, double epsilon);
/* out[0 .. n) of: ms_setup, ms_fock (builds that contained a tuner run are left out), ms_linalg, builds counted in ms_fock, host ms of
 * the first build's timing passes, passes done, two slots that are reserved, always 0, passes whose eigensolve was
 * repeated, trials of the online stream-assignment search so far (handle-wide), 1 once that search has ended, then the Roothaan steps
 * (one per spin and pass; steps, not launches) that went through the one-workgroup kernel of n <= 64, by eigensolve route: refinement of the previous vectors
 * (one launch), tridiagonal start (between two launches), a Jacobi kernel (between two launches) */
#define QC_SCF_NCOUNTERS 14
int qc_scf_counters(qc_scf_state *st, double *out, int n);
void qc_scf_end(qc_scf_state *st);

/* ---- after SCF (not in the reference).  MO coefficients of the state's last Roothaan step, n*n to the host, V[i*n+k] = component i of
 * MO k (the layout of qc_sym_eig), columns in the order of qc_scf_orbital_energies (ascending).  spin 0 / 1 (UHF beta).  QC_ERR_INVALID
 * before the first qc_scf_iterate. */
int qc_scf_coefficients(qc_scf_state *st, int spin, double *out_nxn);

/* ---- MP2 correlation energy, conventional: the AO tensor is built in HBM, transformed to (ia|jb) by four f64 MFMA quarter
 * transformations and freed at the end of the call.  Needs ~8 (n^4 + o n^3 + o v n^2 + ...) bytes of free HBM (QC_ERR_UNSUPPORTED
 * otherwise, and on a sharded handle).  With D = e_i + e_j - e_a - e_b over active orbitals (the lowest n_frozen of each spin take no part):
 *   RHF: e_os = sum (ia|jb)^2 / D,  e_ss = sum (ia|jb) [(ia|jb) - (ib|ja)] / D
 *   UHF: e_os = sum (i_a a_a|j_b b_b)^2 / D,  e_ss = sum over both spins of 1/2 sum (ia|jb) [(ia|jb) - (ib|ja)] / D
 * QC_ERR_INVALID for null pointers, n_frozen < 0 or > min(nocc), or any D >= 0 (checked on the host from the orbital energies, before
 * the device is touched).  Empty blocks (no electrons or no virtuals in one spin) contribute 0.  The result is bitwise reproducible. */
typedef struct {
    double e_os;          /* opposite-spin part of the MP2 correlation energy */
    double e_ss;          /* same-spin part */
    double e_corr;        /* e_os + e_ss */
    double ms_tensor, ms_transform, ms_energy;   /* wall time of the phases (stream-synchronised) */
    int32_t n_frozen;
    int32_t reserved[7];
} qc_mp2_output;

/* MP2 from the state's last C and orbital energies (what qc_scf_coefficients / qc_scf_orbital_energies report).  The state is left
 * exactly as it was: qc_scf_iterate may be called again. */
int qc_scf_mp2(qc_scf_state *st, int32_t n_frozen, qc_mp2_output *out);

/* The same from caller-supplied orbitals (host pointers).  nspin 1: C n*n, eps n, nocc[0] doubly occupied.
 * nspin 2: C = [Ca; Cb] 2*n*n, eps 2*n, nocc = {n_alpha, n_beta}. */
int qc_mp2(qc_system *sys, int nspin, const double *C, const double *eps, const int32_t *nocc, int32_t n_frozen, qc_mp2_output *out);

/* ---- nuclear gradient (after SCF, not in the reference).  dE/dX in Eh/bohr, atoms in input order, components x, y, z:
 *   dE/dX = sum P_t dh/dX + 1/2 sum d(mn|ls)/dX [P_t,mn P_t,ls - P_a,ml P_a,ns - P_b,ml P_b,ns] - sum W dS/dX + dVnn/dX
 * with P_t = P_a + P_b and h = T + V (dV includes the derivative of the operator: the nuclei move too).  This equals the derivative of the
 * energy only at a converged state; at any other state it is the formula above evaluated at the current orbitals.  Shells s to f, pure
 * and Cartesian.  The two-electron quartets follow qc_set_schwarz.  Bitwise reproducible from call to call and across fresh handles.
 * QC_ERR_INVALID for null pointers or nspin not 1 / 2 (checked before the device is touched), QC_ERR_NO_DEVICE without a device,
 * QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator, for more than 682 atoms (the per-workgroup atom rows are held in
 * 32 KB of LDS), and when one quartet class's tables would exceed the 160 KB of LDS of a workgroup (not reached by s..f shells). */

/* The fixed-density contraction from host pointers (the gradient counterpart of qc_fock_rhf / qc_fock_uhf).  nspin 1: D n*n in the
 * qc_fock_rhf convention (the factor 2 included; P_a = P_b = D/2).  nspin 2: D = [Da; Db] 2*n*n.  W: the energy-weighted density, n*n.
 * terms receives 4 x natoms x 3 doubles: nuclear repulsion, core Hamiltonian (kinetic + nuclear attraction, Hellmann-Feynman part
 * included), overlap (-W.S'), two-electron.  The gradient is their sum. */
int qc_gradient(qc_system *sys, int nspin, const double *D, const double *W, double *terms);

/* natoms x 3 doubles: the total gradient at the state's last Roothaan step, RHF or UHF.  P is the state's density (what qc_scf_density
 * returns), W = sum_spin sum_{i occ} n_i e_i c_i c_i^T from the C and orbital energies of qc_scf_coefficients / qc_scf_orbital_energies,
 * both on the device.  QC_ERR_INVALID before the first qc_scf_iterate.  The state is left exactly as it was. */
int qc_scf_gradient(qc_scf_state *st, double *grad);

/* Phase times (ms) of the handle's last gradient call: P/W build (qc_scf_gradient; qc_gradient: the spin combination of the uploaded
 * densities) + Cartesian transform, one-electron terms, two-electron term, sum. */
int qc_gradient_timings(const qc_system *sys, double *ms4);

/* ---- wave-function stability (after SCF, not in the reference).  The lowest eigenvalues of the real orbital Hessian (A + B) at the state's
 * last C and orbital energies (what qc_scf_coefficients / qc_scf_orbital_energies report), by a Davidson iteration on the device whose
 * Hessian-vector product is one direct Fock build per trial vector (always the direct build, whatever qc_set_fock_mode says; no n^4
 * storage).  A negative eigenvalue: the state is a saddle of the HF functional, the eigenvector points downhill.  The diagonal uses the
 * canonical-orbital formula e_a - e_i: at an unconverged state the result is that formula at the current orbitals, as for the gradient.
 *   kind 0  RHF state: singlet (real RHF -> real RHF) instabilities;  UHF state: internal (real UHF -> real UHF) instabilities
 *   kind 1  RHF state only: triplet (RHF -> UHF) instabilities
 * A vector has qc_scf_stability_dim entries: RHF o*v; UHF o_a*v_a + o_b*v_b, alpha block first; each block laid out x[i*v + a] (i occupied,
 * a virtual, both counted from 0 in the order of the orbital energies); |x| = 1 over the whole vector.
 * In:  kind; nroots 1..8 (and <= dim); tol: residual 2-norm every root must reach (0: 1e-6); max_iterations (0: 100).
 * Out: eigenvalues ascending, residual norms, roots converged, iterations, Fock builds, wall time of the call and of its builds (ms).
 * QC_NOT_CONVERGED when the iterations run out (the outputs are filled with the best estimates).  QC_ERR_INVALID: null pointers, bad
 * nroots / kind, kind 1 on a UHF state, a state before its first qc_scf_iterate, dim = 0 - all checked before the device is touched.
 * QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator.  Bitwise reproducible from call to call and across fresh handles.
 * The state is left exactly as it was: qc_scf_iterate may be called again and gives what it would have given. */
typedef struct {
    int32_t kind, nroots, max_iterations, reserved0;
    double tol;
    double eigenvalues[8], residuals[8];
    int32_t nconverged, iterations, builds, reserved1;
    double ms_total, ms_builds;
} qc_stability;
int qc_scf_stability_dim(qc_scf_state *st, int kind);                   /* length of a vector; QC_ERR_INVALID for a bad kind */
int qc_scf_stability(qc_scf_state *st, qc_stability *io, double *vectors /* nullable: nroots x dim doubles on the host */);

/* The determinant rotated along x (a vector of qc_scf_stability): C' = C exp(theta kappa), kappa_ai = x_ia = -kappa_ia in the MO basis - an
 * exact orthogonal rotation for any theta.  Da, Db: n*n each on the host, C_occ' C_occ'^T per spin (no factor 2; an RHF state fills both).
 * RHF kind 0 rotates both spins by theta, RHF kind 1 alpha by +theta and beta by -theta.  angle > 0: theta in radians; angle <= 0: the
 * library evaluates the energy at theta = +-0.1 * 2^k, k = 0..4 (at most ten Fock builds) and returns the lowest.  energy (nullable): the
 * electronic energy of the returned determinant.  Errors as qc_scf_stability; the state is left exactly as it was. */
int qc_scf_rotated_density(qc_scf_state *st, int kind, const double *x, double angle, double *Da, double *Db, double *energy);

/* ---- dipole moment and static dipole polarizability (after SCF, not in the reference).  Atomic units throughout (e bohr; bohr^3).
 * The three dipole matrices M_k = <a| (r - O)_k |b>, k = x, y, z, one after the other (3*n*n doubles, each exactly symmetric), in the
 * library's basis functions: same normalisation and Cartesian-to-pure transform as the overlap.  origin: three doubles, NULL = (0, 0, 0).
 * The first needs no device (like the overlap); the second runs the GPU kernel the properties below use. */
int qc_dipole_matrices(const qc_system *sys, const double *origin, double *out);
int qc_dipole_matrices_gpu(qc_system *sys, const double *origin, double *out);

/* mu_k = sum_A Z_A (R_A - O)_k - tr(P_t M_k) with P_t = P_alpha + P_beta the state's density on the device (what qc_scf_density
 * returns; available from qc_scf_begin_* on).  mu_nuclear (nullable): the first sum alone, computed on the host.  The trace is a fixed-order
 * reduction: two calls give the same bits.  For a neutral system mu does not depend on the origin.  The state is left exactly as it was. */
int qc_scf_dipole(qc_scf_state *st, const double *origin, double mu[3], double mu_nuclear[3]);

/* Static dipole polarizability by coupled-perturbed Hartree-Fock at the state's last C and orbital energies: (A + B) U^q = r^q for the
 * three directions, r^q = C_occ^T M_q C_virt per spin block, alpha_pq = c r^p . U^q with c = 4 (RHF, the singlet operator) or 2 (UHF,
 * the internal operator); vectors laid out as for qc_scf_stability (length: qc_scf_stability_dim of kind 0).  (A + B) x is the product of the stability
 * analysis: one direct Fock build per trial vector, always the direct build, no n^4 storage.  Reduced-space iteration with one subspace
 * of at most 40 vectors shared by the three right-hand sides; the projected systems are solved on the host by LU.  A right-hand side that
 * is exactly zero costs no build, and its row and column of alpha are exactly zero.  At a converged, stable state alpha is minus the
 * second derivative of the energy with respect to a uniform field; the canonical-orbital diagonal e_a - e_i is used as for stability.
 * In:  tol: residual 2-norm every system must reach (0: 1e-6); max_iterations (0: 100).
 * Out: alpha row-major, symmetrised 1/2 (alpha_pq + alpha_qp); asymmetry: the largest |alpha_pq - alpha_qp| before that; residual norms,
 * systems converged, iterations, Fock builds, wall time of the call and of its builds (ms).  response (nullable): the three U^q on the host.
 * QC_NOT_CONVERGED when the iterations run out or a projected system is singular: alpha, response and residuals then all belong to the
 * last estimate that could be formed (before the first solve that is U = 0, whose residuals are the norms of the right-hand sides).  QC_ERR_INVALID:
 * null pointers, a negative or NaN tol, a negative max_iterations, a state before its first qc_scf_iterate - all checked before the
 * device is touched.  No occupied-virtual pair at all: QC_OK, alpha = 0, no build.  QC_ERR_UNSUPPORTED on a sharded handle or one with a
 * communicator.  Bitwise reproducible from call to call and across fresh handles.  The state is left exactly as it was. */
typedef struct {
    int32_t max_iterations, reserved0;
    double tol;
    double alpha[9];
    double residuals[3], asymmetry;
    int32_t nconverged, iterations, builds, reserved1;
    double ms_total, ms_builds;
} qc_polarizability;
int qc_scf_polarizability(qc_scf_state *st, qc_polarizability *io, double *response /* nullable: 3 x dim doubles on the host */);

/* ---- the wave function in space (not in the reference): electron density, orbitals and electrostatic potential on caller-given points.
 * Atomic units, points in bohr as npts x 3 doubles (x, y, z of a point together), f64 throughout.  With phi_a the library's basis
 * functions (normalisation and Cartesian-to-pure transform of qc_overlap) and D a symmetric n x n matrix:
 *   rho(r) = sum_ab D_ab phi_a(r) phi_b(r)          psi_k(r) = sum_a C_ak phi_a(r)
 *   v_elec(r) = -sum_ab D_ab (a| 1/|r' - r| |b)     v_nuc(r) = sum_A Z_A / |r - R_A|     V(r) = v_nuc(r) + v_elec(r)
 * v_nuc is plain IEEE division: a point on a nucleus gives +inf there (and in V), while v_elec is finite and right.
 *
 * Host only, no device needed (like qc_overlap / qc_dipole_matrices).  basis_on_points: out npts x n, row = point.  potential_matrix:
 * out n x n, A_ab = (a| 1/|r' - r| |b) for one point r - the nuclear-attraction integral of a unit charge at r without its -Z; positive
 * and exactly symmetric.  esp_records: the number of stored primitive pairs (records of the potential kernels) of each pair order
 * L = l_a + l_b = 0..6, for work models.  QC_ERR_INVALID: null pointers, npts < 0. */
int qc_basis_on_points(const qc_system *sys, int64_t npts, const double *xyz, double *out);
int qc_potential_matrix(const qc_system *sys, const double r[3], double *out);
int qc_esp_records(const qc_system *sys, int64_t counts[7]);

/* GPU, density or orbitals from host pointers (the grid counterparts of qc_fock_rhf / qc_gradient).  D: n x n (a matrix that is not
 * symmetric is taken as 1/2 (D + D^T) by the potential).  C: n x m, column = orbital, leading dimension m; out: m x npts.  v_nuc is
 * nullable.  Points are processed in batches sized from the free device memory, so any npts works.  Primitive pairs under the
 * library's cut-off (1e-17) are left out of the potential as they are out of the Fock build.
 * QC_ERR_INVALID: null pointers, npts < 0, m <= 0 - checked first.  QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator.
 * npts == 0: QC_OK, nothing is launched and nothing written.  QC_ERR_NO_DEVICE without a device.
 * Bitwise reproducible from call to call and across fresh handles; the value of a point depends neither on the other points of the
 * call nor on how the points are batched (every sum has a fixed order: no atomics). */
int qc_density_on_points(qc_system *sys, const double *D, int64_t npts, const double *xyz, double *rho);
int qc_esp_on_points(qc_system *sys, const double *D, int64_t npts, const double *xyz, double *v_elec, double *v_nuc);
int qc_orbitals_on_points(qc_system *sys, int m, const double *C, int64_t npts, const double *xyz, double *out);

/* GPU, from an SCF state: its densities (what qc_scf_density returns; available from qc_scf_begin_* on, as for qc_scf_dipole) and its
 * orbitals (qc_scf_coefficients) are read where they lie on the device.  density: which 0 = P_alpha + P_beta, 1 = P_alpha - P_beta (an
 * RHF state gives exactly 0).  esp: v_total = v_nuc + v_elec of P_alpha + P_beta; v_elec nullable.  orbitals: `count` orbitals of `spin`
 * from `first`, counted from 0 in the order of qc_scf_orbital_energies; out count x npts.
 * Errors as above; also QC_ERR_INVALID for a bad which / spin / first / count and, for the orbital call, a state before its first
 * qc_scf_iterate.  No Fock build runs and nothing of the state is written: a following qc_scf_iterate gives the bits it would have given. */
int qc_scf_density_on_points(qc_scf_state *st, int which, int64_t npts, const double *xyz, double *rho);
int qc_scf_esp_on_points(qc_scf_state *st, int64_t npts, const double *xyz, double *v_total, double *v_elec);
int qc_scf_orbitals_on_points(qc_scf_state *st, int spin, int first, int count, int64_t npts, const double *xyz, double *out);

/* Phase times (ms, summed over the batches) of the handle's last point call: upload, basis values (potential: the Hermite densities of
 * the call), contraction (GEMM + column dots; potential: the per-point kernels), download. */
int qc_points_timings(const qc_system *sys, double ms[4]);

/* ---- Cartesian multipole moments, population analysis and ESP-fitted charges (after SCF, not in the reference).  Atomic units, host
 * pointers.  Common to the GPU calls below: QC_ERR_INVALID for bad arguments, checked before the device is touched; QC_ERR_NO_DEVICE
 * without a gfx950 device; QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator; bitwise reproducible from call to call
 * and across fresh handles (every sum has a fixed order: no float atomics); a state is left exactly as it was (no Fock build runs).
 *
 * Multipole matrices M_c = <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b> of all orders l = i + j + k <= order, order 0 .. 4:
 * qc_multipole_count(order) = (order+1)(order+2)(order+3)/6 = 1, 4, 10, 20, 35 matrices of n*n doubles one after the other (-1 outside
 * 0 .. 4), each exactly symmetric, in the library's basis functions (normalisation and Cartesian-to-pure transform of the overlap).
 * Components by l ascending, inside an order i descending, then j descending: c = 0 the overlap, 1 .. 3 x y z (the dipole matrices),
 * 4 .. 9 xx xy xz yy yz zz, and so on.  A call of a lower order gives the leading matrices of a higher one bit for bit.
 * origin: three doubles, NULL = (0, 0, 0).  The first needs no device; the second runs the kernel qc_scf_multipoles uses.
 * QC_ERR_INVALID: a null handle or `out`, an order outside 0 .. 4. */
#define QC_MULTIPOLE_MAX_ORDER 4
int qc_multipole_count(int order);
int qc_multipole_matrices(const qc_system *sys, int order, const double *origin, double *out);
int qc_multipole_matrices_gpu(qc_system *sys, int order, const double *origin, double *out);

/* Total Cartesian moments of a state.  In: order (0 .. 4), origin.  Out, per component c < qc_multipole_count(order) (the rest 0):
 * nuclear[c] = sum_A Z_A (R_A - O)^c on the host, electronic[c] = -tr(P_t M_c) with P_t = P_alpha + P_beta the state's density on the
 * device (available from qc_scf_begin_* on, as for qc_scf_dipole), total = nuclear + electronic; total[0] is the molecular charge and
 * total[1 .. 3] the dipole moment.  quadrupole_traceless: xx xy xz yy yz zz of (3 Q_ab - delta_ab tr Q) / 2 from the total second
 * moments Q; 0 when order < 2.  QC_ERR_INVALID: a null pointer, an order outside 0 .. 4. */
typedef struct {
    int32_t order, reserved;
    double origin[3];
    double total[35], nuclear[35], electronic[35];
    double quadrupole_traceless[6];
} qc_multipoles;
int qc_scf_multipoles(qc_scf_state *st, qc_multipoles *io);

/* Population analysis.  scheme 0: Mulliken charges with Mayer bond orders; 1: Loewdin charges with Wiberg indices in the Loewdin basis.
 * With P_t = P_alpha + P_beta, P_s = P_alpha - P_beta, "a in A" = function a sits on atom A, and A_x = P_x S (scheme 0) or
 * A_x = S^1/2 P_x S^1/2 (scheme 1; S^1/2 = S X with X the S^-1/2 of the SCF set-up):
 *   N_A = sum_{a in A} (A_t)_aa,  charges[A] = Z_A - N_A,  spin[A] = sum_{a in A} (A_s)_aa,  orbital[a] = (A_t)_aa,
 *   bond_orders[A, B] = sum_{a in A, b in B} (A_t)_ab (A_t)_ba + (A_s)_ab (A_s)_ba  (exactly symmetric; the diagonal as computed).
 * charges: natoms.  spin (nullable): natoms, exactly 0 for an RHF state or nspin 1.  orbital (nullable): n.  bond_orders (nullable):
 * natoms x natoms.  The first reads the state's densities, S and X where they lie on the device.  The second takes host densities in
 * the qc_fock_rhf / qc_gradient conventions (nspin 1: D n*n with the factor 2; nspin 2: [Da; Db]) and builds S and X itself with the
 * kernels and the eigensolver of the SCF set-up.  QC_ERR_INVALID: a null handle, state, D or `charges`, a scheme outside 0 .. 1, an
 * nspin outside 1 .. 2. */
int qc_scf_populations(qc_scf_state *st, int scheme, double *charges, double *spin, double *orbital, double *bond_orders);
int qc_populations(qc_system *sys, int scheme, int nspin, const double *D, double *charges, double *spin, double *orbital, double *bond_orders);

/* Charges fitted to the electrostatic potential (Merz-Kollman).
 * In (0 = default): nscales (at most 8) and scales - factors of the van der Waals radii of the shells of points, default 4: 1.4 1.6
 * 1.8 2.0; density - points per bohr^2 of sphere surface, default 1 per Angstrom^2 (1 bohr = QC_BOHR_ANGSTROM Angstrom).
 * Out: npts; total_charge (the constraint); rms of V - V_fit over the points and rrms = rms / rms(V); dipole = sum_A q_A R_A (origin 0);
 * wall times of the state call and of its potential (ms).
 * Radii in Angstrom: H 1.20, He 1.40, C 1.70, N 1.55, O 1.52, F 1.47, Ne 1.54, Si 2.10, P 1.80, S 1.80, Cl 1.75, Ar 1.88, all others
 * 2.00.  Grid, deterministic: for each scale f (in the order given), each atom A (input order) and k = 0 .. N - 1 with R = f r_A and
 * N = ceil(density 4 pi R^2): z = 1 - (2k + 1) / N, phi = k pi (3 - sqrt 5), point R_A + R (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi,
 * z); a point is kept if and only if its distance to every other atom B is >= f r_B.
 * qc_esp_fit_points (host only): the grid into xyz (capacity points of 3 doubles) and its size into *npts; capacity < *npts is
 * QC_ERR_INVALID with *npts filled and nothing written (xyz nullable when capacity is 0).
 * qc_esp_fit_solve (host only): the charges that minimise sum_p (v_p - sum_A q_A / |r_p - R_A|)^2 subject to sum_A q_A = total_charge -
 * the (natoms + 1)^2 system [A^T A, 1; 1^T, 0] accumulated in point order, solved by LU with partial pivoting; fills the outputs of io
 * (io's inputs are not read).  QC_ERR_INVALID: null pointers, npts < natoms, a point on a nucleus, a non-finite v, a singular system.
 * qc_scf_esp_charges: the potential of the state on the library's grid for io's inputs (xyz NULL; npts is ignored) or on the caller's
 * npts points - exactly the V of qc_scf_esp_on_points, bit for bit, returned in v_out (nullable; npts or io->npts doubles) - and the
 * fit with total_charge = sum Z - n_alpha - n_beta.  Errors as above and as qc_scf_esp_on_points. */
#define QC_BOHR_ANGSTROM 0.529177210903
typedef struct {
    int32_t nscales, reserved0;
    double scales[8];
    double density;
    int64_t npts;
    double total_charge, rms, rrms;
    double dipole[3];
    double ms_total, ms_potential;
} qc_esp_fit;
int qc_esp_fit_points(const qc_system *sys, const qc_esp_fit *cfg, int64_t capacity, double *xyz, int64_t *npts);
int qc_esp_fit_solve(const qc_system *sys, int64_t npts, const double *xyz, const double *v, double total_charge, qc_esp_fit *io, double *charges);
int qc_scf_esp_charges(qc_scf_state *st, qc_esp_fit *io, int64_t npts, const double *xyz, double *charges, double *v_out);

/* ---- point-charge embedding (not in the reference): the molecule in the field of external point charges, the electrostatic half of a
 * QM/MM driver.  Atomic units, coordinates in bohr, f64 throughout.  A charge set is npc points R_c (npc x 3 doubles) with charges q_c -
 * any finite doubles, negative ones and 0 included.  With A_ab(r) = (a| 1/|r' - r| |b), what qc_potential_matrix returns:
 *   V_pc = -sum_c q_c A(R_c)   (n x n, exactly symmetric)        E_nq = sum_A sum_c Z_A q_c / |R_A - R_c|
 * The charge-charge energy belongs to the caller and appears nowhere.  The charges are not atoms: qc_nelectrons, qc_nuclear_repulsion
 * and qc_hf_output.nuclear_repulsion do not see them.
 *
 * qc_set_point_charges (host only, works without a device): the inputs are copied; npc == 0 removes the set.  QC_ERR_INVALID, with the
 * handle's set left as it was: a null handle, npc < 0, null arrays with npc > 0, a coordinate or charge that is not finite, a charge at
 * distance exactly 0 from an atom.  SCF states begun afterwards take a snapshot of the set: their H = T + V + V_pc, so the Hueckel guess,
 * the electronic energy (it contains tr(P V_pc)), qc_scf_matrix(.., 1) and everything computed from C and the orbital energies belong to
 * the embedded Hamiltonian; the total energy is electronic + nuclear repulsion + E_nq.  States that are alive keep the set they began
 * with (qc_scf_point_charge_count / qc_scf_point_charge_nuclear_energy report it).  The fixed-density calls use the handle's current set.
 * With no charges set nothing changes: no kernel is launched, nothing allocated, every result keeps its bits.
 * qc_point_charge_count: the number of charges of the handle's set.  qc_point_charge_nuclear_energy: E_nq, on the host. */
int qc_set_point_charges(qc_system *sys, int64_t npc, const double *xyz, const double *q);
int64_t qc_point_charge_count(const qc_system *sys);
double qc_point_charge_nuclear_energy(const qc_system *sys);
int64_t qc_scf_point_charge_count(const qc_scf_state *st);
double qc_scf_point_charge_nuclear_energy(const qc_scf_state *st);

/* V_pc of the handle's set, n*n doubles on the host (all zero without charges).  The first runs on the host, serially, and needs no
 * device: the reference statement.  The second runs the kernels the SCF set-up uses (qc_embed.hip): per stored primitive pair the
 * Hermite-Coulomb tables of all charges summed in a fixed order (tiles of 256 charges, each summed in an order that depends on the
 * numbers of records and charges alone, tile sums added ascending), then one assembly from the stored pair data - primitive pairs under the library's cut-off (1e-17) are left out as they are out of the Fock
 * build.  Bitwise reproducible from call to call and across fresh handles; works on a sharded handle (every rank builds it whole).
 * QC_ERR_INVALID: null pointers.  QC_ERR_NO_DEVICE (the second) without a device. */
int qc_point_charge_matrix(const qc_system *sys, double *out);
int qc_point_charge_matrix_gpu(qc_system *sys, double *out);

/* The electric field of the molecule alone (never of the charges) on caller-given points: E = -grad V with V, v_elec and v_nuc exactly
 * those of qc_esp_on_points; outputs npts x 3 doubles (x, y, z of a point together).
 * qc_field_matrix (host only): out = 3 n*n doubles, B^k_ab = dA_ab(r)/dr_k for k = x, y, z - the derivative companion of
 * qc_potential_matrix, each matrix exactly symmetric; e_elec_k(r) = tr(D B^k).
 * qc_field_on_points / qc_scf_field_on_points (GPU): e_elec = -grad v_elec, e_nuc(r) = sum_A Z_A (r - R_A) / |r - R_A|^3, e_total =
 * e_nuc + e_elec.  Nullable arguments (e_nuc; e_elec of the state call), errors, the treatment of npts == 0 and of a matrix that is not
 * symmetric, bitwise reproducibility and the independence of a point's value from the other points of the call are those of
 * qc_esp_on_points / qc_scf_esp_on_points.  A point on a nucleus gives a non-finite e_nuc (and e_total) and a finite, correct e_elec.
 * The phase times of these calls are reported by qc_points_timings. */
int qc_field_matrix(const qc_system *sys, const double r[3], double *out);
int qc_field_on_points(qc_system *sys, const double *D, int64_t npts, const double *xyz, double *e_elec, double *e_nuc);
int qc_scf_field_on_points(qc_scf_state *st, int64_t npts, const double *xyz, double *e_total, double *e_elec);

/* Gradients with point charges.
 * qc_point_charge_gradient: fixed density, in the conventions of qc_gradient (nspin 1: D with the factor 2; nspin 2: [Da; Db]), for the
 * handle's current set.  terms receives 2 x npc x 3 doubles: dE_nq/dR_c, then d tr(P_t V_pc)/dR_c = -q_c e_elec(R_c).
 * qc_scf_point_charge_gradient: grad receives npc x 3 doubles, dE/dR_c at the state for the charges it began with; this is
 * -q_c e_total(R_c) with the field of qc_scf_field_on_points.  Both: npc == 0 is QC_OK with nothing written.
 * qc_gradient on a handle with charges: term 0 gains dE_nq/dR_A, term 1 gains sum_ab P_t,ab d(V_pc)_ab/dR_A - the basis-function
 * derivatives only, because the charges stay put.  qc_scf_gradient on an embedded state returns the full dE/dR_A with both additions,
 * for the charges the state began with.  Without charges both give the bits they gave before.
 * Errors as qc_gradient (QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator).  Bitwise reproducible from call to call and
 * across fresh handles; a state is left exactly as it was. */
int qc_point_charge_gradient(qc_system *sys, int nspin, const double *D, double *terms);
int qc_scf_point_charge_gradient(qc_scf_state *st, double *grad);

/* Phase times (ms) of the handle's last embedding call (qc_point_charge_matrix_gpu, the V_pc of an SCF set-up, the point-charge terms
 * of a gradient call): upload, Hermite sums over the charges, assembly or contraction, download. */
int qc_point_charge_timings(const qc_system *sys, double ms[4]);

/* ---- dense symmetric positive-definite inverse on the GPU (qc_chol.hip; what the continuum below needs, exported for tests).  A, Ainv:
 * n x n f64 on the host, row-major, n >= 1; only A's lower triangle is read.  Blocked Cholesky A = L L^T (64 x 64 diagonal blocks factored
 * and inverted by one workgroup in LDS, panels and trailing updates by the MFMA GEMM), X = L^-1 by block forward substitution,
 * Ainv = X^T X, mirrored so that it is exactly symmetric.  Every sum has a fixed order and there are no atomics: two calls give the same
 * bits.  A pivot that is <= 0 or not finite is replaced by 1, the factorisation runs to its end and the call returns QC_ERR_INVALID
 * (Ainv is then meaningless).  QC_ERR_INVALID also for null pointers or n < 1; QC_ERR_NO_DEVICE without a device. */
int qc_spd_inverse(qc_system *sys, int n, const double *A, double *Ainv);

/* ---- conductor-like continuum solvation, C-PCM / COSMO (not in the reference).  Atomic units.
 * Surface: one sphere per atom, radius R_I = scale * r_I with r_I the van der Waals radius of qc_esp_fit_points (or the caller's radii,
 * bohr, before scaling); on it N_I = ceil(density 4 pi R_I^2) golden-angle points (the rule of qc_esp_fit_points); a point of sphere I
 * is kept if and only if its distance to the centre of every other sphere J is >= R_J.  Order: atom, then k.  A kept point is a surface
 * element at s_i with area a_i = 4 pi R_I^2 / N_I, owned by atom I.  The cut is hard (no switching function): the energy is not smooth
 * in the geometry, and there are no gradients.
 * Cavity matrix, Gaussian-blurred charges (York-Karplus): zeta_i = c / sqrt(a_i), c = 1.0694 pi sqrt 2; S_ii = zeta_i sqrt(2 / pi)
 * (= Klamt's 1.0694 sqrt(4 pi / a_i)); S_ij = erf(zeta_ij r_ij) / r_ij, zeta_ij = zeta_i zeta_j / sqrt(zeta_i^2 + zeta_j^2).  S is a
 * Gram matrix, positive definite for any point set; the point-charge form 1 / r_ij is not.
 * Reaction field: f = (epsilon - 1) / (epsilon + x), x = 0 C-PCM, x = 0.5 COSMO.  v_i = v_nuc(s_i) + v_elec(s_i), the point potentials of
 * qc_esp_on_points for the TOTAL density;  q = K v, K = -f S^-1;  G_pol = 1/2 q.v;  V_R = -sum_i q_i A(s_i) (the matrix of
 * qc_point_charge_matrix for the charges q) = dG_pol/dD, so E_HF[D] + G_pol[D] is variational.
 * SCF: the reference's loop with electronic_hamiltonian := G(D) + V_R(D) (UHF: V_R of the total density in both spins' Fock matrices).
 * A pass reports 1/2 tr[D_new (2 H + G(D_old) + V_R(D_old))] with H the vacuum core Hamiltonian (rhf.rs:84-85 with that substitution);
 * at convergence this is E_HF,el + 1/2 q.v_elec, and the total energy is electronic + nuclear repulsion + 1/2 q.v_nuc.
 *
 * qc_set_solvent (host only): cfg NULL removes the solvent; 0 in scale / density: the defaults 1.2 and 5 points per Angstrom^2 (density is
 * in points per Angstrom^2).  QC_ERR_INVALID, the handle left as it was: epsilon not finite or <= 1, x < 0 or not finite, a negative or
 * non-finite scale or density, a radius <= 0 or not finite, an empty surface.  QC_ERR_UNSUPPORTED: more than 16384 elements.
 * qc_solvent_surface (host only): returns M (QC_ERR_INVALID without a solvent); when capacity >= M also writes xyz (M x 3), area (M)
 * and the owning atoms (M), each nullable.  qc_solvent_matrix (host only): S, M x M, the reference statement. */
typedef struct { double epsilon, x, scale, density; } qc_solvent;   /* 0 in scale / density: defaults 1.2, 5 per A^2 */
int     qc_set_solvent(qc_system *sys, const qc_solvent *cfg /* NULL removes */, const double *radii /* nullable, natoms, bohr */);
int64_t qc_solvent_surface(const qc_system *sys, int64_t capacity, double *xyz, double *area, int32_t *atom);  /* returns M */
int     qc_solvent_matrix(const qc_system *sys, double *S);        /* host statement of S, M x M */
/* GPU (qc_solvent.hip).  matrix_gpu: S by the assembly kernel (device erf; an element and its mirror are one value) and K = -f S^-1 by
 * qc_spd_inverse's kernels, both exactly symmetric, either nullable; K is built once per qc_set_solvent, at its first use, and kept on
 * the handle.  response: at the total density D (host, n x n) the charges q (M), V_R (n x n, exactly symmetric) and
 * energy = {1/2 q.v_nuc, 1/2 q.v_elec}; v_elec by the potential kernels of qc_esp_on_points, q and the dot products by one reaction
 * kernel (fixed summation order), V_R by the kernels of qc_point_charge_matrix_gpu.  Bitwise reproducible from call to call and across
 * fresh handles.  QC_ERR_INVALID: null sys / D / energy, no solvent; QC_ERR_UNSUPPORTED on a sharded handle or one with a communicator. */
int qc_solvent_matrix_gpu(qc_system *sys, double *S /* nullable */, double *K /* nullable */);
int qc_solvent_response(qc_system *sys, const double *D /* host, n*n, total density */, double *q /* M, nullable */,
                        double *V /* n*n, nullable */, double energy[2] /* 1/2 q.v_nuc, 1/2 q.v_elec */);
/* SCF.  States begun while a solvent is set take it with them (like the point charges) and keep it when the handle's is changed.
 * qc_scf_begin_* and the one-shot drivers return QC_ERR_UNSUPPORTED, before the device is touched, for a solvent together with a sharded
 * handle or a communicator, the stored-tensor mode, or point charges.  On a solvated state qc_scf_gradient (no cavity derivative),
 * qc_scf_stability, qc_scf_rotated_density, qc_scf_polarizability, qc_scf_excitations and qc_scf_excitation_matrices (no solvent response
 * term) return QC_ERR_UNSUPPORTED; the properties of the density (dipole, multipoles, populations, points, ESP charges) read the solvated
 * density; qc_scf_mp2 is the correlation energy on the solvated orbitals; qc_scf_matrix(.., 1) is the vacuum H.
 * qc_scf_solvent: 1/2 q.v_nuc, 1/2 q.v_elec, sum q and M for the state's current density (after scf_begin: the guess; after a pass: its
 * new density), q (nullable) the charges.  qc_solvent_last: the same of the last one-shot run on the handle that ended with QC_OK
 * (QC_ERR_INVALID if there is none).  qc_solvent_timings (ms): [0] the one-off set-up (S, factorisation, inverse; host clock), then of the last
 * response evaluation [1] the potential call and [3] the V_R call (host clock around calls that end in a wait: kernels, copies and
 * allocations) and [2] the reaction kernel alone (device events; its copies and the wait behind it are in none of the three).  Without a solvent nothing is launched or allocated and every result
 * keeps its bits. */
typedef struct { double nuclear, electronic, total_charge; int64_t npoints; } qc_solvent_energy;  /* 1/2 q.v_nuc, 1/2 q.v_elec, sum q */
int qc_scf_solvent(qc_scf_state *st, qc_solvent_energy *out, double *q /* nullable, M */);   /* of the last pass */
int qc_solvent_last(const qc_system *sys, qc_solvent_energy *out);                           /* of the last one-shot run on the handle */
int qc_solvent_timings(const qc_system *sys, double ms[4]);   /* set-up (S, factor, inverse); per pass: potential, reaction, matrix */

/* ---- excited states of an RHF state (after SCF, not in the reference): configuration interaction singles (CIS, the Tamm-Dancoff
 * approximation) and time-dependent Hartree-Fock (TDHF, the random-phase approximation), singlets or triplets, at the state's last C and
 * orbital energies.  With (pq|rs) in chemists' notation, i j occupied, a b virtual, Delta = delta_ij delta_ab (e_a - e_i), rows and columns
 * laid out [i * v + a] as for qc_scf_stability (dim = qc_scf_stability_dim of kind 0):
 *   singlets  A + B = Delta + 4 (ia|jb) - (ib|ja) - (ij|ab)        triplets  A + B = Delta - (ib|ja) - (ij|ab)
 *   both      A - B = Delta + (ib|ja) - (ij|ab)                    A = 1/2 [(A + B) + (A - B)]
 * (A + B) of kind k is the operator qc_scf_stability(kind k) applies by direct Fock builds.  Here both matrices are built explicitly: the
 * AO tensor in HBM (as qc_scf_mp2), MFMA quarter transformations to (ia|jb) and (ij|ab), one assembly kernel that makes both matrices
 * exactly symmetric; then every product of the iterative solver is one GEMM over all new trial vectors.  Needs about 8 (n^4 + o n^3) bytes
 * for the tensor phase and 24 dim^2 bytes for the matrices: QC_ERR_UNSUPPORTED when the device cannot hold them.  No frozen core; nothing
 * is cached between calls.
 * CIS: A X = w X by a block Davidson iteration (subspace of at most 40 vectors); any reference is accepted, a negative root is a result.
 * TDHF: (A - B)(A + B) R = w^2 R by the reduced-space algorithm of Stratmann, Scuseria and Frisch, J. Chem. Phys. 109, 8218 (1998), R = X + Y,
 *   L = X - Y = (A + B) R / w.  It needs A + B and A - B positive definite: before it starts, the lowest root theta of each matrix is found to
 *   its own residual rho, and if theta - rho <= 0 for either the call returns QC_NOT_CONVERGED with reference_unstable = 1, nconverged = 0
 *   and no state (RHF -> UHF unstable references have no triplet TDHF states; their CIS triplets exist).
 *   The check runs to tol with a budget of 100 rounds of its own, independent of max_iterations; should it end with rho >= theta > 0
 *   all the same, the reference is reported unstable (the flag then says "not certified", which errs on the safe side).
 * In:  method 0 CIS, 1 TDHF; kind 0 singlets, 1 triplets; nroots 1..8 and <= dim; tol: residual 2-norm every root must reach (0: 1e-6;
 *      TDHF: both |(A+B) R - w L| and |(A-B) L - w R|, residuals[k] is the larger); max_iterations (0: 100).
 * Out: excitation energies (Eh) ascending, residual norms; singlets: the transition dipole mu_k = sqrt 2 r . X_k (CIS) or sqrt 2 r . R_k (TDHF)
 *      with r^q = C_occ^T M_q C_virt (length gauge, origin (0, 0, 0)) and the oscillator strength f_k = 2/3 w_k |mu_k|^2; triplets: both
 *      exactly 0.  The sign of a vector, and with it the sign of mu_k, is arbitrary.  products: matrix-vector products (TDHF: with either
 *      matrix, the two checks of the reference included); iterations: rounds of the solver; wall times of the call, the AO tensor, the
 *      transformation with the assembly, and the solver (ms).
 * vectors (nullable, host): CIS nroots x dim with |X_k| = 1; TDHF 2 x nroots x dim - all R_k first, then all L_k, with L_k . R_k = 1
 *      (X^T X - Y^T Y = 1).
 * QC_NOT_CONVERGED when the iterations run out (the outputs are filled with the best estimates).  QC_ERR_INVALID: a null io, a bad
 * method, kind or nroots, a negative or NaN tol, a negative max_iterations, a state before its first qc_scf_iterate, dim = 0 - all checked
 * before the device is touched.  QC_ERR_UNSUPPORTED: a UHF state, a sharded handle or one with a communicator, too little free memory.
 * Bitwise reproducible from call to call and across fresh handles.  The state is left exactly as it was (no Fock build runs). */
typedef struct {
    int32_t method, kind, nroots, max_iterations;
    double tol;
    double energies[8], residuals[8];
    double oscillator[8], transition_dipole[24];
    int32_t nconverged, iterations, products, reference_unstable;
    double ms_total, ms_tensor, ms_transform, ms_solve;
} qc_excitations;
int qc_scf_excitations(qc_scf_state *st, qc_excitations *io, double *vectors /* nullable, host */);
/* The two matrices themselves, dim x dim doubles each on the host, either pointer nullable: for small systems and for tests.  Errors as
 * qc_scf_excitations (kind 0 or 1). */
int qc_scf_excitation_matrices(qc_scf_state *st, int kind, double *ApB, double *AmB);

/* ---- closed-shell coupled cluster with singles and doubles (CCSD) of an RHF state (after SCF, not in the reference), at the state's last C
 * and orbital energies as qc_scf_mp2.  The canonical-orbital formula is used: the occupied-virtual block of the Fock matrix and the
 * off-diagonal elements of its diagonal blocks are taken as zero, which they are at convergence (as for qc_scf_stability); on a state that
 * is not converged the result is the CCSD of that approximation.  Spin-adapted amplitudes t1[i, a] and t2[i, j, a, b] with
 * t_ij^ab = t_ji^ba over o = nocc - n_frozen active occupied and v virtual orbitals;
 *   E = sum_ijab (2 (ia|jb) - (ib|ja)) (t_ij^ab + t_i^a t_j^b).
 * The AO tensor is built in HBM (as qc_scf_mp2) and transformed to the blocks (ij|kl), (ia|jk), (ij|ab), (ia|jb), (ia|bc), (ab|cd); the
 * call needs about 8 max(n^4 + (o + v) n^3, 2 v^4 + ...) bytes of free HBM, QC_ERR_UNSUPPORTED when the device cannot hold them.  Nothing is
 * cached between calls.  The iteration starts from t1 = 0, t2 = (ia|jb) / D, updates by the denominators and extrapolates by DIIS over
 * the vectors [t1 | t2] with the error t_new - t_old.
 * In:  n_frozen (lowest orbitals left out), max_iterations (0: 100), diis_size (0: 8; 1: no extrapolation; at most 12), tol: the largest
 *      |t_new - t_old| over T1 and T2 at which the iteration stops (0: 1e-8).
 * Out: e_mp2 (from the first T2) and e_ccsd, correlation energies in Eh; t1_diagnostic = sqrt(sum t1^2 / o), the largest |t1| and |t2|,
 *      the last max |t_new - t_old|; iterations, converged; wall times of the call, the AO tensor, the transformation and the iteration (ms).
 * t1 (o x v) and t2 (o^2 x v^2), nullable, host: the last amplitudes.
 * QC_NOT_CONVERGED when the iterations run out (the outputs are filled).  QC_ERR_INVALID, checked before the device is touched: a null st
 * or io, a state before its first qc_scf_iterate, n_frozen < 0 or >= nocc, no virtual orbital, a negative or NaN tol, a negative
 * max_iterations, diis_size < 0 or > 12.  QC_ERR_UNSUPPORTED: a UHF state, a solvated state, a sharded handle or one with a communicator, too
 * little free memory.  Bitwise reproducible from call to call and across fresh handles (no atomics, fixed-order reductions, a split-k
 * GEMM whose slice count depends on the shape alone).  The state is left exactly as it was (no Fock build runs). */
typedef struct {
    int32_t n_frozen, max_iterations, diis_size, reserved0;
    double tol;
    double e_mp2, e_ccsd;
    double t1_diagnostic, t1_max, t2_max, residual;
    int32_t iterations, converged, reserved1[2];
    double ms_total, ms_tensor, ms_transform, ms_solve;
} qc_ccsd;
int qc_scf_ccsd(qc_scf_state *st, qc_ccsd *io, double *t1 /* nullable, host, o_act x v */, double *t2 /* nullable, host, o_act^2 x v^2 */);
/* For tests and timing: C = alpha A B + beta C of dense row-major host matrices (m x k, k x n, m x n) on the GPU, which 0 through the
 * one-wave-per-tile GEMM, 1 through the split-k GEMM of the CCSD ladder.  reps > 1 repeats the product on the same device buffers; ms
 * (nullable, max(reps, 1) doubles) takes the device time of each.  QC_ERR_INVALID: a bad which, m, n, k < 1, null pointers, reps < 0. */
int qc_debug_gemm(int which, int m, int n, int k, double alpha, const double *A, const double *B, double beta, double *C, int reps, double *ms);

/* qc_scf_begin_rhf / qc_scf_begin_uhf with the caller's densities (host, n*n, in the convention of qc_scf_density: the RHF density carries
 * the factor 2) in place of the Hueckel guess: DIIS windows empty, first eigensolve cold.  Null densities are QC_ERR_INVALID (checked
 * before the device is touched). */
int qc_scf_begin_rhf_from(qc_system *sys, const double *D, qc_scf_state **out);
int qc_scf_begin_uhf_from(qc_system *sys, int n_alpha, int n_beta, const double *Da, const double *Db, qc_scf_state **out);

/* ---- Fock mode of the SCF drivers on this handle.  0 (default): direct - quartets are evaluated and digested every pass.
 * 1: stored - the reference's own conventional algorithm with the tensor resident in HBM: molint::eri once (rhf.rs:45),
 * electron_terms (rhf.rs:58-62), then one streaming GEMV per pass (rhf.rs:152-167 / uhf.rs:216-226).  Needs ~18 n^4 bytes
 * during set-up (QC_ERR_UNSUPPORTED if the device cannot hold them); single-GPU only. */
int qc_set_fock_mode(qc_system *sys, int mode);
double qc_scf_tensor_ms(qc_scf_state *st);   /* wall time of the tensor build of a stored-mode state */

/* ---- accumulation of the direct Fock build.  1 (default): every contribution to G is rounded once to a multiple of
 * 2^-S Eh and added as a 64-bit integer - the sum does not depend on the order the GPU serves the adds in, so a build is
 * reproducible bit for bit from run to run and under any stream assignment, and both spins of a UHF build see identical
 * arithmetic, as in the reference (uhf.rs:80-108, 210-227).  (Across DIFFERENT shard layouts - numbers of ranks - the sum of the
 * partial matrices agrees to ~1e-13, not bit for bit: the bra-major kernels first combine the exchange rows of a 64-ket bundle in
 * an f64 LDS buffer, and which kets share a bundle depends on the shard.  Non-finite densities give a NaN matrix, as f64 would.)  S follows the density of the build (a bound on |G| keeps every
 * sum inside 64 bits): 2^-49 Eh = 1.8e-15 for benzene/cc-pVDZ.  0: f64 atomics (last-bit noise from the accumulation
 * order; kept for A/B measurements). */
int qc_set_accumulation(qc_system *sys, int fixed_point);

/* ---- Schwarz screening (the reference's TODO at uhf.rs:49-50: "if we could skip some of them ...").  Once per geometry the
 * GPU evaluates the (ab|ab) quartet of every shell pair; unique quartets with sqrt((ab|ab) (cd|cd)) < tau are left out of
 * the work lists (|(ab|cd)| <= that product).  Default 1e-12; 0 switches it off.  Throughput figures keep counting the
 * enumerated quartets (qc_nquartets).  NOT screened: qc_eri_full, the stored-tensor mode (qc_set_fock_mode) and everything built on
 * the tensor (MP2, excitations) - they run over every class's whole quartet list, not over the screened shard. */
int qc_set_schwarz(qc_system *sys, double tau);
/* The factors of that pass (read-only; initialises the device side if needed): for every STORED shell pair - pairs A >= B whose every
 * primitive pair falls under the primitive cut-off are not stored and have no factor - the shell indices (A,B), 2 ints each, and
 * Q = sqrt(max_ab (ab|ab)); Q == NULL: returns the count only. */
int qc_schwarz_factors(qc_system *sys, int32_t *shell_ab, double *Q, int64_t capacity);

/* ---- multi-GPU (not in the reference, which is single-threaded; BASELINE.json north_star).  One process per GPU.
 * Rank 0 calls qc_comm_unique_id, the host distributes the 128 bytes, every rank calls qc_comm_init, which creates
 * an RCCL communicator on the current device and restricts this handle's Fock builds to shard `rank` of `nranks`. */
/* RCCL is bound at run time (dlopen): $QC_RCCL_LIB, else the librccl.so.1 already mapped into the process (torch's bundled
 * copy in a torch process - one RCCL per process), else librccl.so.1 from the loader's search path (/opt/rocm/lib).
 * qc_rccl_info writes "<path> version <code>" of the copy in use. */
int qc_rccl_info(char *buf, size_t len);
int qc_comm_unique_id(uint8_t id[128]);
int qc_comm_init(qc_system *sys, const uint8_t id[128], int rank, int nranks);
/* Shard without a communicator (tests / external reduction): Fock builds then return the PARTIAL matrix. */
int qc_set_shard(qc_system *sys, int rank, int nranks);
/* Host-only view of the work plan: number of quartets and the cost-model flops assigned to a shard. */
int qc_plan_shard(qc_system *sys, int rank, int nranks, int64_t *nquartets, double *flops);
/* The shard's quartets as shell indices (A,B,C,D), 4 ints each; abcd == NULL: returns the count only. */
int qc_plan_shard_quartets(qc_system *sys, int rank, int nranks, int32_t *abcd, int64_t capacity);

/* ---- test hook (host only): one entry of a bra-major ket list - packed (pair | first primitive << 18 | length << 25; lists of systems
 * with fewer than 2^18 stored shell pairs) or a plain pair index - written and read back the way the library does. */
int qc_debug_ket_entry(int ket, int first_primitive, int length, int packed, int32_t out[3]);

/* ---- measurement hooks */
/* Dispatch lanes of this handle: the GPU dispatches at most four kernels at a time - hardware queues sit in pairs on four
 * pipes, and a pipe works on one grid until all its workgroups are launched - so the concurrent launches of a Fock build go to one stream
 * per pipe.  Which of the handle's streams share a pipe is measured when the handle initialises its device state.  nlanes: streams on
 * distinct pipes (4 on an MI355X with GPU_MAX_HW_QUEUES=8; 7 = not measured: QC_NO_LANES, or dispatches are serialised by a profiler);
 * slot_stream[0..6]: side stream behind assignment slot k (the first nlanes are the lanes), slot_stream[7]: 1 if slot 0 shares the pipe of
 * the handle's own stream (its chain then runs on that stream itself). */
int qc_dispatch_lanes(qc_system *sys, int32_t *nlanes, int32_t slot_stream[8]);
/* The assignment of a build's launches to the lanes is refined in instalments of extra builds inside later builds (paid for by use,
 * DESIGN.md 3.2).  A harness that is about to TIME builds ends that search here and now, with the best assignment found so far, so that
 * no instalment falls into its timed region.  Results never depend on the assignment. */
int qc_freeze_assignment(qc_system *sys);
int qc_set_stream(qc_system *sys, void *hip_stream);  /* run on the caller's stream (e.g. torch's current stream) */
int qc_device_ready(void);                             /* QC_OK if a gfx950 device is usable */
/* Algorithmic work of one Fock build on this handle's shard (SURVEY.md 8d model): */
typedef struct {
    int64_t quartets;          /* unique shell quartets enumerated */
    int64_t prim_quartets;     /* primitive quartets */
    double bytes_alg;          /* pair data + 6 D blocks read + 6 F blocks read/write, bytes */
    double flops_alg;          /* Boys + R table + Hermite contraction + digestion, flops */
    int32_t nclasses;          /* kernel launches per build */
    int64_t quartets_enumerated;   /* all unique quartets of the molecule (what the reference visits; all ranks) */
    int64_t quartets_screened_out; /* of those, dropped by the Schwarz bound (all ranks); 0 before the device pass has run */
    double schwarz_tau;            /* threshold in force (0: none) */
} qc_work_stats;
int qc_work_stats_get(qc_system *sys, qc_work_stats *out);
/* Time `reps` Fock builds (RHF digestion of dD) per kernel class with hipEvents on the handle's stream.
 * class_ms: caller buffer of `nclasses` floats (average ms per launch of each class bucket); class_id: (BM << 12) | (LAB << 8) |
 * (LCD << 4) | LGC: Hermite orders of the bra / ket pairs, log2 of the lane-group width, BM = 1 for the bra-major kernels. */
int qc_fock_profile(qc_system *sys, const double *dD, double *dG, int reps, float *class_ms, int32_t *class_id,
                    int64_t *class_quartets, double *class_bytes, double *class_flops, float *total_ms);

/* Same for the launch units of an un-instrumented build.  Units 0..13: kernel qc_fock_tier_kernel<LAB, TIER> gathers every
 * class bucket of bra class LAB with LCD <= 3 (TIER 0) or LCD >= 4 (TIER 1), unit = 2 * LAB + TIER.  Units 14..17: the
 * bra-major kernels qc_fock_bm_kernel<LCD, HI> (ket pair ss / ps, bra class LAB <= 2 / LAB >= 3), unit = 14 + 2 * LCD + HI; unit 18:
 * qc_fock_bm_kernel<2, 0>, p.p kets against p.p / d.s bras.
 * All arrays: QC_PROFILE_UNITS entries. */
#define QC_PROFILE_UNITS 20
/* Shell quartets of this rank's shard per launch unit (QC_PROFILE_UNITS entries; no device work). */
int qc_unit_quartets(qc_system *sys, int64_t *unit_quartets);
int qc_fock_profile_tiers(qc_system *sys, const double *dD, double *dG, int reps, float *unit_ms, int64_t *unit_quartets,
                          double *unit_bytes, double *unit_flops, float *total_ms);

/* Measured ceilings of the device the library runs on (bench.py quotes the roofline against them next to the datasheet peaks;
 * SURVEY.md App. F): a register-resident v_fma_f64 loop over the whole chip (TFLOP/s) and a 1 GiB -> 1 GiB streaming copy with
 * 16-byte accesses (GB/s, bytes read + bytes written).  Harness only: no reference counterpart. */
int qc_measure_peaks(double *fp64_tflops, double *hbm_copy_gbs);

#ifdef __cplusplus
}
#endif
#endif
