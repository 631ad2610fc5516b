//! Raw declarations of `include/qchem_hip.h` (the subset a `core::hf` replacement needs).
use std::os::raw::{c_double, c_int, c_void};

#[repr(C)]
pub struct QcSystem { _p: [u8; 0] }
#[repr(C)]
pub struct QcScfState { _p: [u8; 0] }

#[repr(C)]
pub struct QcHfConfig {
    pub max_iterations: usize,
    pub epsilon: f64,
    pub n_alpha: i32,
    pub n_beta: i32,
    pub reserved: [i32; 6],
}

#[repr(C)]
pub struct QcHfOutput {
    pub orbital_energies: *mut c_double,
    pub orbital_energies_beta: *mut c_double,
    pub electronic_energy: f64,
    pub nuclear_repulsion: f64,
    pub iterations: usize,
    pub ms_setup: f64,
    pub ms_fock_total: f64,
    pub ms_linalg_total: f64,
    pub ms_total: f64,
    pub ms_tuner: f64,
}

/// MP2 correlation energy (`qc_scf_mp2` / `qc_mp2`).
#[repr(C)]
pub struct QcMp2Output {
    pub e_os: f64,
    pub e_ss: f64,
    pub e_corr: f64,
    pub ms_tensor: f64,
    pub ms_transform: f64,
    pub ms_energy: f64,
    pub n_frozen: i32,
    pub reserved: [i32; 7],
}

/// In / out block of `qc_scf_stability`: set kind, nroots (1..8), tol (0: 1e-6), max_iterations (0: 100), zero the rest.
#[repr(C)]
pub struct QcStability {
    pub kind: i32,
    pub nroots: i32,
    pub max_iterations: i32,
    pub reserved0: i32,
    pub tol: f64,
    pub eigenvalues: [f64; 8],
    pub residuals: [f64; 8],
    pub nconverged: i32,
    pub iterations: i32,
    pub builds: i32,
    pub reserved1: i32,
    pub ms_total: f64,
    pub ms_builds: f64,
}

/// qc_polarizability (include/qchem_hip.h): in max_iterations (0: 100), tol (0: 1e-6); out alpha (row-major, symmetrised), residual
/// norms, the asymmetry before symmetrisation, counts and times.
#[repr(C)]
pub struct QcPolarizability {
    pub max_iterations: i32,
    pub reserved0: i32,
    pub tol: f64,
    pub alpha: [f64; 9],
    pub residuals: [f64; 3],
    pub asymmetry: f64,
    pub nconverged: i32,
    pub iterations: i32,
    pub builds: i32,
    pub reserved1: i32,
    pub ms_total: f64,
    pub ms_builds: f64,
}

/// qc_multipoles (include/qchem_hip.h): in order (0..4), origin; out the total, nuclear and electronic Cartesian moments of the
/// orders 0..order (components by order ascending, then x power descending, then y power descending; the rest zero) and the traceless
/// quadrupole xx xy xz yy yz zz of the total second moments.
/// Conductor-like continuum (C-PCM x = 0, COSMO x = 0.5); 0 in scale / density: the defaults 1.2 and 5 points per Angstrom^2.
#[repr(C)]
pub struct QcSolvent {
    pub epsilon: f64,
    pub x: f64,
    pub scale: f64,
    pub density: f64,
}

/// 1/2 q.v_nuc, 1/2 q.v_elec, sum q and the number of surface elements.
#[repr(C)]
pub struct QcSolventEnergy {
    pub nuclear: f64,
    pub electronic: f64,
    pub total_charge: f64,
    pub npoints: i64,
}

#[repr(C)]
pub struct QcMultipoles {
    pub order: i32,
    pub reserved: i32,
    pub origin: [f64; 3],
    pub total: [f64; 35],
    pub nuclear: [f64; 35],
    pub electronic: [f64; 35],
    pub quadrupole_traceless: [f64; 6],
}

/// qc_esp_fit (include/qchem_hip.h): in (0 = default) nscales and scales of the van der Waals radii (4: 1.4 1.6 1.8 2.0), density in
/// points per bohr^2 (1 per Angstrom^2); out the number of points, the constraint, rms and relative rms of the fit, the dipole of the
/// charges (origin 0), and times (ms).
#[repr(C)]
pub struct QcEspFit {
    pub nscales: i32,
    pub reserved0: i32,
    pub scales: [f64; 8],
    pub density: f64,
    pub npts: i64,
    pub total_charge: f64,
    pub rms: f64,
    pub rrms: f64,
    pub dipole: [f64; 3],
    pub ms_total: f64,
    pub ms_potential: f64,
}

/// qc_excitations (include/qchem_hip.h): in method (0 CIS, 1 TDHF), kind (0 singlets, 1 triplets), nroots (1..8), max_iterations
/// (0: 100), tol (0: 1e-6); out excitation energies (Eh, ascending), residual norms, oscillator strengths, transition dipoles
/// (x, y, z per state; both zero for triplets), counts, the flag of a reference TDHF refuses, and times.
#[repr(C)]
pub struct QcExcitations {
    pub method: i32,
    pub kind: i32,
    pub nroots: i32,
    pub max_iterations: i32,
    pub tol: f64,
    pub energies: [f64; 8],
    pub residuals: [f64; 8],
    pub oscillator: [f64; 8],
    pub transition_dipole: [f64; 24],
    pub nconverged: i32,
    pub iterations: i32,
    pub products: i32,
    pub reference_unstable: i32,
    pub ms_total: f64,
    pub ms_tensor: f64,
    pub ms_transform: f64,
    pub ms_solve: f64,
}

pub const QC_OK: c_int = 0;
pub const QC_NOT_CONVERGED: c_int = 1;
pub const QC_DIIS_SINGULAR: c_int = 2;
pub const QC_EIG_NOT_CONVERGED: c_int = 3;   // the Jacobi sweeps of an eigensolve ran out: an error, not the reference's `None`

extern "C" {
    pub fn qc_system_create(natoms: c_int, z: *const i32, xyz: *const f64, nshells: c_int, shell_atom: *const i32,
        shell_l: *const i32, shell_pure: *const i32, shell_nprim: *const i32, exponents: *const f64,
        coefficients: *const f64, out: *mut *mut QcSystem) -> c_int;
    pub fn qc_system_destroy(sys: *mut QcSystem);
    pub fn qc_nbasis(sys: *const QcSystem) -> c_int;
    pub fn qc_nuclear_repulsion(sys: *const QcSystem) -> f64;
    pub fn qc_overlap(sys: *const QcSystem, out: *mut f64) -> c_int;
    pub fn qc_kinetic(sys: *const QcSystem, out: *mut f64) -> c_int;
    pub fn qc_nuclear(sys: *const QcSystem, out: *mut f64) -> c_int;
    pub fn qc_one_electron_gpu(sys: *mut QcSystem, which: c_int, out: *mut f64) -> c_int;
    pub fn qc_eri_full(sys: *mut QcSystem, out: *mut f64) -> c_int;
    pub fn qc_fock_rhf(sys: *mut QcSystem, d: *const f64, g: *mut f64) -> c_int;
    pub fn qc_fock_uhf(sys: *mut QcSystem, da: *const f64, db: *const f64, ga: *mut f64, gb: *mut f64) -> c_int;
    pub fn qc_sym_eig(sys: *mut QcSystem, n: c_int, a: *const f64, v: *mut f64, w: *mut f64) -> c_int;
    pub fn qc_scf_rhf(sys: *mut QcSystem, cfg: *const QcHfConfig, out: *mut QcHfOutput) -> c_int;
    pub fn qc_scf_uhf(sys: *mut QcSystem, cfg: *const QcHfConfig, out: *mut QcHfOutput) -> c_int;
    pub fn qc_scf_begin_rhf(sys: *mut QcSystem, out: *mut *mut QcScfState) -> c_int;
    pub fn qc_scf_begin_uhf(sys: *mut QcSystem, n_alpha: c_int, n_beta: c_int, out: *mut *mut QcScfState) -> c_int;
    pub fn qc_scf_iterate(st: *mut QcScfState, electronic_energy: *mut f64, density_rms: *mut f64) -> c_int;
    pub fn qc_scf_orbital_energies(st: *mut QcScfState, spin: c_int, out: *mut f64) -> c_int;
    pub fn qc_scf_density(st: *mut QcScfState, spin: c_int, out: *mut f64) -> c_int;
    pub fn qc_scf_spin_square(st: *mut QcScfState, s2: *mut f64) -> c_int;
    pub fn qc_freeze_assignment(sys: *mut QcSystem) -> c_int;
    pub fn qc_dispatch_lanes(sys: *mut QcSystem, nlanes: *mut i32, slot_stream: *mut i32) -> c_int;
    pub fn qc_scf_set_stop_rule(st: *mut QcScfState, epsilon: f64) -> c_int;
    pub fn qc_scf_counters(st: *mut QcScfState, out: *mut f64, n: c_int) -> c_int;
    pub fn qc_scf_end(st: *mut QcScfState);
    /// MO coefficients of the last Roothaan step, row-major n x n: out[i*n+k] = component i of MO k (ascending energies).
    pub fn qc_scf_coefficients(st: *mut QcScfState, spin: c_int, out: *mut f64) -> c_int;
    /// MP2 from the state's last orbitals; the state is left as it was.
    pub fn qc_scf_mp2(st: *mut QcScfState, n_frozen: i32, out: *mut QcMp2Output) -> c_int;
    /// MP2 from caller orbitals: nspin 1 (C n*n, eps n, nocc[0]) or 2 (C 2*n*n, eps 2*n, nocc = [n_alpha, n_beta]).
    pub fn qc_mp2(sys: *mut QcSystem, nspin: c_int, c: *const f64, eps: *const f64, nocc: *const i32, n_frozen: i32,
                  out: *mut QcMp2Output) -> c_int;
    /// Nuclear gradient terms for fixed densities: terms = 4 x natoms x 3 (nuclear repulsion, core Hamiltonian, overlap,
    /// two-electron), Eh/bohr.  nspin 1: D n*n (qc_fock_rhf convention); nspin 2: D = [Da; Db].  W: energy-weighted density n*n.
    pub fn qc_gradient(sys: *mut QcSystem, nspin: c_int, d: *const f64, w: *const f64, terms: *mut f64) -> c_int;
    /// Total gradient (natoms x 3) at the state's last Roothaan step; the state is left as it was.
    pub fn qc_scf_gradient(st: *mut QcScfState, grad: *mut f64) -> c_int;
    /// Phase times (ms) of the handle's last gradient: transform, one-electron, two-electron, sum.
    pub fn qc_gradient_timings(sys: *const QcSystem, ms: *mut f64) -> c_int;
    /// Length of a stability vector: RHF o*v (kinds 0 singlet, 1 triplet); UHF o_a*v_a + o_b*v_b (kind 0), alpha block first, x[i*v + a].
    pub fn qc_scf_stability_dim(st: *mut QcScfState, kind: c_int) -> c_int;
    /// Lowest eigenpairs of the orbital Hessian (A+B) at the state's last orbitals; vectors: null or nroots x dim.  The state is left as it was.
    pub fn qc_scf_stability(st: *mut QcScfState, io: *mut QcStability, vectors: *mut f64) -> c_int;
    /// Densities (n*n per spin) and electronic energy of the determinant rotated along x; angle <= 0: the library's ladder of angles.
    pub fn qc_scf_rotated_density(st: *mut QcScfState, kind: c_int, x: *const f64, angle: f64, da: *mut f64, db: *mut f64,
                                  energy: *mut f64) -> c_int;
    /// qc_scf_begin_rhf / qc_scf_begin_uhf from the caller's densities (the convention of qc_scf_density) instead of the Hueckel guess.
    pub fn qc_scf_begin_rhf_from(sys: *mut QcSystem, d: *const f64, out: *mut *mut QcScfState) -> c_int;
    pub fn qc_scf_begin_uhf_from(sys: *mut QcSystem, n_alpha: c_int, n_beta: c_int, da: *const f64, db: *const f64,
                                 out: *mut *mut QcScfState) -> c_int;
    /// Dipole matrices <a|(r - origin)_k|b>, k = x, y, z: 3*n*n doubles; origin: three doubles or null (0, 0, 0).  Host only.
    pub fn qc_dipole_matrices(sys: *const QcSystem, origin: *const f64, out: *mut f64) -> c_int;
    /// The same from the GPU kernel the SCF properties use.
    pub fn qc_dipole_matrices_gpu(sys: *mut QcSystem, origin: *const f64, out: *mut f64) -> c_int;
    /// Dipole moment (e bohr) of the state's density: mu[3]; mu_nuclear[3] (nullable): the nuclear part.  The state is left as it was.
    pub fn qc_scf_dipole(st: *mut QcScfState, origin: *const f64, mu: *mut f64, mu_nuclear: *mut f64) -> c_int;
    /// Static dipole polarizability (bohr^3) by coupled-perturbed HF at the state's last orbitals; response: null or 3 x
    /// qc_scf_stability_dim(st, 0) doubles.  The state is left as it was.
    pub fn qc_scf_polarizability(st: *mut QcScfState, io: *mut QcPolarizability, response: *mut f64) -> c_int;
    /// CIS / TDHF excited states of an RHF state from explicit A + B and A - B matrices; vectors: null, or nroots x dim (CIS) /
    /// 2 x nroots x dim (TDHF: all R = X + Y, then all L = X - Y) doubles, dim = qc_scf_stability_dim(st, 0).  The state is left as it was.
    pub fn qc_scf_excitations(st: *mut QcScfState, io: *mut QcExcitations, vectors: *mut f64) -> c_int;
    /// A + B and A - B of kind 0 (singlets) or 1 (triplets), dim x dim doubles each, either pointer null.
    pub fn qc_scf_excitation_matrices(st: *mut QcScfState, kind: c_int, apb: *mut f64, amb: *mut f64) -> c_int;
    /// Basis functions on points (npts x 3 doubles, bohr): out npts x n, row = point.  Host only.
    pub fn qc_basis_on_points(sys: *const QcSystem, npts: i64, xyz: *const f64, out: *mut f64) -> c_int;
    /// A_ab = (a| 1/|r' - r| |b) for one point r (three doubles): n*n doubles, positive, exactly symmetric.  Host only.
    pub fn qc_potential_matrix(sys: *const QcSystem, r: *const f64, out: *mut f64) -> c_int;
    /// Stored primitive pairs of each pair order L = 0..6 (seven counts): the records the potential kernels walk per point.
    pub fn qc_esp_records(sys: *const QcSystem, counts: *mut i64) -> c_int;
    /// rho(r) = sum_ab D_ab phi_a(r) phi_b(r) on npts points, D n*n on the host.  GPU, batched over the points, bitwise reproducible.
    pub fn qc_density_on_points(sys: *mut QcSystem, d: *const f64, npts: i64, xyz: *const f64, rho: *mut f64) -> c_int;
    /// v_elec(r) = -sum_ab D_ab (a| 1/|r' - r| |b); v_nuc (nullable) = sum_A Z_A / |r - R_A|, +inf on a nucleus.
    pub fn qc_esp_on_points(sys: *mut QcSystem, d: *const f64, npts: i64, xyz: *const f64, v_elec: *mut f64, v_nuc: *mut f64) -> c_int;
    /// psi_k(r) for the m columns of C (n x m, leading dimension m): out m x npts.
    pub fn qc_orbitals_on_points(sys: *mut QcSystem, m: c_int, c: *const f64, npts: i64, xyz: *const f64, out: *mut f64) -> c_int;
    /// The same from a state's device-resident densities and orbitals; the state is left as it was.  which 0: P_alpha + P_beta, 1: P_alpha - P_beta.
    pub fn qc_scf_density_on_points(st: *mut QcScfState, which: c_int, npts: i64, xyz: *const f64, rho: *mut f64) -> c_int;
    /// v_total = v_nuc + v_elec of the state's total density; v_elec nullable.
    pub fn qc_scf_esp_on_points(st: *mut QcScfState, npts: i64, xyz: *const f64, v_total: *mut f64, v_elec: *mut f64) -> c_int;
    /// Orbitals first .. first + count - 1 of `spin` (order of qc_scf_orbital_energies): out count x npts.
    pub fn qc_scf_orbitals_on_points(st: *mut QcScfState, spin: c_int, first: c_int, count: c_int, npts: i64, xyz: *const f64,
                                     out: *mut f64) -> c_int;
    /// Phase times (ms) of the handle's last point call: upload, basis values / Hermite densities, contraction, download.
    pub fn qc_points_timings(sys: *const QcSystem, ms: *mut f64) -> c_int;
    /// Number of Cartesian components of the orders 0..order: 1, 4, 10, 20, 35; -1 outside 0..4.
    pub fn qc_multipole_count(order: c_int) -> c_int;
    /// Multipole matrices <a| (x-Ox)^i (y-Oy)^j (z-Oz)^k |b>: qc_multipole_count(order) x n*n doubles, each exactly symmetric; origin
    /// null = 0.  Host only.
    pub fn qc_multipole_matrices(sys: *const QcSystem, order: c_int, origin: *const f64, out: *mut f64) -> c_int;
    /// The same from the GPU kernel qc_scf_multipoles uses.
    pub fn qc_multipole_matrices_gpu(sys: *mut QcSystem, order: c_int, origin: *const f64, out: *mut f64) -> c_int;
    /// Total Cartesian moments of the state's density up to io.order about io.origin.  The state is left as it was.
    pub fn qc_scf_multipoles(st: *mut QcScfState, io: *mut QcMultipoles) -> c_int;
    /// scheme 0 Mulliken (Mayer bond orders), 1 Loewdin (Wiberg indices).  charges: natoms; spin, orbital (n), bond_orders
    /// (natoms x natoms) nullable.  The state is left as it was.
    pub fn qc_scf_populations(st: *mut QcScfState, scheme: c_int, charges: *mut f64, spin: *mut f64, orbital: *mut f64,
                              bond_orders: *mut f64) -> c_int;
    /// The same from host densities: nspin 1 (D n*n, the factor 2 included) or 2 ([Da; Db]).
    pub fn qc_populations(sys: *mut QcSystem, scheme: c_int, nspin: c_int, d: *const f64, charges: *mut f64, spin: *mut f64,
                          orbital: *mut f64, bond_orders: *mut f64) -> c_int;
    /// The Merz-Kollman grid: capacity points of three doubles; capacity < *npts is QC_ERR_INVALID with *npts filled.  Host only.
    pub fn qc_esp_fit_points(sys: *const QcSystem, cfg: *const QcEspFit, capacity: i64, xyz: *mut f64, npts: *mut i64) -> c_int;
    /// Charges fitted to the potential v on the points, sum = total_charge; fills io's outputs.  Host only.
    pub fn qc_esp_fit_solve(sys: *const QcSystem, npts: i64, xyz: *const f64, v: *const f64, total_charge: f64, io: *mut QcEspFit,
                            charges: *mut f64) -> c_int;
    /// Charges fitted to the state's potential on the library's grid (xyz null) or the caller's points; v_out nullable.
    pub fn qc_scf_esp_charges(st: *mut QcScfState, io: *mut QcEspFit, npts: i64, xyz: *const f64, charges: *mut f64,
                              v_out: *mut f64) -> c_int;
    /// External point charges of the handle: npc points (npc x 3 doubles, bohr) with npc charges, copied; npc == 0 removes the set.
    /// Host only.  SCF states begun afterwards are embedded (H = T + V + V_pc); states that are alive keep their set.
    pub fn qc_set_point_charges(sys: *mut QcSystem, npc: i64, xyz: *const f64, q: *const f64) -> c_int;
    pub fn qc_point_charge_count(sys: *const QcSystem) -> i64;
    /// E_nq = sum_A sum_c Z_A q_c / |R_A - R_c| of the handle's set (host).
    pub fn qc_point_charge_nuclear_energy(sys: *const QcSystem) -> f64;
    /// Count and E_nq of the set the state began with.
    pub fn qc_scf_point_charge_count(st: *const QcScfState) -> i64;
    pub fn qc_scf_point_charge_nuclear_energy(st: *const QcScfState) -> f64;
    /// V_pc = -sum_c q_c A(R_c), n*n doubles, exactly symmetric: on the host, and by the kernels the SCF set-up uses.
    pub fn qc_point_charge_matrix(sys: *const QcSystem, out: *mut f64) -> c_int;
    pub fn qc_point_charge_matrix_gpu(sys: *mut QcSystem, out: *mut f64) -> c_int;
    /// B^k_ab = dA_ab(r)/dr_k, k = x, y, z: 3 n*n doubles.  Host only.
    pub fn qc_field_matrix(sys: *const QcSystem, r: *const f64, out: *mut f64) -> c_int;
    /// E = -grad V of the molecule alone on npts points, npts x 3 doubles each; e_nuc nullable.
    pub fn qc_field_on_points(sys: *mut QcSystem, d: *const f64, npts: i64, xyz: *const f64, e_elec: *mut f64, e_nuc: *mut f64) -> c_int;
    /// The same from the state's total density: e_total = e_nuc + e_elec; e_elec nullable.  The state is left as it was.
    pub fn qc_scf_field_on_points(st: *mut QcScfState, npts: i64, xyz: *const f64, e_total: *mut f64, e_elec: *mut f64) -> c_int;
    /// terms: 2 x npc x 3 doubles, dE_nq/dR_c then d tr(P_t V_pc)/dR_c at a fixed density (conventions of qc_gradient).
    pub fn qc_point_charge_gradient(sys: *mut QcSystem, nspin: c_int, d: *const f64, terms: *mut f64) -> c_int;
    /// grad: npc x 3 doubles, dE/dR_c = -q_c E_total(R_c) at the state, for the charges it began with.
    pub fn qc_scf_point_charge_gradient(st: *mut QcScfState, grad: *mut f64) -> c_int;
    /// Phase times (ms) of the handle's last embedding call: upload, Hermite sums over the charges, assembly or contraction, download.
    pub fn qc_point_charge_timings(sys: *const QcSystem, ms: *mut f64) -> c_int;
    /// Ainv = A^-1 of a symmetric positive-definite n x n matrix (host pointers) by the device Cholesky factorisation, exactly symmetric;
    /// QC_ERR_INVALID when a pivot is <= 0 or not finite.
    pub fn qc_spd_inverse(sys: *mut QcSystem, n: c_int, a: *const f64, ainv: *mut f64) -> c_int;
    /// Conductor-like continuum of the handle: cfg null removes it; radii (nullable): natoms doubles, bohr, before scaling.  Host only.
    /// SCF states begun afterwards are solvated; states that are alive keep theirs.
    pub fn qc_set_solvent(sys: *mut QcSystem, cfg: *const QcSolvent, radii: *const f64) -> c_int;
    /// Returns M; with capacity >= M also writes xyz (M x 3), area (M) and the owning atoms (M), each nullable.  Host only.
    pub fn qc_solvent_surface(sys: *const QcSystem, capacity: i64, xyz: *mut f64, area: *mut f64, atom: *mut i32) -> i64;
    /// S of the cavity, M x M: the host statement, and S and K = -f S^-1 by the device kernels (either nullable).
    pub fn qc_solvent_matrix(sys: *const QcSystem, s: *mut f64) -> c_int;
    pub fn qc_solvent_matrix_gpu(sys: *mut QcSystem, s: *mut f64, k: *mut f64) -> c_int;
    /// At the total density d (n*n): the charges q (M, nullable), V_R (n*n, nullable) and energy = {1/2 q.v_nuc, 1/2 q.v_elec}.
    pub fn qc_solvent_response(sys: *mut QcSystem, d: *const f64, q: *mut f64, v: *mut f64, energy: *mut f64) -> c_int;
    /// The reaction field of the state's current density; q (nullable): M doubles.
    pub fn qc_scf_solvent(st: *mut QcScfState, out: *mut QcSolventEnergy, q: *mut f64) -> c_int;
    /// The same at the end of the last one-shot run on the handle.
    pub fn qc_solvent_last(sys: *const QcSystem, out: *mut QcSolventEnergy) -> c_int;
    /// ms: set-up (S, factorisation, inverse); of the last response: potential, reaction kernel, V_R.
    pub fn qc_solvent_timings(sys: *const QcSystem, ms: *mut f64) -> c_int;
    pub fn qc_set_fock_mode(sys: *mut QcSystem, mode: c_int) -> c_int;
    /// 1 (default): exact, order-independent accumulation of G; 0: f64 atomics.
    pub fn qc_set_accumulation(sys: *mut QcSystem, fixed_point: c_int) -> c_int;
    /// Schwarz threshold of the work lists (default 1e-12; 0 = every quartet, uhf.rs:49-50).
    pub fn qc_set_schwarz(sys: *mut QcSystem, tau: f64) -> c_int;
    /// 0 overlap, 1 core Hamiltonian, 2 X = S^-1/2 of a state (rhf.rs:41,48,124-131).
    pub fn qc_scf_matrix(st: *mut QcScfState, which: c_int, out: *mut f64) -> c_int;
    /// "<path> version <code>" of the RCCL copy bound at run time.
    pub fn qc_rccl_info(buf: *mut std::os::raw::c_char, len: usize) -> c_int;
    pub fn qc_comm_unique_id(id: *mut u8) -> c_int;
    pub fn qc_comm_init(sys: *mut QcSystem, id: *const u8, rank: c_int, nranks: c_int) -> c_int;
    pub fn qc_set_stream(sys: *mut QcSystem, hip_stream: *mut c_void) -> c_int;
}
