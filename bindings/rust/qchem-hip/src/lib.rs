//! Safe wrapper with the shape of qchem-rs's `core::hf` API (`core/src/hf/mod.rs:5-15`, `rhf.rs:11-35`,
//! `uhf.rs:12-39`): the same config struct, the same output structs, `Option` for "not converged", a panic for
//! "DIIS failed".  Input is a flattened description of the molecule and its segmented shells, because the reference's
//! `MolecularSystem` lives in the `molint` crate, which is not part of the reference tree; a `From<&MolecularSystem>`
//! for `FlatSystem` is the one piece a maintainer with `molint` at hand has to add.
//!
//! SOURCE ONLY - not compiled in the image this was written in (no Rust toolchain there).
pub mod ffi;

use std::ptr::null_mut;

/// `core::hf::HartreeFockConfig` (hf/mod.rs:9-15)
pub struct HartreeFockConfig { pub max_iterations: usize, pub epsilon: f64 }

/// rhf.rs:14-24
#[non_exhaustive]
pub struct RestrictedHartreeFockOutput { pub orbital_energies: Vec<f64>, pub electronic_energy: f64, pub nuclear_repulsion: f64, pub iterations: usize }
impl RestrictedHartreeFockOutput { pub fn total_energy(&self) -> f64 { self.electronic_energy + self.nuclear_repulsion } }

/// uhf.rs:15-27
#[non_exhaustive]
pub struct UnrestrictedHartreeFockOutput {
    pub orbital_energies_alpha: Vec<f64>, pub orbital_energies_beta: Vec<f64>,
    pub electronic_energy: f64, pub nuclear_repulsion: f64, pub iterations: usize,
}
impl UnrestrictedHartreeFockOutput { pub fn total_energy(&self) -> f64 { self.electronic_energy + self.nuclear_repulsion } }

/// What `qc_system_create` takes: atoms (Z, bohr), segmented shells (centre, L, pure flag, primitives).
pub struct FlatSystem {
    pub z: Vec<i32>, pub xyz: Vec<f64>,
    pub shell_atom: Vec<i32>, pub shell_l: Vec<i32>, pub shell_pure: Vec<i32>, pub shell_nprim: Vec<i32>,
    pub exponents: Vec<f64>, pub coefficients: Vec<f64>,
}

/// Owning handle: pair data, work lists and device buffers live behind it.  Not `Sync`: one handle, one thread.
pub struct GpuSystem { ptr: *mut ffi::QcSystem }
impl GpuSystem {
    pub fn new(s: &FlatSystem) -> Option<Self> {
        let mut ptr = null_mut();
        let rc = unsafe {
            ffi::qc_system_create(s.z.len() as i32, s.z.as_ptr(), s.xyz.as_ptr(), s.shell_l.len() as i32, s.shell_atom.as_ptr(),
                s.shell_l.as_ptr(), s.shell_pure.as_ptr(), s.shell_nprim.as_ptr(), s.exponents.as_ptr(), s.coefficients.as_ptr(), &mut ptr)
        };
        if rc == ffi::QC_OK { Some(GpuSystem { ptr }) } else { None }
    }
    pub fn n_basis(&self) -> usize { unsafe { ffi::qc_nbasis(self.ptr) as usize } }
    pub fn as_ptr(&self) -> *mut ffi::QcSystem { self.ptr }
}
impl Drop for GpuSystem { fn drop(&mut self) { unsafe { ffi::qc_system_destroy(self.ptr) } } }

fn config(c: &HartreeFockConfig) -> ffi::QcHfConfig {
    ffi::QcHfConfig { max_iterations: c.max_iterations, epsilon: c.epsilon, n_alpha: 0, n_beta: 0, reserved: [0; 6] }
}

/// `core::hf::restricted_hartree_fock` (rhf.rs:32-108) on the GPU.
pub fn restricted_hartree_fock(system: &FlatSystem, config_in: &HartreeFockConfig) -> Option<RestrictedHartreeFockOutput> {
    let h = GpuSystem::new(system)?;
    let mut eps = vec![0.0f64; h.n_basis()];
    let cfg = config(config_in);
    let mut out: ffi::QcHfOutput = unsafe { std::mem::zeroed() };
    out.orbital_energies = eps.as_mut_ptr();
    match unsafe { ffi::qc_scf_rhf(h.ptr, &cfg, &mut out) } {
        ffi::QC_OK => Some(RestrictedHartreeFockOutput { orbital_energies: eps, electronic_energy: out.electronic_energy,
                                                        nuclear_repulsion: out.nuclear_repulsion, iterations: out.iterations }),
        ffi::QC_NOT_CONVERGED => None,                       // rhf.rs:106-107
        ffi::QC_DIIS_SINGULAR => panic!("DIIS failed"),      // rhf.rs:73
        e => panic!("qchem_hip error {e}"),
    }
}

/// `core::hf::unrestricted_hartree_fock` (uhf.rs:36-167) on the GPU.
pub fn unrestricted_hartree_fock(system: &FlatSystem, config_in: &HartreeFockConfig) -> Option<UnrestrictedHartreeFockOutput> {
    let h = GpuSystem::new(system)?;
    let n = h.n_basis();
    let (mut ea, mut eb) = (vec![0.0f64; n], vec![0.0f64; n]);
    let cfg = config(config_in);
    let mut out: ffi::QcHfOutput = unsafe { std::mem::zeroed() };
    out.orbital_energies = ea.as_mut_ptr();
    out.orbital_energies_beta = eb.as_mut_ptr();
    match unsafe { ffi::qc_scf_uhf(h.ptr, &cfg, &mut out) } {
        ffi::QC_OK => Some(UnrestrictedHartreeFockOutput { orbital_energies_alpha: ea, orbital_energies_beta: eb,
                                                          electronic_energy: out.electronic_energy, nuclear_repulsion: out.nuclear_repulsion,
                                                          iterations: out.iterations }),
        ffi::QC_NOT_CONVERGED => None,                       // uhf.rs:165-166
        ffi::QC_DIIS_SINGULAR => panic!("DIIS failed"),      // uhf.rs:95-97
        e => panic!("qchem_hip error {e}"),
    }
}

/// The convergence loop owned by Rust (the north-star wording): one FFI call per pass of rhf.rs:66-104.
pub fn restricted_hartree_fock_stepwise(system: &FlatSystem, config: &HartreeFockConfig) -> Option<RestrictedHartreeFockOutput> {
    let h = GpuSystem::new(system)?;
    let mut st = null_mut();
    if unsafe { ffi::qc_scf_begin_rhf(h.ptr, &mut st) } != ffi::QC_OK { return None; }
    let mut result = None;
    for iteration in 0..=config.max_iterations {             // inclusive, rhf.rs:66
        let (mut e, mut rms) = (0.0f64, 0.0f64);
        match unsafe { ffi::qc_scf_iterate(st, &mut e, &mut rms) } {
            ffi::QC_OK => {}
            ffi::QC_DIIS_SINGULAR => { unsafe { ffi::qc_scf_end(st) }; panic!("DIIS failed") }
            ffi::QC_EIG_NOT_CONVERGED => { unsafe { ffi::qc_scf_end(st) }; panic!("eigensolve did not converge") }
            _ => break,
        }
        if rms < config.epsilon {                            // rhf.rs:94
            let mut eps = vec![0.0f64; h.n_basis()];
            unsafe { ffi::qc_scf_orbital_energies(st, 0, eps.as_mut_ptr()) };
            result = Some(RestrictedHartreeFockOutput { orbital_energies: eps, electronic_energy: e,
                                                        nuclear_repulsion: unsafe { ffi::qc_nuclear_repulsion(h.ptr) }, iterations: iteration });
            break;
        }
    }
    unsafe { ffi::qc_scf_end(st) };
    result
}

/// Lowest eigenvalue of the real orbital Hessian (A+B) of a state that has done at least one pass (`qc_scf_stability`): kind 0 = RHF
/// singlet / UHF internal, 1 = RHF -> UHF.  Negative: the determinant is a saddle of the HF functional.  None on any error or when the
/// Davidson iteration runs out.  The state is left as it was.
pub fn lowest_hessian_eigenvalue(st: *mut ffi::QcScfState, kind: i32) -> Option<f64> {
    let mut io = ffi::QcStability { kind, nroots: 1, max_iterations: 0, reserved0: 0, tol: 0.0, eigenvalues: [0.0; 8], residuals: [0.0; 8],
                                    nconverged: 0, iterations: 0, builds: 0, reserved1: 0, ms_total: 0.0, ms_builds: 0.0 };
    match unsafe { ffi::qc_scf_stability(st, &mut io, null_mut()) } {
        ffi::QC_OK => Some(io.eigenvalues[0]),
        _ => None,
    }
}

/// Dipole moment (e bohr, origin 0) of a state's density (`qc_scf_dipole`).  None on any error.  (Uncompiled, like the rest of this crate.)
pub fn dipole_moment(st: *mut ffi::QcScfState) -> Option<[f64; 3]> {
    let mut mu = [0.0f64; 3];
    match unsafe { ffi::qc_scf_dipole(st, std::ptr::null(), mu.as_mut_ptr(), null_mut()) } {
        ffi::QC_OK => Some(mu),
        _ => None,
    }
}

/// The lowest `nroots` (1..8) excitation energies (Eh) and oscillator strengths of a state that has done at least one pass
/// (`qc_scf_excitations`, default tolerance): `tdhf` false CIS, true TDHF; `triplets` false singlets, true triplets (oscillator strengths
/// then zero).  None on any error, when the roots do not converge, or when TDHF refuses an unstable reference.  The state is left as it was.
pub fn excited_states(st: *mut ffi::QcScfState, tdhf: bool, triplets: bool, nroots: usize) -> Option<(Vec<f64>, Vec<f64>)> {
    if nroots == 0 || nroots > 8 { return None; }
    let mut io = ffi::QcExcitations { method: tdhf as i32, kind: triplets as i32, nroots: nroots as i32, max_iterations: 0, tol: 0.0,
                                      energies: [0.0; 8], residuals: [0.0; 8], oscillator: [0.0; 8], transition_dipole: [0.0; 24],
                                      nconverged: 0, iterations: 0, products: 0, reference_unstable: 0, ms_total: 0.0, ms_tensor: 0.0,
                                      ms_transform: 0.0, ms_solve: 0.0 };
    match unsafe { ffi::qc_scf_excitations(st, &mut io, null_mut()) } {
        ffi::QC_OK => Some((io.energies[..nroots].to_vec(), io.oscillator[..nroots].to_vec())),
        _ => None,
    }
}

/// Put the molecule of a handle into a conductor-like continuum of dielectric constant `epsilon` (`qc_set_solvent`; C-PCM, or COSMO with
/// `cosmo`; default cavity: van der Waals radii times 1.2, 5 points per Angstrom^2).  SCF states begun afterwards are solvated; their total
/// energy is electronic + nuclear repulsion + `solvent_energy(st).nuclear`.  False on a bad epsilon.
pub fn set_solvent(system: &GpuSystem, epsilon: f64, cosmo: bool) -> bool {
    let cfg = ffi::QcSolvent { epsilon, x: if cosmo { 0.5 } else { 0.0 }, scale: 0.0, density: 0.0 };
    unsafe { ffi::qc_set_solvent(system.as_ptr(), &cfg, std::ptr::null()) == ffi::QC_OK }
}

/// 1/2 q.v_nuc, 1/2 q.v_elec, sum q and the number of surface elements for a solvated state's current density (`qc_scf_solvent`).
/// None for a state in vacuum.
pub fn solvent_energy(st: *mut ffi::QcScfState) -> Option<ffi::QcSolventEnergy> {
    let mut out = ffi::QcSolventEnergy { nuclear: 0.0, electronic: 0.0, total_charge: 0.0, npoints: 0 };
    match unsafe { ffi::qc_scf_solvent(st, &mut out, null_mut()) } {
        ffi::QC_OK => Some(out),
        _ => None,
    }
}

/// Static dipole polarizability (bohr^3, row-major 3 x 3, symmetrised) of a state that has done at least one pass
/// (`qc_scf_polarizability`, default tolerance).  None on any error or when the response equations do not converge.  The state is left
/// as it was.
pub fn static_polarizability(st: *mut ffi::QcScfState) -> Option<[f64; 9]> {
    let mut io = ffi::QcPolarizability { max_iterations: 0, reserved0: 0, tol: 0.0, alpha: [0.0; 9], residuals: [0.0; 3], asymmetry: 0.0,
                                         nconverged: 0, iterations: 0, builds: 0, reserved1: 0, ms_total: 0.0, ms_builds: 0.0 };
    match unsafe { ffi::qc_scf_polarizability(st, &mut io, null_mut()) } {
        ffi::QC_OK => Some(io.alpha),
        _ => None,
    }
}
