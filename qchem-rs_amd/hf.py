"""Host-side mirror of the reference's `core::hf` API over the C ABI of libqchem_hip.so (include/qchem_hip.h).

Names, argument meaning and error behaviour follow the reference so the parity tests read like its callers:
  HartreeFockConfig{max_iterations, epsilon}            core/src/hf/mod.rs:9-15
  restricted_hartree_fock(system, config) -> Option     core/src/hf/rhf.rs:32-35   (None = not converged, rhf.rs:107)
  unrestricted_hartree_fock(system, config) -> Option   core/src/hf/uhf.rs:36-39
  RestrictedHartreeFockOutput / UnrestrictedHartreeFockOutput incl. total_energy()   rhf.rs:14-30, uhf.rs:15-34
  overlap / kinetic / nuclear / eri                     the molint free functions called at rhf.rs:41-45
A singular DIIS system raises RuntimeError("DIIS failed") where the reference panics (rhf.rs:73, uhf.rs:95-97).

This module is ctypes plumbing only: no arithmetic of the hot path happens in Python, and there is no CPU fallback -
every compute call goes to the HIP library and raises if the library or a gfx950 device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .loader import MolecularSystem

# The Fock build launches its class kernels on several HIP streams.  The chip has four dispatch pipes; with ROCm's default of 4
# hardware queues, streams that land on one queue serialise completely, with 8 the library can pick one queue per pipe for its
# concurrent launches and keep the handle's own stream apart (the library measures which streams share a pipe).
# Must be set before the HIP runtime initialises, hence at import time.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QCHEM_HIP_LIB") or os.path.join(_HERE, "libqchem_hip.so")

QC_OK, QC_NOT_CONVERGED, QC_DIIS_SINGULAR, QC_EIG_NOT_CONVERGED = 0, 1, 2, 3
QC_ERR_INVALID, QC_ERR_NO_DEVICE, QC_ERR_HIP, QC_ERR_RCCL, QC_ERR_UNSUPPORTED = -1, -2, -3, -4, -5
_ERR = {-1: "invalid argument", -2: "no gfx950 device visible (there is no CPU fallback)", -3: "HIP runtime error",
        -4: "RCCL error", -5: "unsupported (angular momentum > f, or n too large for the in-LDS eigensolver)"}

EXPORTS = ["qc_system_create", "qc_system_destroy", "qc_nbasis", "qc_nelectrons", "qc_nshells", "qc_nquartets",
           "qc_nuclear_repulsion", "qc_overlap", "qc_kinetic", "qc_nuclear", "qc_one_electron_gpu", "qc_eri_full", "qc_fock_rhf", "qc_fock_uhf",
           "qc_fock_rhf_device", "qc_fock_uhf_device", "qc_sym_eig", "qc_scf_rhf", "qc_scf_uhf", "qc_comm_unique_id",
           "qc_comm_init", "qc_set_shard", "qc_plan_shard", "qc_set_stream", "qc_device_ready", "qc_work_stats_get",
           "qc_fock_profile", "qc_plan_shard_quartets", "qc_scf_begin_rhf", "qc_scf_begin_uhf", "qc_scf_iterate",
           "qc_scf_orbital_energies", "qc_scf_density", "qc_scf_spin_square", "qc_scf_timings", "qc_scf_end", "qc_fock_profile_tiers", "qc_unit_quartets", "qc_sym_eig_warm", "qc_set_fock_mode", "qc_scf_tensor_ms", "qc_set_accumulation", "qc_set_schwarz", "qc_scf_matrix", "qc_rccl_info", "qc_measure_peaks",
           "qc_scf_set_stop_rule", "qc_scf_counters", "qc_debug_ket_entry", "qc_dispatch_lanes", "qc_freeze_assignment",
           "qc_scf_coefficients", "qc_scf_mp2", "qc_mp2", "qc_gradient", "qc_scf_gradient", "qc_gradient_timings",
           "qc_scf_stability_dim", "qc_scf_stability", "qc_scf_rotated_density", "qc_scf_begin_rhf_from", "qc_scf_begin_uhf_from",
           "qc_dipole_matrices", "qc_dipole_matrices_gpu", "qc_scf_dipole", "qc_scf_polarizability",
           "qc_scf_excitations", "qc_scf_excitation_matrices", "qc_schwarz_factors", "qc_scf_ccsd", "qc_debug_gemm",
           "qc_basis_on_points", "qc_potential_matrix", "qc_esp_records", "qc_density_on_points", "qc_esp_on_points", "qc_orbitals_on_points",
           "qc_scf_density_on_points", "qc_scf_esp_on_points", "qc_scf_orbitals_on_points", "qc_points_timings",
           "qc_multipole_count", "qc_multipole_matrices", "qc_multipole_matrices_gpu", "qc_scf_multipoles",
           "qc_scf_populations", "qc_populations", "qc_esp_fit_points", "qc_esp_fit_solve", "qc_scf_esp_charges",
           "qc_set_point_charges", "qc_point_charge_count", "qc_point_charge_nuclear_energy", "qc_scf_point_charge_count",
           "qc_scf_point_charge_nuclear_energy", "qc_point_charge_matrix", "qc_point_charge_matrix_gpu", "qc_field_matrix",
           "qc_field_on_points", "qc_scf_field_on_points", "qc_point_charge_gradient", "qc_scf_point_charge_gradient",
           "qc_point_charge_timings",
           "qc_spd_inverse", "qc_set_solvent", "qc_solvent_surface", "qc_solvent_matrix", "qc_solvent_matrix_gpu", "qc_solvent_response",
           "qc_scf_solvent", "qc_solvent_last", "qc_solvent_timings"]

POPULATION_SCHEMES = {"mulliken": 0, "lowdin": 1}
BOHR_ANGSTROM = 0.529177210903   # QC_BOHR_ANGSTROM in include/qchem_hip.h


EXCITATION_METHODS = {"cis": 0, "tdhf": 1}


SOLVENT_MODELS = {"cpcm": 0.0, "cosmo": 0.5}     # x of f = (eps - 1) / (eps + x)


class QcError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("max_iterations", C.c_size_t), ("epsilon", C.c_double), ("n_alpha", C.c_int32), ("n_beta", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class _Output(C.Structure):
    _fields_ = [("orbital_energies", C.POINTER(C.c_double)), ("orbital_energies_beta", C.POINTER(C.c_double)),
                ("electronic_energy", C.c_double), ("nuclear_repulsion", C.c_double), ("iterations", C.c_size_t),
                ("ms_setup", C.c_double), ("ms_fock_total", C.c_double), ("ms_linalg_total", C.c_double),
                ("ms_total", C.c_double), ("ms_tuner", C.c_double)]


class _Mp2Output(C.Structure):
    _fields_ = [("e_os", C.c_double), ("e_ss", C.c_double), ("e_corr", C.c_double), ("ms_tensor", C.c_double),
                ("ms_transform", C.c_double), ("ms_energy", C.c_double), ("n_frozen", C.c_int32), ("reserved", C.c_int32 * 7)]


@dataclass
class Mp2Output:
    """qc_mp2_output: the MP2 correlation energy split by spin, and the wall time of its three phases (ms)."""
    e_os: float
    e_ss: float
    e_corr: float
    ms_tensor: float
    ms_transform: float
    ms_energy: float
    n_frozen: int

    @classmethod
    def _from(cls, o: "_Mp2Output") -> "Mp2Output":
        return cls(o.e_os, o.e_ss, o.e_corr, o.ms_tensor, o.ms_transform, o.ms_energy, int(o.n_frozen))


class _Stability(C.Structure):
    _fields_ = [("kind", C.c_int32), ("nroots", C.c_int32), ("max_iterations", C.c_int32), ("reserved0", C.c_int32), ("tol", C.c_double),
                ("eigenvalues", C.c_double * 8), ("residuals", C.c_double * 8), ("nconverged", C.c_int32), ("iterations", C.c_int32),
                ("builds", C.c_int32), ("reserved1", C.c_int32), ("ms_total", C.c_double), ("ms_builds", C.c_double)]


@dataclass
class StabilityOutput:
    """qc_stability: the lowest eigenvalues of the real orbital Hessian (A + B), ascending, with their residual norms; `vectors`
    (nroots, dim) when asked for.  converged: every root reached the tolerance."""
    kind: int
    eigenvalues: np.ndarray
    residuals: np.ndarray
    converged: bool
    iterations: int
    builds: int
    ms_total: float
    ms_builds: float
    vectors: Optional[np.ndarray] = None


class _Polarizability(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reserved0", C.c_int32), ("tol", C.c_double), ("alpha", C.c_double * 9),
                ("residuals", C.c_double * 3), ("asymmetry", C.c_double), ("nconverged", C.c_int32), ("iterations", C.c_int32),
                ("builds", C.c_int32), ("reserved1", C.c_int32), ("ms_total", C.c_double), ("ms_builds", C.c_double)]


@dataclass
class PolarizabilityOutput:
    """qc_polarizability: the static dipole polarizability (3, 3) in bohr^3, symmetrised; isotropic = trace / 3; residual norms of the three
    response equations; asymmetry: the largest |alpha_pq - alpha_qp| before the symmetrisation; `response` (3, dim) when asked for.
    converged: every equation reached the tolerance."""
    alpha: np.ndarray
    isotropic: float
    residuals: np.ndarray
    converged: bool
    iterations: int
    builds: int
    ms_total: float
    ms_builds: float
    asymmetry: float = 0.0
    response: Optional[np.ndarray] = None


class _Multipoles(C.Structure):
    _fields_ = [("order", C.c_int32), ("reserved", C.c_int32), ("origin", C.c_double * 3), ("total", C.c_double * 35),
                ("nuclear", C.c_double * 35), ("electronic", C.c_double * 35), ("quadrupole_traceless", C.c_double * 6)]


def multipole_components(order: int):
    """the exponents (i, j, k) of the Cartesian components up to `order`, in the library's order: by i + j + k ascending, then i
    descending, then j descending"""
    return [(i, j, l - i - j) for l in range(order + 1) for i in range(l, -1, -1) for j in range(l - i, -1, -1)]


@dataclass
class MultipolesOutput:
    """qc_multipoles: the total, nuclear and electronic Cartesian moments (count,) of the orders 0 .. order about `origin`, in e bohr^l,
    components as multipole_components(order); quadrupole_traceless (3, 3) = (3 Q_ab - delta_ab tr Q) / 2 of the total second moments
    (zero when order < 2)."""
    order: int
    origin: np.ndarray
    total: np.ndarray
    nuclear: np.ndarray
    electronic: np.ndarray
    quadrupole_traceless: np.ndarray

    def of_order(self, l: int) -> np.ndarray:
        """the total moments of order l alone"""
        lo = l * (l + 1) * (l + 2) // 6
        return self.total[lo:lo + (l + 1) * (l + 2) // 2]


@dataclass
class PopulationsOutput:
    """qc_scf_populations / qc_populations: charges (natoms,), spin populations N_A(alpha) - N_A(beta) (natoms,; exactly zero for a closed
    shell), gross populations per basis function (n,), and with bond_orders the Mayer (Mulliken) or Wiberg (Loewdin) matrix
    (natoms, natoms), diagonal as computed."""
    scheme: str
    charges: np.ndarray
    spin: np.ndarray
    orbital: np.ndarray
    bond_orders: Optional[np.ndarray] = None


class _EspFit(C.Structure):
    _fields_ = [("nscales", C.c_int32), ("reserved0", C.c_int32), ("scales", C.c_double * 8), ("density", C.c_double), ("npts", C.c_int64),
                ("total_charge", C.c_double), ("rms", C.c_double), ("rrms", C.c_double), ("dipole", C.c_double * 3),
                ("ms_total", C.c_double), ("ms_potential", C.c_double)]


def _esp_cfg(scales, density) -> "_EspFit":
    io = _EspFit()
    if scales is not None:
        sc = [float(x) for x in scales]
        if not 1 <= len(sc) <= 8:
            raise QcError("esp fit: 1 to 8 scales")
        io.nscales = len(sc)
        for k, x in enumerate(sc):
            io.scales[k] = x
    if density is not None:
        io.density = float(density)
    return io


@dataclass
class EspChargesOutput:
    """qc_esp_fit: charges (natoms,) fitted to the potential on `points` (npts, 3) with sum = total_charge; rms of V - V_fit and
    rrms = rms / rms(V); dipole = sum_A q_A R_A (origin 0); potential: the fitted V (npts,) when the call computed it."""
    charges: np.ndarray
    total_charge: float
    rms: float
    rrms: float
    dipole: np.ndarray
    points: np.ndarray
    potential: Optional[np.ndarray] = None
    ms_total: float = 0.0
    ms_potential: float = 0.0


class _Excitations(C.Structure):
    _fields_ = [("method", C.c_int32), ("kind", C.c_int32), ("nroots", C.c_int32), ("max_iterations", C.c_int32), ("tol", C.c_double),
                ("energies", C.c_double * 8), ("residuals", C.c_double * 8), ("oscillator", C.c_double * 8), ("transition_dipole", C.c_double * 24),
                ("nconverged", C.c_int32), ("iterations", C.c_int32), ("products", C.c_int32), ("reference_unstable", C.c_int32),
                ("ms_total", C.c_double), ("ms_tensor", C.c_double), ("ms_transform", C.c_double), ("ms_solve", C.c_double)]


@dataclass
class ExcitationsOutput:
    """qc_excitations: excitation energies (Eh, ascending) of the CIS or TDHF states of an RHF determinant with their residual norms,
    oscillator strengths and transition dipoles (nroots, 3) - both exactly zero for triplets; the sign of a vector and of its transition
    dipole is arbitrary.  converged: every root reached the tolerance.  reference_unstable: TDHF was refused because A + B or A - B is not
    positive definite (then converged is False and no state is returned).  vectors, when asked for: CIS (nroots, dim) with |X| = 1;
    TDHF (2, nroots, dim) - R = X + Y, then L = X - Y, with L_k . R_k = 1."""
    method: str
    kind: int
    energies: np.ndarray
    residuals: np.ndarray
    oscillator: np.ndarray
    transition_dipole: np.ndarray
    converged: bool
    reference_unstable: bool
    nconverged: int
    iterations: int
    products: int
    ms_total: float
    ms_tensor: float
    ms_transform: float
    ms_solve: float
    vectors: Optional[np.ndarray] = None


class _Ccsd(C.Structure):
    _fields_ = [("n_frozen", C.c_int32), ("max_iterations", C.c_int32), ("diis_size", C.c_int32), ("reserved0", C.c_int32), ("tol", C.c_double),
                ("e_mp2", C.c_double), ("e_ccsd", C.c_double), ("t1_diagnostic", C.c_double), ("t1_max", C.c_double), ("t2_max", C.c_double),
                ("residual", C.c_double), ("iterations", C.c_int32), ("converged", C.c_int32), ("reserved1", C.c_int32 * 2),
                ("ms_total", C.c_double), ("ms_tensor", C.c_double), ("ms_transform", C.c_double), ("ms_solve", C.c_double)]


@dataclass
class CcsdOutput:
    """qc_ccsd: the MP2 (from the first T2) and CCSD correlation energies (Eh) of an RHF determinant, the T1 diagnostic
    sqrt(sum t1^2 / o), the largest |t1| and |t2|, the last max |t_new - t_old|, and the wall times of the phases (ms).  t1 (o, v) and
    t2 (o, o, v, v) with t2[i, j, a, b] = t2[j, i, b, a], when asked for; o counts the active occupied orbitals."""
    e_mp2: float
    e_ccsd: float
    t1_diagnostic: float
    t1_max: float
    t2_max: float
    residual: float
    iterations: int
    converged: bool
    n_frozen: int
    ms_total: float
    ms_tensor: float
    ms_transform: float
    ms_solve: float
    t1: Optional[np.ndarray] = None
    t2: Optional[np.ndarray] = None


class _Solvent(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("x", C.c_double), ("scale", C.c_double), ("density", C.c_double)]


class _SolventEnergy(C.Structure):
    _fields_ = [("nuclear", C.c_double), ("electronic", C.c_double), ("total_charge", C.c_double), ("npoints", C.c_int64)]


@dataclass
class SolventOutput:
    """The reaction field of a density (qc_scf_solvent / qc_solvent_last): nuclear = 1/2 q.v_nuc, electronic = 1/2 q.v_elec (their sum is
    G_pol), total_charge = sum q, npoints = M; charges: q (M,) where the call returns them."""
    nuclear: float
    electronic: float
    total_charge: float
    npoints: int
    charges: Optional[np.ndarray] = None

    def polarization_energy(self) -> float:
        return self.nuclear + self.electronic

    @classmethod
    def _from(cls, o: "_SolventEnergy", q=None) -> "SolventOutput":
        return cls(o.nuclear, o.electronic, o.total_charge, int(o.npoints), q)


class WorkStats(C.Structure):
    _fields_ = [("quartets", C.c_int64), ("prim_quartets", C.c_int64), ("bytes_alg", C.c_double),
                ("flops_alg", C.c_double), ("nclasses", C.c_int32), ("quartets_enumerated", C.c_int64),
                ("quartets_screened_out", C.c_int64), ("schwarz_tau", C.c_double)]


_lib = None
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


def build_library(force: bool = False) -> str:
    """Compile libqchem_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", csrc, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", csrc])
    return LIB_PATH


def lib():
    """The loaded HIP library.  Raises if it has not been built - the product path never falls back to the CPU."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QcError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(qchem-rs_amd has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.qc_system_create.argtypes = [C.c_int, _ip, _dp, C.c_int, _ip, _ip, _ip, _ip, _dp, _dp, C.POINTER(vp)]
        L.qc_system_destroy.argtypes = [vp]; L.qc_system_destroy.restype = None
        for f in ("qc_nbasis", "qc_nelectrons", "qc_nshells"):
            getattr(L, f).argtypes = [vp]
        L.qc_nquartets.argtypes = [vp]; L.qc_nquartets.restype = C.c_int64
        L.qc_nuclear_repulsion.argtypes = [vp]; L.qc_nuclear_repulsion.restype = C.c_double
        for f in ("qc_overlap", "qc_kinetic", "qc_nuclear", "qc_eri_full"):
            getattr(L, f).argtypes = [vp, _dp]
        L.qc_one_electron_gpu.argtypes = [vp, C.c_int, _dp]
        L.qc_fock_rhf.argtypes = [vp, _dp, _dp]
        L.qc_fock_uhf.argtypes = [vp, _dp, _dp, _dp, _dp]
        L.qc_fock_rhf_device.argtypes = [vp, vp, vp]
        L.qc_fock_uhf_device.argtypes = [vp, vp, vp, vp, vp]
        L.qc_sym_eig.argtypes = [vp, C.c_int, _dp, _dp, _dp]
        L.qc_sym_eig_warm.argtypes = [vp, C.c_int, _dp, _dp, _dp, _dp]
        L.qc_scf_rhf.argtypes = [vp, C.POINTER(_Config), C.POINTER(_Output)]
        L.qc_scf_uhf.argtypes = [vp, C.POINTER(_Config), C.POINTER(_Output)]
        L.qc_comm_unique_id.argtypes = [C.c_char_p]
        L.qc_comm_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.qc_set_shard.argtypes = [vp, C.c_int, C.c_int]
        L.qc_plan_shard.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.qc_plan_shard_quartets.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64]
        L.qc_set_stream.argtypes = [vp, vp]
        L.qc_device_ready.argtypes = []
        L.qc_work_stats_get.argtypes = [vp, C.POINTER(WorkStats)]
        L.qc_fock_profile.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.qc_fock_profile_tiers.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        L.qc_unit_quartets.argtypes = [vp, vp]
        L.qc_set_fock_mode.argtypes = [vp, C.c_int]
        L.qc_set_accumulation.argtypes = [vp, C.c_int]
        L.qc_set_schwarz.argtypes = [vp, C.c_double]
        L.qc_schwarz_factors.argtypes = [vp, vp, vp, C.c_int64]
        L.qc_scf_tensor_ms.argtypes = [vp]; L.qc_scf_tensor_ms.restype = C.c_double
        L.qc_scf_begin_rhf.argtypes = [vp, C.POINTER(vp)]
        L.qc_scf_begin_uhf.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.qc_scf_iterate.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.qc_scf_orbital_energies.argtypes = [vp, C.c_int, _dp]
        L.qc_scf_density.argtypes = [vp, C.c_int, _dp]
        L.qc_scf_matrix.argtypes = [vp, C.c_int, _dp]
        L.qc_scf_spin_square.argtypes = [vp, C.POINTER(C.c_double)]
        L.qc_scf_timings.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.qc_scf_end.argtypes = [vp]; L.qc_scf_end.restype = None
        L.qc_scf_set_stop_rule.argtypes = [vp, C.c_double]
        L.qc_scf_counters.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
        L.qc_scf_coefficients.argtypes = [vp, C.c_int, _dp]
        L.qc_scf_mp2.argtypes = [vp, C.c_int32, C.POINTER(_Mp2Output)]
        L.qc_mp2.argtypes = [vp, C.c_int, _dp, _dp, _ip, C.c_int32, C.POINTER(_Mp2Output)]
        L.qc_gradient.argtypes = [vp, C.c_int, _dp, _dp, _dp]
        L.qc_scf_gradient.argtypes = [vp, _dp]
        L.qc_gradient_timings.argtypes = [vp, _dp]
        L.qc_scf_stability_dim.argtypes = [vp, C.c_int]
        L.qc_scf_stability.argtypes = [vp, C.POINTER(_Stability), vp]
        L.qc_scf_rotated_density.argtypes = [vp, C.c_int, vp, C.c_double, vp, vp, C.POINTER(C.c_double)]
        L.qc_scf_begin_rhf_from.argtypes = [vp, vp, C.POINTER(vp)]
        L.qc_scf_begin_uhf_from.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
        L.qc_dipole_matrices.argtypes = [vp, vp, vp]
        L.qc_dipole_matrices_gpu.argtypes = [vp, vp, vp]
        L.qc_scf_dipole.argtypes = [vp, vp, vp, vp]
        L.qc_scf_polarizability.argtypes = [vp, C.POINTER(_Polarizability), vp]
        L.qc_scf_excitations.argtypes = [vp, C.POINTER(_Excitations), vp]
        L.qc_scf_excitation_matrices.argtypes = [vp, C.c_int, vp, vp]
        L.qc_scf_ccsd.argtypes = [vp, C.POINTER(_Ccsd), vp, vp]
        L.qc_debug_gemm.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, C.c_double, vp, C.c_int, vp]
        L.qc_basis_on_points.argtypes = [vp, C.c_int64, vp, vp]
        L.qc_potential_matrix.argtypes = [vp, vp, vp]
        L.qc_esp_records.argtypes = [vp, vp]
        L.qc_density_on_points.argtypes = [vp, vp, C.c_int64, vp, vp]
        L.qc_esp_on_points.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.qc_orbitals_on_points.argtypes = [vp, C.c_int, vp, C.c_int64, vp, vp]
        L.qc_scf_density_on_points.argtypes = [vp, C.c_int, C.c_int64, vp, vp]
        L.qc_scf_esp_on_points.argtypes = [vp, C.c_int64, vp, vp, vp]
        L.qc_scf_orbitals_on_points.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int64, vp, vp]
        L.qc_points_timings.argtypes = [vp, vp]
        L.qc_multipole_count.argtypes = [C.c_int]
        L.qc_multipole_matrices.argtypes = [vp, C.c_int, vp, vp]
        L.qc_multipole_matrices_gpu.argtypes = [vp, C.c_int, vp, vp]
        L.qc_scf_multipoles.argtypes = [vp, C.POINTER(_Multipoles)]
        L.qc_scf_populations.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.qc_populations.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
        L.qc_esp_fit_points.argtypes = [vp, C.POINTER(_EspFit), C.c_int64, vp, C.POINTER(C.c_int64)]
        L.qc_esp_fit_solve.argtypes = [vp, C.c_int64, vp, vp, C.c_double, C.POINTER(_EspFit), vp]
        L.qc_scf_esp_charges.argtypes = [vp, C.POINTER(_EspFit), C.c_int64, vp, vp, vp]
        L.qc_set_point_charges.argtypes = [vp, C.c_int64, vp, vp]
        L.qc_point_charge_count.argtypes = [vp]; L.qc_point_charge_count.restype = C.c_int64
        L.qc_point_charge_nuclear_energy.argtypes = [vp]; L.qc_point_charge_nuclear_energy.restype = C.c_double
        L.qc_scf_point_charge_count.argtypes = [vp]; L.qc_scf_point_charge_count.restype = C.c_int64
        L.qc_scf_point_charge_nuclear_energy.argtypes = [vp]; L.qc_scf_point_charge_nuclear_energy.restype = C.c_double
        L.qc_point_charge_matrix.argtypes = [vp, vp]
        L.qc_point_charge_matrix_gpu.argtypes = [vp, vp]
        L.qc_field_matrix.argtypes = [vp, vp, vp]
        L.qc_field_on_points.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.qc_scf_field_on_points.argtypes = [vp, C.c_int64, vp, vp, vp]
        L.qc_point_charge_gradient.argtypes = [vp, C.c_int, vp, vp]
        L.qc_scf_point_charge_gradient.argtypes = [vp, vp]
        L.qc_point_charge_timings.argtypes = [vp, vp]
        L.qc_spd_inverse.argtypes = [vp, C.c_int, vp, vp]
        L.qc_set_solvent.argtypes = [vp, C.POINTER(_Solvent), vp]
        L.qc_solvent_surface.argtypes = [vp, C.c_int64, vp, vp, vp]; L.qc_solvent_surface.restype = C.c_int64
        L.qc_solvent_matrix.argtypes = [vp, vp]
        L.qc_solvent_matrix_gpu.argtypes = [vp, vp, vp]
        L.qc_solvent_response.argtypes = [vp, vp, vp, vp, vp]
        L.qc_scf_solvent.argtypes = [vp, C.POINTER(_SolventEnergy), vp]
        L.qc_solvent_last.argtypes = [vp, C.POINTER(_SolventEnergy)]
        L.qc_solvent_timings.argtypes = [vp, vp]
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc < 0:
        raise QcError(f"{what}: {_ERR.get(rc, rc)}")
    if rc == QC_EIG_NOT_CONVERGED:
        raise QcError(f"{what}: the Jacobi sweeps of an eigensolve ran out before convergence")
    return rc


def device_ready() -> bool:
    return lib().qc_device_ready() == QC_OK


class System:
    """Owning wrapper of a `qc_system` handle (the `&MolecularSystem` the reference drivers borrow)."""

    def __init__(self, mol: MolecularSystem):
        self.mol = mol
        self._h = C.c_void_p()
        _check(lib().qc_system_create(len(mol.atoms), mol.atomic_numbers(), mol.coordinates(), mol.n_shells, mol.shell_atom,
                                      mol.shell_L, mol.shell_pure, mol.shell_nprim, mol.exponents, mol.coefficients,
                                      C.byref(self._h)), "qc_system_create")
        self.n = lib().qc_nbasis(self._h)
        self.last_solvent = None     # SolventOutput of the last run of this module's drivers on the handle (None: in vacuum, or that run did not converge)

    def close(self):
        if self._h:
            lib().qc_system_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self): return self._h
    def n_basis(self) -> int: return self.n
    def n_electrons(self) -> int: return lib().qc_nelectrons(self._h)
    def n_quartets(self) -> int: return lib().qc_nquartets(self._h)
    def nuclear_repulsion(self) -> float: return lib().qc_nuclear_repulsion(self._h)

    def _mat(self, fn):
        M = np.zeros((self.n, self.n)); _check(getattr(lib(), fn)(self._h, M), fn); return M

    def overlap(self): return self._mat("qc_overlap")
    def kinetic(self): return self._mat("qc_kinetic")
    def nuclear(self): return self._mat("qc_nuclear")

    def one_electron_gpu(self, which: int):
        """S (0), T (1) or V (2) computed by the GPU kernels the SCF drivers use (qc_one_electron.hip)."""
        M = np.zeros((self.n, self.n))
        _check(lib().qc_one_electron_gpu(self._h, which, M.reshape(-1)), "qc_one_electron_gpu")
        return M

    def dipole_matrices(self, origin=None, gpu: bool = False):
        """(3, n, n): M_k = <a| (r - origin)_k |b>, k = x, y, z (origin None: 0) - qc_dipole_matrices on the host, or with gpu=True the
        kernel the SCF properties use (qc_dipole_matrices_gpu)."""
        M = np.zeros((3, self.n, self.n))
        fn = "qc_dipole_matrices_gpu" if gpu else "qc_dipole_matrices"
        _check(getattr(lib(), fn)(self._h, _origin_ptr(origin), M.ctypes.data_as(C.c_void_p)), fn)
        return M

    def multipole_matrices(self, order: int, origin=None, gpu: bool = False):
        """(count, n, n): the Cartesian multipole matrices <a| (x - O_x)^i (y - O_y)^j (z - O_z)^k |b> of the orders 0 .. order <= 4,
        components as multipole_components(order) - qc_multipole_matrices on the host, or with gpu=True the kernel the SCF moments use."""
        count = lib().qc_multipole_count(int(order))
        if count < 0:
            raise QcError("qc_multipole_matrices: " + _ERR[QC_ERR_INVALID])
        M = np.zeros((count, self.n, self.n))
        fn = "qc_multipole_matrices_gpu" if gpu else "qc_multipole_matrices"
        _check(getattr(lib(), fn)(self._h, int(order), _origin_ptr(origin), _ptr(M)), fn)
        return M

    def populations(self, D, scheme: str = "mulliken", Db=None, bond_orders: bool = False) -> "PopulationsOutput":
        """Population analysis of host densities on the GPU (qc_populations).  RHF: D in the qc_fock_rhf convention (the factor 2
        included); UHF: D = D_alpha, Db = D_beta.  scheme "mulliken" (Mayer bond orders) or "lowdin" (Wiberg indices)."""
        if scheme not in POPULATION_SCHEMES:
            raise QcError("populations: scheme must be 'mulliken' or 'lowdin'")
        n, na = self.n, len(self.mol.atoms)
        Dm = np.ascontiguousarray(D if Db is None else np.concatenate([np.asarray(D).reshape(n, n), np.asarray(Db).reshape(n, n)]), dtype=np.float64)
        if Dm.size != (1 if Db is None else 2) * n * n:
            raise QcError("qc_populations: densities must be n x n")
        q, sp, orb = np.zeros(na), np.zeros(na), np.zeros(n)
        bo = np.zeros((na, na)) if bond_orders else None
        _check(lib().qc_populations(self._h, POPULATION_SCHEMES[scheme], 1 if Db is None else 2, _ptr(Dm), _ptr(q), _ptr(sp), _ptr(orb),
                                    None if bo is None else _ptr(bo)), "qc_populations")
        return PopulationsOutput(scheme, q, sp, orb, bo)

    def esp_fit_points(self, scales=None, density=None):
        """(npts, 3): the Merz-Kollman grid of the molecule (qc_esp_fit_points, host only) - golden-spiral points on the van der Waals
        spheres scaled by `scales` (default 1.4 1.6 1.8 2.0) at `density` points per bohr^2 (default 1 per Angstrom^2), outside every
        other atom's scaled sphere."""
        cfg, k = _esp_cfg(scales, density), C.c_int64()
        rc = lib().qc_esp_fit_points(self._h, C.byref(cfg), 0, None, C.byref(k))
        if rc != QC_OK and k.value == 0:
            _check(rc, "qc_esp_fit_points")
        P = np.zeros((k.value, 3))
        _check(lib().qc_esp_fit_points(self._h, C.byref(cfg), k.value, _ptr(P), C.byref(k)), "qc_esp_fit_points")
        return P

    def esp_fit_solve(self, points, v, total_charge: float = 0.0) -> "EspChargesOutput":
        """Charges on the atoms that reproduce the potential v on `points` best in the least-squares sense, with sum = total_charge
        (qc_esp_fit_solve, host only)."""
        P, vv = _points(points), np.ascontiguousarray(v, np.float64).reshape(-1)
        if vv.size != len(P):
            raise QcError("qc_esp_fit_solve: one potential value per point")
        io, q = _EspFit(), np.zeros(len(self.mol.atoms))
        _check(lib().qc_esp_fit_solve(self._h, len(P), _ptr(P), _ptr(vv), float(total_charge), C.byref(io), _ptr(q)), "qc_esp_fit_solve")
        return EspChargesOutput(q, io.total_charge, io.rms, io.rrms, np.array(io.dipole), P)

    def basis_on_points(self, points):
        """(npts, n): the basis functions on points (bohr; anything that reshapes to (npts, 3)) - qc_basis_on_points, host only."""
        P = _points(points)
        out = np.zeros((len(P), self.n))
        _check(lib().qc_basis_on_points(self._h, len(P), _ptr(P), _ptr(out)), "qc_basis_on_points")
        return out

    def potential_matrix(self, r):
        """(n, n): A_ab = (a| 1/|r' - r| |b), the potential of a unit charge at r in the basis (qc_potential_matrix, host only)."""
        A = np.zeros((self.n, self.n))
        _check(lib().qc_potential_matrix(self._h, _origin_ptr(r), _ptr(A)), "qc_potential_matrix")
        return A

    def esp_records(self):
        """stored primitive pairs of each pair order L = 0..6: the records the potential kernels walk per point (qc_esp_records)"""
        c = np.zeros(7, np.int64)
        _check(lib().qc_esp_records(self._h, _ptr(c)), "qc_esp_records")
        return c

    def _density_arg(self, D, what):
        Dm = np.ascontiguousarray(D, np.float64)
        if Dm.size != self.n * self.n:
            raise QcError(what + ": D must be n x n")
        return Dm

    def density_on_points(self, D, points):
        """(npts,): rho(r) = sum_ab D_ab phi_a(r) phi_b(r) on the GPU (qc_density_on_points)."""
        Dm, P = self._density_arg(D, "qc_density_on_points"), _points(points)
        rho = np.zeros(len(P))
        _check(lib().qc_density_on_points(self._h, _ptr(Dm), len(P), _ptr(P), _ptr(rho)), "qc_density_on_points")
        return rho

    def esp_on_points(self, D, points, parts: bool = False):
        """(npts,): the electrostatic potential V = v_nuc + v_elec of the nuclei and the density D on the GPU (qc_esp_on_points);
        parts=True: (V, v_elec, v_nuc).  A point on a nucleus has v_nuc = V = +inf and a finite v_elec."""
        Dm, P = self._density_arg(D, "qc_esp_on_points"), _points(points)
        ve, vn = np.zeros(len(P)), np.zeros(len(P))
        _check(lib().qc_esp_on_points(self._h, _ptr(Dm), len(P), _ptr(P), _ptr(ve), _ptr(vn)), "qc_esp_on_points")
        return (vn + ve, ve, vn) if parts else vn + ve

    def orbitals_on_points(self, C_mo, points):
        """(m, npts): psi_k(r) = sum_a C_ak phi_a(r) for the m columns of C (n, m) on the GPU (qc_orbitals_on_points)."""
        Cm = np.ascontiguousarray(C_mo, np.float64)
        if Cm.ndim == 1:
            Cm = Cm.reshape(-1, 1)
        if Cm.ndim != 2 or Cm.shape[0] != self.n or Cm.shape[1] < 1:
            raise QcError("qc_orbitals_on_points: C must be n x m")
        P = _points(points)
        out = np.zeros((Cm.shape[1], len(P)))
        _check(lib().qc_orbitals_on_points(self._h, Cm.shape[1], _ptr(Cm), len(P), _ptr(P), _ptr(out)), "qc_orbitals_on_points")
        return out

    def points_timings(self):
        """Phase times (ms) of the handle's last point call: upload, basis values / Hermite densities, contraction, download."""
        ms = np.zeros(4); _check(lib().qc_points_timings(self._h, _ptr(ms)), "qc_points_timings"); return ms

    # ---- point-charge embedding (include/qchem_hip.h, "point-charge embedding")
    def set_point_charges(self, positions=None, charges=None):
        """The handle's external point charges: positions (npc, 3) in bohr, charges (npc,) - any finite values; None or empty removes
        the set (qc_set_point_charges, host only).  SCF states begun afterwards are embedded; states that are alive keep their set."""
        P = _points(positions if positions is not None else np.zeros((0, 3)))
        q = np.ascontiguousarray(charges if charges is not None else np.zeros(0), np.float64).reshape(-1)
        if q.size != len(P):
            raise QcError("qc_set_point_charges: one charge per position")
        _check(lib().qc_set_point_charges(self._h, len(P), _ptr(P) if len(P) else None, _ptr(q) if len(P) else None), "qc_set_point_charges")

    def point_charge_count(self) -> int: return int(lib().qc_point_charge_count(self._h))

    def point_charge_nuclear_energy(self) -> float:
        """E_nq = sum_A sum_c Z_A q_c / |R_A - R_c| of the handle's set (0.0 without charges)."""
        return lib().qc_point_charge_nuclear_energy(self._h)

    def point_charge_matrix(self, gpu: bool = False):
        """(n, n): V_pc = -sum_c q_c A(R_c) of the handle's set - qc_point_charge_matrix on the host, or with gpu=True the kernels the
        SCF set-up uses (qc_point_charge_matrix_gpu)."""
        V = np.zeros((self.n, self.n))
        fn = "qc_point_charge_matrix_gpu" if gpu else "qc_point_charge_matrix"
        _check(getattr(lib(), fn)(self._h, _ptr(V)), fn)
        return V

    def field_matrix(self, r):
        """(3, n, n): B^k_ab = dA_ab(r)/dr_k, the derivative companion of potential_matrix (qc_field_matrix, host only)."""
        B = np.zeros((3, self.n, self.n))
        _check(lib().qc_field_matrix(self._h, _origin_ptr(r), _ptr(B)), "qc_field_matrix")
        return B

    def field_on_points(self, D, points, parts: bool = False):
        """(npts, 3): the electric field E = -grad V of the nuclei and the density D on the GPU (qc_field_on_points); parts=True:
        (E, e_elec, e_nuc).  A point on a nucleus has a non-finite e_nuc and a finite e_elec."""
        Dm, P = self._density_arg(D, "qc_field_on_points"), _points(points)
        ee, en = np.zeros((len(P), 3)), np.zeros((len(P), 3))
        _check(lib().qc_field_on_points(self._h, _ptr(Dm), len(P), _ptr(P), _ptr(ee), _ptr(en)), "qc_field_on_points")
        with np.errstate(invalid="ignore"):
            return (en + ee, ee, en) if parts else en + ee

    def point_charge_gradient(self, D, Db=None):
        """(2, npc, 3): dE_nq/dR_c and d tr(P_t V_pc)/dR_c of the handle's charges at a fixed density (qc_point_charge_gradient).
        RHF: D in the qc_fock_rhf convention; UHF: D = D_alpha, Db = D_beta."""
        n, npc = self.n, self.point_charge_count()
        Dm = np.ascontiguousarray(D if Db is None else np.concatenate([np.asarray(D).reshape(n, n), np.asarray(Db).reshape(n, n)]), dtype=np.float64)
        if Dm.size != (1 if Db is None else 2) * n * n:
            raise QcError("qc_point_charge_gradient: densities must be n x n")
        t = np.zeros((2, npc, 3))
        _check(lib().qc_point_charge_gradient(self._h, 1 if Db is None else 2, _ptr(Dm), _ptr(t)), "qc_point_charge_gradient")
        return t

    def point_charge_timings(self):
        """Phase times (ms) of the handle's last embedding call: upload, Hermite sums over the charges, assembly or contraction, download."""
        ms = np.zeros(4); _check(lib().qc_point_charge_timings(self._h, _ptr(ms)), "qc_point_charge_timings"); return ms

    # ---- conductor-like continuum solvation
    def set_solvent(self, epsilon=None, model: str = "cpcm", scale: float = 0.0, density: float = 0.0, radii=None, x=None):
        """Put the molecule into a conductor-like continuum of dielectric constant `epsilon` (qc_set_solvent, host only), or with
        epsilon=None take it out again.  model: "cpcm" (x = 0) or "cosmo" (x = 0.5), or x itself; scale: factor of the radii (0: 1.2);
        density: surface points per Angstrom^2 (0: 5); radii: per-atom radii in bohr before scaling (None: the van der Waals table).
        SCF states begun afterwards are solvated; states that are alive keep theirs."""
        if epsilon is None:
            _check(lib().qc_set_solvent(self._h, None, None), "qc_set_solvent")
            return
        if x is None:
            if model not in SOLVENT_MODELS:
                raise QcError(f"qc_set_solvent: model must be one of {sorted(SOLVENT_MODELS)}")
            x = SOLVENT_MODELS[model]
        cfg = _Solvent(float(epsilon), float(x), float(scale), float(density))
        r = None
        if radii is not None:
            r = np.ascontiguousarray(radii, np.float64).reshape(-1)
            if len(r) != len(self.mol.atoms):
                raise QcError("qc_set_solvent: one radius per atom")
        _check(lib().qc_set_solvent(self._h, C.byref(cfg), _ptr(r) if r is not None else None), "qc_set_solvent")

    def solvent_points(self) -> int:
        """M, the number of surface elements of the handle's cavity."""
        return int(_check(lib().qc_solvent_surface(self._h, 0, None, None, None), "qc_solvent_surface"))

    def solvent_surface(self):
        """(xyz (M, 3), area (M,), atom (M,) int32): the surface elements of the handle's cavity (qc_solvent_surface)."""
        M = self.solvent_points()
        xyz, area, atom = np.zeros((M, 3)), np.zeros(M), np.zeros(M, np.int32)
        _check(lib().qc_solvent_surface(self._h, M, _ptr(xyz), _ptr(area), _ptr(atom)), "qc_solvent_surface")
        return xyz, area, atom

    def solvent_matrix(self, gpu: bool = False, inverse: bool = False):
        """(M, M): S of the cavity - qc_solvent_matrix on the host, or with gpu=True the assembly kernel; inverse=True (GPU): (S, K) with
        K = -f S^-1 as the SCF uses it (qc_solvent_matrix_gpu)."""
        M = self.solvent_points()
        Sm = np.zeros((M, M))
        if not gpu and not inverse:
            _check(lib().qc_solvent_matrix(self._h, _ptr(Sm)), "qc_solvent_matrix")
            return Sm
        K = np.zeros((M, M)) if inverse else None
        _check(lib().qc_solvent_matrix_gpu(self._h, _ptr(Sm), _ptr(K) if inverse else None), "qc_solvent_matrix_gpu")
        return (Sm, K) if inverse else Sm

    def solvent_response(self, D):
        """(q (M,), V_R (n, n), (1/2 q.v_nuc, 1/2 q.v_elec)) of the total density D (qc_solvent_response, GPU)."""
        Dm = self._density_arg(D, "qc_solvent_response")
        q, V, e = np.zeros(self.solvent_points()), np.zeros((self.n, self.n)), np.zeros(2)
        _check(lib().qc_solvent_response(self._h, _ptr(Dm), _ptr(q), _ptr(V), _ptr(e)), "qc_solvent_response")
        return q, V, (float(e[0]), float(e[1]))

    def solvent_last(self) -> "SolventOutput":
        """The reaction field at the end of the last one-shot run on this handle (qc_solvent_last)."""
        o = _SolventEnergy()
        _check(lib().qc_solvent_last(self._h, C.byref(o)), "qc_solvent_last")
        return SolventOutput._from(o)

    def solvent_timings(self):
        """ms: the one-off set-up (S, factorisation, inverse), then of the last response: the potential call, the reaction kernel
        alone (device events), the V_R call."""
        ms = np.zeros(4); _check(lib().qc_solvent_timings(self._h, _ptr(ms)), "qc_solvent_timings"); return ms

    def spd_inverse(self, A):
        """The inverse of a symmetric positive-definite matrix by the device Cholesky factorisation (qc_spd_inverse); QcError when a pivot
        is <= 0 or not finite."""
        Am = np.ascontiguousarray(A, np.float64)
        if Am.ndim != 2 or Am.shape[0] != Am.shape[1] or Am.shape[0] < 1:
            raise QcError("qc_spd_inverse: A must be n x n, n >= 1")
        out = np.zeros_like(Am)
        _check(lib().qc_spd_inverse(self._h, Am.shape[0], _ptr(Am), _ptr(out)), "qc_spd_inverse")
        return out

    def eri(self):
        I = np.zeros((self.n,) * 4); _check(lib().qc_eri_full(self._h, I.reshape(-1)), "qc_eri_full"); return I

    def fock_rhf(self, D):
        G = np.zeros((self.n, self.n))
        _check(lib().qc_fock_rhf(self._h, np.ascontiguousarray(D, np.float64), G), "qc_fock_rhf"); return G

    def fock_uhf(self, Da, Db):
        Ga, Gb = np.zeros((self.n, self.n)), np.zeros((self.n, self.n))
        _check(lib().qc_fock_uhf(self._h, np.ascontiguousarray(Da, np.float64), np.ascontiguousarray(Db, np.float64), Ga, Gb),
               "qc_fock_uhf")
        return Ga, Gb

    def sym_eig(self, A):
        A = np.ascontiguousarray(A, np.float64); n = A.shape[0]
        V = np.zeros((n, n)); w = np.zeros(n)
        _check(lib().qc_sym_eig(self._h, n, A, V, w), "qc_sym_eig"); return V, w

    def sym_eig_warm(self, A, V0):
        A = np.ascontiguousarray(A, np.float64); n = A.shape[0]
        V = np.zeros((n, n)); w = np.zeros(n)
        _check(lib().qc_sym_eig_warm(self._h, n, A, np.ascontiguousarray(V0, np.float64), V, w), "qc_sym_eig_warm"); return V, w

    def mp2(self, C_mo, eps, nocc, n_frozen: int = 0) -> "Mp2Output":
        """MP2 correlation energy from caller-supplied orbitals (qc_mp2).  RHF: C n x n, eps n, nocc an int (doubly occupied).
        UHF: C (2, n, n) = [Ca, Cb], eps (2, n), nocc (n_alpha, n_beta).  Columns of C are MOs, in the order of eps."""
        nocc = np.atleast_1d(np.asarray(nocc, np.int32))
        nspin = len(nocc)
        Cm = np.ascontiguousarray(C_mo, np.float64).reshape(-1)
        e = np.ascontiguousarray(eps, np.float64).reshape(-1)
        if nspin not in (1, 2) or Cm.size != nspin * self.n * self.n or e.size != nspin * self.n:
            raise QcError("qc_mp2: %d spin(s) need C of %d and eps of %d doubles" % (nspin, nspin * self.n * self.n, nspin * self.n))
        o = _Mp2Output()
        _check(lib().qc_mp2(self._h, nspin, Cm, e, np.ascontiguousarray(nocc), int(n_frozen), C.byref(o)), "qc_mp2")
        return Mp2Output._from(o)

    def gradient(self, D, W, Db=None):
        """The four terms of the nuclear gradient for fixed densities (qc_gradient), each a (natoms, 3) array in Eh/bohr: nuclear
        repulsion, core Hamiltonian, overlap (-W.S'), two-electron.  RHF: D in the qc_fock_rhf convention; UHF: D = D_alpha, Db = D_beta."""
        n = self.n
        Dm = np.ascontiguousarray(D if Db is None else np.concatenate([np.asarray(D).reshape(n, n), np.asarray(Db).reshape(n, n)]), dtype=np.float64)
        Wm = np.ascontiguousarray(W, dtype=np.float64)
        if Dm.size != (1 if Db is None else 2) * n * n or Wm.size != n * n:
            raise QcError("qc_gradient: D and W must be n x n")
        natoms = len(self.mol.atoms)
        t = np.zeros((4, natoms, 3))
        _check(lib().qc_gradient(self._h, 1 if Db is None else 2, Dm, Wm, t), "qc_gradient")
        return t[0], t[1], t[2], t[3]

    def gradient_timings(self):
        """Phase times (ms) of the handle's last gradient: density transform, one-electron terms, two-electron term, sum."""
        ms = np.zeros(4); _check(lib().qc_gradient_timings(self._h, ms), "qc_gradient_timings"); return ms

    def set_fock_mode(self, mode: str):
        """'direct' (default) or 'stored' (the reference's conventional algorithm, tensor resident in HBM)."""
        _check(lib().qc_set_fock_mode(self._h, {"direct": 0, "stored": 1}[mode]), "qc_set_fock_mode")

    def set_accumulation(self, mode: str):
        """'fixed' (default: order-independent 64-bit fixed-point sums, bitwise reproducible) or 'f64' (atomics)."""
        _check(lib().qc_set_accumulation(self._h, {"fixed": 1, "f64": 0}[mode]), "qc_set_accumulation")

    def set_schwarz(self, tau: float):
        """Schwarz threshold of the work lists (default 1e-12; 0 = every quartet, like the reference)."""
        _check(lib().qc_set_schwarz(self._h, float(tau)), "qc_set_schwarz")

    def schwarz_factors(self):
        """(ab, Q): the shell indices (A, B), A >= B, of every stored shell pair and its Schwarz factor sqrt(max (ab|ab)) as the GPU
        computed it (qc_schwarz_factors); pairs below the primitive cut-off are not stored and do not appear."""
        k = _check(lib().qc_schwarz_factors(self._h, None, None, 0), "qc_schwarz_factors")
        ab = np.zeros((k, 2), np.int32); Q = np.zeros(k)
        _check(lib().qc_schwarz_factors(self._h, ab.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p), k), "qc_schwarz_factors")
        return ab, Q

    def set_shard(self, rank, nranks): _check(lib().qc_set_shard(self._h, rank, nranks), "qc_set_shard")

    def plan_shard(self, rank, nranks):
        nq, fl = C.c_int64(), C.c_double()
        _check(lib().qc_plan_shard(self._h, rank, nranks, C.byref(nq), C.byref(fl)), "qc_plan_shard")
        return nq.value, fl.value

    def plan_shard_quartets(self, rank, nranks):
        k = _check(lib().qc_plan_shard_quartets(self._h, rank, nranks, None, 0), "qc_plan_shard_quartets")
        out = np.zeros((k, 4), np.int32)
        _check(lib().qc_plan_shard_quartets(self._h, rank, nranks, out.ctypes.data_as(C.c_void_p), k), "qc_plan_shard_quartets")
        return out

    def comm_init(self, uid: bytes, rank: int, nranks: int):
        _check(lib().qc_comm_init(self._h, uid, rank, nranks), "qc_comm_init")

    def freeze_assignment(self):
        """End the search for the stream assignment of the build's launches with what it has found (before timing builds)."""
        _check(lib().qc_freeze_assignment(self._h), "qc_freeze_assignment")

    def dispatch_lanes(self):
        """(number of dispatch lanes, side stream behind every assignment slot, whether slot 0 is the pipe of the handle's own stream)."""
        n = C.c_int32(); sl = (C.c_int32 * 8)()
        _check(lib().qc_dispatch_lanes(self._h, C.byref(n), sl), "qc_dispatch_lanes")
        return n.value, [int(x) for x in sl[:7]], bool(sl[7])

    def set_stream(self, stream_ptr: int): _check(lib().qc_set_stream(self._h, C.c_void_p(stream_ptr)), "qc_set_stream")

    def unit_quartets(self):
        """Shell quartets of this rank's shard per launch unit (see unit_name)."""
        nq = np.zeros(PROFILE_UNITS, np.int64)
        _check(lib().qc_unit_quartets(self._h, nq.ctypes.data_as(C.c_void_p)), "qc_unit_quartets"); return nq

    def work_stats(self) -> WorkStats:
        ws = WorkStats(); _check(lib().qc_work_stats_get(self._h, C.byref(ws)), "qc_work_stats_get"); return ws

    def fock_rhf_device(self, dD_ptr: int, dG_ptr: int):
        _check(lib().qc_fock_rhf_device(self._h, C.c_void_p(dD_ptr), C.c_void_p(dG_ptr)), "qc_fock_rhf_device")

    def fock_profile(self, dD_ptr: int, dG_ptr: int, reps: int):
        k = self.work_stats().nclasses
        ms = np.zeros(k, np.float32); cid = np.zeros(k, np.int32); nq = np.zeros(k, np.int64)
        by = np.zeros(k); fl = np.zeros(k); tot = C.c_float()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().qc_fock_profile(self._h, C.c_void_p(dD_ptr), C.c_void_p(dG_ptr), reps, p(ms), p(cid), p(nq), p(by), p(fl),
                                     C.cast(C.byref(tot), C.c_void_p)), "qc_fock_profile")
        return dict(class_ms=ms, class_id=cid, quartets=nq, bytes=by, flops=fl, total_ms=tot.value)


def _origin_ptr(origin):
    """three doubles for the C ABI (None: the null pointer = the coordinate origin); the array is kept alive by the returned object"""
    if origin is None:
        return None
    o = np.ascontiguousarray(origin, np.float64).reshape(-1)
    if o.size != 3:
        raise QcError("origin needs three coordinates")
    return (C.c_double * 3)(*o.tolist())


def _points(points) -> np.ndarray:
    """(npts, 3) C-contiguous doubles from anything that reshapes to it"""
    P = np.ascontiguousarray(points, np.float64)
    if P.size % 3:
        raise QcError("points must reshape to (npts, 3)")
    return P.reshape(-1, 3)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


PROFILE_UNITS = 20   # QC_PROFILE_UNITS in include/qchem_hip.h


def unit_name(u: int) -> str:
    """Kernel instantiation behind launch unit `u` of qc_fock_profile_tiers.  (Inside a build some units share a launch - the wide-ket
    buckets of several bra classes, the ss-ket / high-bra with the ps-ket / low-bra bundles, DESIGN.md 3.1 - and are then reported under
    the unit of the group's last member: its name here, the merged kernel qc_fock_tier1_low_kernel<V> / qc_fock_bm_kernel<3, 0> in a trace.)"""
    return "qc_fock_tier_kernel<%d, %d>" % (u // 2, u % 2) if u < 14 else "qc_fock_bm_kernel<%d, %d>" % ((u - 14) // 2, (u - 14) % 2)


def _fock_profile_tiers(self, dD_ptr: int, dG_ptr: int, reps: int):
    ms = np.zeros(PROFILE_UNITS, np.float32); nq = np.zeros(PROFILE_UNITS, np.int64); by = np.zeros(PROFILE_UNITS); fl = np.zeros(PROFILE_UNITS); tot = C.c_float()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().qc_fock_profile_tiers(self._h, C.c_void_p(dD_ptr), C.c_void_p(dG_ptr), reps, p(ms), p(nq), p(by), p(fl),
                                       C.cast(C.byref(tot), C.c_void_p)), "qc_fock_profile_tiers")
    return dict(unit_ms=ms, quartets=nq, bytes=by, flops=fl, total_ms=tot.value)


System.fock_profile_tiers = _fock_profile_tiers


class ScfStepper:
    """One loop-body pass per call (`qc_scf_begin_* / qc_scf_iterate / qc_scf_end`): what a host that owns the
    convergence loop binds, and what bench.py times."""

    def __init__(self, system: "System", uhf: bool = False, n_alpha: int = 0, n_beta: int = 0, stop_rule: float = 0.0, density=None):
        """stop_rule > 0: the caller's loop ends once the reference's test holds at that epsilon (rhf.rs:94 / uhf.rs:139); told to the
        library (qc_scf_set_stop_rule), which checks the value and otherwise ignores it.
        density: start from it instead of the Hueckel guess (qc_scf_begin_*_from) - RHF: D (n, n) in the convention of density(), the
        factor 2 included; UHF: (D_alpha, D_beta)."""
        self.system = system
        self.uhf = uhf
        self._st = C.c_void_p()
        if density is not None:
            n = system.n
            Ds = [np.ascontiguousarray(d, np.float64) for d in (density if uhf else [density])]
            if len(Ds) != (2 if uhf else 1) or any(d.shape != (n, n) for d in Ds):
                raise QcError("ScfStepper: density must be %s of shape (%d, %d)" % ("(D_alpha, D_beta)" if uhf else "one matrix", n, n))
            ptr = [d.ctypes.data_as(C.c_void_p) for d in Ds]
            if uhf:
                _check(lib().qc_scf_begin_uhf_from(system.handle, n_alpha, n_beta, ptr[0], ptr[1], C.byref(self._st)), "qc_scf_begin_uhf_from")
            else:
                _check(lib().qc_scf_begin_rhf_from(system.handle, ptr[0], C.byref(self._st)), "qc_scf_begin_rhf_from")
        elif uhf:
            _check(lib().qc_scf_begin_uhf(system.handle, n_alpha, n_beta, C.byref(self._st)), "qc_scf_begin_uhf")
        else:
            _check(lib().qc_scf_begin_rhf(system.handle, C.byref(self._st)), "qc_scf_begin_rhf")
        if stop_rule > 0.0:
            _check(lib().qc_scf_set_stop_rule(self._st, float(stop_rule)), "qc_scf_set_stop_rule")
        # (the per-pass call is a host's inner loop: the foreign function and its out-parameters are bound once)
        self._iterate = lib().qc_scf_iterate
        self._e, self._r = C.c_double(), C.c_double()
        self._pe, self._pr = C.byref(self._e), C.byref(self._r)

    def iterate(self):
        rc = self._iterate(self._st, self._pe, self._pr)
        if rc != 0:
            if rc == QC_DIIS_SINGULAR:
                raise RuntimeError("DIIS failed")
            _check(rc, "qc_scf_iterate")
        return self._e.value, self._r.value

    def orbital_energies(self, spin=0):
        w = np.zeros(self.system.n); _check(lib().qc_scf_orbital_energies(self._st, spin, w), "qc_scf_orbital_energies"); return w

    def density(self, spin=0):
        D = np.zeros((self.system.n, self.system.n)); _check(lib().qc_scf_density(self._st, spin, D), "qc_scf_density"); return D

    def coefficients(self, spin=0):
        """MO coefficients of the last Roothaan step: column k is the MO of orbital_energies(spin)[k]."""
        Cm = np.zeros((self.system.n, self.system.n))
        _check(lib().qc_scf_coefficients(self._st, spin, Cm), "qc_scf_coefficients"); return Cm

    def mp2(self, n_frozen: int = 0) -> "Mp2Output":
        """MP2 correlation energy from the state's last orbitals (qc_scf_mp2); the state is left as it was."""
        o = _Mp2Output()
        _check(lib().qc_scf_mp2(self._st, int(n_frozen), C.byref(o)), "qc_scf_mp2")
        return Mp2Output._from(o)

    def gradient(self):
        """Total nuclear gradient (natoms, 3), Eh/bohr, at the state's last Roothaan step (qc_scf_gradient); the state is left as it was."""
        g = np.zeros((len(self.system.mol.atoms), 3))
        _check(lib().qc_scf_gradient(self._st, g), "qc_scf_gradient"); return g

    def stability_dim(self, kind: int = 0) -> int:
        dim = lib().qc_scf_stability_dim(self._st, int(kind))           # (a length, not a status: 3 is a valid answer)
        if dim < 0:
            _check(dim, "qc_scf_stability_dim")
        return dim

    def stability(self, kind: int = 0, nroots: int = 1, tol: float = 0.0, max_iterations: int = 0, vectors: bool = False) -> "StabilityOutput":
        """Lowest eigenvalues of the orbital Hessian (A + B) at the state's last orbitals (qc_scf_stability); the state is left as it was.
        kind 0: RHF singlet / UHF internal; kind 1: RHF -> UHF (triplet).  tol 0: 1e-6; max_iterations 0: 100."""
        io = _Stability(kind=int(kind), nroots=int(nroots), max_iterations=int(max_iterations), tol=float(tol))
        X = np.zeros((int(nroots), self.stability_dim(kind))) if vectors else None
        rc = _check(lib().qc_scf_stability(self._st, C.byref(io), None if X is None else X.ctypes.data_as(C.c_void_p)), "qc_scf_stability")
        return StabilityOutput(int(kind), np.array(io.eigenvalues[:nroots]), np.array(io.residuals[:nroots]), rc == QC_OK, int(io.iterations),
                               int(io.builds), io.ms_total, io.ms_builds, X)

    def dipole(self, origin=None, nuclear: bool = False):
        """Dipole moment (3,) in e bohr of the state's density (qc_scf_dipole); origin None: 0.  nuclear=True: (mu, mu_nuclear)."""
        mu, nuc = np.zeros(3), np.zeros(3)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().qc_scf_dipole(self._st, _origin_ptr(origin), p(mu), p(nuc)), "qc_scf_dipole")
        return (mu, nuc) if nuclear else mu

    def multipoles(self, order: int = 2, origin=None) -> "MultipolesOutput":
        """Total Cartesian multipole moments of the state up to `order` <= 4 about `origin` (None: 0) - qc_scf_multipoles; the state is
        left as it was."""
        io = _Multipoles(order=int(order))
        if origin is not None:
            o = _origin_ptr(origin)
            for k in range(3):
                io.origin[k] = o[k]
        _check(lib().qc_scf_multipoles(self._st, C.byref(io)), "qc_scf_multipoles")
        cnt = lib().qc_multipole_count(int(order))
        t = io.quadrupole_traceless
        Q = np.array([[t[0], t[1], t[2]], [t[1], t[3], t[4]], [t[2], t[4], t[5]]])
        return MultipolesOutput(int(order), np.array(io.origin), np.array(io.total[:cnt]), np.array(io.nuclear[:cnt]), np.array(io.electronic[:cnt]), Q)

    def populations(self, scheme: str = "mulliken", bond_orders: bool = False) -> "PopulationsOutput":
        """Charges, spin populations and gross orbital populations of the state, "mulliken" or "lowdin", and with bond_orders the Mayer or
        Wiberg bond-order matrix (qc_scf_populations); the state is left as it was."""
        if scheme not in POPULATION_SCHEMES:
            raise QcError("populations: scheme must be 'mulliken' or 'lowdin'")
        na = len(self.system.mol.atoms)
        q, sp, orb = np.zeros(na), np.zeros(na), np.zeros(self.system.n)
        bo = np.zeros((na, na)) if bond_orders else None
        _check(lib().qc_scf_populations(self._st, POPULATION_SCHEMES[scheme], _ptr(q), _ptr(sp), _ptr(orb), None if bo is None else _ptr(bo)),
               "qc_scf_populations")
        return PopulationsOutput(scheme, q, sp, orb, bo)

    def esp_charges(self, points=None, scales=None, density=None) -> "EspChargesOutput":
        """Charges fitted to the state's electrostatic potential (qc_scf_esp_charges) on the library's Merz-Kollman grid (points None;
        scales / density as System.esp_fit_points) or on the caller's points; the state is left as it was."""
        io = _esp_cfg(scales, density)
        P = self.system.esp_fit_points(scales, density) if points is None else _points(points)
        q, v = np.zeros(len(self.system.mol.atoms)), np.zeros(len(P))
        _check(lib().qc_scf_esp_charges(self._st, C.byref(io), len(P), None if points is None else _ptr(P), _ptr(q), _ptr(v)), "qc_scf_esp_charges")
        return EspChargesOutput(q, io.total_charge, io.rms, io.rrms, np.array(io.dipole), P, v, io.ms_total, io.ms_potential)

    def density_on_points(self, points, spin: bool = False):
        """(npts,): the state's electron density P_alpha + P_beta on points (bohr), or with spin=True the spin density
        P_alpha - P_beta (exactly zero for RHF) - qc_scf_density_on_points; the state is left as it was."""
        P = _points(points)
        rho = np.zeros(len(P))
        _check(lib().qc_scf_density_on_points(self._st, 1 if spin else 0, len(P), _ptr(P), _ptr(rho)), "qc_scf_density_on_points")
        return rho

    def esp_on_points(self, points, parts: bool = False):
        """(npts,): the electrostatic potential of the nuclei and the state's density (qc_scf_esp_on_points); parts=True:
        (V, v_elec, v_nuc).  The state is left as it was."""
        P = _points(points)
        v, ve = np.zeros(len(P)), np.zeros(len(P))
        _check(lib().qc_scf_esp_on_points(self._st, len(P), _ptr(P), _ptr(v), _ptr(ve)), "qc_scf_esp_on_points")
        if not parts:
            return v
        with np.errstate(invalid="ignore"):
            return v, ve, v - ve

    def field_on_points(self, points, parts: bool = False):
        """(npts, 3): the electric field of the nuclei and the state's density, E = -grad V of esp_on_points (qc_scf_field_on_points);
        parts=True: (E, e_elec, e_nuc).  The state is left as it was."""
        P = _points(points)
        e, ee = np.zeros((len(P), 3)), np.zeros((len(P), 3))
        _check(lib().qc_scf_field_on_points(self._st, len(P), _ptr(P), _ptr(e), _ptr(ee)), "qc_scf_field_on_points")
        if not parts:
            return e
        with np.errstate(invalid="ignore"):
            return e, ee, e - ee

    def point_charge_count(self) -> int:
        """charges of the set the state began with (its H contains their V_pc)"""
        return int(lib().qc_scf_point_charge_count(self._st))

    def embedding_nuclear_energy(self) -> float:
        """E_nq of the charges the state began with: total energy = electronic + nuclear repulsion + this."""
        return lib().qc_scf_point_charge_nuclear_energy(self._st)

    def solvent(self, charges: bool = False) -> Optional["SolventOutput"]:
        """The reaction field that goes with the state's current density (qc_scf_solvent), or None for a state in vacuum."""
        o = _SolventEnergy()
        if lib().qc_scf_solvent(self._st, C.byref(o), None) != QC_OK:
            return None
        q = None
        if charges:
            q = np.zeros(int(o.npoints))
            _check(lib().qc_scf_solvent(self._st, C.byref(o), _ptr(q)), "qc_scf_solvent")
        return SolventOutput._from(o, q)

    def solvent_nuclear_energy(self) -> float:
        """1/2 q.v_nuc of a solvated state (0 in vacuum): what the total energy adds to electronic + nuclear repulsion."""
        s = self.solvent()
        return s.nuclear if s is not None else 0.0

    def point_charge_gradient(self):
        """(npc, 3): dE/dR_c at the state for the charges it began with, -q_c E(R_c) (qc_scf_point_charge_gradient); the state is left
        as it was."""
        g = np.zeros((self.point_charge_count(), 3))
        _check(lib().qc_scf_point_charge_gradient(self._st, _ptr(g)), "qc_scf_point_charge_gradient")
        return g

    def orbitals_on_points(self, points, orbitals, spin: int = 0):
        """(len(orbitals), npts): MOs of the state's last Roothaan step on points; `orbitals`: an index or a sequence of indices, counted
        from 0 in the order of orbital_energies(spin) - qc_scf_orbitals_on_points, one call per run of consecutive indices."""
        P = _points(points)
        idx = [int(i) for i in np.atleast_1d(np.asarray(orbitals)).reshape(-1)]
        out = np.zeros((len(idx), len(P)))
        j = 0
        while j < len(idx):
            run = 1
            while j + run < len(idx) and idx[j + run] == idx[j] + run:
                run += 1
            blk = np.zeros((run, len(P)))
            _check(lib().qc_scf_orbitals_on_points(self._st, int(spin), idx[j], run, len(P), _ptr(P), _ptr(blk)), "qc_scf_orbitals_on_points")
            out[j:j + run] = blk
            j += run
        return out

    def polarizability(self, tol: float = 0.0, max_iterations: int = 0, response: bool = False) -> "PolarizabilityOutput":
        """Static dipole polarizability by coupled-perturbed HF at the state's last orbitals (qc_scf_polarizability); the state is left as
        it was.  tol 0: 1e-6; max_iterations 0: 100; response=True: the three solution vectors (3, stability_dim(0))."""
        io = _Polarizability(max_iterations=int(max_iterations), tol=float(tol))
        U = np.zeros((3, self.stability_dim(0))) if response else None
        rc = _check(lib().qc_scf_polarizability(self._st, C.byref(io), None if U is None else U.ctypes.data_as(C.c_void_p)), "qc_scf_polarizability")
        alpha = np.array(io.alpha).reshape(3, 3)
        return PolarizabilityOutput(alpha, float(np.trace(alpha)) / 3.0, np.array(io.residuals), rc == QC_OK, int(io.iterations), int(io.builds),
                                    io.ms_total, io.ms_builds, io.asymmetry, U)

    def excitations(self, method: str = "cis", kind: int = 0, nroots: int = 1, tol: float = 0.0, max_iterations: int = 0,
                    vectors: bool = False) -> "ExcitationsOutput":
        """CIS or TDHF excited states of an RHF state at its last orbitals (qc_scf_excitations); the state is left as it was.
        method "cis" | "tdhf"; kind 0 singlets, 1 triplets; nroots 1..8; tol 0: 1e-6; max_iterations 0: 100."""
        if method not in EXCITATION_METHODS:
            raise QcError("excitations: method must be 'cis' or 'tdhf'")
        code, nroots = EXCITATION_METHODS[method], int(nroots)
        io = _Excitations(method=code, kind=int(kind), nroots=nroots, max_iterations=int(max_iterations), tol=float(tol))
        X = None
        if vectors:
            dim = self.stability_dim(0)
            X = np.zeros((2, nroots, dim) if code == 1 else (nroots, dim))
        rc = _check(lib().qc_scf_excitations(self._st, C.byref(io), None if X is None else X.ctypes.data_as(C.c_void_p)), "qc_scf_excitations")
        return ExcitationsOutput(method, int(kind), np.array(io.energies[:nroots]), np.array(io.residuals[:nroots]), np.array(io.oscillator[:nroots]),
                                 np.array(io.transition_dipole[:3 * nroots]).reshape(nroots, 3), rc == QC_OK, bool(io.reference_unstable),
                                 int(io.nconverged), int(io.iterations), int(io.products), io.ms_total, io.ms_tensor, io.ms_transform, io.ms_solve, X)

    def ccsd(self, n_frozen: int = 0, tol: float = 0.0, max_iterations: int = 0, diis_size: int = 0, amplitudes: bool = False) -> "CcsdOutput":
        """Closed-shell CCSD correlation energy of an RHF state at its last orbitals (qc_scf_ccsd); the state is left as it was.
        tol 0: 1e-8 on max |t_new - t_old|; max_iterations 0: 100; diis_size 0: 8 (1: no extrapolation)."""
        io = _Ccsd(n_frozen=int(n_frozen), max_iterations=int(max_iterations), diis_size=int(diis_size), tol=float(tol))
        t1 = t2 = None
        if amplitudes:
            nocc = self.system.n_electrons() // 2
            o, v = nocc - int(n_frozen), self.system.n - nocc
            t1, t2 = np.zeros((max(o, 0), max(v, 0))), np.zeros((max(o, 0), max(o, 0), max(v, 0), max(v, 0)))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = _check(lib().qc_scf_ccsd(self._st, C.byref(io), p(t1), p(t2)), "qc_scf_ccsd")
        return CcsdOutput(io.e_mp2, io.e_ccsd, io.t1_diagnostic, io.t1_max, io.t2_max, io.residual, int(io.iterations), rc == QC_OK, int(io.n_frozen),
                          io.ms_total, io.ms_tensor, io.ms_transform, io.ms_solve, t1, t2)

    def excitation_matrices(self, kind: int = 0):
        """(A + B, A - B) of an RHF state, (dim, dim) each, rows and columns [i * v + a] (qc_scf_excitation_matrices): kind 0 singlets,
        1 triplets.  Both exactly symmetric."""
        dim = self.stability_dim(0)
        P, M = np.zeros((dim, dim)), np.zeros((dim, dim))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().qc_scf_excitation_matrices(self._st, int(kind), p(P), p(M)), "qc_scf_excitation_matrices")
        return P, M

    def rotated_density(self, x, angle: float = 0.0, kind: int = 0):
        """(D_alpha, D_beta, electronic energy) of the determinant rotated along x by `angle` radians (qc_scf_rotated_density);
        angle <= 0: the library picks the lowest energy among +-0.1 * 2^k, k = 0..4.  The state is left as it was."""
        n = self.system.n
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        if x.size != self.stability_dim(kind):
            raise QcError("rotated_density: x needs %d entries" % self.stability_dim(kind))
        Da, Db, e = np.zeros((n, n)), np.zeros((n, n)), C.c_double()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().qc_scf_rotated_density(self._st, int(kind), p(x), float(angle), p(Da), p(Db), C.byref(e)), "qc_scf_rotated_density")
        return Da, Db, e.value

    def matrix(self, which: str):
        """Set-up matrix of the state: 'S' (overlap), 'H' (core Hamiltonian) or 'X' (S^-1/2, rhf.rs:124-131)."""
        M = np.zeros((self.system.n, self.system.n))
        _check(lib().qc_scf_matrix(self._st, {"S": 0, "H": 1, "X": 2}[which], M), "qc_scf_matrix"); return M

    def spin_square(self) -> float:
        """<S^2> of the current UHF determinant (0 for RHF)."""
        v = C.c_double(); _check(lib().qc_scf_spin_square(self._st, C.byref(v)), "qc_scf_spin_square"); return v.value

    def tensor_ms(self):
        return lib().qc_scf_tensor_ms(self._st)

    def timings(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(lib().qc_scf_timings(self._st, C.byref(a), C.byref(b), C.byref(c)), "qc_scf_timings")
        return dict(setup=a.value, fock=b.value, linalg=c.value)

    def counters(self):
        """ms_setup, ms_fock (builds with a tuner run left out), ms_linalg, builds behind ms_fock, host ms of tuner runs, passes,
        spec_hits / spec_lost (reserved, always 0), passes whose eigensolve was repeated."""
        v = (C.c_double * 11)()
        _check(lib().qc_scf_counters(self._st, v, 11), "qc_scf_counters")
        k = ("setup", "fock", "linalg", "builds_timed", "tuner", "passes", "spec_hits", "spec_lost", "redos", "assign_trials", "assign_frozen")
        return dict(zip(k, [float(x) for x in v]))

    def close(self):
        if self._st:
            lib().qc_scf_end(self._st); self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_info() -> str:
    """Path and version of the RCCL library libqchem_hip.so has bound (dlopen; see include/qchem_hip.h)."""
    buf = C.create_string_buffer(512)
    lib().qc_rccl_info(buf, 512)
    return buf.value.decode()


def measure_peaks():
    """(FP64 TFLOP/s of a register-resident v_fma_f64 loop, GB/s of a 1 GiB streaming copy) measured on the current device."""
    f, b = C.c_double(0.0), C.c_double(0.0)
    _check(lib().qc_measure_peaks(C.byref(f), C.byref(b)), "qc_measure_peaks")
    return f.value, b.value


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(lib().qc_comm_unique_id(buf), "qc_comm_unique_id")
    return buf.raw


# ------------------------------------------------------------------ the reference's public API (hf/mod.rs:5-15)
@dataclass
class HartreeFockConfig:
    max_iterations: int = 100      # CLI default, main.rs:33
    epsilon: float = 1e-6          # CLI default, main.rs:36
    n_alpha: int = 0               # extension (uhf only); 0/0 = the reference's N/2 rule (uhf.rs:43-45)
    n_beta: int = 0


@dataclass
class RestrictedHartreeFockOutput:
    orbital_energies: List[float]
    electronic_energy: float
    nuclear_repulsion: float
    iterations: int
    timings_ms: dict = field(default_factory=dict)
    embedding_nuclear_energy: float = 0.0    # E_nq of the point charges the run was embedded in (System.set_point_charges)
    solvent_nuclear_energy: float = 0.0      # 1/2 q.v_nuc of the continuum the run was solvated in (System.set_solvent)

    def total_energy(self) -> float:
        return self.electronic_energy + self.nuclear_repulsion + self.embedding_nuclear_energy + self.solvent_nuclear_energy


@dataclass
class UnrestrictedHartreeFockOutput:
    orbital_energies_alpha: List[float]
    orbital_energies_beta: List[float]
    electronic_energy: float
    nuclear_repulsion: float
    iterations: int
    timings_ms: dict = field(default_factory=dict)
    embedding_nuclear_energy: float = 0.0    # E_nq of the point charges the run was embedded in (System.set_point_charges)
    solvent_nuclear_energy: float = 0.0      # 1/2 q.v_nuc of the continuum the run was solvated in (System.set_solvent)

    def total_energy(self) -> float:
        return self.electronic_energy + self.nuclear_repulsion + self.embedding_nuclear_energy + self.solvent_nuclear_energy


def _as_system(system) -> System:
    return system if isinstance(system, System) else System(system)


def _run(fn, system, config, uhf):
    sysh = _as_system(system)
    sysh.last_solvent = None
    n = sysh.n
    wa, wb = np.zeros(n), np.zeros(n)
    cfg = _Config(int(config.max_iterations), float(config.epsilon), int(config.n_alpha), int(config.n_beta))
    out = _Output()
    out.orbital_energies = wa.ctypes.data_as(C.POINTER(C.c_double))
    out.orbital_energies_beta = wb.ctypes.data_as(C.POINTER(C.c_double))
    rc = getattr(lib(), fn)(sysh.handle, C.byref(cfg), C.byref(out))
    if rc == QC_DIIS_SINGULAR:
        raise RuntimeError("DIIS failed")                 # rhf.rs:73 / uhf.rs:95-97
    _check(rc, fn)
    if rc == QC_NOT_CONVERGED:
        return None                                       # rhf.rs:106-107
    t = dict(setup=out.ms_setup, fock=out.ms_fock_total, linalg=out.ms_linalg_total, total=out.ms_total, tuner=out.ms_tuner)
    o = _SolventEnergy()
    sysh.last_solvent = SolventOutput._from(o) if lib().qc_solvent_last(sysh.handle, C.byref(o)) == QC_OK else None   # (None: no solvent)
    e_solv = sysh.last_solvent.nuclear if sysh.last_solvent is not None else 0.0
    if uhf:
        return UnrestrictedHartreeFockOutput(wa.tolist(), wb.tolist(), out.electronic_energy, out.nuclear_repulsion,
                                             int(out.iterations), t, sysh.point_charge_nuclear_energy(), e_solv)
    return RestrictedHartreeFockOutput(wa.tolist(), out.electronic_energy, out.nuclear_repulsion, int(out.iterations), t,
                                       sysh.point_charge_nuclear_energy(), e_solv)


def restricted_hartree_fock(system, config: HartreeFockConfig) -> Optional[RestrictedHartreeFockOutput]:
    return _run("qc_scf_rhf", system, config, False)


def unrestricted_hartree_fock(system, config: HartreeFockConfig) -> Optional[UnrestrictedHartreeFockOutput]:
    return _run("qc_scf_uhf", system, config, True)


def _stepped(system, config: HartreeFockConfig, uhf: bool, after):
    """The reference's loop (rhf.rs:67-108 / uhf.rs:82-167) driven pass by pass, as cli.run_uhf does, then `after` (MP2, gradient) on the
    converged state."""
    sysh = _as_system(system)
    sysh.last_solvent = None
    if uhf:
        n_alpha, n_beta = int(config.n_alpha), int(config.n_beta)
        st = ScfStepper(sysh, uhf=True, n_alpha=n_alpha, n_beta=n_beta, stop_rule=float(config.epsilon))
    else:
        st = ScfStepper(sysh, stop_rule=float(config.epsilon))
    try:
        for it in range(int(config.max_iterations) + 1):                   # 0..=max_iterations, rhf.rs:67 / uhf.rs:82
            e, rms = st.iterate()
            if (rms / 2.0 if uhf else rms) < config.epsilon:                # uhf.rs:139 / rhf.rs:94
                t = st.timings()
                sysh.last_solvent = st.solvent()
                if uhf:
                    out = UnrestrictedHartreeFockOutput(st.orbital_energies(0).tolist(), st.orbital_energies(1).tolist(), e,
                                                        sysh.nuclear_repulsion(), it, t, st.embedding_nuclear_energy(), st.solvent_nuclear_energy())
                else:
                    out = RestrictedHartreeFockOutput(st.orbital_energies(0).tolist(), e, sysh.nuclear_repulsion(), it, t,
                                                      st.embedding_nuclear_energy(), st.solvent_nuclear_energy())
                return out, after(st)
        return None
    finally:
        st.close()


def debug_gemm(A, B, Cm=None, alpha: float = 1.0, beta: float = 0.0, splitk: bool = True, reps: int = 0):
    """alpha A B + beta C on the GPU through the split-k GEMM of the CCSD ladder (splitk) or the one-wave-per-tile GEMM (qc_debug_gemm).
    Returns the product, or (product, times in ms) when reps > 0."""
    A, B = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(B, np.float64)
    m, k = A.shape
    n = B.shape[1]
    out = np.zeros((m, n)) if Cm is None else np.array(Cm, np.float64, order="C")
    ms = np.zeros(max(int(reps), 1))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().qc_debug_gemm(1 if splitk else 0, m, n, k, float(alpha), p(A), p(B), float(beta), p(out), int(reps), p(ms)), "qc_debug_gemm")
    return (out, ms) if reps > 0 else out


def restricted_mp2(system, config: HartreeFockConfig, n_frozen: int = 0):
    """(RestrictedHartreeFockOutput, Mp2Output), or None when the SCF does not converge."""
    return _stepped(system, config, False, lambda st: st.mp2(n_frozen))


def unrestricted_mp2(system, config: HartreeFockConfig, n_frozen: int = 0):
    """(UnrestrictedHartreeFockOutput, Mp2Output), or None when the SCF does not converge.  config.n_alpha / n_beta as for
    unrestricted_hartree_fock."""
    return _stepped(system, config, True, lambda st: st.mp2(n_frozen))


def restricted_gradient(system, config: HartreeFockConfig):
    """(RestrictedHartreeFockOutput, gradient (natoms, 3) in Eh/bohr), or None when the SCF does not converge."""
    return _stepped(system, config, False, lambda st: st.gradient())


def unrestricted_gradient(system, config: HartreeFockConfig, n_alpha: int, n_beta: int):
    """(UnrestrictedHartreeFockOutput, gradient (natoms, 3) in Eh/bohr), or None when the SCF does not converge."""
    cfg = HartreeFockConfig(config.max_iterations, config.epsilon, int(n_alpha), int(n_beta))
    return _stepped(system, cfg, True, lambda st: st.gradient())


def restricted_polarizability(system, config: HartreeFockConfig, tol: float = 0.0):
    """(RestrictedHartreeFockOutput, PolarizabilityOutput), or None when the SCF does not converge."""
    return _stepped(system, config, False, lambda st: st.polarizability(tol=tol))


def unrestricted_polarizability(system, config: HartreeFockConfig, n_alpha: int, n_beta: int, tol: float = 0.0):
    """(UnrestrictedHartreeFockOutput, PolarizabilityOutput), or None when the SCF does not converge."""
    cfg = HartreeFockConfig(config.max_iterations, config.epsilon, int(n_alpha), int(n_beta))
    return _stepped(system, cfg, True, lambda st: st.polarizability(tol=tol))


@dataclass
class StabilizeOutput:
    """Result of stabilize(): the last converged output (Restricted... while the state stayed RHF, Unrestricted... after an RHF -> UHF
    instability was followed or for a UHF start), per cycle (electronic energy, lowest eigenvalue, kind of that eigenvalue), whether the
    last state is stable, its <S^2>, and its density."""
    output: object
    history: list
    stable: bool
    spin_square: float = 0.0
    density: object = None            # the last state's density: D (RHF, factor 2 included) or (D_alpha, D_beta) - a start for ScfStepper(density=...)


def stabilize(system, config: HartreeFockConfig, n_alpha: int = 0, n_beta: int = 0, max_cycles: int = 8, threshold: float = 1e-5,
              uhf: Optional[bool] = None, tol: float = 0.0) -> Optional[StabilizeOutput]:
    """Converge; ask for the lowest eigenvalue of the orbital Hessian; if it is below -threshold, rotate along its eigenvector
    (rotated_density with the library's angle ladder), start again from that determinant and repeat, at most max_cycles times.
    An RHF state (uhf None: n_alpha == n_beta; or uhf False) is checked for RHF -> UHF instabilities first (the followed state is UHF),
    then for singlet ones.  threshold absorbs exact zero modes, which come out as +-1e-9.  None when an SCF does not converge."""
    sysh = _as_system(system)
    if n_alpha <= 0 and n_beta <= 0:
        n_alpha = n_beta = sysh.n_electrons() // 2
    is_uhf = (n_alpha != n_beta) if uhf is None else bool(uhf)
    density, history = None, []
    for cycle in range(int(max_cycles) + 1):
        st = ScfStepper(sysh, uhf=is_uhf, n_alpha=n_alpha, n_beta=n_beta, stop_rule=float(config.epsilon), density=density)
        try:
            e = None
            for it in range(int(config.max_iterations) + 1):
                e, rms = st.iterate()
                if (rms / 2.0 if is_uhf else rms) < config.epsilon:
                    break
            else:
                return None
            if is_uhf:
                out = UnrestrictedHartreeFockOutput(st.orbital_energies(0).tolist(), st.orbital_energies(1).tolist(), e,
                                                    sysh.nuclear_repulsion(), it, st.timings(), st.embedding_nuclear_energy())
            else:
                out = RestrictedHartreeFockOutput(st.orbital_energies(0).tolist(), e, sysh.nuclear_repulsion(), it, st.timings(),
                                                  st.embedding_nuclear_energy())
            s2 = st.spin_square()
            follow, lowest = None, None
            for kind in ((0,) if is_uhf else (1, 0)):
                if st.stability_dim(kind) == 0:
                    continue
                r = st.stability(kind=kind, nroots=1, tol=tol, vectors=True)
                ev = float(r.eigenvalues[0])
                if lowest is None or ev < lowest[0]:
                    lowest = (ev, kind)
                if ev < -threshold:
                    follow = (kind, r.vectors[0])
                    break
            if lowest is None:
                lowest = (0.0, 0)
            history.append((e, lowest[0], lowest[1]))
            if follow is None or cycle == max_cycles:
                return StabilizeOutput(out, history, follow is None, s2, (st.density(0), st.density(1)) if is_uhf else st.density(0))
            Da, Db, _ = st.rotated_density(follow[1], 0.0, kind=follow[0])
            if is_uhf:
                density = (Da, Db)
            elif follow[0] == 1:
                is_uhf, density = True, (Da, Db)
            else:
                density = 2.0 * Da
        finally:
            st.close()
    return None
