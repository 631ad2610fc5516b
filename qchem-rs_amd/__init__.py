"""qchem-rs_amd: MI355X-native Hartree-Fock hot path behind the qchem-rs `core::hf` API."""
from .loader import Atom, BasisSet, MolecularSystem, ShellDef  # noqa: F401
from .hf import (CcsdOutput, EspChargesOutput, ExcitationsOutput, HartreeFockConfig, Mp2Output, MultipolesOutput, PolarizabilityOutput, PopulationsOutput, QcError, RestrictedHartreeFockOutput, ScfStepper, SolventOutput, StabilityOutput, StabilizeOutput, System,  # noqa: F401
                 UnrestrictedHartreeFockOutput, build_library, comm_unique_id, device_ready, lib, measure_peaks, rccl_info,
                 restricted_gradient, restricted_hartree_fock, restricted_mp2, restricted_polarizability, stabilize, unrestricted_gradient, unrestricted_hartree_fock,
                 unrestricted_mp2, unrestricted_polarizability)
