"""`qchem-hip rhf|uhf ...`: the reference's command line (/root/reference/qchem-cli/src/main.rs) in front of libqchem_hip.so.

Same sub-commands, flags, defaults and printed lines as `qchem-cli` (main.rs:20-62 flags, :98-105 / :143-151 output: three
decimals, Rust's `{:3.3}` / `{:3.3?}` / Duration `{:0.2?}` formats), so a user of the reference finds the contract unchanged.
Three additions, all opt-in:
  * `--json` prints one JSON object with full-precision fields after the reference's lines;
  * `uhf -c/--charge -s/--spin-multiplicity` are honoured (the reference parses and ignores them, main.rs:111 "TODO"):
    with either given, n_alpha / n_beta follow from charge and multiplicity and an `<S^2>` line is added.  With both left at
    0 the behaviour is the reference's N/2 rule (uhf.rs:43-45);
  * `--mp2 [--frozen-core N]` adds the MP2 correlation energy of the converged determinant after the reference's lines (the SCF
    then runs pass by pass through hf.ScfStepper; its lines are those of the run without the flag);
  * `rhf --ccsd [--frozen-core N]` adds the closed-shell CCSD correlation energy of the converged determinant after any MP2 lines: the
    MP2 (from the first T2, under a name of its own) and CCSD correlation energies, the total energy, the T1 diagnostic and the iteration count; `--json` then carries a "ccsd"
    object; the exit status is 101 when the amplitudes do not converge;
  * `--gradient` adds the analytic nuclear gradient of the converged determinant (Eh/bohr), one line per atom - index, Z, gx, gy,
    gz - after the reference's lines and any MP2 lines; `--json` then carries a "gradient" array;
  * `--stability` adds the lowest eigenvalue of the orbital Hessian of the converged determinant (rhf: triplet and singlet kind; uhf:
    internal) and a `wave function: stable` / `unstable` line; `--json` then carries a "stability" object;
  * `--follow` runs hf.stabilize instead: converge, follow the lowest negative eigenvalue, converge again - one `cycle` line each - and
    prints the final determinant's lines (those of uhf once an rhf run has followed a triplet instability); `--json` carries "follow".
  * `--dipole` adds the dipole moment of the converged determinant (origin 0): `dipole moment (a.u.): x y z`, the same in Debye, and
    `|mu|`; `--polarizability` adds the static dipole polarizability (coupled-perturbed HF, bohr^3): three rows and the isotropic value;
    `--json` then carries "dipole" / "polarizability" objects.  Neither combines with `--follow`.
  * `--cube WHAT --cube-file PATH [--cube-spacing 0.2] [--cube-margin 4.0]` writes a Gaussian cube file of the converged determinant:
    WHAT = density, spin (uhf only), esp, homo, lumo or mo:K (K from 0; uhf: alpha orbitals).  The grid is the bounding box of the nuclei
    plus the margin, steps of the spacing (bohr) along x, y, z.  Nothing is printed for it; `--json` then carries a "cube" object (what,
    file, shape, origin, spacing, min, max, integral = sum of the values x spacing^3).  In the esp file a nucleus closer than half a step
    to a grid point counts at half a step (on the nucleus the potential is +inf).  Does not combine with `--follow`.
  * `rhf --cis N` / `--tdhf N` (N = 1..8) add the lowest N CIS or TDHF excited states of the converged determinant, singlets or, with
    `--triplets`, triplets: one line per state - index, energy in Eh and in eV, and for singlets the oscillator strength f; `--json` then
    carries an "excitations" list, one object per flag given (CIS first).  States that do not converge, or a reference that TDHF refuses,
    are reported on stderr and end the command with exit status 1 after everything else has been printed.  The flags do not exist on
    `uhf` and do not combine with `--follow`.
  * `--multipoles [ORDER]` (0..4, default 2) adds the total Cartesian multipole moments of the converged determinant (origin 0), one
    `multipole moments order L (a.u.):` line per order, and the traceless quadrupole in a.u. and Debye Angstrom; `--charges` with a comma
    list of mulliken, lowdin, esp adds per scheme a `SCHEME charges:` line and one line per atom - index, element, charge and, for `uhf`,
    the spin population (esp: no spin; then an `esp fit:` line with the number of points, rms and rrms, and the dipole of the charges);
    `--bond-orders` adds `mayer bond orders:` and one line per atom pair above 0.05.  `--json` then carries "multipoles", "charges" (a
    list, one object per scheme) and "bond_orders" (the whole matrix).  None combines with `--follow`.
  * `--point-charges FILE` embeds the molecule in external point charges: FILE is a JSON list of `{"charge": q, "position": [x, y, z]}`,
    positions in bohr like the molecule files, any real charges.  One line comes first, `point charges: N, nuclei-charges energy: E_nq`;
    the `electronic energy` then contains tr(P V_pc), `nuclear repulsion energy` stays the atoms' own and `hartree fock energy` is
    their sum plus E_nq (never the charge-charge energy).  With `--gradient` the atoms' rows are the full dE/dR_A and one row per charge
    follows - `qI gx gy gz`, dE/dR_c; `--json` then carries a "point_charges" object (count, nuclear_energy, gradient).  Does not
    combine with `--follow`.  Output without the flag is unchanged.
  * `--solvent EPS [--solvent-model cpcm|cosmo] [--solvent-density D]` solvates the molecule in a conductor-like continuum (C-PCM, the
    default, or COSMO) of dielectric constant EPS with D surface points per Angstrom^2 (default 5).  One line comes first, `solvent: MODEL,
    epsilon EPS, surface elements: M`; the `electronic energy` then contains 1/2 q.v_elec and `hartree fock energy` is electronic +
    nuclear repulsion + 1/2 q.v_nuc; two lines follow the orbital energies, `solvent 1/2 q.v: nuclei .., electrons .., total ..` and
    `solvent surface charge: sum q`; `--json` carries a "solvent" object.  `--mp2` is then the correlation energy on the solvated
    orbitals.  Does not combine with `--point-charges`, `--gradient`, `--stability`, `--follow`, `--polarizability`, `--cis`, `--tdhf`.
Host-side plumbing only: loaders (loader.py) -> C ABI (hf.py) -> HIP kernels; nothing here computes.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import hf
from .loader import BasisSet, MolecularSystem


# ---- Rust formatting, as far as main.rs uses it -------------------------------------------------------------------
def fmt_f(x: float) -> str:
    """`{x:3.3}`: three decimals (the minimum width of 3 never binds)."""
    return "%.3f" % x


def fmt_vec(v: Sequence[float]) -> str:
    """`{v:3.3?}` on a Vec<f64>."""
    return "[" + ", ".join(fmt_f(x) for x in v) + "]"


def fmt_duration(seconds: float, precision: Optional[int]) -> str:
    """`{:0.2?}` (precision 2, main.rs:100) and `{:?}` (precision None, main.rs:145) of a std::time::Duration."""
    ns = int(round(seconds * 1e9))
    if ns >= 1_000_000_000:
        value, unit = ns / 1e9, "s"
    elif ns >= 1_000_000:
        value, unit = ns / 1e6, "ms"
    elif ns >= 1_000:
        value, unit = ns / 1e3, "µs"
    else:
        value, unit = float(ns), "ns"
    if precision is not None:
        return "%.*f%s" % (precision, value, unit)
    digits = {"s": 9, "ms": 6, "µs": 3, "ns": 0}[unit]           # Rust prints the exact nanosecond count, zeros trimmed
    text = "%.*f" % (digits, value)
    if "." in text:
        text = text.rstrip("0").rstrip(".")
    return text + unit


# ---- arguments (clap derive of main.rs:9-62) ------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="qchem-hip", description="Hartree-Fock on an MI355X behind the qchem-rs command line")
    p.add_argument("-v", "--verbose", action="store_false", default=True)      # ArgAction::SetFalse, main.rs:16-17
    sub = p.add_subparsers(dest="command", required=True)
    for name in ("rhf", "uhf"):
        s = sub.add_parser(name)
        s.add_argument("-b", "--basis-set", required=True, help="What basis set to use for the hartree fock calculation")
        s.add_argument("-m", "--molecule", required=True, help="A path to the molecule to perform the calculation on")
        if name == "uhf":
            s.add_argument("-c", "--charge", type=int, default=0, help="The charge of the molecule")
            s.add_argument("-s", "--spin-multiplicity", type=int, default=0, help="The spin multiplicity of the molecule")
        s.add_argument("--max-iterations", type=int, default=100)
        s.add_argument("--epsilon", type=float, default=1e-6)
        s.add_argument("--json", action="store_true", help="also print one JSON object with full-precision fields")
        s.add_argument("--mp2", action="store_true", help="also compute the MP2 correlation energy of the converged determinant")
        s.add_argument("--frozen-core", type=int, default=None, metavar="N",
                       help="leave the lowest N orbitals of each spin out of the MP2 and CCSD sums (requires --mp2 or --ccsd)")
        s.add_argument("--gradient", action="store_true", help="also print the analytic nuclear gradient (Eh/bohr) of the converged determinant")
        s.add_argument("--stability", action="store_true", help="also print the lowest eigenvalue(s) of the orbital Hessian and whether the determinant is a minimum")
        s.add_argument("--dipole", action="store_true", help="also print the dipole moment of the converged determinant (a.u. and Debye)")
        s.add_argument("--polarizability", action="store_true", help="also print the static dipole polarizability (coupled-perturbed HF, bohr^3)")
        s.add_argument("--multipoles", type=int, nargs="?", const=2, default=None, metavar="ORDER",
                       help="also print the total Cartesian multipole moments up to ORDER (0..4, default 2) and the traceless quadrupole")
        s.add_argument("--charges", default=None, metavar="SCHEMES", help="also print atomic charges: a comma list of mulliken, lowdin, esp")
        s.add_argument("--bond-orders", action="store_true", help="also print the Mayer bond orders above 0.05")
        if name == "rhf":
            s.add_argument("--ccsd", action="store_true", help="also compute the CCSD correlation energy of the converged determinant (combines with --frozen-core)")
            s.add_argument("--cis", type=int, default=0, metavar="N", help="also print the lowest N CIS excited states (1..8)")
            s.add_argument("--tdhf", type=int, default=0, metavar="N", help="also print the lowest N TDHF (RPA) excited states (1..8)")
            s.add_argument("--triplets", action="store_true", help="triplet instead of singlet excited states (requires --cis or --tdhf)")
        s.add_argument("--follow", action="store_true", help="follow instabilities downhill until the determinant is stable (at most 8 cycles)")
        s.add_argument("--cube", default=None, metavar="WHAT",
                       help="also write a Gaussian cube file of the converged determinant: density, " + ("spin, " if name == "uhf" else "")
                       + "esp, homo, lumo or mo:K (K from 0" + ("; alpha orbitals)" if name == "uhf" else ")") + " (requires --cube-file)")
        s.add_argument("--cube-file", default=None, metavar="PATH", help="where --cube writes")
        s.add_argument("--cube-spacing", type=float, default=0.2, metavar="BOHR", help="grid spacing of --cube along x, y and z (default 0.2)")
        s.add_argument("--point-charges", default=None, metavar="FILE",
                       help='embed the molecule in external point charges: a JSON list of {"charge": q, "position": [x, y, z]} (bohr)')
        s.add_argument("--solvent", type=float, default=None, metavar="EPS",
                       help="solvate the molecule in a conductor-like continuum of dielectric constant EPS (> 1)")
        s.add_argument("--solvent-model", choices=("cpcm", "cosmo"), default="cpcm", help="f = (eps - 1) / (eps + x): cpcm x = 0 (default), cosmo x = 0.5")
        s.add_argument("--solvent-density", type=float, default=0.0, metavar="D", help="surface points per Angstrom^2 (default 5)")
        s.add_argument("--cube-margin", type=float, default=4.0, metavar="BOHR", help="margin of --cube around the bounding box of the nuclei (default 4.0)")
    return p


def cube_what(text: str, uhf: bool):
    """("density" | "spin" | "esp" | "homo" | "lumo" | "mo", K or None) of a --cube argument, None if it is not one"""
    if text in ("density", "esp", "homo", "lumo") or (text == "spin" and uhf):
        return text, None
    if text.startswith("mo:") and text[3:].isdigit():
        return "mo", int(text[3:])
    return None


def parse_args(argv: Optional[List[str]] = None) -> argparse.Namespace:
    p = build_parser()
    args = p.parse_args(argv)
    if args.frozen_core is not None and not (args.mp2 or getattr(args, "ccsd", False)):
        p.error("--frozen-core requires --mp2" + (" or --ccsd" if args.command == "rhf" else ""))
    if args.frozen_core is not None and args.frozen_core < 0:
        p.error("--frozen-core must not be negative")
    if args.follow and (args.mp2 or args.gradient or args.dipole or args.polarizability):
        p.error("--follow cannot be combined with --mp2, --gradient, --dipole or --polarizability")
    if args.multipoles is not None and not 0 <= args.multipoles <= 4:
        p.error("--multipoles takes an order from 0 to 4")
    if args.charges is not None and charge_schemes(args.charges) is None:
        p.error("--charges takes a comma list of mulliken, lowdin and esp")
    if args.follow and wants_charge_properties(args):
        p.error("--follow cannot be combined with --multipoles, --charges or --bond-orders")
    if args.command == "rhf":
        for flag, nstates in (("--cis", args.cis), ("--tdhf", args.tdhf)):
            if nstates < 0 or nstates > 8:
                p.error(flag + " takes 1 to 8 states")
        if args.triplets and not (args.cis or args.tdhf):
            p.error("--triplets requires --cis or --tdhf")
        if args.follow and (args.cis or args.tdhf):
            p.error("--follow cannot be combined with --cis or --tdhf")
        if args.follow and args.ccsd:
            p.error("--follow cannot be combined with --ccsd")
    if args.follow and args.point_charges:
        p.error("--follow cannot be combined with --point-charges")
    if args.solvent is None and (args.solvent_model != "cpcm" or args.solvent_density != 0.0):
        p.error("--solvent-model and --solvent-density require --solvent")
    if args.solvent is not None:
        if not (1.0 < args.solvent < float("inf")) or not (0.0 <= args.solvent_density < float("inf")):
            p.error("--solvent takes a dielectric constant above 1, --solvent-density must not be negative")
        for flag, on in (("--point-charges", args.point_charges), ("--gradient", args.gradient), ("--stability", args.stability),
                         ("--follow", args.follow), ("--polarizability", args.polarizability), ("--cis", getattr(args, "cis", 0)),
                         ("--tdhf", getattr(args, "tdhf", 0)), ("--ccsd", getattr(args, "ccsd", False))):
            if on:
                p.error("--solvent cannot be combined with " + flag)
    if args.cube is not None:
        if cube_what(args.cube, args.command == "uhf") is None:
            p.error("--cube takes density, %sesp, homo, lumo or mo:K" % ("spin, " if args.command == "uhf" else ""))
        if not args.cube_file:
            p.error("--cube requires --cube-file")
        if not (args.cube_spacing > 0.0) or not (args.cube_margin >= 0.0):
            p.error("--cube-spacing must be positive and --cube-margin must not be negative")
        if args.follow:
            p.error("--follow cannot be combined with --cube")
    elif args.cube_file:
        p.error("--cube-file requires --cube")
    return args


def _print_mp2(mp2: "hf.Mp2Output", e_hf: float) -> None:
    print("mp2 correlation energy: " + fmt_f(mp2.e_corr))
    print("mp2 total energy: " + fmt_f(e_hf + mp2.e_corr))


def _print_ccsd(cc: "hf.CcsdOutput", e_hf: float) -> None:
    # (ten decimals: the lines are not the reference's, and a correlation energy to three decimals is of little use)
    print("ccsd first-iteration (mp2) correlation energy: %.10f" % cc.e_mp2)
    print("ccsd correlation energy: %.10f" % cc.e_ccsd)
    print("ccsd total energy: %.10f" % (e_hf + cc.e_ccsd))
    print("ccsd t1 diagnostic: %.6f" % cc.t1_diagnostic)
    print("ccsd %s after %d iterations" % ("converged" if cc.converged else "did not converge", cc.iterations))


def _ccsd_json(cc: "hf.CcsdOutput", e_hf: float) -> dict:
    return {"e_mp2": cc.e_mp2, "e_ccsd": cc.e_ccsd, "e_total": e_hf + cc.e_ccsd, "t1_diagnostic": cc.t1_diagnostic, "t1_max": cc.t1_max,
            "t2_max": cc.t2_max, "residual": cc.residual, "iterations": cc.iterations, "converged": cc.converged, "n_frozen": cc.n_frozen,
            "timings_ms": {"total": cc.ms_total, "tensor": cc.ms_tensor, "transform": cc.ms_transform, "solve": cc.ms_solve}}


def _mp2_json(mp2: "hf.Mp2Output", e_hf: float) -> dict:
    return {"e_os": mp2.e_os, "e_ss": mp2.e_ss, "e_corr": mp2.e_corr, "e_total": e_hf + mp2.e_corr, "n_frozen": mp2.n_frozen,
            "timings_ms": {"tensor": mp2.ms_tensor, "transform": mp2.ms_transform, "energy": mp2.ms_energy}}


def load_point_charges(path: str):
    """(positions (npc, 3) in bohr, charges (npc,)) of a --point-charges file: a JSON list of {"charge": q, "position": [x, y, z]},
    positions read as the molecule files are"""
    with open(path) as f:
        doc = json.load(f)
    pos = np.array([[float(x) for x in c["position"]] for c in doc], float).reshape(-1, 3)
    return pos, np.array([float(c["charge"]) for c in doc], float)


def _embedded(system: MolecularSystem, args):
    """what the drivers run on: the molecule itself, or with --point-charges a handle that carries the charges (one line is printed)"""
    if args.solvent is not None:
        handle = hf.System(system)
        handle.set_solvent(args.solvent, model=args.solvent_model, density=args.solvent_density)
        print("solvent: %s, epsilon %s, surface elements: %d" % (args.solvent_model, fmt_f(args.solvent), handle.solvent_points()))
        return handle
    if not args.point_charges:
        return system
    pos, q = load_point_charges(args.point_charges)
    handle = hf.System(system)
    handle.set_point_charges(pos, q)
    print("point charges: %d, nuclei-charges energy: %s" % (len(q), fmt_f(handle.point_charge_nuclear_energy())))
    return handle


def _solvent_json(sv: "hf.SolventOutput", args) -> dict:
    return {"model": args.solvent_model, "epsilon": args.solvent, "points": sv.npoints, "nuclear_energy": sv.nuclear,
            "electronic_energy": sv.electronic, "polarization_energy": sv.polarization_energy(), "total_charge": sv.total_charge}


def _print_solvent(sv: "hf.SolventOutput") -> None:
    print("solvent 1/2 q.v: nuclei %s, electrons %s, total %s" % (fmt_f(sv.nuclear), fmt_f(sv.electronic), fmt_f(sv.polarization_energy())))
    print("solvent surface charge: " + fmt_f(sv.total_charge))


def _gradient(st, pc_rows: list):
    """the nuclear gradient of a state; the rows of its point charges, if it has any, go to pc_rows"""
    if st.point_charge_count() > 0:
        pc_rows.append(st.point_charge_gradient())
    return st.gradient()


def _print_charge_gradient(rows) -> None:
    for i, row in enumerate(rows):
        print("q%d %.10f %.10f %.10f" % (i, row[0], row[1], row[2]))


def _print_gradient(system: MolecularSystem, g) -> None:
    for i, (atom, row) in enumerate(zip(system.atoms, g)):
        print("%d %d %.10f %.10f %.10f" % (i, atom.ordinal, row[0], row[1], row[2]))


AU_TO_DEBYE = 2.541746473


def _dipole_json(mu) -> dict:
    norm = float((mu ** 2).sum() ** 0.5)
    return {"au": mu.tolist(), "debye": (mu * AU_TO_DEBYE).tolist(), "norm_au": norm, "norm_debye": norm * AU_TO_DEBYE, "origin": [0.0, 0.0, 0.0]}


def _print_dipole(d: dict) -> None:
    print("dipole moment (a.u.): %.8f %.8f %.8f" % tuple(d["au"]))
    print("dipole moment (Debye): %.8f %.8f %.8f" % tuple(d["debye"]))
    print("|mu|: %.8f a.u. = %.8f Debye" % (d["norm_au"], d["norm_debye"]))


def _polarizability_json(r: "hf.PolarizabilityOutput") -> dict:
    return {"alpha": r.alpha.tolist(), "isotropic": r.isotropic, "residuals": r.residuals.tolist(), "converged": r.converged,
            "iterations": r.iterations, "builds": r.builds, "timings_ms": {"total": r.ms_total, "builds": r.ms_builds}}


def _print_polarizability(d: dict) -> None:
    print("polarizability (a.u.):")
    for row in d["alpha"]:
        print("  %.8f %.8f %.8f" % tuple(row))
    print("isotropic polarizability: %.8f" % d["isotropic"])
    if not d["converged"]:
        print("polarizability: the response equations did not converge", file=sys.stderr)


def _properties(st, args):
    """(dipole, polarizability) JSON objects of the flags given, from the converged state"""
    return (_dipole_json(st.dipole()) if args.dipole else None, _polarizability_json(st.polarizability()) if args.polarizability else None)


AU_TO_DEBYE_ANGSTROM = AU_TO_DEBYE * hf.BOHR_ANGSTROM
CHARGE_SCHEMES = ("mulliken", "lowdin", "esp")
ELEMENTS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr").split()


def element(z: int) -> str:
    return ELEMENTS[z] if 0 < z < len(ELEMENTS) else "Z%d" % z


def charge_schemes(text: str):
    """the schemes of a --charges argument (a comma list of mulliken, lowdin, esp) in the order given, None if it is not one"""
    names = [t.strip() for t in text.split(",")]
    return names if names and all(t in CHARGE_SCHEMES for t in names) and len(set(names)) == len(names) else None


def wants_charge_properties(args) -> bool:
    return args.multipoles is not None or args.charges is not None or args.bond_orders


def _multipoles_json(r: "hf.MultipolesOutput") -> dict:
    qt = r.quadrupole_traceless[np.triu_indices(3)]
    return {"order": r.order, "origin": r.origin.tolist(), "components": ["x" * i + "y" * j + "z" * k for i, j, k in hf.multipole_components(r.order)],
            "total": r.total.tolist(), "nuclear": r.nuclear.tolist(), "electronic": r.electronic.tolist(),
            "quadrupole_traceless_au": qt.tolist(), "quadrupole_traceless_debye_angstrom": (qt * AU_TO_DEBYE_ANGSTROM).tolist()}


def _print_multipoles(d: dict) -> None:
    lo = 0
    for l in range(d["order"] + 1):
        cnt = (l + 1) * (l + 2) // 2
        print("multipole moments order %d (a.u.): %s" % (l, " ".join("%.8f" % x for x in d["total"][lo:lo + cnt])))
        lo += cnt
    if d["order"] >= 2:
        print("traceless quadrupole (a.u.): %.8f %.8f %.8f %.8f %.8f %.8f" % tuple(d["quadrupole_traceless_au"]))
        print("traceless quadrupole (Debye Angstrom): %.8f %.8f %.8f %.8f %.8f %.8f" % tuple(d["quadrupole_traceless_debye_angstrom"]))


def _charges_json(st, scheme: str) -> dict:
    if scheme == "esp":
        r = st.esp_charges()
        return {"scheme": scheme, "charges": r.charges.tolist(), "npts": len(r.points), "rms": r.rms, "rrms": r.rrms, "dipole": r.dipole.tolist(),
                "total_charge": r.total_charge, "timings_ms": {"total": r.ms_total, "potential": r.ms_potential}}
    r = st.populations(scheme)
    return {"scheme": scheme, "charges": r.charges.tolist(), "spin": r.spin.tolist()}


def _print_charges(system: MolecularSystem, d: dict, uhf: bool) -> None:
    print("%s charges:" % d["scheme"])
    for i, (atom, c) in enumerate(zip(system.atoms, d["charges"])):
        line = "%d %s %.8f" % (i, element(atom.ordinal), c)
        print(line + " %.8f" % d["spin"][i] if uhf and "spin" in d else line)
    if d["scheme"] == "esp":
        print("esp fit: %d points, rms %.8f, rrms %.8f" % (d["npts"], d["rms"], d["rrms"]))
        print("esp charges dipole (a.u.): %.8f %.8f %.8f" % tuple(d["dipole"]))


BOND_ORDER_PRINT_THRESHOLD = 0.05


def _print_bond_orders(system: MolecularSystem, bo) -> None:
    print("mayer bond orders:")
    for i in range(len(bo)):
        for j in range(i + 1, len(bo)):
            if bo[i][j] > BOND_ORDER_PRINT_THRESHOLD:
                print("%d %s - %d %s %.8f" % (i, element(system.atoms[i].ordinal), j, element(system.atoms[j].ordinal), bo[i][j]))


def _charge_properties(st, args):
    """{"multipoles", "charges", "bond_orders"} JSON objects of the flags given, from the converged state; None without any of them"""
    if not wants_charge_properties(args):
        return None
    out = {}
    if args.multipoles is not None:
        out["multipoles"] = _multipoles_json(st.multipoles(args.multipoles))
    if args.charges is not None:
        out["charges"] = [_charges_json(st, scheme) for scheme in charge_schemes(args.charges)]
    if args.bond_orders:
        out["bond_orders"] = st.populations("mulliken", bond_orders=True).bond_orders.tolist()
    return out


def _print_charge_properties(system: MolecularSystem, chg: dict, uhf: bool) -> None:
    if "multipoles" in chg:
        _print_multipoles(chg["multipoles"])
    for d in chg.get("charges", []):
        _print_charges(system, d, uhf)
    if "bond_orders" in chg:
        _print_bond_orders(system, chg["bond_orders"])


def cube_grid(system: MolecularSystem, spacing: float, margin: float):
    """(origin (3,), shape (3,), points (nx * ny * nz, 3)) of the --cube grid: the bounding box of the nuclei plus the margin, steps of
    `spacing` bohr along x, y, z from its low corner; points in the order of the file, x outermost and z innermost."""
    xyz = system.coordinates()
    origin = xyz.min(axis=0) - margin
    shape = [int(np.floor(e / spacing + 1e-9)) + 1 for e in (xyz.max(axis=0) + margin - origin)]
    ax = [origin[k] + spacing * np.arange(shape[k]) for k in range(3)]
    pts = np.stack(np.meshgrid(ax[0], ax[1], ax[2], indexing="ij"), axis=-1).reshape(-1, 3)
    return origin, shape, pts


def write_cube(path: str, system: MolecularSystem, what: str, origin, shape, spacing: float, values) -> None:
    """Gaussian cube: two comment lines, atom count and origin, three voxel vectors, one line per atom, then the values - x outermost, z
    innermost, six per line, a line break after every z run.  Orbitals are written as plain volumetric data (positive atom count)."""
    v = np.asarray(values, float).reshape(shape)
    with open(path, "w") as f:
        f.write("qchem-hip cube: %s\n" % what)
        f.write("atomic units; x outermost, z innermost\n")
        f.write("%5d%12.6f%12.6f%12.6f\n" % (len(system.atoms), origin[0], origin[1], origin[2]))
        for k in range(3):
            vec = [spacing if j == k else 0.0 for j in range(3)]
            f.write("%5d%12.6f%12.6f%12.6f\n" % (shape[k], vec[0], vec[1], vec[2]))
        for a in system.atoms:
            f.write("%5d%12.6f%12.6f%12.6f%12.6f\n" % (a.ordinal, float(a.ordinal), a.position[0], a.position[1], a.position[2]))
        for ix in range(shape[0]):
            for iy in range(shape[1]):
                run = v[ix, iy]
                for z0 in range(0, shape[2], 6):
                    f.write("".join("%13.5E" % x for x in run[z0:z0 + 6]) + "\n")


def _cube(st, system: MolecularSystem, args, uhf: bool, n_alpha: int = 0) -> dict:
    """writes the file of --cube from the converged state and returns the "cube" JSON object.  esp: the potential on a grid point closer
    than half a step to a nucleus takes that nucleus at half a step (a grid point ON a nucleus would be +inf), everything else is the
    library's value."""
    what, k = cube_what(args.cube, uhf)
    spacing = float(args.cube_spacing)
    origin, shape, pts = cube_grid(system, spacing, float(args.cube_margin))
    if what == "density":
        val = st.density_on_points(pts)
    elif what == "spin":
        val = st.density_on_points(pts, spin=True)
    elif what == "esp":
        _, v_elec, _ = st.esp_on_points(pts, parts=True)
        val = v_elec.copy()
        for a in system.atoms:
            val += a.ordinal / np.maximum(np.sqrt(((pts - np.asarray(a.position, float)) ** 2).sum(axis=1)), 0.5 * spacing)
    else:
        nocc = n_alpha if uhf and n_alpha > 0 else system.n_electrons // 2
        k = {"homo": nocc - 1, "lumo": nocc}.get(what, k)
        if k < 0 or k >= system.n_basis():
            raise SystemExit("--cube %s: there is no orbital %d (%d basis functions)" % (args.cube, k, system.n_basis()))
        val = st.orbitals_on_points(pts, k)[0]
    write_cube(args.cube_file, system, args.cube, origin, shape, spacing, val)
    return {"what": args.cube, "file": args.cube_file, "shape": list(shape), "origin": [float(x) for x in origin], "spacing": spacing,
            "min": float(val.min()), "max": float(val.max()), "integral": float(val.sum() * spacing ** 3)}


HARTREE_TO_EV = 27.211386245988
EXCITATIONS_FAILED = 1            # exit status when excited states did not converge or TDHF refused the reference (the SCF's own is 101)


def _excitations_json(r: "hf.ExcitationsOutput") -> dict:
    return {"method": r.method, "kind": "triplets" if r.kind else "singlets", "energies": r.energies.tolist(),
            "energies_ev": (r.energies * HARTREE_TO_EV).tolist(), "oscillator_strengths": r.oscillator.tolist(),
            "transition_dipoles": r.transition_dipole.tolist(), "residuals": r.residuals.tolist(), "converged": r.converged,
            "reference_unstable": r.reference_unstable, "iterations": r.iterations, "products": r.products,
            "timings_ms": {"total": r.ms_total, "tensor": r.ms_tensor, "transform": r.ms_transform, "solve": r.ms_solve}}


def _print_excitations(d: dict) -> None:
    if d["reference_unstable"]:
        print("%s %s: the reference is unstable (A + B or A - B is not positive definite), no states" % (d["method"], d["kind"]), file=sys.stderr)
        return
    for k, (e, ev, f) in enumerate(zip(d["energies"], d["energies_ev"], d["oscillator_strengths"])):
        line = "%s %s state %d: %.8f Eh = %.6f eV" % (d["method"], d["kind"][:-1], k + 1, e, ev)
        print(line if d["kind"] == "triplets" else line + ", f = %.8f" % f)
    if not d["converged"]:
        print("%s: the excited states did not converge" % d["method"], file=sys.stderr)


def _excitations(st, args) -> list:
    """the "excitations" JSON objects of the flags given (CIS first), from the converged state"""
    kind = 1 if args.triplets else 0
    return [_excitations_json(st.excitations(method=m, kind=kind, nroots=k)) for m, k in (("cis", args.cis), ("tdhf", args.tdhf)) if k]


STABILITY_THRESHOLD = 1e-5        # eigenvalues above -threshold count as stable (exact zero modes come out as +-1e-9)
KIND_NAME = {(False, 0): "singlet", (False, 1): "triplet", (True, 0): "internal"}


def _stability(st, uhf: bool) -> dict:
    """The lowest eigenvalue of every kind the state has (hf.ScfStepper.stability)."""
    ev = {}
    for kind in ((0,) if uhf else (1, 0)):
        if st.stability_dim(kind) > 0:
            ev[KIND_NAME[(uhf, kind)]] = float(st.stability(kind=kind, nroots=1).eigenvalues[0])
    return {"eigenvalues": ev, "stable": all(v >= -STABILITY_THRESHOLD for v in ev.values()), "threshold": STABILITY_THRESHOLD}


def _print_stability(stab: dict) -> None:
    for name, v in stab["eigenvalues"].items():
        print("stability %s: lowest eigenvalue %.8f" % (name, v))
    print("wave function: " + ("stable" if stab["stable"] else "unstable"))


def run_follow(args, uhf: bool, n_alpha: int = 0, n_beta: int = 0) -> int:
    basis = BasisSet.load(args.basis_set)
    system = MolecularSystem.load(args.molecule, basis)
    start = time.perf_counter()
    res = hf.stabilize(system, hf.HartreeFockConfig(args.max_iterations, args.epsilon), n_alpha, n_beta, threshold=STABILITY_THRESHOLD, uhf=uhf)
    elapsed = time.perf_counter() - start
    if res is None:
        return _not_converged()
    for k, (e, ev, kind) in enumerate(res.history):
        print("cycle %d: electronic energy %.9f, lowest eigenvalue %.8f" % (k, e, ev))
    out = res.output
    now_uhf = isinstance(out, hf.UnrestrictedHartreeFockOutput)
    print("hartree fock converged after %d iterations and %s" % (out.iterations, fmt_duration(elapsed, None if now_uhf else 2)))
    print("electronic energy: " + fmt_f(out.electronic_energy))
    print("nuclear repulsion energy: " + fmt_f(out.nuclear_repulsion))
    print("hartree fock energy: " + fmt_f(out.total_energy()))
    if now_uhf:
        print("orbital energies alpha spin:   " + fmt_vec(out.orbital_energies_alpha))
        print("orbital energies beta spin: " + fmt_vec(out.orbital_energies_beta))
        print("<S^2>: " + fmt_f(res.spin_square))
    else:
        print("orbital energies: " + fmt_vec(out.orbital_energies))
    print("wave function: " + ("stable" if res.stable else "unstable"))
    if args.json:
        doc = {"method": "uhf" if now_uhf else "rhf", "iterations": out.iterations, "electronic_energy": out.electronic_energy,
               "nuclear_repulsion": out.nuclear_repulsion, "total_energy": out.total_energy(), "seconds": elapsed,
               "follow": {"history": [{"electronic_energy": e, "lowest_eigenvalue": ev, "kind": kind} for e, ev, kind in res.history],
                          "stable": res.stable, "spin_square": res.spin_square, "threshold": STABILITY_THRESHOLD}}
        print(json.dumps(doc))
    return 0


def occupations(n_electrons_neutral: int, charge: int, multiplicity: int) -> Tuple[int, int]:
    """(n_alpha, n_beta) of the extension; multiplicity 0 = the lowest one the electron count allows."""
    n = n_electrons_neutral - charge
    if n <= 0:
        raise ValueError("charge %d leaves no electrons" % charge)
    if multiplicity == 0:
        multiplicity = 1 + (n & 1)
    unpaired = multiplicity - 1
    if unpaired > n or (n - unpaired) % 2:
        raise ValueError("multiplicity %d is impossible with %d electrons" % (multiplicity, n))
    n_beta = (n - unpaired) // 2
    return n_beta + unpaired, n_beta


def _not_converged() -> int:
    print("hartree fock did not converge", file=sys.stderr)                 # panic!, main.rs:106 / :152
    return 101                                                              # exit status of a Rust panic


def run_rhf(args) -> int:
    if args.follow:
        return run_follow(args, False)
    basis = BasisSet.load(args.basis_set)                                   # main.rs:76
    system = MolecularSystem.load(args.molecule, basis)                     # main.rs:77
    start = time.perf_counter()
    mp2 = grad = stab = dip = pol = cube = chg = cc = None
    exc, pc_rows = [], []
    molecule, system = system, _embedded(system, args)
    config = hf.HartreeFockConfig(args.max_iterations, args.epsilon)
    if args.stability or args.dipole or args.polarizability or args.cis or args.tdhf or args.ccsd or args.cube or wants_charge_properties(args):
        res = hf._stepped(system, config, False, lambda st: (st.mp2(args.frozen_core or 0) if args.mp2 else None,
                                                             _gradient(st, pc_rows) if args.gradient else None,
                                                             _stability(st, False) if args.stability else None) + _properties(st, args)
                                                            + (_excitations(st, args), _cube(st, molecule, args, False) if args.cube else None,
                                                               _charge_properties(st, args), st.ccsd(args.frozen_core or 0) if args.ccsd else None))
        out, (mp2, grad, stab, dip, pol, exc, cube, chg, cc) = res if res is not None else (None, (None,) * 5 + ([], None, None, None))
    elif args.gradient:
        res = hf._stepped(system, config, False, lambda st: (st.mp2(args.frozen_core or 0) if args.mp2 else None, _gradient(st, pc_rows)))
        out, (mp2, grad) = res if res is not None else (None, (None, None))
    elif args.mp2:
        res = hf.restricted_mp2(system, config, args.frozen_core or 0)
        out, mp2 = res if res is not None else (None, None)
    else:
        out = hf.restricted_hartree_fock(system, config)
    elapsed = time.perf_counter() - start
    if out is None:
        return _not_converged()
    print("hartree fock converged after %d iterations and %s" % (out.iterations, fmt_duration(elapsed, 2)))
    print("electronic energy: " + fmt_f(out.electronic_energy))
    print("nuclear repulsion energy: " + fmt_f(out.nuclear_repulsion))
    print("hartree fock energy: " + fmt_f(out.total_energy()))
    print("orbital energies: " + fmt_vec(out.orbital_energies))
    solv = system.last_solvent if args.solvent is not None else None
    if solv is not None:
        _print_solvent(solv)
    if mp2 is not None:
        _print_mp2(mp2, out.total_energy())
    if cc is not None:
        _print_ccsd(cc, out.total_energy())
    if grad is not None:
        _print_gradient(molecule, grad)
    for rows in pc_rows:
        _print_charge_gradient(rows)
    if stab is not None:
        _print_stability(stab)
    if dip is not None:
        _print_dipole(dip)
    if pol is not None:
        _print_polarizability(pol)
    for e in exc:
        _print_excitations(e)
    if chg is not None:
        _print_charge_properties(molecule, chg, False)
    if args.json:
        doc = {"method": "rhf", "iterations": out.iterations, "electronic_energy": out.electronic_energy,
               "nuclear_repulsion": out.nuclear_repulsion, "total_energy": out.total_energy(),
               "orbital_energies": list(out.orbital_energies), "seconds": elapsed, "timings_ms": out.timings_ms}
        if mp2 is not None:
            doc["mp2"] = _mp2_json(mp2, out.total_energy())
        if cc is not None:
            doc["ccsd"] = _ccsd_json(cc, out.total_energy())
        if grad is not None:
            doc["gradient"] = grad.tolist()
        if solv is not None:
            doc["solvent"] = _solvent_json(solv, args)
        if args.point_charges:
            doc["point_charges"] = {"count": system.point_charge_count(), "nuclear_energy": out.embedding_nuclear_energy}
            if pc_rows:
                doc["point_charges"]["gradient"] = pc_rows[0].tolist()
        if stab is not None:
            doc["stability"] = stab
        if dip is not None:
            doc["dipole"] = dip
        if pol is not None:
            doc["polarizability"] = pol
        if exc:
            doc["excitations"] = exc
        if cube is not None:
            doc["cube"] = cube
        if chg is not None:
            doc.update(chg)
        print(json.dumps(doc))
    if cc is not None and not cc.converged:
        print("ccsd did not converge", file=sys.stderr)
        return 101                                                          # (as an SCF that does not converge)
    if any(not e["converged"] for e in exc):
        return EXCITATIONS_FAILED
    return 0


def run_uhf(args) -> int:
    basis = BasisSet.load(args.basis_set)
    system = MolecularSystem.load(args.molecule, basis)
    extension = args.charge != 0 or args.spin_multiplicity != 0
    n_alpha = n_beta = 0
    if extension:
        n_alpha, n_beta = occupations(system.n_electrons, args.charge, args.spin_multiplicity)
    if args.follow:
        return run_follow(args, True, n_alpha, n_beta)
    start = time.perf_counter()
    s2 = mp2 = grad = stab = dip = pol = cube = chg = solv = None
    pc_rows = []
    embedded = _embedded(system, args)
    if (not extension and not args.mp2 and not args.gradient and not args.stability and not args.dipole and not args.polarizability and not args.cube
            and not wants_charge_properties(args)):
        out = hf.unrestricted_hartree_fock(embedded, hf.HartreeFockConfig(args.max_iterations, args.epsilon))
        solv = embedded.last_solvent if args.solvent is not None else None
    else:
        # the same loop (uhf.rs:82-160) driven pass by pass, so that <S^2> and the MP2 energy of the final determinant can be read
        handle = embedded if args.point_charges or args.solvent is not None else hf.System(system)
        st = hf.ScfStepper(handle, uhf=True, n_alpha=n_alpha, n_beta=n_beta)
        out = None
        try:
            for it in range(args.max_iterations + 1):                       # 0..=max_iterations, uhf.rs:82
                e, rms = st.iterate()
                if rms / 2.0 < args.epsilon:                                # uhf.rs:139
                    if extension:
                        s2 = st.spin_square()
                    out = hf.UnrestrictedHartreeFockOutput(list(st.orbital_energies(0)), list(st.orbital_energies(1)), e,
                                                           handle.nuclear_repulsion(), it,
                                                           embedding_nuclear_energy=st.embedding_nuclear_energy(),
                                                           solvent_nuclear_energy=st.solvent_nuclear_energy())
                    solv = st.solvent()
                    if args.mp2:
                        mp2 = st.mp2(args.frozen_core or 0)
                    if args.gradient:
                        grad = _gradient(st, pc_rows)
                    if args.stability:
                        stab = _stability(st, True)
                    dip, pol = _properties(st, args)
                    if args.cube:
                        cube = _cube(st, system, args, True, n_alpha)
                    chg = _charge_properties(st, args)
                    break
        finally:
            st.close()
            handle.close()
    elapsed = time.perf_counter() - start
    if out is None:
        return _not_converged()
    print("hartree fock converged after %d iterations and %s" % (out.iterations, fmt_duration(elapsed, None)))
    print("electronic energy: " + fmt_f(out.electronic_energy))
    print("nuclear repulsion energy: " + fmt_f(out.nuclear_repulsion))
    print("hartree fock energy: " + fmt_f(out.total_energy()))
    print("orbital energies alpha spin:   " + fmt_vec(out.orbital_energies_alpha))
    print("orbital energies beta spin: " + fmt_vec(out.orbital_energies_beta))
    if solv is not None:
        _print_solvent(solv)
    if s2 is not None:
        print("<S^2>: %s (n_alpha %d, n_beta %d)" % (fmt_f(s2), n_alpha, n_beta))
    if mp2 is not None:
        _print_mp2(mp2, out.total_energy())
    if grad is not None:
        _print_gradient(system, grad)
    for rows in pc_rows:
        _print_charge_gradient(rows)
    if stab is not None:
        _print_stability(stab)
    if dip is not None:
        _print_dipole(dip)
    if pol is not None:
        _print_polarizability(pol)
    if chg is not None:
        _print_charge_properties(system, chg, True)
    if args.json:
        doc = {"method": "uhf", "iterations": out.iterations, "electronic_energy": out.electronic_energy,
               "nuclear_repulsion": out.nuclear_repulsion, "total_energy": out.total_energy(),
               "orbital_energies_alpha": list(out.orbital_energies_alpha),
               "orbital_energies_beta": list(out.orbital_energies_beta), "n_alpha": n_alpha, "n_beta": n_beta,
               "spin_square": s2, "seconds": elapsed, "timings_ms": out.timings_ms}
        if mp2 is not None:
            doc["mp2"] = _mp2_json(mp2, out.total_energy())
        if grad is not None:
            doc["gradient"] = grad.tolist()
        if solv is not None:
            doc["solvent"] = _solvent_json(solv, args)
        if args.point_charges:
            doc["point_charges"] = {"count": len(load_point_charges(args.point_charges)[1]), "nuclear_energy": out.embedding_nuclear_energy}
            if pc_rows:
                doc["point_charges"]["gradient"] = pc_rows[0].tolist()
        if stab is not None:
            doc["stability"] = stab
        if dip is not None:
            doc["dipole"] = dip
        if pol is not None:
            doc["polarizability"] = pol
        if cube is not None:
            doc["cube"] = cube
        if chg is not None:
            doc.update(chg)
        print(json.dumps(doc))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    return run_rhf(args) if args.command == "rhf" else run_uhf(args)


if __name__ == "__main__":
    sys.exit(main())
