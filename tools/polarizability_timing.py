"""Cost of the static polarizability (qc_scf_polarizability) on converged states: Fock builds, iterations, wall time per call and the part
of it spent outside the Fock builds (dipole integrals, right-hand sides, pseudo-density and projection GEMMs, the subspace kernels, the
host's small linear systems), next to the warm Fock-build time of the same handle inside its SCF passes, and the dipole moment call.

    python tools/polarizability_timing.py [--reps 3] [--tol 1e-6]

Prints one JSON line per system.  Kernel-level times come from a `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import qchem_rs_amd as q  # noqa: E402

SYSTEMS = [("water", "cc-pVTZ", False, 0, 0), ("benzene", "cc-pVDZ", False, 0, 0), ("oxygen", "cc-pVDZ", True, 9, 7)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("polarizability_timing: no gfx950 device")
    for mol, basis, uhf, na, nb in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        for _ in range(1500):
            _, rms = st.iterate()
            if (rms / 2.0 if uhf else rms) < 1e-8:
                break
        c = st.counters()
        warm_build_ms = c["fock"] / max(c["builds_timed"], 1.0)
        runs = [st.polarizability(tol=args.tol) for _ in range(args.reps + 1)][1:]          # (the first call loads code objects)
        best = min(runs, key=lambda r: r.ms_total)
        dip_ms = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter(); mu = st.dipole(); dip_ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"system": f"{mol}/{basis}", "method": "uhf" if uhf else "rhf", "n": s.n, "dim": st.stability_dim(0), "tol": args.tol,
                          "converged": best.converged, "alpha": best.alpha.tolist(), "isotropic": best.isotropic, "residuals": best.residuals.tolist(),
                          "asymmetry": best.asymmetry, "iterations": best.iterations, "builds": best.builds, "ms_call": best.ms_total,
                          "ms_builds": best.ms_builds, "ms_per_build": best.ms_builds / max(best.builds, 1),
                          "share_outside_builds": 1.0 - best.ms_builds / best.ms_total, "warm_scf_build_ms": warm_build_ms,
                          "dipole": mu.tolist(), "ms_dipole_call": min(dip_ms[1:])}), flush=True)
        st.close(); s.close()


if __name__ == "__main__":
    main()
