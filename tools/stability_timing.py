"""Cost of the stability analysis (qc_scf_stability) on converged states: Fock builds per root, wall time per call, the part of it spent
outside the Fock builds (pseudo-density and projection GEMMs, the Davidson kernels, the host's subspace eigenproblem), next to the warm
Fock-build time of the same handle inside its SCF passes.

    python tools/stability_timing.py [--reps 3] [--tol 1e-6]

Prints one JSON line per (system, kind, nroots).  Kernel-level times come from a `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import qchem_rs_amd as q  # noqa: E402

SYSTEMS = [("oxygen", "cc-pVDZ", True, 9, 7), ("benzene", "cc-pVDZ", False, 0, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("stability_timing: no gfx950 device")
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
        for kind in ((0,) if uhf else (1, 0)):
            for nroots in (1, 4):
                runs = [st.stability(kind=kind, nroots=nroots, tol=args.tol) for _ in range(args.reps + 1)][1:]   # (the first call loads code objects)
                best = min(runs, key=lambda r: r.ms_total)
                print(json.dumps({"system": f"{mol}/{basis}", "n": s.n, "dim": st.stability_dim(kind), "kind": kind, "nroots": nroots,
                                  "tol": args.tol, "converged": best.converged, "eigenvalues": best.eigenvalues.tolist(),
                                  "iterations": best.iterations, "builds": best.builds, "builds_per_root": best.builds / nroots,
                                  "ms_call": best.ms_total, "ms_builds": best.ms_builds, "ms_per_build": best.ms_builds / best.builds,
                                  "share_outside_builds": 1.0 - best.ms_builds / best.ms_total, "warm_scf_build_ms": warm_build_ms}), flush=True)
        st.close(); s.close()


if __name__ == "__main__":
    main()
