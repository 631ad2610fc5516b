"""Cost of the conductor-like continuum.  Two measurements, one JSON line each:

  a warm SCF pass of water/cc-pVTZ and benzene/cc-pVDZ with and without a solvent (dielectric constant 78.39, default cavity): the median
  wall time of --passes calls of qc_scf_iterate after --warm untimed ones, through the stepped API, and for the solvated state the
  library's split of the reaction field behind a pass (qc_solvent_timings: potential, reaction kernel, V_R) as medians over the same passes;

  the one-off set-up (S, Cholesky factorisation, inverse: qc_solvent_timings[0]) at M of about 200, 500 and 2000 surface elements - water
  at 5, chloroform at 5 and benzene at 20 points per Angstrom^2 - on a fresh handle each, median of --reps.

    python tools/solvent_timing.py [--passes 12] [--warm 6] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS = 78.39
PASS_SYSTEMS = [("water", "cc-pVTZ"), ("benzene", "cc-pVDZ")]
SETUP_SURFACES = [("water", 5.0), ("chloroform", 5.0), ("benzene", 20.0)]


def load(q, mol, basis):
    return q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"), q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))


def passes(q, s, warm, count):
    """median wall time of a pass (ms) and, for a solvated handle, the medians of the three per-pass phases"""
    st = q.ScfStepper(s)
    try:
        for _ in range(warm):
            st.iterate()
        s.freeze_assignment()
        ts, ph = [], []
        for _ in range(count):
            t0 = time.perf_counter(); st.iterate(); ts.append((time.perf_counter() - t0) * 1e3)
            if st.solvent() is not None:
                ph.append(s.solvent_timings()[1:].tolist())
        out = {"pass_ms": {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}}
        if ph:
            out["potential_ms"], out["reaction_ms"], out["matrix_ms"] = (statistics.median(p[k] for p in ph) for k in range(3))
        return out
    finally:
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import qchem_rs_amd as q
    if not q.device_ready():
        raise SystemExit("solvent_timing: no gfx950 device")
    for mol, basis in PASS_SYSTEMS:
        s = q.System(load(q, mol, basis))
        row = {"system": f"{mol}/{basis}", "n": s.n, "vacuum": passes(q, s, args.warm, args.passes)}
        s.set_solvent(EPS)
        row["surface_elements"] = s.solvent_points()
        row["solvated"] = passes(q, s, args.warm, args.passes)
        row["setup_ms"] = float(s.solvent_timings()[0])
        print(json.dumps(row), flush=True)
        s.close()
    for mol, density in SETUP_SURFACES:
        m = load(q, mol, "STO-3G")
        ts, M = [], 0
        for _ in range(args.reps + 1):                       # (the first: code objects, allocator)
            s = q.System(m)
            s.set_solvent(EPS, density=density)
            M = s.solvent_points()
            s.solvent_matrix(inverse=True)
            ts.append(float(s.solvent_timings()[0]))
            s.close()
        ts = ts[1:]
        print(json.dumps({"setup": f"{mol} at {density:g} per A^2", "surface_elements": M,
                          "setup_ms": {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}}), flush=True)


if __name__ == "__main__":
    main()
