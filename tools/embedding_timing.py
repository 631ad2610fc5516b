"""Cost of the point-charge embedding on benzene/cc-pVDZ and water/cc-pVTZ at 10^3, 10^4 and 10^5 charges: wall time per
call and the library's phase times (upload, Hermite sums over the charges, assembly or contraction, download) of
  the matrix build            qc_point_charge_matrix_gpu
  the field at the charges    qc_field_on_points
  the charges' gradient       qc_point_charge_gradient (the field kernels at the charges + the host's nuclear part)
  the atoms' gradient term    the point-charge part of qc_gradient (its phase times; the whole call also runs the vacuum gradient)
Warm: one untimed call per shape, then --reps calls; median, minimum and maximum.

    python tools/embedding_timing.py [--reps 7] [--skip-large]

And the one comparison with a target: at 1024 charges the matrix build against the only route a handle without this feature has,
qc_one_electron_gpu(which = 2) on the ghost system (the molecule plus 1024 shell-less atoms of Z = 1), the two alternating inside one
process, --ab-reps times each.  Both are whole calls that end in a download to the host.  Prints one JSON line per (system, charges)
and one per comparison.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYSTEMS = [("benzene", "cc-pVDZ"), ("water", "cc-pVTZ")]
SIZES = [1000, 10000, 100000]


def timed(fn, reps):
    fn()                                                     # warm: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def charges(m, npc, seed):
    """npc unit-scale charges in the box of the molecule plus 12 bohr, none closer than 0.5 bohr to a nucleus"""
    import numpy as np
    rng = np.random.default_rng(seed)
    R = m.coordinates()
    lo, hi = R.min(axis=0) - 12.0, R.max(axis=0) + 12.0
    P = lo + (hi - lo) * rng.random((2 * npc + 64, 3))
    keep = np.sqrt(((P[:, None, :] - R[None, :, :]) ** 2).sum(axis=2)).min(axis=1) >= 0.5
    return np.ascontiguousarray(P[keep][:npc]), rng.standard_normal(npc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-reps", type=int, default=15)
    ap.add_argument("--skip-large", action="store_true", help="leave the 10^5 charges out")
    args = ap.parse_args()
    import numpy as np
    import qchem_rs_amd as q
    if not q.device_ready():
        raise SystemExit("embedding_timing: no gfx950 device")
    for mol, basis in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        rng = np.random.default_rng(1)
        D = rng.standard_normal((s.n, s.n)) * 0.1
        D = 0.5 * (D + D.T)
        W = 0.5 * D
        for npc in SIZES:
            if npc > 10000 and args.skip_large:
                continue
            P, c = charges(m, npc, 7)
            s.set_point_charges(P, c)
            row = {"system": f"{mol}/{basis}", "n": s.n, "charges": npc, "records": [int(x) for x in s.esp_records()]}
            row["matrix_ms"] = timed(lambda: s.point_charge_matrix(gpu=True), args.reps)
            row["matrix_phases_ms"] = s.point_charge_timings().tolist()
            row["field_ms"] = timed(lambda: s.field_on_points(D, P), args.reps)
            row["field_phases_ms"] = s.points_timings().tolist()
            row["charge_gradient_ms"] = timed(lambda: s.point_charge_gradient(D), args.reps)
            row["charge_gradient_phases_ms"] = s.point_charge_timings().tolist()
            s.gradient(D, W)
            row["atom_gradient_term_phases_ms"] = s.point_charge_timings().tolist()
            row["atom_gradient_term_ms"] = float(sum(row["atom_gradient_term_phases_ms"]))
            print(json.dumps(row), flush=True)
        # the target: 1024 charges, the new build against the nuclear-attraction kernel on the ghost system, alternating
        P, _ = charges(m, 1024, 9)
        s.set_point_charges(P, np.ones(1024))
        atoms = [q.Atom(a.ordinal, list(a.position)) for a in m.atoms] + [q.Atom(1, [float(x) for x in r]) for r in P]
        ghost = q.System(q.MolecularSystem(atoms, m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim, m.exponents, m.coefficients))
        new = lambda: s.point_charge_matrix(gpu=True)
        old = lambda: ghost.one_electron_gpu(2)
        Vn, Vo = new(), old() - s.one_electron_gpu(2)
        old(); new()
        tn, to = [], []
        for _ in range(args.ab_reps):
            t0 = time.perf_counter(); new(); tn.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); old(); to.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"system": f"{mol}/{basis}", "comparison": "1024 charges: qc_point_charge_matrix_gpu vs qc_one_electron_gpu(2) on the ghost system",
                          "new_ms": {"median": statistics.median(tn), "min": min(tn), "max": max(tn)},
                          "ghost_ms": {"median": statistics.median(to), "min": min(to), "max": max(to)},
                          "new_phases_ms": s.point_charge_timings().tolist(), "max_abs_difference": float(np.abs(Vn - Vo).max())}), flush=True)
        ghost.close(); s.close()


if __name__ == "__main__":
    main()
