"""Cost of the charge and moment properties of an SCF state: wall time per call of ScfStepper.multipoles (order 2 and 4),
.populations (Mulliken and Loewdin, with bond orders) and .esp_charges (the library's grid; with the share of the potential) on
water/cc-pVTZ and benzene/cc-pVDZ.  The state is a converged RHF determinant (epsilon 1e-8).  Warm: one untimed call each, then --reps
calls, median.

    python tools/properties_timing.py [--reps 5]

Whole-call times (allocations, copies and launch gaps included), not kernel times; those come from a `rocprofv3 --kernel-trace --stats`
run of this script.  Prints one JSON line per system.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYSTEMS = [("water", "cc-pVTZ"), ("benzene", "cc-pVDZ")]


def timed(fn, reps):
    fn()                                                     # warm: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import qchem_rs_amd as q
    if not q.device_ready():
        raise SystemExit("properties_timing: no gfx950 device")
    for mol, basis in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        st = q.ScfStepper(s)
        for passes in range(1, 201):
            _, rms = st.iterate()
            if rms < 1e-8:
                break
        else:
            raise SystemExit("properties_timing: %s/%s did not converge" % (mol, basis))
        row = {"system": f"{mol}/{basis}", "n": s.n, "natoms": len(m.atoms), "scf_passes": passes}
        for label, fn in (("multipoles_order2", lambda: st.multipoles(2)), ("multipoles_order4", lambda: st.multipoles(4)),
                          ("mulliken_mayer", lambda: st.populations("mulliken", bond_orders=True)),
                          ("lowdin_wiberg", lambda: st.populations("lowdin", bond_orders=True)), ("esp_charges", lambda: st.esp_charges())):
            med, lo, hi = timed(fn, args.reps)
            row.update({label + "_ms": med, label + "_ms_min": lo, label + "_ms_max": hi})
        r = st.esp_charges()
        row.update(esp_npts=len(r.points), esp_potential_ms=r.ms_potential, esp_library_ms=r.ms_total, esp_rrms=r.rrms)
        print(json.dumps(row), flush=True)
        st.close(); s.close()


if __name__ == "__main__":
    main()
