"""Every word of the SCF runs that go through the one-workgroup Roothaan kernel (qc_scf_small.hip), as hex: the electronic energy and the
rms of every pass, the final orbital energies (per spin), `redos` and the passes used.
    python tools/record_small_bits.py [out.json]        (default: tests/golden/small_roothaan_bits.json; QCHEM_HIP_LIB selects the build)
tests/test_small_roothaan_bits_gpu.py replays the same runs (run_case) and compares every word with the committed file, which was
recorded with the library of the commit before the kernel's latency work: that work may not change one bit."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# name: (molecule, basis, uhf, (n_alpha, n_beta), passes, environment)
CASES = {
    "h2o_sto3g": ("water", "STO-3G", False, (0, 0), 12, {}),            # n = 7: one tile per wave; the DIIS window grows 1 .. 6
    "h2o_dz": ("water", "cc-pVDZ", False, (0, 0), 15, {}),              # n = 24: one tile per wave, tridiagonal cold route
    "c2h4_631gss": ("ethylene", "6-31G_st_st", False, (0, 0), 15, {}),  # n = 50: 2 x 2 tiles, partial edge tiles
    "h2o_tz": ("water", "cc-pVTZ", False, (0, 0), 15, {}),              # n = 58: cold and warm passes, one to three refinement passes
    "h2o_tz_repeat": ("water", "cc-pVTZ", False, (0, 0), 15, {"QC_EIG_WARM_RMS": "0.5"}),   # refinement reports ROTATE, eigensolve repeated
    "o2_uhf": ("oxygen", "cc-pVDZ", True, (9, 7), 20, {}),              # n = 28: pre | Jacobi | post, generic-order dots, two spins
}


def hexword(x):
    return float(x).hex()


def run_case(name):
    """The run `name` of CASES -> {"energy": [...], "rms": [...], "orbital_energies": [[...], ...], "redos": int, "passes": int}."""
    import qchem_rs_amd as q
    from conftest import load_system
    mol, basis, uhf, (na, nb), npass, env = CASES[name]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                               # (read by the library once per SCF state)
    try:
        s = q.System(load_system(mol, basis))
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        tr = [st.iterate() for _ in range(npass)]
        w = [st.orbital_energies(spin) for spin in range(2 if uhf else 1)]
        c = st.counters()
        st.close(); s.close()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    return {"n": int(len(w[0])), "energy": [hexword(e) for e, _ in tr], "rms": [hexword(r) for _, r in tr],
            "orbital_energies": [[hexword(x) for x in ws] for ws in w], "redos": int(c["redos"]), "passes": int(c["passes"])}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "small_roothaan_bits.json")
    rec = {name: run_case(name) for name in CASES}
    for name, r in rec.items():
        print("%-14s n %2d  passes %2d  redos %d  E %s" % (name, r["n"], r["passes"], r["redos"], float.fromhex(r["energy"][-1])))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out)
