"""Every word of the SCF runs that go through the one-workgroup Roothaan kernel (qc_scf_small.hip), as hex: the electronic energy and the
rms of every pass, the final orbital energies (per spin), `redos` and the passes used.
    python tools/record_small_bits.py [out.json]        (default: tests/golden/small_roothaan_bits.json; QCHEM_HIP_LIB selects the build)
tests/test_small_roothaan_bits_gpu.py replays the same runs (run_case) and compares every word with the committed file, which was
recorded with the library of the commit before the kernel's latency work: that work may not change one bit.

A second table, PASS_CASES, does the same for the forms of an SCF pass that the first table does not reach - the generic launch sequence,
spins side by side and serial, the event wait, stored mode, a one-rank communicator, each with and without the repeat of an eigensolve:
    python tools/record_small_bits.py --pass [out.json]  (default: tests/golden/scf_pass_bits.json)
tests/test_scf_pass_bits_gpu.py replays them against that file, recorded with the library of the commit before the SCF driver
(qc_scf.cpp) was rewritten as a sequence of steps: that rewrite may not change one bit either."""
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

# name: (molecule, basis, uhf, (n_alpha, n_beta), passes, environment, options); options: "fock_mode" ("stored"), "comm" (a one-rank
# communicator).  All n <= 64; the generic launch sequence is reached with QC_NO_SMALL_FUSED.  Every "repeat" case showed redos >= 1 with
# the recording (parent) library at the threshold given here; none had to be changed for that.
# (QC_NO_OPEN_SHELL_FUSED is read once per process, so inside a test session that has already run an SCF it selects nothing any more:
# o2_uhf_generic sets QC_NO_SMALL_FUSED - read per SCF state - next to it, which selects the same generic sequence.)
GENERIC = {"QC_NO_SMALL_FUSED": "1"}
REPEAT = {"QC_EIG_WARM_RMS": "0.5"}
PASS_CASES = {
    "h2o_dz_generic": ("water", "cc-pVDZ", False, (0, 0), 15, GENERIC, {}),        # n = 24 = QC_TRI_MIN_N: Tridiag, then Refine
    "h2o_tz_generic_repeat": ("water", "cc-pVTZ", False, (0, 0), 15, {**GENERIC, **REPEAT}, {}),   # roothaan_redo_eig, generic path
    "c2h4_uhf_generic": ("ethylene", "6-31G_st_st", True, (8, 8), 15, GENERIC, {}),   # beta step + density on the side stream, qc_spin_join
    "c2h4_uhf_generic_serial": ("ethylene", "6-31G_st_st", True, (8, 8), 15, {**GENERIC, "QC_NO_SPIN_PARALLEL": "1"}, {}),
    "o2_uhf_generic": ("oxygen", "cc-pVDZ", True, (9, 7), 20, {**GENERIC, "QC_NO_OPEN_SHELL_FUSED": "1"}, {}),   # rotation-only routes, generic
    "h2o_tz_uhf": ("water", "cc-pVTZ", True, (5, 5), 15, {}, {}),                  # fused, spins side by side: Tridiag / Refine phases, qc_spin_join_end
    "h2o_tz_uhf_repeat": ("water", "cc-pVTZ", True, (5, 5), 15, REPEAT, {}),       # repeat after a side-by-side fused pass
    "h2o_tz_event_wait": ("water", "cc-pVTZ", False, (0, 0), 15, {"QC_EVENT_WAIT": "1"}, {}),
    "h2o_sto3g_stored": ("water", "STO-3G", False, (0, 0), 12, {}, {"fock_mode": "stored"}),   # tensor GEMV build, no prepare step
    "h2o_sto3g_stored_uhf": ("water", "STO-3G", True, (5, 5), 12, {}, {"fock_mode": "stored"}),
    "c2h4_dz_comm": ("ethylene", "cc-pVDZ", False, (0, 0), 15, {}, {"comm": True}),   # d_sync packing, all-reduce, ranks_agree, unused-slot memset
    "c2h4_dz_comm_repeat": ("ethylene", "cc-pVDZ", False, (0, 0), 15, REPEAT, {"comm": True}),   # second collective of a pass
}
# A third table, SHAPE_CASES (format of CASES), holds the shapes at which the kernel's predication, addressing and per-shape instances can
# go wrong and that the first table does not reach:
#     python tools/record_small_bits.py --shapes [out.json]  (default: tests/golden/small_roothaan_shapes_bits.json)
# tests/test_small_roothaan_shapes_bits_gpu.py replays them against that file, recorded with the library of the commit before the
# kernel's instruction diet.  Each run is long enough to hold a cold pass (tridiagonal start; below n = 24 a Jacobi kernel) and a warm one
# (refinement from the previous vectors), the open-shell run its Jacobi launches; the test asserts that from the step counts by route of
# qc_scf_counters.
SHAPE_CASES = {
    "h2o_631g": ("water", "6-31G", False, (0, 0), 12, {}),              # n = 13: odd, a single tile
    "chcl3_sto3g": ("chloroform", "STO-3G", False, (0, 0), 12, {}),     # n = 33: odd, first size of the 2 x 2 form, one row and column in the second tile
    "c6h6_sto3g": ("benzene", "STO-3G", False, (0, 0), 12, {}),         # n = 36
    "chcl3_631g": ("chloroform", "6-31G", False, (0, 0), 12, {}),       # n = 50
    "o2_tz_uhf": ("oxygen", "cc-pVTZ", True, (9, 7), 12, {}),           # n = 60: per-spin pre | Jacobi | post, generic-order dots
    "chcl3_sto3g_repeat": ("chloroform", "STO-3G", False, (0, 0), 12, {"QC_EIG_WARM_RMS": "0.5"}),   # the repeat of an eigensolve
}
REPEAT_CASES = ("h2o_tz_repeat", "h2o_tz_generic_repeat", "h2o_tz_uhf_repeat", "c2h4_dz_comm_repeat")   # redos >= 1 in the record
# (case, table of the twin, twin): the same run by another order of issue or another wait - the two records are equal word for word
SAME_AS = (("c2h4_uhf_generic_serial", "pass", "c2h4_uhf_generic"), ("h2o_tz_event_wait", "small", "h2o_tz"))


def hexword(x):
    return float(x).hex()


def small_steps(st):
    """Roothaan steps of the state that went through the one-workgroup kernel, by eigensolve route (qc_scf_counters 11 .. 13): "warm" one
    launch that refines the previous vectors, "cold" the tridiagonal start between two launches, "jacobi" a Jacobi kernel between two."""
    import ctypes as C
    import qchem_rs_amd as q
    v = (C.c_double * 14)()
    assert q.lib().qc_scf_counters(st._st, v, 14) == 0
    return {"warm": int(v[11]), "cold": int(v[12]), "jacobi": int(v[13])}


def run_case(name):
    """The run `name` of CASES, PASS_CASES or SHAPE_CASES -> {"energy": [...], "rms": [...], "orbital_energies": [[...], ...], "redos": int,
    "passes": int}; a run of SHAPE_CASES also has "small_steps": {...}, which is of the library at hand and not part of a record."""
    import qchem_rs_amd as q
    from conftest import load_system
    mol, basis, uhf, (na, nb), npass, env, *opt = next(t[name] for t in (CASES, PASS_CASES, SHAPE_CASES) if name in t)
    opt = opt[0] if opt else {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                               # (read by the library once per SCF state)
    try:
        s = q.System(load_system(mol, basis))
        if "fock_mode" in opt:
            s.set_fock_mode(opt["fock_mode"])
        if opt.get("comm"):
            s.comm_init(q.comm_unique_id(), 0, 1)
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        tr = [st.iterate() for _ in range(npass)]
        w = [st.orbital_energies(spin) for spin in range(2 if uhf else 1)]
        c = st.counters()
        steps = small_steps(st)
        st.close(); s.close()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    out = {"n": int(len(w[0])), "energy": [hexword(e) for e, _ in tr], "rms": [hexword(r) for _, r in tr],
           "orbital_energies": [[hexword(x) for x in ws] for ws in w], "redos": int(c["redos"]), "passes": int(c["passes"])}
    if name in SHAPE_CASES:
        out["small_steps"] = steps
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a not in ("--pass", "--shapes")]
    table, default = (PASS_CASES, "scf_pass_bits.json") if "--pass" in sys.argv[1:] else (CASES, "small_roothaan_bits.json")
    if "--shapes" in sys.argv[1:]:
        table, default = SHAPE_CASES, "small_roothaan_shapes_bits.json"
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", default)
    rec = {name: run_case(name) for name in table}
    for name, r in rec.items():
        r.pop("small_steps", None)
        print("%-24s n %2d  passes %2d  redos %d  E %s" % (name, r["n"], r["passes"], r["redos"], float.fromhex(r["energy"][-1])))
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out)
