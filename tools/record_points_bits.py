"""Every word of what the values-on-points and point-charge-embedding code gives (qc_points.hip, qc_embed.hip, the host matrices of
qc_system.cpp), as a SHA-256 of each output's bytes plus its first eight words as hex for diagnosis.
    python tools/record_points_bits.py [--gpu | --host] [out.json]   (default: both parts into tests/golden/points_embed_bits.json;
                                                                       QCHEM_HIP_LIB selects the build)
tests/test_points_embed_bits_gpu.py replays the same runs (run_gpu, run_uhf, run_host) and compares every entry with the committed file,
which was recorded with the library of the commit before the potential and the field were made one record walk: that work may not change
one bit.  The "host" part needs no device and was recorded on a CPU-only machine; --gpu / --host rewrite one part and keep the other.

Inputs: those of tests/test_embed_gpu.py - test_points_gpu.ALL, 300 points of points_reference.sample_points (one full 256-lane workgroup
and a masked remainder of 44), 300 charges of embed_reference.charge_set (a full tile of 256 and a remainder), D = rand_sym(n, 60 + k).
  water/cc-pVTZ  n = 58: f shells on one centre, so every pair order 0..6 has records - all seven instances of each points kernel, the
                 L + 1 = 7 table of the field and the LT = 7 Lambda of the atoms' gradient; the groups of order 0, 1 and 2 (760, 396, 220
                 records) span two LDS tiles each, the second partial (both asserted below from esp_records())
  far            n = 32: both sides of the Boys switch
  deep           n = 18: deep contractions, many records per pair"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SYSTEMS = ("water/cc-pVTZ", "far", "deep")
UHF_PASSES = 6
UHF_CHARGE_SCALE = 0.05                    # 300 charges of order 1 inside the molecule are no SCF problem; scaled, they are a perturbation
HOST_POINTS = 3


def esp_tile(L):
    """records of pair order L per LDS tile (esp_tile, qc_esp.h)"""
    return 2048 // (4 + (L + 1) * (L + 2) * (L + 3) // 6)


def digest(a):
    a = np.ascontiguousarray(a, np.float64)
    w = a.reshape(-1).view(np.uint64)
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest(), "head": ["%016x" % int(x) for x in w[:8]]}


def inputs(name):
    """(molecule, points, charge positions, charges, D, W) of a system, as test_embed_gpu.case builds them"""
    import embed_reference as ER
    import points_reference as PR
    import synthetic_systems as Y
    from test_points_gpu import ALL
    m = ALL[name]()
    k = list(ALL).index(name)
    import qchem_rs_amd as q
    s = q.System(m)
    n = s.n                                # (creating a handle needs no device)
    s.close()
    C, qc = ER.charge_set(m, 500 + k)
    P = PR.sample_points(m, 300 + k, boys_switch=(name == "far"))
    return m, P, C, qc, Y.rand_sym(n, 60 + k), Y.rand_sym(n, 5)


def _with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                 # (the switches are read by a handle at its first embedding call)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def check_coverage(counts):
    """water/cc-pVTZ: every pair order has records, and one group spans at least two tiles with a partial last one"""
    assert len(counts) == 7 and all(int(c) > 0 for c in counts), counts
    assert any(int(c) > esp_tile(L) and int(c) % esp_tile(L) for L, c in enumerate(counts)), (counts, [esp_tile(L) for L in range(7)])


def run_gpu(name):
    """the device outputs of one system -> {output: digest}"""
    import qchem_rs_amd as q
    m, P, C, qc, D, W = inputs(name)
    s = q.System(m)
    if name == "water/cc-pVTZ":
        check_coverage(s.esp_records())
    s.set_point_charges(C, qc)
    out = {"v_elec": s.esp_on_points(D, P, parts=True)[1], "e_elec": s.field_on_points(D, P, parts=True)[1], "rho": s.density_on_points(D, P),
           "V_pc_auto": s.point_charge_matrix(gpu=True), "point_charge_gradient": s.point_charge_gradient(D)}
    for term, t in zip(("nuclear", "core", "overlap", "two_electron"), s.gradient(D, W)):
        out["gradient_" + term] = t
    s.close()

    def forced():
        h = q.System(m)
        h.set_point_charges(C, qc)
        V = h.point_charge_matrix(gpu=True)
        h.close()
        return V
    for orient in ("record", "charge"):
        out["V_pc_" + orient] = _with_env({"QC_PC_ORIENT": orient}, forced)
    return {k: digest(v) for k, v in out.items()}


def run_uhf():
    """water/cc-pVTZ, UHF(5, 5) with the scaled charge set, after UHF_PASSES passes: the state's entry points"""
    import qchem_rs_amd as q
    m, P, C, qc, _, _ = inputs("water/cc-pVTZ")
    s = q.System(m)
    s.set_point_charges(C, UHF_CHARGE_SCALE * qc)
    st = q.ScfStepper(s, uhf=True, n_alpha=5, n_beta=5)
    for _ in range(UHF_PASSES):
        st.iterate()
    out = {"esp_on_points": st.esp_on_points(P, parts=True)[1], "field_on_points": st.field_on_points(P, parts=True)[1],
           "gradient": st.gradient(), "point_charge_gradient": st.point_charge_gradient()}
    st.close(); s.close()
    assert all(np.all(np.isfinite(v)) for v in out.values())
    return {k: digest(v) for k, v in out.items()}


def run_host(name):
    """the host entries (no device): potential and field matrices of three points, the embedding matrix of the 300 charges"""
    import qchem_rs_amd as q
    m, P, C, qc, _, _ = inputs(name)
    s = q.System(m)
    s.set_point_charges(C, qc)
    pts = P[len(m.atoms) + 1:len(m.atoms) + 1 + HOST_POINTS]             # the point 1e-7 bohr off a nucleus and the first midpoints
    out = {"point_charge_matrix": s.point_charge_matrix()}
    for i, r in enumerate(pts):
        out["potential_matrix_%d" % i] = s.potential_matrix(r)
        out["field_matrix_%d" % i] = s.field_matrix(r)
    s.close()
    return {k: digest(v) for k, v in out.items()}


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a in ("--gpu", "--host")]
    args = [a for a in sys.argv[1:] if a not in ("--gpu", "--host")]
    path = args[0] if args else os.path.join(ROOT, "tests", "golden", "points_embed_bits.json")
    rec = json.load(open(path)) if os.path.exists(path) else {}
    if "--gpu" not in flags:
        rec["host"] = {name: run_host(name) for name in SYSTEMS}
    if "--host" not in flags:
        rec["gpu"] = {name: run_gpu(name) for name in SYSTEMS}
        rec["uhf"] = run_uhf()
    for part, val in rec.items():
        for name, r in (val.items() if part != "uhf" else [("water/cc-pVTZ", val)]):
            print("%-5s %-14s %2d outputs  %s" % (part, name, len(r), " ".join(d["sha256"][:8] for d in r.values())))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)
