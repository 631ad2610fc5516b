"""Two case tables, one file each.  CASES: every output of the column Fock kernels' body (qc_fock_body, qc_fock_kernel.h) on the smallest systems that reach each of its pieces:
the SHA-256 of the bytes of fock_rhf(D), fock_uhf(Da, Db), eri() and schwarz_factors() - densities from _rand_sym with the seeds below -,
each array's sum and max-abs as hex words (so that a mismatch says how far off it is), and the {class id: quartets} map of one
instrumented build.
    python tools/record_fock_bits.py [out.json]        (default: tests/golden/fock_column_bits.json; QCHEM_HIP_LIB selects the build)
tests/test_fock_column_bits_gpu.py replays the same cases (run_case) and compares them with the committed file, which was recorded with
the library of the commit before the bra-run mode was removed and the body split into pieces: neither may change one bit.  The sums are
fixed-point, so the words do not depend on the launch order or the replica count.  The file is never re-recorded with a changed kernel.
BM_CASES: the same words for the bra-major kernels (qc_fock_bm_kernel<LCD, HI>, qc_fock_bm.hip), plus G of both builds with QC_BM_NO_ROWBUF=1
(exchange contributions as global atomics, another summation order: words of their own) and the quartets of each bra-major launch:
    python tools/record_fock_bits.py bm [out.json]     (default: tests/golden/fock_bm_bits.json)
tests/test_fock_bm_bits_gpu.py replays them against the file recorded with the library of the commit before qc_bm_pass / qc_bm_body were
carved into pieces and the unused variants removed."""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED_D, SEED_DA, SEED_DB = 1, 2, 3                                       # _rand_sym seeds of D (RHF) and of Da, Db (UHF)


def _cls(c):
    return c >> 12, (c >> 8) & 15, (c >> 4) & 15, c & 15                 # (bra-major, LAB, LCD, LGC) of a class id


def _has(classes, pred):
    return any(k > 0 and pred(*_cls(c)) for c, k in classes.items())


# What the class map of a case must hold for the case to reach what it is there for: (what, predicate over (bm, LAB, LCD, LGC)).
PP_COLUMN = ("p.p kets on the column kernels, 16-lane groups", lambda bm, lab, lcd, lgc: not bm and lcd == 2 and lgc == 4)
NO_BM_PP = ("no bra-major p.p class", None)
# name: (molecule, basis, every shell Cartesian, environment while the System is created, n, required classes)
CASES = {
    # a p.p list below QC_BM_PP_MIN goes back to the column kernels: hoisted form, 16-lane groups, tier<., 0>
    "h2o_sto3g": ("water", "STO-3G", False, {}, 7, [PP_COLUMN, NO_BM_PP]),
    # d kets, 16- and 32-lane groups, the TIER == 2 instance (MFMA_OK = false) of a basis without f
    "h2o_dz": ("water", "cc-pVDZ", False, {}, 24, [
        ("d.d kets in 32-lane groups", lambda bm, lab, lcd, lgc: not bm and lcd == 4 and lgc == 5),
        ("d.p kets in 16-lane groups", lambda bm, lab, lcd, lgc: not bm and lcd == 3 and lgc == 4),
        ("d.d kets under d.p / d.d bras", lambda bm, lab, lcd, lgc: not bm and lcd == 4 and lab >= 3)]),
    # the long p.p list on the column kernels
    "h2o_dz_no_bm_pp": ("water", "cc-pVDZ", False, {"QC_NO_BM_PP": "1"}, 24, [PP_COLUMN, NO_BM_PP]),
    # f kets: matrix-core tiles with their column split, the cooperative R table for L >= 7 under low bras, the three merged launches,
    # the 64-lane digestion (UHF too: its two-spin branch)
    "h2o_tz": ("water", "cc-pVTZ", False, {}, 58, [
        ("f kets under low bras (cooperative R table)", lambda bm, lab, lcd, lgc: not bm and lcd >= 5 and lab <= 2),
        ("f kets under high bras (matrix-core tiles)", lambda bm, lab, lcd, lgc: not bm and lcd >= 5 and lab >= 3 and lgc == 6),
        ("short d.d / f.p-ket lists as matrix-core tiles", lambda bm, lab, lcd, lgc: not bm and lcd == 4 and lab >= 3 and lgc == 6)]),
    # the 32-lane VALU form inside the f-capable kernels
    "h2o_tz_valu": ("water", "cc-pVTZ", False, {"QC_MFMA4_MAX": "0"}, 58, [
        ("d.d / f.p kets in the 32-lane VALU form", lambda bm, lab, lcd, lgc: not bm and lgc == 5 and lcd == 4 and lab >= 3)]),
    # ncd = 100 > 64: the second column pass and the wide-block branches
    "h2o_tz_cartesian": ("water", "cc-pVTZ", True, {}, 65, [
        ("f.f kets (100 columns) under high bras", lambda bm, lab, lcd, lgc: not bm and lcd == 6 and lab >= 3 and lgc == 6),
        ("f.f kets (100 columns) under low bras", lambda bm, lab, lcd, lgc: not bm and lcd == 6 and lab <= 2 and lgc == 6)]),
    # UHF with Da != Db on d kets
    "o2_dz": ("oxygen", "cc-pVDZ", False, {}, 28, [
        ("d.d kets in 32-lane groups", lambda bm, lab, lcd, lgc: not bm and lcd == 4 and lgc == 5)]),
}


# ---- bra-major cases.  A requirement is (what, predicate over (classes, units)): classes = {class id: quartets}, units = {"LCD, HI":
# quartets of the launch qc_fock_bm_kernel<LCD, HI>} as the build issues them (a merged launch carries its guests' quartets).
def _bm(lcd, labs):
    return lambda classes, units: all(_has(classes, lambda bm, lab, l, lgc, want=want: bm and l == lcd and lab == want) for want in labs)


def _launch(unit, yes=True):
    return lambda classes, units: (units[unit] > 0) == yes


SS_LOW = ("bm<0,0> with LAB 0, 1, 2 (paired passes and their tail)", _bm(0, (0, 1, 2)))
PS_LOW = ("bm<1,0> with LAB 1, 2 (packed ps records)", _bm(1, (1, 2)))
PP_BM = ("bm<2,0>: p.p kets against p.p bras, three axis instances", lambda c, u: _bm(2, (2,))(c, u) and u["2, 0"] > 0)
HIGH = ("LAB 3 and 4 against ss and ps kets (staged step 3; register pre-stage at LAB 3)", lambda c, u: _bm(0, (3, 4))(c, u) and _bm(1, (3, 4))(c, u))
MERGED = ("ss kets / high bras riding in bm<3,0>: no launch bm<0,1>", lambda c, u: u["0, 1"] == 0 and u["1, 0"] > 0 and _bm(0, (3,))(c, u))
APART = ("bm<0,1>, bm<1,0>, bm<1,1> as launches of their own", lambda c, u: u["0, 1"] > 0 and u["1, 0"] > 0 and u["1, 1"] > 0)
# (Cartesian d.d bras: 36 function pairs; a ps-ket wave's I block is 36 * 3 * 65 doubles = 56 KB, four of them pass the 160 KB of a CU)
LDS_CUT = ("d.d Cartesian bras against ps kets: fewer than four waves fit the LDS", _bm(1, (4,)))
# name: (molecule, basis, every shell Cartesian, environment while the System is created, n, requirements)
BM_CASES = {
    "h2o_sto3g": ("water", "STO-3G", False, {}, 7, [SS_LOW, PS_LOW, ("no p.p class", _launch("2, 0", False))]),
    "h2o_sto3g_pp": ("water", "STO-3G", False, {"QC_BM_PP_MIN": "1"}, 7, [PP_BM]),
    "h2o_dz": ("water", "cc-pVDZ", False, {}, 24, [HIGH, MERGED, ("bm<1,1>", _launch("1, 1"))]),
    "h2o_dz_no_merge": ("water", "cc-pVDZ", False, {"QC_NO_BM_MERGE": "1"}, 24, [HIGH, APART]),
    "h2o_dz_cartesian": ("water", "cc-pVDZ", True, {}, 25, [HIGH, LDS_CUT]),
    "h2o_dz_plain_units": ("water", "cc-pVDZ", False, {"QC_BM_UNIT": "0", "QC_BM_PP_UNIT": "0"}, 24, [SS_LOW, PS_LOW, HIGH]),
    # UHF with Da != Db on every instance, the p.p kets included
    "o2_dz": ("oxygen", "cc-pVDZ", False, {"QC_BM_PP_MIN": "1"}, 28, [SS_LOW, PS_LOW, HIGH, PP_BM]),
}
BM_UNITS = ("0, 0", "0, 1", "1, 0", "1, 1", "2, 0")


def check_bm_case(name, classes, units):
    """Asserts that the class map and the launches' quartets of bra-major case `name` hold what the case is there for."""
    for what, pred in BM_CASES[name][5]:
        assert pred(classes, units), "%s: %s - not in classes %s, launches %s" % (name, what, {hex(c): k for c, k in classes.items()}, units)


def check_classes(name, classes):
    """Asserts that the class map of case `name` holds every class form the case is there for."""
    for what, pred in CASES[name][5]:
        if pred is None:
            assert not _has(classes, lambda bm, lab, lcd, lgc: bm and lab == 2 and lcd == 2), (name, what, classes)
        else:
            assert _has(classes, pred), "%s: no class with %s in %s" % (name, what, {hex(c): k for c, k in classes.items()})


def _words(*arrays):
    a = np.concatenate([np.ascontiguousarray(x, np.float64).reshape(-1) for x in arrays])
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "sum": float(a.sum()).hex(), "maxabs": float(np.abs(a).max()).hex()}


@contextlib.contextmanager
def _environ(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def run_case(name, bm=False):
    """The case `name` of CASES -> {"n", "fock_rhf", "fock_uhf", "eri", "schwarz": {sha256, sum, maxabs}, "schwarz_pairs", "classes"};
    of BM_CASES (bm): also "no_rowbuf": {"fock_rhf", "fock_uhf"} and "units": {"LCD, HI": quartets of that bra-major launch}."""
    import qchem_rs_amd as q
    from conftest import load_system
    from test_gpu_parity import _column_classes, _rand_sym
    mol, basis, cartesian, env, n, _ = (BM_CASES if bm else CASES)[name]
    m = load_system(mol, basis)
    if cartesian:
        m.shell_pure[:] = 0
    # (the planner's switches are read once per handle, so they are set only while it is created; the handle stays out of the process-wide
    # pool of stream sets from creation to close, so a test session finds the pool as this case found it)
    with _environ({"QC_NO_STREAM_POOL": "1"}):
        with _environ(env):
            s = q.System(m)
        assert s.n == n, (name, s.n)
        ab, Q = s.schwarz_factors()
        out = {"n": int(s.n), "fock_rhf": _words(s.fock_rhf(_rand_sym(n, SEED_D))),
               "fock_uhf": _words(*s.fock_uhf(_rand_sym(n, SEED_DA), _rand_sym(n, SEED_DB))),
               "eri": _words(s.eri()), "schwarz": _words(Q), "schwarz_pairs": hashlib.sha256(ab.tobytes()).hexdigest(),
               "classes": {str(c): k for c, k in sorted(_column_classes(s, n).items())}}
        if bm:
            with _environ({"QC_BM_NO_ROWBUF": "1"}):                     # (read at every launch)
                out["no_rowbuf"] = {"fock_rhf": _words(s.fock_rhf(_rand_sym(n, SEED_D))),
                                    "fock_uhf": _words(*s.fock_uhf(_rand_sym(n, SEED_DA), _rand_sym(n, SEED_DB)))}
            nq = s.unit_quartets()
            out["units"] = {u: int(sum(nq[i] for i in range(q.hf.PROFILE_UNITS) if q.hf.unit_name(i) == "qc_fock_bm_kernel<%s>" % u))
                            for u in BM_UNITS}
        s.close()
    classes = {int(c): k for c, k in out["classes"].items()}
    if bm: check_bm_case(name, classes, out["units"])
    else: check_classes(name, classes)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    bm = bool(args) and args[0] == "bm"
    out = args[bm] if len(args) > bm else os.path.join(ROOT, "tests", "golden", "fock_bm_bits.json" if bm else "fock_column_bits.json")
    rec = {}
    for name in (BM_CASES if bm else CASES):
        rec[name] = r = run_case(name, bm)
        print("%-18s n %2d  classes %2d  G %s  I %s" % (name, r["n"], len(r["classes"]), r["fock_rhf"]["sha256"][:12], r["eri"]["sha256"][:12]),
              flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out)
