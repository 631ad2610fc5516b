"""Phase times of the GPU CCSD (qc_scf_ccsd: ms_tensor, ms_transform, ms_solve, time per iteration) on converged RHF states, and the
A/B of the split-k GEMM: the ladder product tau[o^2, v^2] . W[v^2, v^2] and the other few-row or long-k product shapes of a pass, each
through qc_gemm_splitk and through qc_gemm (one wave per 16 x 16 tile), on the same device buffers in the same process (qc_debug_gemm),
alternating, after a warm-up.

    python tools/ccsd_timing.py [--reps 5] [--gemm-reps 20] [--frozen-core 0] [--tol 1e-8]

Prints one JSON line per system: the median and the spread (min, max) of the repeated runs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import qchem_rs_amd as q  # noqa: E402
from qchem_rs_amd import hf  # noqa: E402

SYSTEMS = [("water", "cc-pVTZ"), ("benzene", "cc-pVDZ")]


def stats(x):
    x = np.asarray(x, float)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "runs": len(x)}


def gemm_ab(m, n, k, reps):
    """one product shape on random operands: times (ms) through split-k and through qc_gemm, alternating blocks after one warm-up each"""
    rng = np.random.default_rng(7)
    A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    out, times = {}, {True: [], False: []}
    for _ in range(2):                                                # (two rounds: a drift of the clock shows as a difference between them)
        for splitk in (True, False):
            C, ms = hf.debug_gemm(A, B, None, 1.0, 0.0, splitk=splitk, reps=reps + 1)
            times[splitk] += ms[1:].tolist()                          # (the first launch loads the code object)
            out[splitk] = C
    return {"shape": [m, n, k], "splitk_ms": stats(times[True]), "qc_gemm_ms": stats(times[False]),
            "max_abs_difference": float(np.abs(out[True] - out[False]).max())}


def product_shapes(o, v):
    """the ladder and the other products of a pass that have few rows or a long k: (name, m, n, k)"""
    return [("ladder tau.W", o * o, v * v, v * v), ("Foo", o, o, o * v * v), ("Fvv", v, v, o * o * v), ("Fov", o * v, 1, o * v),
            ("Woooo", o * o, o * o, v * v), ("Z", o * o, o * v, v * v), ("R1 from ovvv", o, v, o * v * v), ("Wvoov", o * v, o * v, o * v)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gemm-reps", type=int, default=20)
    ap.add_argument("--frozen-core", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--systems", default=None, help="comma list of mol/basis (default: water/cc-pVTZ, benzene/cc-pVDZ)")
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("ccsd_timing: no gfx950 device")
    systems = [tuple(x.split("/")) for x in args.systems.split(",")] if args.systems else SYSTEMS
    for mol, basis in systems:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        st = q.ScfStepper(s)
        for _ in range(500):
            _, rms = st.iterate()
            if rms < 1e-8:
                break
        nocc, n = s.n_electrons() // 2, s.n
        o, v = nocc - args.frozen_core, n - nocc
        rec = {"system": f"{mol}/{basis}", "n": n, "o": o, "v": v, "n_frozen": args.frozen_core, "tol": args.tol}
        try:
            runs = [st.ccsd(n_frozen=args.frozen_core, tol=args.tol) for _ in range(args.reps + 1)][1:]      # (the first call loads code objects)
        except q.QcError as e:
            rec["error"] = str(e)
            print(json.dumps(rec), flush=True)
            st.close()
            s.close()
            continue
        r = runs[0]
        rec.update(e_mp2=r.e_mp2, e_ccsd=r.e_ccsd, iterations=r.iterations, converged=r.converged, t1_diagnostic=r.t1_diagnostic,
                   ms_total=stats([x.ms_total for x in runs]), ms_tensor=stats([x.ms_tensor for x in runs]),
                   ms_transform=stats([x.ms_transform for x in runs]), ms_solve=stats([x.ms_solve for x in runs]),
                   ms_per_iteration=stats([x.ms_solve / x.iterations for x in runs]))
        rec["products"] = {name: gemm_ab(m_, n_, k_, args.gemm_reps) for name, m_, n_, k_ in product_shapes(o, v)}
        print(json.dumps(rec), flush=True)
        st.close()
        s.close()


if __name__ == "__main__":
    main()
