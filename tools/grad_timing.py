"""Phase times of the analytic gradient (qc_scf_gradient on converged states): P/W build + Cartesian transform, one-electron terms,
two-electron term, sum - next to the same process's warm Fock build and the SCF passes to convergence, and the two-electron kernel's
FLOP rate under the work model of DESIGN.md 3.7 against the device's measured FP64 peak (qc_measure_peaks).

    python tools/grad_timing.py [--reps 3]

Prints one JSON line per system.  The FLOP rate is taken from a run without Schwarz screening (tau = 0), where the work model counts
exactly the quartets the kernel evaluates.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import qchem_rs_amd as q  # noqa: E402

SYSTEMS = [("water", "cc-pVTZ", False, 0, 0), ("benzene", "cc-pVDZ", False, 0, 0), ("oxygen", "cc-pVDZ", True, 9, 7)]


def nherm(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


def work_model(m):
    """FLOPs of the two-electron kernel over all unique shell quartets, per primitive quartet:
    16 nab ncd Nh(Lcd+1)                                    ket Hermite densities K, KC_x,y,z
    + nab (2 Nh(Lab+1) Nh(Lcd) + 6 Nh(Lab) Nh(Lcd+1))       bra side against R
    + 3 (L+1) Nh(L), L = Lab + Lcd + 1                      R_tuv
    Returns (executed, useful, primitive quartets).  The kernel forms K / KC for every primitive quartet, but they depend on the ket
    primitive pair alone: `useful` counts them once per ket primitive pair and quartet, the rate a kernel that shared them would need."""
    Ls, npr = np.asarray(m.shell_L), np.asarray(m.shell_nprim)
    a, b = np.tril_indices(len(Ls))
    lab, kab = Ls[a] + Ls[b], npr[a] * npr[b]
    nab = ((Ls[a] + 1) * (Ls[a] + 2) // 2) * ((Ls[b] + 1) * (Ls[b] + 2) // 2)
    P, Q = np.tril_indices(len(a))
    l1, l2, n1, n2 = lab[P], lab[Q], nab[P], nab[Q]
    L = l1 + l2 + 1
    fk = (16 * n1 * n2 * nherm(l2 + 1)).astype(np.float64)
    fr = (n1 * (2 * nherm(l1 + 1) * nherm(l2) + 6 * nherm(l1) * nherm(l2 + 1)) + 3 * (L + 1) * nherm(L)).astype(np.float64)
    kb, kk = kab[P].astype(np.float64), kab[Q].astype(np.float64)
    return float(np.sum((fk + fr) * kb * kk)), float(np.sum(fk * kk + fr * kb * kk)), int(np.sum(kab[P].astype(np.int64) * kab[Q]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("grad_timing: no gfx950 device")
    fp64, _ = q.measure_peaks()
    print(json.dumps({"fp64_tflops": fp64}), flush=True)
    for mol, basis, uhf, na, nb in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        rec = {"system": f"{mol}/{basis}", "method": "uhf" if uhf else "rhf"}
        for tau in (None, 0.0):
            s = q.System(m)
            if tau is not None:
                s.set_schwarz(tau)
            st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
            t0 = time.perf_counter()
            passes = 0
            for _ in range(500):
                _, rms = st.iterate()
                passes += 1
                if (rms / 2.0 if uhf else rms) < 1e-8:
                    break
            scf_ms = (time.perf_counter() - t0) * 1e3
            st.gradient()                                              # (the first call loads code objects)
            best, phases = None, None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                st.gradient()
                t = (time.perf_counter() - t0) * 1e3
                if best is None or t < best:
                    best, phases = t, s.gradient_timings()
            # warm Fock build of the same process: one more pass's worth (timed by the library)
            D = st.density(0)
            s.fock_rhf(D)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                s.fock_rhf(D)
            fock_ms = (time.perf_counter() - t0) * 1e3 / args.reps
            st.close()
            key = "" if tau is None else "_tau0"
            rec.update({"n": s.n, "natoms": len(m.atoms)} if tau is None else {})
            rec.update({"ms_gradient" + key: best, "ms_pw_transform" + key: float(phases[0]), "ms_one_electron" + key: float(phases[1]),
                        "ms_two_electron" + key: float(phases[2]), "ms_sum" + key: float(phases[3])})
            if tau is None:
                rec.update({"ms_fock_build_host": fock_ms, "scf_passes": passes, "ms_scf_to_convergence": scf_ms,
                            "gradient_over_fock": best / fock_ms, "gradient_over_scf": best / scf_ms})
            else:
                flops, useful, pq = work_model(m)
                rate = lambda f: f / (phases[2] * 1e-3) / 1e12
                rec.update({"prim_quartets": pq, "gflop_executed": flops / 1e9, "gflop_useful": useful / 1e9,
                            "two_electron_tflops_executed": rate(flops), "two_electron_tflops_useful": rate(useful),
                            "useful_fraction_of_fp64_peak": rate(useful) / fp64})
            s.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
