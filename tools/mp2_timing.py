"""Phase times of the GPU MP2 (qc_scf_mp2: ms_tensor, ms_transform, ms_energy) on converged states, next to a numpy MP2 of the same
tensor on 16 host threads, and the device's measured copy bandwidth (qc_measure_peaks) that step 1 of the transform - one pass over
the n^4 AO tensor - is to be read against.

    python tools/mp2_timing.py [--reps 3]

Prints one JSON line per system.  Kernel-level times (which quarter transformation takes what) come from a
`rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(k, "16")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import qchem_rs_amd as q  # noqa: E402

SYSTEMS = [("water", "cc-pVTZ", False, 0, 0), ("benzene", "cc-pVDZ", False, 0, 0), ("oxygen", "cc-pVDZ", True, 9, 7)]


def numpy_mp2(I, Cs, es, nocc):
    """Conventional MP2 with tensordot quarter transforms (the definitions of include/qchem_hip.h), all electrons."""
    def ovov(Ci, Ca, Cj, Cb):
        T = np.tensordot(Ci, I, axes=(0, 0))
        T = np.tensordot(T, Ca, axes=(1, 0))
        T = np.tensordot(T, Cj, axes=(1, 0))
        return np.tensordot(T, Cb, axes=(1, 0))

    def den(e1, n1, e2, n2):
        return e1[:n1, None, None, None] - e1[None, n1:, None, None] + e2[None, None, :n2, None] - e2[None, None, None, n2:]
    if len(Cs) == 1:
        C, e, no = Cs[0], es[0], nocc[0]
        W = ovov(C[:, :no], C[:, no:], C[:, :no], C[:, no:])
        D = den(e, no, e, no)
        return float((W * W / D).sum() + (W * (W - W.transpose(0, 3, 2, 1)) / D).sum())
    e_corr = 0.0
    for s in (0, 1):
        C, e, no = Cs[s], es[s], nocc[s]
        W = ovov(C[:, :no], C[:, no:], C[:, :no], C[:, no:])
        e_corr += 0.5 * float((W * (W - W.transpose(0, 3, 2, 1)) / den(e, no, e, no)).sum())
    (Ca, Cb), (ea, eb), (na, nb) = Cs, es, nocc
    W = ovov(Ca[:, :na], Ca[:, na:], Cb[:, :nb], Cb[:, nb:])
    return e_corr + float((W * W / den(ea, na, eb, nb)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("mp2_timing: no gfx950 device")
    fp64, copy_gbs = q.measure_peaks()
    print(json.dumps({"fp64_tflops": fp64, "hbm_copy_gbs": copy_gbs}), flush=True)
    for mol, basis, uhf, na, nb in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
        for _ in range(500):
            _, rms = st.iterate()
            if (rms / 2.0 if uhf else rms) < 1e-8:
                break
        runs = [st.mp2() for _ in range(args.reps + 1)][1:]            # (the first call loads code objects)
        best = min(runs, key=lambda r: r.ms_tensor + r.ms_transform + r.ms_energy)
        nspin = 2 if uhf else 1
        nocc = [na, nb] if uhf else [s.n_electrons() // 2]
        Cs = [st.coefficients(k) for k in range(nspin)]
        es = [st.orbital_energies(k) for k in range(nspin)]
        st.close()
        n = s.n
        rec = {"system": f"{mol}/{basis}", "method": "ump2" if uhf else "rmp2", "n": n, "nocc": nocc, "e_corr": best.e_corr,
               "ms_tensor": best.ms_tensor, "ms_transform": best.ms_transform, "ms_energy": best.ms_energy,
               "tensor_gb": n ** 4 * 8 / 1e9,
               # step 1 streams the tensor once per spin: its time at the measured copy rate (read + written bytes per second)
               "step1_floor_ms": n ** 4 * 8 * nspin / (copy_gbs * 1e9) * 1e3}
        if not args.no_numpy:
            I = s.eri()
            t0 = time.perf_counter()
            e_np = numpy_mp2(I, Cs, es, nocc)
            rec["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            rec["numpy_threads"] = int(os.environ["OMP_NUM_THREADS"])
            rec["numpy_minus_gpu"] = e_np - best.e_corr
            del I
        s.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
