"""Phase times of the GPU excited states (qc_scf_excitations: ms_tensor, ms_transform, ms_solve, products, rounds) on converged RHF states,
next to the same problem in numpy on 16 host threads: the dense A + B and A - B from the stored tensor (tensordot quarter transforms),
numpy.linalg.eigh for CIS and numpy.linalg.eig of (A - B)(A + B) for TDHF.

    python tools/excitations_timing.py [--reps 3] [--nroots 8] [--no-numpy]

Prints one JSON line per system and method (singlets).  Kernel-level times come from a `rocprofv3 --kernel-trace --stats` run of this script.
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

SYSTEMS = [("water", "cc-pVTZ"), ("benzene", "cc-pVDZ")]


def numpy_matrices(I, C, eps, nocc):
    """singlet (A + B, A - B) by tensordot quarter transforms (the definitions of include/qchem_hip.h)"""
    def mo(C1, C2, C3, C4):
        T = np.tensordot(C1, I, axes=(0, 0))
        T = np.tensordot(T, C2, axes=(1, 0))
        T = np.tensordot(T, C3, axes=(1, 0))
        return np.tensordot(T, C4, axes=(1, 0))
    Co, Cv = C[:, :nocc], C[:, nocc:]
    d = nocc * Cv.shape[1]
    ovov = mo(Co, Cv, Co, Cv)
    x = ovov.transpose(0, 3, 2, 1).reshape(d, d)
    g = mo(Co, Co, Cv, Cv).transpose(0, 2, 1, 3).reshape(d, d)
    delta = np.diag((eps[None, nocc:] - eps[:nocc, None]).reshape(-1))
    return delta + 4.0 * ovov.reshape(d, d) - x - g, delta + x - g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nroots", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("excitations_timing: no gfx950 device")
    for mol, basis in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        st = q.ScfStepper(s)
        for _ in range(500):
            _, rms = st.iterate()
            if rms < 1e-8:
                break
        nocc, n = s.n_electrons() // 2, s.n
        ref = {}
        if not args.no_numpy:
            I, C, eps = s.eri(), st.coefficients(0), st.orbital_energies(0)
            t0 = time.perf_counter()
            P, M = numpy_matrices(I, C, eps, nocc)
            t1 = time.perf_counter()
            w_cis = np.linalg.eigvalsh(0.5 * (P + M))
            t2 = time.perf_counter()
            w2 = np.sort(np.linalg.eigvals(M @ P).real)
            w_tdhf = np.sqrt(w2) if w2[0] > 0.0 else None              # (None: A + B or A - B is not positive definite)
            t3 = time.perf_counter()
            ref = {"cis": (w_cis, (t1 - t0 + t2 - t1) * 1e3), "tdhf": (w_tdhf, (t1 - t0 + t3 - t2) * 1e3), "matrices_ms": (t1 - t0) * 1e3}
            del I, P, M
        for method in ("cis", "tdhf"):
            runs = [st.excitations(method, kind=0, nroots=args.nroots, tol=args.tol) for _ in range(args.reps + 1)][1:]   # (the first call loads code objects)
            best = min(runs, key=lambda r: r.ms_total)
            rec = {"system": f"{mol}/{basis}", "method": method, "n": n, "nocc": nocc, "dim": nocc * (n - nocc), "nroots": args.nroots, "tol": args.tol,
                   "converged": best.converged, "reference_unstable": best.reference_unstable, "energies": best.energies.tolist(), "oscillator": best.oscillator.tolist(), "ms_total": best.ms_total,
                   "ms_tensor": best.ms_tensor, "ms_transform": best.ms_transform, "ms_solve": best.ms_solve, "products": best.products,
                   "rounds": best.iterations, "matrix_mb": (nocc * (n - nocc)) ** 2 * 8 / 1e6}
            if ref:
                w, ms = ref[method]
                rec.update(numpy_ms=ms, numpy_matrices_ms=ref["matrices_ms"], numpy_threads=int(os.environ["OMP_NUM_THREADS"]),
                           numpy_reference_unstable=w is None,
                           max_abs_energy_difference=None if w is None else float(np.abs(w[:args.nroots] - best.energies).max()))
            print(json.dumps(rec), flush=True)
        st.close()
        s.close()


if __name__ == "__main__":
    main()
