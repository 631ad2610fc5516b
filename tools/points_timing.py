"""Cost of the values on points (qc_density_on_points, qc_esp_on_points): wall time per call and the library's phase times (upload, basis
values / Hermite densities, contraction, download) on water/cc-pVTZ and benzene/cc-pVDZ for 10^3, 10^5 and an 80^3 box of points, next to
numpy on the host (basis values + einsum for rho, --numpy-threads threads).  Warm: one untimed call per shape, then --reps calls, median.

    python tools/points_timing.py [--reps 5] [--numpy-threads 16] [--skip-numpy]

For the potential it reports point x record pairs per second and FLOP/s by the work model of DESIGN.md 3.11 (flops per point and record of
pair order L, below) against the measured FP64 ceiling of qc_measure_peaks.  These are whole-call rates (copies and launch gaps included),
not a kernel's share of peak; kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line per
(system, npts).
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
SIZES = [("1e3", 10), ("1e5", 100000), ("80^3", 80)]


def nherm(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


def esp_flops_per_point_record(L):
    """argument 9; Boys 16 (L = 0: Horner) or 36 + 3 L (Horner, exp(-x), downward recursion); seeds 2 (L + 1); the table
    3 per entry above the seeds (C(L+4, 4) - (L + 1) entries: a multiply and a fused multiply-add at the most); the dot 2 nherm(L)"""
    rwork = (L + 1) * (L + 2) * (L + 3) * (L + 4) // 24
    return 9 + (16 if L == 0 else 36 + 3 * L) + 2 * (L + 1) + 3 * (rwork - (L + 1)) + 2 * nherm(L)


def box(m, n):
    """n^3 points on the --cube box of the molecule (bounding box of the nuclei plus 4 bohr)"""
    import numpy as np
    xyz = m.coordinates()
    lo, hi = xyz.min(axis=0) - 4.0, xyz.max(axis=0) + 4.0
    ax = [np.linspace(lo[k], hi[k], n) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def timed(fn, reps):
    fn()                                                     # warm: code objects, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-threads", type=int, default=16)
    ap.add_argument("--skip-numpy", action="store_true")
    args = ap.parse_args()
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ.setdefault(v, str(args.numpy_threads))
    import numpy as np
    import qchem_rs_amd as q
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import points_reference as PR
    if not q.device_ready():
        raise SystemExit("points_timing: no gfx950 device")
    peak_tflops, _ = q.measure_peaks()
    for mol, basis in SYSTEMS:
        m = q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"),
                                   q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))
        s = q.System(m)
        rng = np.random.default_rng(1)
        D = rng.standard_normal((s.n, s.n)) * 0.1
        D = 0.5 * (D + D.T)
        rec = s.esp_records()
        flops_pt = float(sum(int(rec[L]) * esp_flops_per_point_record(L) for L in range(7)))
        for label, n in SIZES:
            P = box(m, n) if n <= 100 else np.ascontiguousarray(box(m, 47)[:n])          # (n: points along an axis, or a count cut from 47^3)
            npts = len(P)
            row = {"system": f"{mol}/{basis}", "n": s.n, "points": label, "npts": npts, "records": [int(x) for x in rec],
                   "esp_flops_per_point": flops_pt}
            med, lo, hi = timed(lambda: s.density_on_points(D, P), args.reps)
            row.update(density_ms=med, density_ms_min=lo, density_ms_max=hi, density_phases_ms=s.points_timings().tolist())
            med, lo, hi = timed(lambda: s.esp_on_points(D, P), args.reps)
            ph = s.points_timings().tolist()
            row.update(esp_ms=med, esp_ms_min=lo, esp_ms_max=hi, esp_phases_ms=ph,
                       esp_point_records_per_s=npts * float(rec.sum()) / (med * 1e-3), esp_tflops_call=npts * flops_pt / (med * 1e-3) / 1e12,
                       esp_tflops_kernels=npts * flops_pt / (max(ph[2], 1e-9) * 1e-3) / 1e12, fp64_peak_tflops_measured=peak_tflops)
            if not args.skip_numpy and npts <= 200000:
                def ref():
                    phi = PR.phi(m, P)
                    return np.einsum("ka,ka->k", phi @ D, phi)
                med, lo, hi = timed(ref, max(1, min(args.reps, 3)))
                row.update(numpy_density_ms=med, numpy_threads=args.numpy_threads)
            print(json.dumps(row), flush=True)
        s.close()


if __name__ == "__main__":
    main()
