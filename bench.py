#!/usr/bin/env python3
"""bench.py - SCF-iteration time and ERI shell-quartet throughput of the MI355X Hartree-Fock path.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N = 1 runs in this process.  N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`
(one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), or started plainly - then this process,
before it touches any GPU, starts that launcher itself as a child, relays rank 0's JSON line and exits with the child's code.

A *step* is one pass of the SCF loop body (rhf.rs:67-88): direct-SCF Fock build over every unique shell quartet (ERI evaluation
+ J/K digestion), F = H + G, commutator, DIIS, F' = X^T F X, eigensolve, new density, energy, rms - through the step-wise C ABI
(`qc_scf_iterate`), all operands resident in HBM before the timed region starts.  The timed passes are the passes of REAL SCF
runs from the Hueckel guess: pass 0, 1, ... until the reference's stopping rule fires at epsilon = 1e-10, then the next run
starts again at pass 0 (the runs' set-up - one-electron integrals, S^-1/2, guess - happens before the clock starts).

Workloads (BASELINE.json configs; inputs are the fixture files under data/, nothing is random):
  N = 1  -> H2O / cc-pVTZ RHF (configs[2], the configuration the metric is quoted on; 58 bf, 32 131 unique quartets)
  N > 1  -> C6H6 / cc-pVDZ RHF (configs[4]): the class-sorted quartet list is dealt across the ranks, every rank digests its
            shard and the partial Fock matrices are summed by one RCCL all-reduce per build (strong scaling).  With --full the N = 1
            line carries the same workload's single-GPU numbers under "scaling_reference", and every N > 1 line under
            "same_workload_1gpu" (rank 0 times the unsharded workload on its own GPU before the sharded run, with the speed-up).
`value` = unique shell quartets enumerated per step x K / elapsed (max over ranks), whole job.  `ms_per_step` = SCF-iteration time.

A plain run does only what the headline needs: set-up, warm-up, the K timed steps and the JSON line, whose "roofline" (the Fock build:
hipEvent-timed inside the timed passes on the library's stream, binding roof first) is computed from those steps.  Everything that takes
runs of its own is behind --full: the measured FP64 / HBM peaks and every launch of a build timed alone (roofline), the accumulation A/B,
a cold SCF, the stored-tensor mode, the benzene scaling reference and, for N > 1, the same workload on one GPU, and "cpu_baseline" (the
oracle - a CPU restatement of the reference algorithm - on this host's cores).  --no-extras, --no-scaling-reference and --no-cpu-baseline
leave parts of that out again.

--dump-outputs DIR: after the timed steps, what the last timed step handed its caller (qc_scf_iterate's electronic energy and rms, the
state's density and orbital energies, float64) as DIR/<name>.npy.  The inputs are the fixture files, so two builds of the project run
with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "h2o_ccpvtz": ("water", "cc-pVTZ", "H2O/cc-pVTZ RHF"),
    "c6h6_ccpvdz": ("benzene", "cc-pVDZ", "C6H6/cc-pVDZ RHF"),
    "h2o_sto3g": ("water", "STO-3G", "H2O/STO-3G RHF"),
    "c6h6_631gss": ("benzene", "6-31G_st_st", "C6H6/6-31G** RHF"),
}
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
FP64_PEAK_TF = 78.6         # MI355X FP64 vector peak = FP64 matrix (MFMA) peak (MI355X_MICROARCH.md)
EPS = 1e-10                 # stopping rule of the timed SCF runs (the parity tests' epsilon)
PROFILE_ROUND = "r04"


def load(q, key):
    mol, basis, _ = WORKLOADS[key]
    b = q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json"))
    return q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", mol + ".json"), b)


class Host:
    """Host-side rendezvous of the ranks (barrier, max of the elapsed times, unique-id broadcast) over gloo: the GPUs' only
    collective is the library's RCCL all-reduce of the partial Fock matrix."""

    def __init__(self, world, torch, dist):
        self.world, self.torch, self.dist = world, torch, dist

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def max(self, x):
        if self.world == 1:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())


def timed_scf_passes(q, sysh, host, sync, steps, warmup, world_single=True):
    """`steps` timed passes of real SCF runs (see the module docstring); returns elapsed seconds, what the passes were and what the
    last of them computed."""
    # warm-up: one whole SCF run (code upload, stream tuning, Schwarz pass), at least `warmup` passes; it also tells how many
    # runs the timed region needs
    st = q.ScfStepper(sysh, stop_rule=EPS)
    kconv = None
    for k in range(max(warmup, 200)):
        _, rms = st.iterate()
        if kconv is None and rms < EPS:
            kconv = k
        if kconv is not None and k + 1 >= warmup:
            break
    frozen = st.counters()["assign_frozen"] > 0
    st.close()
    # The stream assignment of the build's launches is refined online from the passes' own build times (no tuner run, qc_fock.hip): more
    # untimed SCF runs until that search has ended (at most 40), so that the timed passes measure the steady state and not the search.
    # (multi-rank: every rank runs its own search on its shard; the decision to go on warming up is taken together - max over the ranks)
    warm_runs = 1
    while host.max(0.0 if frozen else 1.0) > 0.0 and warm_runs < 40:
        st = q.ScfStepper(sysh, stop_rule=EPS)
        for k in range((kconv + 1) if kconv is not None else 30):
            st.iterate()
        frozen = st.counters()["assign_frozen"] > 0
        st.close()
        warm_runs += 1
    sysh.freeze_assignment()          # (whatever the search has found by now stays: no instalment of it inside the timed passes)
    per_run = (kconv + 1) if kconv is not None else steps
    # (stop_rule: this loop ends a run once rms < EPS - said to the library, which issues each pass's successor build ahead of time and
    # can then empty the one queued behind a converging pass on the device instead of running it for nothing)
    runs = [q.ScfStepper(sysh, stop_rule=EPS) for _ in range((steps + per_run - 1) // per_run)]          # set-up outside the timed region
    host.barrier(); sync()
    t0 = time.perf_counter()
    done, cur, passes, restarts = 0, 0, [], 0
    k_in_run = 0
    while done < steps:
        e, rms = runs[cur].iterate()            # synchronises the library's stream at the end of every pass
        passes.append(k_in_run)
        done += 1; k_in_run += 1
        if rms < EPS and done < steps and cur + 1 < len(runs):
            cur += 1; k_in_run = 0; restarts += 1
    sync(); host.barrier()
    dt = host.max(time.perf_counter() - t0)
    cs = [r.counters() for r in runs]
    fock = sum(c["fock"] for c in cs) / max(1.0, sum(c["builds_timed"] for c in cs))          # hipEvent ms inside the passes
    linalg = sum(c["linalg"] for c in cs) / steps
    D = runs[0].density(0)
    outputs = {"electronic_energy": np.array([e]), "rms": np.array([rms]), "density": runs[cur].density(0),
               "orbital_energies": runs[cur].orbital_energies(0)}
    for r in runs:
        r.close()
    info = {"passes_timed": "SCF passes %s of %d run(s) from the Hueckel guess, stopping rule rms < %g (converges at pass %s)"
            % ("0..%d" % max(passes), restarts + 1, EPS, kconv), "converges_at_pass": kconv,
            "warmup_runs": warm_runs, "assignment_search_ended": bool(frozen),
            "speculative_builds": {"consumed": int(sum(c["spec_hits"] for c in cs)), "discarded": int(sum(c["spec_lost"] for c in cs)),
                                   "builds_timed": int(sum(c["builds_timed"] for c in cs))}}
    return dt, fock, linalg, D, info, outputs


_PEAKS = None


def measured_peaks(q):
    """Measured ceilings of this device (qc_measure_peaks: register-resident v_fma_f64 loop; 1 GiB streaming copy) - once per process,
    outside every timed region."""
    global _PEAKS
    if _PEAKS is None:
        _PEAKS = q.measure_peaks()
    return _PEAKS


def roofline_of(ws, fock_ms, n_launches, peaks=None):
    """Both roofs of the Fock build: t_roof = max(bytes_alg / BW_HBM, flops_alg / P_FP64); the binding one on top."""
    t = fock_ms * 1e-3
    gbs, tfs = ws.bytes_alg / t / 1e9, ws.flops_alg / t / 1e12
    t_hbm, t_fp = ws.bytes_alg / (HBM_PEAK_GBS * 1e9), ws.flops_alg / (FP64_PEAK_TF * 1e12)
    hbm = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}
    fp = {"bound": "fp64", "achieved": tfs, "peak": FP64_PEAK_TF, "unit": "TFLOP/s", "frac": tfs / FP64_PEAK_TF}
    if peaks:       # the same achieved figures against what a v_fma_f64 loop / a streaming copy reach on this device
        fp.update({"peak_measured": peaks[0], "frac_of_measured": tfs / peaks[0]})
        hbm.update({"peak_measured": peaks[1], "frac_of_measured": gbs / peaks[1]})
    top, other = (fp, hbm) if t_fp >= t_hbm else (hbm, fp)
    out = dict(top)
    out.update({
        "traffic": None,
        "other_roof": other,
        "t_roof_us": {"fp64": t_fp * 1e6, "hbm": t_hbm * 1e6},
        "kernel": "qc_fock_tier_kernel<LAB, TIER> + qc_fock_bm_kernel<LCD, HI>: %d concurrent launches = one Fock build" % n_launches,
        "kernel_ms": fock_ms,
        "kernel_ms_source": "hipEvents on the library's stream around the build of every timed pass (mean)",
        "kernel_quartets": int(ws.quartets), "kernel_alg_bytes": float(ws.bytes_alg), "kernel_alg_flops": float(ws.flops_alg),
        "note": "f64 gather-compute-scatter on the FP64 ridge; FP64 vector peak = FP64 MFMA peak = 78.6 TFLOP/s on this chip",
    })
    return out


def unit_profile(torch, q, sysh, D_host, reps):
    """Every launch of a build timed alone (hipEvents, serial) next to the concurrent build."""
    dD = torch.from_numpy(D_host).cuda()
    dG = torch.zeros_like(dD)
    torch.cuda.synchronize()
    tp = sysh.fock_profile_tiers(dD.data_ptr(), dG.data_ptr(), reps)
    units = [{"kernel": q.hf.unit_name(u), "ms_alone": float(tp["unit_ms"][u]), "quartets": int(tp["quartets"][u]),
              "alg_MB": float(tp["bytes"][u]) / 1e6, "alg_GF": float(tp["flops"][u]) / 1e9,
              "TFLOPs_alone": float(tp["flops"][u]) / (float(tp["unit_ms"][u]) * 1e-3) / 1e12}
             for u in range(len(tp["unit_ms"])) if tp["quartets"][u] > 0]
    return {"build_ms_standalone": float(tp["total_ms"]), "sum_units_serial_ms": float(tp["unit_ms"].sum()), "units_alone": units}


def committed_counters(key):
    """HBM traffic of the build and MFMA utilisation of the eigensolve from the rocprofv3 --pmc passes committed under profiles/
    (tools/run_pmc.sh + tools/make_pmc_summary.py; separate passes, corrected as MI355X_MICROARCH.md prescribes)."""
    for rnd in (PROFILE_ROUND, "r03"):          # (this round's set once tools/run_profiles.sh has written it)
        f = os.path.join(ROOT, "profiles", "%s_pmc_%s.json" % (rnd, key))
        if os.path.exists(f):
            try:
                d = json.load(open(f))
                d["_round"] = rnd
                return d
            except Exception:
                pass
    return None


def accumulation_ab(q, mol, passes=12):
    """Cost of the exact fixed-point accumulation next to plain f64 atomics: build time (hipEvents) over the same SCF passes.  Each mode
    first runs a whole SCF on its handle - the stream tuner and its second opinion finish there - and the sample is counted in builds
    that contained no tuner run (qc_scf_counters), so that the figure is the build and not the tuning."""
    out = {}
    for mode in ("fixed", "f64"):
        s = q.System(mol); s.set_accumulation(mode)
        warm = q.ScfStepper(s)
        for _ in range(16):
            warm.iterate()
        warm.close()
        s.freeze_assignment()
        st = q.ScfStepper(s)
        for _ in range(4):
            st.iterate()
        c0 = st.counters()
        for _ in range(passes):
            st.iterate()
        c1 = st.counters()
        out[mode] = (c1["fock"] - c0["fock"]) / max(1.0, c1["builds_timed"] - c0["builds_timed"])
        st.close(); s.close()
    return {"default": "fixed point (2 x 64-bit integer atomics per contribution: exact, order-independent, bitwise reproducible)",
            "fock_build_ms_fixed_point": out["fixed"], "fock_build_ms_f64_atomics": out["f64"],
            "cost_of_determinism": out["fixed"] / out["f64"] - 1.0}


def cold_scf(q, mol, eps=1e-10):
    """Time to solution of ONE cold `restricted_hartree_fock` call on a fresh handle (what the reference's CLI times, main.rs:79-101):
    handle creation (pair data on the host), device set-up (Schwarz pass, dispatch-lane probe, one-electron matrices, S^-1/2, guess),
    the stream tuner inside the first build, and the passes."""
    t0 = time.perf_counter()
    s = q.System(mol)
    t1 = time.perf_counter()
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, eps))
    t2 = time.perf_counter()
    s.close()
    t = out.timings_ms if out is not None else {}
    return {"wall_ms": (t2 - t0) * 1e3, "handle_ms": (t1 - t0) * 1e3, "ms_total": t.get("total"), "ms_setup": t.get("setup"),
            "ms_tuner": t.get("tuner"), "ms_fock": t.get("fock"), "ms_linalg": t.get("linalg"),
            "passes": (out.iterations + 1) if out is not None else None, "epsilon": eps,
            "note": "first call in a warm process (code objects loaded); ms_total = qc_scf_rhf as the library clocks it"}


def cpu_baseline(mol, budget_s=12.0):
    """The oracle (CPU restatement of the reference's conventional SCF) on this host: all cores (OpenMP over shell quartets) and
    one thread - the reference itself is single-threaded."""
    from oracle.oracle import Oracle
    o = Oracle(mol)
    nq = o.n_unique_quartets()
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(cores, 16)                 # a one-GPU lease of the pool owns 16 of the host's cores
    t0 = time.perf_counter(); _, c = o.eri_strided_mt(0, 50, 1, store=False); probe = time.perf_counter() - t0
    est_full = probe * nq / max(c, 1)
    stride1 = max(1, int(est_full / budget_s + 0.999))
    # (a small workload is repeated until the sample is a few seconds of CPU work: one pass over H2O/cc-pVTZ is 0.4 s on one thread)
    rep1 = max(1, int(0.4 * budget_s / max(est_full / stride1, 1e-3)))
    t0 = time.perf_counter()
    c1 = sum(o.eri_strided_mt(0, stride1, 1, store=False)[1] for _ in range(rep1)); dt1 = time.perf_counter() - t0
    stride_mt = max(1, int(est_full / cores / budget_s * 1.5 + 0.999))
    o.eri_strided_mt(0, max(stride_mt * 50, 50), cores, store=False)             # thread start-up outside the timing
    repm = max(1, int(0.4 * budget_s / max(est_full / cores / stride_mt, 1e-3)))
    t0 = time.perf_counter()
    cm = sum(o.eri_strided_mt(0, stride_mt, cores, store=False)[1] for _ in range(repm)); dtm = time.perf_counter() - t0
    out = {"value": cm / dtm, "unit": "shell-quartets/s", "cores": cores, "kind": "port",
           "sample": "%d x every %d-th of the %d unique shell quartets of the same workload (%d quartets, %.2f s) on %d threads, "
                     "oracle/qc_oracle.c orc_eri_full_strided_mt" % (repm, stride_mt, nq, cm, dtm, cores),
           "one_thread": {"value": c1 / dt1, "cores": 1, "sample": "%d x every %d-th quartet (%d quartets, %.2f s)" % (rep1, stride1, c1, dt1),
                          "note": "the reference is single-threaded: this is its configuration"}}
    if stride1 == 1 and o.n <= 64:
        # whole reference-style SCF on the CPU: n^4 contraction per iteration (rhf.rs:152-167) on the stored tensor
        I = o.eri()
        t0 = time.perf_counter(); r = o.rhf(100, EPS, eri=I); dt2 = time.perf_counter() - t0
        out["scf_iter_ms"] = dt2 * 1e3 / (r["iterations"] + 1)
        out["scf_note"] = "conventional SCF iteration (dense n^4 contraction + Jacobi eigensolve), one thread, tensor precomputed"
        # whole reference-style SCF: the tensor once on all threads (measured rate above) + the passes on one thread
        out["scf_whole_ms"] = nq / (cm / dtm) * 1e3 + dt2 * 1e3
        out["scf_whole_note"] = "ERI tensor on %d threads + %d passes on one thread (eps %g)" % (cores, r["iterations"] + 1, EPS)
    return out


def measure(torch, q, host, key, steps, warmup, world, rank, uid=None, with_units=True, with_peaks=True):
    mol = load(q, key)
    sysh = q.System(mol)
    if world > 1:
        sysh.comm_init(uid, rank, world)        # shard the quartet list, RCCL communicator for the partial-Fock all-reduce
    nq_total = sysh.n_quartets()
    dt, fock_ms, linalg_ms, D, info, outputs = timed_scf_passes(q, sysh, host, torch.cuda.synchronize, steps, warmup, world == 1)
    ws = sysh.work_stats()
    res = {
        "value": nq_total * steps / dt, "ms_per_step": dt * 1e3 / steps, "steps": steps,
        "n_basis": sysh.n, "unique_quartets": int(nq_total),
        "quartets_enumerated": int(ws.quartets_enumerated),
        "quartets_after_schwarz": int(ws.quartets_enumerated - ws.quartets_screened_out), "schwarz_tau": ws.schwarz_tau,
        "iter_breakdown_ms": {"fock_build": fock_ms, "diis_eig_density": linalg_ms},
        "timed": info,
    }
    res["roofline"] = roofline_of(ws, fock_ms, 0, measured_peaks(q) if with_peaks else None)
    if with_units:
        up = unit_profile(torch, q, sysh, D, reps=3)      # collective when sharded: every rank calls it
        res["roofline"]["kernel"] = "qc_fock_tier_kernel<LAB, TIER> + qc_fock_bm_kernel<LCD, HI>: %d concurrent launches = one Fock build" % len(up["units_alone"])
        res["roofline"]["n_launches"] = len(up["units_alone"])
        res["roofline"]["fock_build"] = up
    else:
        res["roofline"]["kernel"] = "qc_fock_tier_kernel<LAB, TIER> + qc_fock_bm_kernel<LCD, HI>: the concurrent launches of one Fock build"
    res["roofline"]["shard"] = "rank 0's shard of %d" % world if world > 1 else "all quartets"
    pmc = committed_counters(key)
    if pmc and world == 1:
        # PMC passes cannot run inside this process: these are the COMMITTED counters of the same workload (separate rocprofv3
        # --pmc runs, tools/run_profiles.sh), quoted with their source - not a measurement of this run
        src = "profiles/%s_pmc_%s.json (committed rocprofv3 --pmc passes, not this run)" % (pmc.get("_round", PROFILE_ROUND), key)
        res["roofline"]["traffic"] = pmc.get("fock_build_hbm_bytes")
        res["roofline"]["traffic_source"] = src
        res["committed_counters"] = {"source": src, "fock_build": pmc.get("fock_build"), "eigensolve": pmc.get("eigensolve")}
    sysh.close()
    return res, mol, outputs


MAX_LINE_BYTES = 4096      # the driver keeps an ~8 KB tail of stdout: the record must fit with room to spare
MAX_DUMP_BYTES = 64 << 20


def dump_outputs(path, outputs):
    """--dump-outputs: every array as float64 in `path`/<name>.npy (the whole outputs: about 100 KB at the largest workload)."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > MAX_DUMP_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes exceed the %d-byte limit" % (total, MAX_DUMP_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def _r(x, sig=6):
    """Numbers on the compact line carry `sig` significant digits (the detail file keeps everything)."""
    if isinstance(x, float):
        return float("%.*g" % (sig, x))
    return x


def _compact_roofline(rf):
    keep = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel_ms", "kernel_alg_bytes",
            "kernel_alg_flops", "peak_measured", "frac_of_measured")
    out = {k: _r(rf[k]) for k in keep if k in rf}
    out["kernel"] = "qc_fock_tier_kernel+qc_fock_bm_kernel (%s launches = 1 Fock build)" % rf.get("n_launches", "all")
    if "other_roof" in rf:
        o = rf["other_roof"]
        out["other_roof"] = {k: _r(o[k]) for k in ("bound", "achieved", "peak", "unit", "frac", "peak_measured", "frac_of_measured") if k in o}
    return out


def _compact_cpu(cb):
    out = {k: _r(cb[k]) for k in ("value", "unit", "cores", "kind") if k in cb}
    out["sample"] = cb.get("sample_short", cb.get("sample", ""))[:160]
    if "one_thread" in cb:
        out["one_thread_value"] = _r(cb["one_thread"]["value"])
    if "scf_iter_ms" in cb:
        out["scf_iter_ms"] = _r(cb["scf_iter_ms"])
    if "scf_whole_ms" in cb:
        out["scf_whole_ms"] = _r(cb["scf_whole_ms"])
    return out


def compact_line(full, detail_path=None):
    """The ONE stdout line the driver parses: the contract's keys only, < MAX_LINE_BYTES.  Everything else `measure` collects
    (launches timed alone, per-kernel counters, accumulation A/B, stored mode, the whole benzene block) is in the detail file."""
    line = {k: _r(full[k]) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                     "scaling", "vs_baseline", "dtype", "data") if k in full}
    cfg = full.get("config", {})
    line["config"] = {k: cfg[k] for k in ("workload", "n_basis", "unique_quartets", "quartets_after_schwarz", "passes", "parallelism")
                      if k in cfg}
    if "iter_breakdown_ms" in full:
        line["iter_breakdown_ms"] = {k: _r(v) for k, v in full["iter_breakdown_ms"].items()}
    if "roofline" in full:
        line["roofline"] = _compact_roofline(full["roofline"])
    if "cpu_baseline" in full:
        line["cpu_baseline"] = _compact_cpu(full["cpu_baseline"])
    sr = full.get("scaling_reference")
    if sr:
        rf = sr.get("roofline", {})
        line["scaling_reference"] = {
            "workload": sr["workload"], "n_gpus": sr["n_gpus"], "value": _r(sr["value"]), "ms_per_step": _r(sr["ms_per_step"]),
            "steps": sr["steps"], "converges_at_pass": sr.get("converges_at_pass"),
            "fock_build_ms": _r(sr["iter_breakdown_ms"]["fock_build"]), "diis_eig_density_ms": _r(sr["iter_breakdown_ms"]["diis_eig_density"]),
            "roofline_bound": rf.get("bound"), "roofline_frac": _r(rf.get("frac")),
        }
        if "cpu_baseline" in sr:
            line["scaling_reference"]["cpu_value"] = _r(sr["cpu_baseline"]["value"])
    if "stored_mode" in full:
        sm = full["stored_mode"]
        line["stored_mode"] = {"ms_per_step": _r(sm["ms_per_step"]), "gemv_GBs": _r(sm["gemv_GBs"])}
    if "rccl" in full:
        line["rccl"] = str(full["rccl"])[:120]
    if "same_workload_1gpu" in full:
        line["same_workload_1gpu"] = {k: _r(v) for k, v in full["same_workload_1gpu"].items()}
    if "cold_scf" in full:
        line["cold_scf"] = {k: _r(v, 4) for k, v in full["cold_scf"].items() if k in ("wall_ms", "ms_total", "ms_setup", "ms_tuner", "passes")}
    if detail_path:
        line["detail"] = detail_path
    # never hand the driver a line it cannot keep: shed optional blocks one by one, measuring again after each, then cut the strings
    size = lambda: len(json.dumps(line, separators=(",", ":")))
    for k in ("stored_mode", "same_workload_1gpu", "rccl", "cold_scf", "scaling_reference"):
        if size() < MAX_LINE_BYTES:
            break
        line.pop(k, None)
    if size() >= MAX_LINE_BYTES and "roofline" in line:
        line["roofline"].pop("other_roof", None)
        line["roofline"]["traffic_source"] = str(line["roofline"].get("traffic_source", ""))[:40]
    if size() >= MAX_LINE_BYTES:
        if "cpu_baseline" in line:
            line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:40]
        line["config"]["passes"] = str(line["config"].get("passes", ""))[:40]
        line["data"] = str(line.get("data", ""))[:40]
    assert size() < MAX_LINE_BYTES, size()
    return line


def self_launch(args):
    """`python bench.py --gpus N` started plainly: become the launcher's parent (no GPU call has happened in this process)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = None
    for ln in p.stdout.splitlines():
        try:
            d = json.loads(ln)
            if isinstance(d, dict) and "metric" in d:
                line = ln
                continue
        except ValueError:
            pass
        print(ln, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    sys.exit(p.returncode if p.returncode else (0 if line is not None else 1))


def dry_run(args, world, rank):
    """Harness test without a GPU (tests/test_bench_launch.py): same launch, rendezvous, timing and JSON path; a step is the
    product's host-side shard planner instead of the kernels.  Not a measurement."""
    import torch
    import torch.distributed as dist
    import qchem_rs_amd as q
    if world > 1:
        dist.init_process_group("gloo")
    host = Host(world, torch, dist)
    sysh = q.System(load(q, "h2o_sto3g"))
    for _ in range(args.warmup):
        sysh.plan_shard(rank, world)
    host.barrier()
    t0 = time.perf_counter()
    mine = 0
    for _ in range(args.steps):
        mine = sysh.plan_shard(rank, world)[0]
    host.barrier()
    dt = host.max(time.perf_counter() - t0)
    tot = torch.tensor([mine], dtype=torch.int64)
    if world > 1:
        dist.all_reduce(tot)
    if rank == 0:
        print(json.dumps({"metric": "DRY RUN (no GPU): bench.py launch/rendezvous harness test, not a measurement", "value": 0.0,
                          "unit": "shell-quartets/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": dt * 1e3 / args.steps, "dry_run": True, "quartets_over_all_ranks": int(tot.item()),
                          "quartets_expected": int(sysh.n_quartets())}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)      # (two whole SCF runs of the headline workload: passes 0..14 twice)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="auto", choices=["auto"] + sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true", help="also everything beyond the headline (module docstring): peaks, per-launch "
                    "profile, accumulation A/B, cold SCF, stored mode, scaling reference, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--no-scaling-reference", action="store_true", help="with --full: no scaling reference / one-GPU run of the workload")
    ap.add_argument("--no-extras", action="store_true", help="with --full: only the headline measurement and the measured peaks (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--dry-run", action="store_true", help="harness test without a GPU (not a measurement)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)                                  # never returns
    if args.gpus != world:
        raise SystemExit("bench.py --gpus %d inside a launcher with WORLD_SIZE=%d" % (args.gpus, world))
    if args.dry_run:
        return dry_run(args, world, rank)

    import torch
    import torch.distributed as dist
    import qchem_rs_amd as q

    if not torch.cuda.is_available() or not q.device_ready():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    uid = None
    if world > 1:
        dist.init_process_group("gloo")                    # host-side rendezvous only
        box = [q.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        uid = box[0]
    host = Host(world, torch, dist)

    key = args.workload if args.workload != "auto" else ("h2o_ccpvtz" if world == 1 else "c6h6_ccpvdz")
    same_workload_1gpu = None
    if world > 1 and args.full and not args.no_scaling_reference:
        # The N = 1 line of this benchmark is H2O/cc-pVTZ (the configuration the metric is quoted on), the N > 1 lines are the sharded
        # benzene workload: rank 0 first times the SAME workload unsharded on its own GPU (outside the timed region, the other ranks wait),
        # so that every multi-GPU line carries the single-GPU figure its speed-up is measured against.
        if rank == 0:
            # (bounded: the other ranks sit in the barrier below meanwhile)
            r1, _, _ = measure(torch, q, Host(1, torch, dist), key, max(8, min(args.steps, 12)), 2, 1, 0, None, with_units=False)
            same_workload_1gpu = {"workload": WORKLOADS[key][2] + " direct-SCF iteration", "n_gpus": 1, "value": r1["value"],
                                  "ms_per_step": r1["ms_per_step"], "fock_build_ms": r1["iter_breakdown_ms"]["fock_build"],
                                  "diis_eig_density_ms": r1["iter_breakdown_ms"]["diis_eig_density"]}
        host.barrier()
    res, mol, outputs = measure(torch, q, host, key, args.steps, args.warmup, world, rank, uid,
                                with_units=args.full and not args.no_extras, with_peaks=args.full)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs)
    line = {
        "metric": "ERI shell-quartets/sec through one SCF iteration (ms_per_step = SCF iter time), RHF",
        "value": res["value"], "unit": "shell-quartets/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": res["ms_per_step"], "higher_is_better": True,
        "scaling": "strong" if world > 1 else "weak", "vs_baseline": None, "dtype": "f64",
        "data": "fixture molecule + basis files under data/ (no randomness); densities are the SCF's own iterates from the Hueckel guess",
        "config": {"workload": WORKLOADS[key][2] + " direct-SCF iteration", "n_basis": res["n_basis"], "unique_quartets": res["unique_quartets"],
                   "quartets_after_schwarz": res["quartets_after_schwarz"], "schwarz_tau": res["schwarz_tau"],
                   "passes": res["timed"]["passes_timed"], "spec": res["timed"].get("speculative_builds"),
                   "parallelism": "1 GPU" if world == 1 else "quartet shards over %d GPUs + 1 RCCL all-reduce of G per build" % world},
        "iter_breakdown_ms": res["iter_breakdown_ms"],
        "roofline": res["roofline"],
    }
    if "committed_counters" in res:
        line["committed_counters"] = res["committed_counters"]
    if world > 1 and rank == 0:
        line["rccl"] = q.rccl_info()
        if same_workload_1gpu:
            same_workload_1gpu["speedup"] = res["value"] / same_workload_1gpu["value"]
            line["same_workload_1gpu"] = same_workload_1gpu
    if world == 1 and args.full and not args.no_extras:
        line["accumulation"] = accumulation_ab(q, mol)
        line["cold_scf"] = cold_scf(q, mol, EPS)
        if not args.no_scaling_reference and key == "h2o_ccpvtz":
            k2 = max(8, min(args.steps, 24))
            r2, m2, _ = measure(torch, q, host, "c6h6_ccpvdz", k2, 2, 1, 0, None, with_units=True)
            line["scaling_reference"] = {"workload": WORKLOADS["c6h6_ccpvdz"][2] + " direct-SCF iteration", "n_gpus": 1,
                                         "value": r2["value"], "ms_per_step": r2["ms_per_step"], "steps": k2,
                                         "passes": r2["timed"]["passes_timed"], "converges_at_pass": r2["timed"]["converges_at_pass"],
                                         "iter_breakdown_ms": r2["iter_breakdown_ms"], "unique_quartets": r2["unique_quartets"],
                                         "quartets_after_schwarz": r2["quartets_after_schwarz"], "roofline": r2["roofline"],
                                         "accumulation": accumulation_ab(q, m2, passes=8)}
            if "committed_counters" in r2:
                line["scaling_reference"]["committed_counters"] = r2["committed_counters"]
            if not args.no_cpu_baseline:      # the oracle on a bounded sample of the same 1.1 M quartets
                line["scaling_reference"]["cpu_baseline"] = cpu_baseline(m2, budget_s=6.0)
        if key in ("h2o_ccpvtz", "h2o_sto3g", "c6h6_ccpvdz"):
            # the reference's own (conventional) algorithm on the same GPU: tensor resident in HBM, one streaming GEMV per pass
            s3 = q.System(mol); s3.set_fock_mode("stored")
            st3 = q.ScfStepper(s3)
            for _ in range(3):
                st3.iterate()
            t0 = st3.timings(); w0 = time.perf_counter()
            for _ in range(args.steps):
                st3.iterate()
            dt3 = time.perf_counter() - w0
            t1 = st3.timings(); n3 = s3.n
            gemv_bytes = 8.0 * (n3 * (n3 + 1) // 2) * n3 * n3
            fock_ms3 = (t1["fock"] - t0["fock"]) / args.steps
            line["stored_mode"] = {"ms_per_step": dt3 * 1e3 / args.steps, "tensor_build_ms": st3.tensor_ms(),
                                   "gemv_ms": fock_ms3, "gemv_alg_bytes": gemv_bytes,
                                   "gemv_GBs": gemv_bytes / (fock_ms3 * 1e-3) / 1e9, "gemv_frac_of_8TBs": gemv_bytes / (fock_ms3 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                   "note": "rhf.rs:45,58-62,152-167 as written: molint::eri once, electron_terms, dense n^4 contraction per pass; "
                                           "the headline value above is the direct-SCF path the north star asks for"}
            st3.close(); s3.close()
        if not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(mol)
    if rank == 0:
        detail = os.environ.get("QC_BENCH_DETAIL", os.path.join(ROOT, "bench_detail.json"))
        try:
            with open(detail, "w") as f:
                json.dump(line, f, indent=1)
        except OSError as e:                      # read-only checkout: the compact line is what counts
            print("bench.py: cannot write %s: %s" % (detail, e), file=sys.stderr)
            detail = None
        print(json.dumps(compact_line(line, os.path.relpath(detail, ROOT) if detail else None), separators=(",", ":")), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
