"""bench.py's launch contract on the CPU: `python bench.py --gpus N` started plainly must start its own one-process-per-rank
launcher (before any GPU call), rendezvous, time, and relay exactly one JSON line from rank 0.  `--dry-run` swaps the GPU step
for the product's host-side shard planner; everything else is the path the GPU run takes.  One GPU test runs a plain single-GPU
benchmark and checks what --dump-outputs wrote."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, env_extra=None):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks_prints_one_line():
    d = _run(["--gpus", "2"])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["dry_run"] is True
    assert d["quartets_over_all_ranks"] == d["quartets_expected"] == 120          # the two shards cover H2O/STO-3G's quartets


def test_single_rank_runs_in_process():
    d = _run([])
    assert d["n_gpus"] == 1 and d["quartets_over_all_ranks"] == d["quartets_expected"]


def test_dry_run_line_fits_the_drivers_tail():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "2", "--warmup", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    last = [ln for ln in p.stdout.splitlines() if ln.strip()][-1]
    assert len(last) < 4096
    json.loads(last)


def test_compact_line_from_a_full_measurement_stays_under_4k():
    """The line the driver parses is built from everything `measure` collects; round 2's full record was 21.6 KB on one line and
    the driver's ~8 KB stdout tail cut its head off.  The canned record is that very line (profiles/r02_bench_default.json)."""
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r02_bench_default.json")))
    assert len(json.dumps(full)) > 8192                                  # the canned record is the oversized one
    full["roofline"]["peak_measured"] = 54.321; full["roofline"]["frac_of_measured"] = 0.04
    full["roofline"]["traffic_source"] = "profiles/r03_pmc_h2o_ccpvtz.json (committed rocprofv3 --pmc passes, not this run)"
    full["rccl"] = "x" * 500
    line = bench.compact_line(full, "bench_detail.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.MAX_LINE_BYTES == 4096
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "iter_breakdown_ms", "roofline", "cpu_baseline", "detail"):
        assert k in line, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel", "kernel_ms", "kernel_alg_bytes",
              "kernel_alg_flops", "other_roof", "peak_measured", "frac_of_measured"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample", "one_thread_value", "scf_iter_ms"):
        assert k in line["cpu_baseline"], k
    assert line["config"]["workload"].startswith("H2O/cc-pVTZ")
    assert len(line["scaling_reference"]) <= 12
    # nothing bulky leaks through
    for k in ("units_alone", "traffic_detail", "eigensolve_counters", "accumulation", "committed_counters"):
        assert k not in text
    # a pathological record still yields a line that fits: optional blocks are shed
    full["scaling_reference"]["workload"] = "y" * 5000
    assert len(json.dumps(bench.compact_line(full, "bench_detail.json"), separators=(",", ":"))) < 4096


def test_dump_outputs_writes_float64_arrays(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    outs = {"density": np.arange(9.0).reshape(3, 3), "rms": np.array([1e-11]), "orbital_energies": np.arange(3, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "out"), outs)
    for k, v in outs.items():
        a = np.load(tmp_path / "out" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape == v.shape and np.array_equal(a, v)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.MAX_DUMP_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run measures the headline only (nothing that --full adds), times exactly --steps steps, and --dump-outputs holds what the
    last of them computed: with 4 steps, pass 3 of an SCF run from the Hueckel guess, which a stepper of its own reproduces."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    env = dict(os.environ, QC_BENCH_DETAIL=str(tmp_path / "detail.json"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f64"
    assert d["config"]["passes"].startswith("SCF passes 0..3 of 1 run(s)")
    for k in ("cpu_baseline", "scaling_reference", "stored_mode", "cold_scf"):
        assert k not in d, k
    assert "peak_measured" not in d["roofline"]
    got = {k: np.load(out / (k + ".npy")) for k in ("electronic_energy", "rms", "density", "orbital_energies")}
    assert all(a.dtype == np.float64 for a in got.values())
    import qchem_rs_amd as q
    s = q.System(bench.load(q, "h2o_ccpvtz"))
    st = q.ScfStepper(s, stop_rule=bench.EPS)
    for _ in range(4):
        e, rms = st.iterate()
    assert abs(got["electronic_energy"][0] - e) < 1e-10 and abs(got["rms"][0] - rms) < 1e-10
    assert got["density"].shape == (s.n, s.n) and np.abs(got["density"] - st.density(0)).max() < 1e-10
    assert np.abs(got["orbital_energies"] - st.orbital_energies(0)).max() < 1e-10
    st.close(); s.close()
