"""Before / after proof for a change of the work-list planner (run on the CPU, no GPU needed):
    python tools/plan_dump_ab.py <source tree> <out dir>
builds tests/host/plan_dump_main.cpp of THIS tree against <source tree>/qchem-rs_amd/csrc (qc_system.cpp, and qc_plan.cpp where the tree
has one) with the system C++ compiler and -fsanitize=address,undefined, runs it over the systems, shards and A/B switches below and
writes one line per combination - bytes and sha256 of the dump - to <out dir>/SUMMARY.txt.  Run it once per tree (a `git archive` of
the other commit will do) and compare the two summaries: equal lines = the pair table and every class, slot and bundle are equal entry
for entry.  --keep also stores each dump as <out dir>/<n>.txt for diffing."""
import hashlib, os, shutil, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_system

SYSTEMS = [("water", "STO-3G"), ("water", "cc-pVDZ"), ("water", "cc-pVTZ"), ("oxygen", "cc-pVTZ"), ("ethylene", "6-31G_st_st"),
           ("chloroform", "6-311++G_st_st"), ("benzene", "cc-pVDZ")]
SHARDS = [(0, 1), (1, 3), (7, 8)]
SWITCH_SYSTEMS = [("water", "cc-pVDZ"), ("water", "cc-pVTZ"), ("benzene", "cc-pVDZ")]
SWITCHES = ["QC_BM_PP_MIN=1", "QC_NO_BM_PP=1", "QC_NO_BM_PS4=1", "QC_MFMA4_MAX=0", "QC_NO_T1_MERGE=1", "QC_NO_BM_MERGE=1", "QC_BM_UNIT=0",
            "QC_BM_GAIN=100"]

args = [a for a in sys.argv[1:] if a != "--keep"]
keep = "--keep" in sys.argv
tree, out = os.path.abspath(args[0]), os.path.abspath(args[1])
os.makedirs(out, exist_ok=True)
csrc = os.path.join(tree, "qchem-rs_amd", "csrc")
rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
srcs = [os.path.join(csrc, f) for f in ("qc_system.cpp", "qc_plan.cpp") if os.path.exists(os.path.join(csrc, f))]
exe = os.path.join(out, "plan_dump_main")
subprocess.check_call([shutil.which("c++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", csrc, os.path.join(ROOT, "tests", "host", "plan_dump_main.cpp")]
                      + srcs + ["-o", exe, "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])

combos = [(m, b, r, n, s, "") for m, b in SYSTEMS for r, n in SHARDS for s in (0, 1)]
combos += [(m, b, 0, 1, 0, sw) for m, b in SWITCH_SYSTEMS for sw in SWITCHES]
env0 = {k: v for k, v in os.environ.items() if not k.startswith("QC_")}
with open(os.path.join(out, "SUMMARY.txt"), "w") as summary:
    for i, (mol, bas, rank, nranks, schwarz, sw) in enumerate(combos):
        inp = os.path.join(out, "%s_%s.in" % (mol, bas))
        if not os.path.exists(inp):
            m = load_system(mol, bas)
            with open(inp, "wb") as f:
                np.asarray([len(m.atoms), m.n_shells, len(m.exponents)], np.int32).tofile(f)
                for a in (m.atomic_numbers(), m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim):
                    np.asarray(a, np.int32).tofile(f)
                for a in (m.coordinates(), m.exponents, m.coefficients):
                    np.asarray(a, np.float64).tofile(f)
        env = dict(env0)
        if sw:
            env[sw.split("=")[0]] = sw.split("=")[1]
        p = subprocess.run([exe, inp, str(rank), str(nranks), str(schwarz)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        if p.returncode != 0:
            sys.exit("%s/%s rank %d/%d schwarz %d %s: exit %d\n%s" % (mol, bas, rank, nranks, schwarz, sw, p.returncode, p.stderr.decode()[-4000:]))
        if keep:
            with open(os.path.join(out, "%d.txt" % i), "wb") as f:
                f.write(p.stdout)
        line = "%-10s %-15s rank %d/%d schwarz %d %-18s %10d bytes sha256 %s" % (mol, bas, rank, nranks, schwarz, sw or "default", len(p.stdout), hashlib.sha256(p.stdout).hexdigest())
        print(line, flush=True)
        summary.write(line + "\n")
