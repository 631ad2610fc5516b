"""Phase stamps of qc_scf_small_kernel side by side, from the output of runs with libraries built with -DQC_SMALL_TIMING
(tools/build_variant_lib.sh NAME "-DQC_SMALL_TIMING" qc_scf_small), e.g. of water/cc-pVTZ, 15 passes:
    python tools/small_stamps.py parent=parent.log change=change.log
A launch prints "[small n=.. phases P m ..] stamps (10 ns): ...", one interval per phase.  Launches are grouped into kinds by their
phases and their number of intervals (a refinement pass adds four); per kind the median of every interval over its launches is
printed in microseconds, one column per log, the difference of the last to the first, and the sums."""
import re, statistics, sys
from collections import defaultdict

PRE = ["loads (+ zero fill)", "F D", "(F D) S", "error + dots", "DIIS solve | X", "combination", "F X", "X^T (F X)"]
PASS = ["A X, X^T A X, X^T X", "statistics + decisions", "update matrix", "X (I + E)"]
POST = ["start of post", "C, density", "energy sums + scalars"]


def labels(phases, count):
    out = list(PRE) if phases & 1 else []
    if phases & 2:
        out.append("start of refine")
        npass = (count - len(out) - 1 - (len(POST) if phases & 4 else 0)) // len(PASS)
        for k in range(npass): out += ["%s [pass %d]" % (l, k + 1) for l in PASS]
        out.append("sort + columns + C' out")
    if phases & 4: out += POST
    return out if len(out) == count else ["interval %d" % k for k in range(count)]


def read(path):
    kinds = defaultdict(list)
    for line in open(path):
        m = re.match(r"\[small n=(\d+) phases (\d+) m (\d+)\] stamps \(10 ns\):(.*)", line)
        if m:
            v = [int(x) / 100.0 for x in m.group(4).split()]
            kinds[(int(m.group(2)), len(v))].append(v)
    return kinds


if __name__ == "__main__":
    logs = [(n, read(p)) for n, p in (a.split("=", 1) for a in sys.argv[1:])]
    for kind in sorted(set().union(*[set(k) for _, k in logs])):
        counts = ", ".join("%s %d" % (n, len(k.get(kind, []))) for n, k in logs)
        print("phases %d, %d intervals (launches: %s), medians in us" % (kind + (counts,)))
        print("  %-38s" % "phase" + "".join("%10s" % n for n, _ in logs) + "      diff")
        med = [[statistics.median(col) for col in zip(*k[kind])] if kind in k else None for _, k in logs]
        for r, lab in enumerate(labels(*kind) + ["sum"]):
            row = [(sum(m) if lab == "sum" else m[r]) if m else float("nan") for m in med]
            print("  %-38s" % lab + "".join("%10.2f" % x for x in row) + "%10.2f" % (row[-1] - row[0]))
        print()
