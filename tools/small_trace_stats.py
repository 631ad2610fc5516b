"""qc_scf_small_kernel in rocprofv3 --kernel-trace output of the H2O/cc-pVTZ bench command (--steps 30 --warmup 3):
    python tools/small_trace_stats.py [--last 40] name=dir [name=dir ...]
One line per directory: the launches of all instances of the kernel over the timed passes (the last 40: 20 warm passes of one launch,
10 cold ones of two) with their mean, minimum, maximum and total duration in microseconds, then the number and mean of all launches."""
import csv, glob, os, sys


def launches(d):
    out = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "qc_scf_small_kernel" in r["Kernel_Name"]:
                out.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    return [us for _, us in sorted(out)]


if __name__ == "__main__":
    args = sys.argv[1:]
    last = int(args.pop(args.index("--last") + 1)) if "--last" in args else 40
    for name, d in (a.split("=", 1) for a in args if a != "--last"):
        v = launches(d)
        s = v[-last:]
        print('%s: "qc_scf_small_kernel",%d,%.2f,%.2f,%.2f,%.1f,%d,%.2f' % (name, len(s), sum(s) / len(s), min(s), max(s), sum(s), len(v), sum(v) / len(v)))
