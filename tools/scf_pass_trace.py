"""Launch-for-launch A/B of two library builds over four forms of an SCF pass (cases of record_small_bits.PASS_CASES): the sequence of
kernel names per queue of a rocprofv3 kernel trace must be the same.  On the GPU box, one trace per case and library (no counters in it):
    for c in $(python tools/scf_pass_trace.py cases); do
        QCHEM_HIP_LIB=<lib> rocprofv3 --kernel-trace --output-format csv -d traces/<tag>/$c -- python tools/scf_pass_trace.py run $c
    done
then    python tools/scf_pass_trace.py cmp traces/<tagA> traces/<tagB>
Queues are matched by the order of their first dispatch (their ids differ from process to process); within a queue, dispatch order.
The launch units of a Fock build (qc_fock_tier* / qc_fock_bm_kernel) are dealt to the queues from the times the process measured, so
two runs of ONE library can place them differently: where the full sequences differ, they are compared again without those kernels,
which leaves every launch of the SCF driver, the build's set-up and fold, the joins and the copies."""
import csv
import glob
import os
import re
import sys

CASES = ("c2h4_uhf_generic", "h2o_tz_uhf", "h2o_tz_generic_repeat", "c2h4_dz_comm")


def queues(case_dir):
    """[[kernel name, ...] per queue], queues in the order of their first dispatch"""
    files = glob.glob(os.path.join(case_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (case_dir, files)
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    per = {}
    for r in rows:
        per.setdefault((r.get("Agent_Id", ""), r["Queue_Id"]), []).append(r["Kernel_Name"])
    return list(per.values())


def without_units(qs):
    return [[k for k in q if not re.search(r"qc_fock_(tier|bm)", k)] for q in qs]


def main():
    if sys.argv[1] == "cases":
        print(" ".join(CASES))
    elif sys.argv[1] == "run":
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import record_small_bits as rec
        r = rec.run_case(sys.argv[2])
        print(sys.argv[2], "passes", r["passes"], "redos", r["redos"], "E", float.fromhex(r["energy"][-1]))
    else:
        bad = 0
        for c in CASES:
            a, b = queues(os.path.join(sys.argv[2], c)), queues(os.path.join(sys.argv[3], c))
            head = "%-24s queues %d / %d  launches per queue %s / %s  " % (c, len(a), len(b), [len(x) for x in a], [len(x) for x in b])
            verdict = "same sequence of kernel names on every queue"
            if a != b:
                a, b = without_units(a), without_units(b)
                verdict = ("build units placed differently; without them %s launches, the same sequence on every queue" % [len(x) for x in a]
                           if a == b else "DIFFERENT")
            bad += a != b
            print(head + verdict)
            for qa, qb in zip(a, b):
                d = [i for i, (x, y) in enumerate(zip(qa, qb)) if x != y]
                if d:
                    print("    first difference at launch %d of a queue: %s | %s" % (d[0], qa[d[0]][:60], qb[d[0]][:60]))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
