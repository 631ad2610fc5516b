"""Summary of the counter runs of tools/small_issue_pmc.sh for qc_scf_small_kernel:
    python tools/small_issue_pmc.py name=dir [name=dir ...] > profiles/r17_small_issue_pmc.json
Every dispatch of the kernel is one workgroup of four waves.  The dispatches are sorted into launch kinds by their vector-memory reads
and their LDS instructions (launches of different phases, DIIS windows and numbers of refinement passes differ in one of the two; a
kind is the set of dispatches that agree in both within 1 %), and per kind and counter the median over its dispatches is given, then
the derived figures: instructions per wave, clocks per instruction, the active / waiting / issue-stalled shares of the wave's cycles,
fetch requests, misses and the mean fetch latency (level / fetches).  The SQ cycle counters (SQ_WAVE_CYCLES, SQ_BUSY_CYCLES, SQ_WAIT_*,
SQ_ACTIVE_INST_*) count units of four clocks, summed over the waves: a launch of 78 us shows 4 x 46 400 of them.
"Instructions" is the sum of the six SQ_INSTS_* classes collected (VALU, SALU, SMEM, LDS, VMEM_RD, VMEM_WR): branches, s_waitcnt, s_nop
and barriers are in none of them, so the true count is higher and clocks per instruction lower than given (the static mix of
tools/isa_mix.py has one branch, wait or nop for every six other instructions)."""
import csv, glob, json, os, statistics, sys
from collections import defaultdict


def dispatches(d):
    """{dispatch id: {counter: value}} of one run's counter_collection csv (values of a counter summed over its rows of a dispatch)."""
    out = defaultdict(lambda: defaultdict(float))
    for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "qc_scf_small_kernel" in r["Kernel_Name"]:
                out[int(r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
    return out


def summarise(d):
    runs = {t: dispatches(os.path.join(d, t)) for t in ("issue", "insts", "fetch")}
    # the n-th dispatch of the kernel is the same launch in every run (the bench command is deterministic)
    order = {t: sorted(v) for t, v in runs.items()}
    nd = min(len(o) for o in order.values())
    rows = []
    for k in range(nd):
        row = {}
        for t in runs:
            row.update(runs[t][order[t][k]])
        rows.append(row)
    kinds = []                                                           # [(representative reads, [rows])]
    for row in rows:
        rd = (row["SQ_INSTS_VMEM_RD"], row["SQ_INSTS_LDS"])
        for rep, members in kinds:
            if all(abs(x - y) <= 0.01 * y for x, y in zip(rd, rep)):
                members.append(row); break
        else:
            kinds.append((rd, [row]))
    out = {"dispatches": nd, "kinds": [],
           "note": "instructions_per_wave sums SQ_INSTS_VALU, SALU, SMEM, LDS, VMEM_RD, VMEM_WR only: branches, waits, nops and barriers are not counted, "
                   "so clocks_per_instruction is an upper bound; cycle counters are units of four clocks"}
    for rep, members in sorted(kinds, key=lambda x: -len(x[1])):
        med = {c: statistics.median(m[c] for m in members) for c in members[0]}
        waves = med["SQ_WAVES"] or 4.0
        insts = sum(med[c] for c in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR"))
        wc = med["SQ_WAVE_CYCLES"]
        der = {"instructions_per_wave": insts / waves, "clocks_per_wave": 4.0 * wc / waves,
               "clocks_per_instruction": 4.0 * wc / insts if insts else None,
               "active_share": med["SQ_ACTIVE_INST_ANY"] / wc if wc else None, "wait_any_share": med["SQ_WAIT_ANY"] / wc if wc else None,
               "wait_inst_any_share": med["SQ_WAIT_INST_ANY"] / wc if wc else None,
               "ifetch_requests": med["SQ_IFETCH"], "ifetch_mean_latency_clocks": 4.0 * med["SQ_IFETCH_LEVEL"] / med["SQ_IFETCH"] if med["SQ_IFETCH"] else None,
               "icache_requests": med["SQC_ICACHE_REQ"], "icache_misses": med["SQC_ICACHE_MISSES"],
               "icache_miss_share": med["SQC_ICACHE_MISSES"] / med["SQC_ICACHE_REQ"] if med["SQC_ICACHE_REQ"] else None}
        out["kinds"].append({"dispatches": len(members), "median_counters": med, "derived": der})
    return out


if __name__ == "__main__":
    print(json.dumps({n: summarise(d) for n, d in (a.split("=", 1) for a in sys.argv[1:])}, indent=1))
