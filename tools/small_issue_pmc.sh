# Issue, wait and instruction-fetch counters of qc_scf_small_kernel over the H2O/cc-pVTZ bench command, one library:
#   bash tools/small_issue_pmc.sh <out dir> [lib.so]
# Three counter runs of their own (no tracing beside them; the SQ block takes eight counters a run), restricted to that kernel.
# tools/small_issue_pmc.py turns the three directories into the summary of profiles/r17_small_issue_pmc.json.
O=$1; L=$2
R=$(cd "$(dirname "$0")/.." && pwd)
if [ -n "$L" ]; then export QCHEM_HIP_LIB=$L; fi
mkdir -p $O
run() {
  T=$1; shift
  timeout -k 10 240 rocprofv3 --pmc "$@" --kernel-include-regex qc_scf_small_kernel --output-format csv -d $O/$T -- \
      python $R/bench.py --gpus 1 --workload h2o_ccpvtz --no-extras --no-cpu-baseline --steps 30 --warmup 3 > $O/$T.json 2> $O/$T.err
}
run issue SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU &&
run insts SQ_WAVES SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_IFETCH SQ_IFETCH_LEVEL SQ_WAVE_CYCLES &&
run fetch SQ_WAVES SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES
