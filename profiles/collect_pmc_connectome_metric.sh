#!/bin/bash
# Counter passes over the connectome's two per-row kernels: what bounds
# k_tract_sample_mean, and k_connectome_assign beside it on the same rows.
#   bash profiles/collect_pmc_connectome_metric.sh [outdir]
# One rocprofv3 --pmc pass per SQ group (counters only, no tracing beside them) over the kernel
# legs of benchmarks/bench_connectome_metric.py at 3 repetitions; per-kernel averages ->
# <outdir>/connectome_metric_pmc.txt.  Every pass has its own time limit and the chain stops
# at the first one that fails.  A pass over the GRBM busy counters aborted inside the profiler
# and is not made; the cache counters (TCP, TCC) were not tried.
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
R=${1:-profiles}
W=$(mktemp -d)
mkdir -p "$R"
OUT=$R/connectome_metric_pmc.txt
: > "$OUT"
i=0
while read -r group; do
  [ -z "$group" ] && continue
  i=$((i+1))
  echo "## pass $i: $group" >> "$OUT"
  timeout -k 10 180 rocprofv3 --pmc $group --output-format csv -d "$W/p$i" -- \
    python3 benchmarks/bench_connectome_metric.py --legs kernels --reps 3 > /dev/null 2> "$W/p$i.log" \
    || { echo "pass $i failed" >> "$OUT"; tail -5 "$W/p$i.log" >> "$OUT"; rm -rf "$W"; exit 1; }
  for k in k_tract_sample_mean k_connectome_assign; do
    python3 profiles/pmc_any.py "$W/p$i" $k >> "$OUT" 2>&1
  done
  rm -rf "$W/p$i"
done <<'GROUPS'
SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_WAVES
SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_INST_LEVEL_VMEM
GROUPS
rm -rf "$W"
wc -l "$OUT"
