#!/bin/bash
# The tracker's output stage, from one box and one invocation:
#   bash profiles/collect_tracker_output.sh r05 [outdir]
# 1. python3 benchmarks/bench_tracker_output.py --reps 5   -> <tag>_tracker_output.json
# 2. the same with --reps 3 under rocprofv3 --kernel-trace --stats
#        -> <tag>_tracker_output_kernel_stats.csv, <tag>_tracker_output_under_rocprof.json
# Every GPU step has its own time limit and the chain stops at the first failure.
set -o pipefail
tag=${1:-r05}
R=${2:-profiles}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
W=$(mktemp -d)
mkdir -p "$R"
timeout -k 10 420 python3 benchmarks/bench_tracker_output.py --reps 5 > "$R/${tag}_tracker_output.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$W/prof" -- python3 benchmarks/bench_tracker_output.py --reps 3 > "$R/${tag}_tracker_output_under_rocprof.json" 2> "$W/rocprof.log" &&
cp "$(find "$W/prof" -name '*kernel_stats.csv' | head -1)" "$R/${tag}_tracker_output_kernel_stats.csv"
rc=$?
rm -rf "$W"
exit $rc
