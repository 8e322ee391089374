#!/bin/bash
# Same-box A/B of the in-step re-bucket of the processing order (TTL_ORDER_INSTEP,
# DESIGN 3.2) against an older checkout under _ab/<name> (built there), all runs
# alternating on one box:
#   1. period sweep: plain `python bench.py` (one 12-step window from a fresh reset;
#      then 20 steps after 5 of warm-up), the parent and this tree at P = 0..4 in
#      turn, ROUNDS times;
#   2. rocprofv3 --kernel-trace --stats of the headline leg: the parent, this tree at
#      its default, at P = 1 and P = 2, and P = 2 with the scatter behind the gather;
#   3. `--full --legs weak,shapes` (whole episode and the other shapes), twice each.
#   bash benchmarks/instep_ab.sh parent 5 > profiles/r05_instep_ab.log
# Every GPU step runs under its own time limit; the script stops at the first
# step that does not end cleanly.
name=${1:-parent}
rounds=${2:-5}
cd "$(dirname "$0")/.."
ROOT=$PWD
A=$ROOT/_ab/$name
tmp=$(mktemp -d)
export TMPDIR=/tmp

one() { # tag dir P bench-args...: one plain bench.py run, one line
  local tag=$1 dir=$2 P=$3; shift 3
  ( cd $dir; [ -n "$P" ] && export TTL_ORDER_INSTEP=$P
    timeout -k 10 200 python bench.py "$@" 2>/dev/null | tail -1 > $tmp/one.json )
  local rc=$?
  [ $rc = 0 ] || { echo "$tag: rc=$rc, stopping"; exit 1; }
  python3 -c "import json; d=json.load(open('$tmp/one.json')); print('%-8s %s  %7.1f M  %6.1f us/step' % ('$tag', '$*', d['value']/1e6, d['ms_per_step']*1e3))"
}

echo "# 1. period sweep ($rounds rounds, alternating)"
for args in "--steps 12 --warmup 3" "--steps 20 --warmup 5"; do
  for r in $(seq 1 $rounds); do
    one parent $A "" $args || exit 1
    for P in 0 1 2 3 4; do one P=$P $ROOT $P $args || exit 1; done
  done
done

stats() { # tag dir env...: kernel stats of the headline leg
  local tag=$1 dir=$2; shift 2
  ( cd $dir; for kv in "$@"; do export $kv; done
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $tmp/prof_$tag -- \
      python3 bench.py --full --no-cpu-baseline --no-whole-episode --legs weak > $tmp/$tag.json 2> $tmp/$tag.log )
  local rc=$?
  [ $rc = 0 ] || { echo "$tag: rc=$rc, stopping"; tail -5 $tmp/$tag.log; exit 1; }
  python3 - "$(find $tmp/prof_$tag -name '*kernel_stats.csv' | head -1)" $tmp/$tag.json "$tag" <<'PY'
import csv, json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('%s: %.1f M under the profiler' % (sys.argv[3], d['value'] / 1e6))
for r in csv.DictReader(open(sys.argv[1])):
    n = r['Name'].replace('(anonymous namespace)::', '').replace('void ', '')
    if n.startswith(('k_state_dd', 'k_tail', 'k_order_scatter', 'k_advance', 'k_scripted')):
        print('   %-36s calls %5s  avg %8.2f us' % (n.split('(')[0], r['Calls'], float(r['AverageNs']) / 1e3))
PY
  rm -rf $tmp/prof_$tag
}

echo "# 2. kernel stats, headline leg"
stats parent $A || exit 1
stats tree_default $ROOT || exit 1
stats tree_P1 $ROOT TTL_ORDER_INSTEP=1 || exit 1
stats tree_P2 $ROOT TTL_ORDER_INSTEP=2 || exit 1
stats tree_P2_scatter_behind_gather $ROOT TTL_ORDER_INSTEP=2 TTL_ORDER_INSTEP_AFTER=1 || exit 1
stats tree_P0 $ROOT TTL_ORDER_INSTEP=0 || exit 1

full() { # tag dir
  local tag=$1 dir=$2
  ( cd $dir; timeout -k 10 600 python bench.py --full --no-cpu-baseline --legs weak,shapes 2>/dev/null | tail -1 > $tmp/full.json )
  local rc=$?
  [ $rc = 0 ] || { echo "full $tag: rc=$rc, stopping"; exit 1; }
  python3 - $tmp/full.json $tag <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
w = d['windows']
print('%-8s headline %.1f M (windows %.1f .. %.1f)' % (sys.argv[2], d['value'] / 1e6, w['value_min'] / 1e6, w['value_max'] / 1e6))
we = d.get('whole_episode') or {}
print('   whole_episode ' + '  '.join('%s %.1f M' % (k, v / 1e6) for k, v in we.items()
                                      if isinstance(v, float) and v > 1e6))
for k, v in (d.get('other_shapes') or {}).items():
    if isinstance(v, dict) and 'value' in v:
        print('   %-18s %8.1f M (windows %.1f .. %.1f)' % (k, v['value'] / 1e6, v['value_min'] / 1e6, v['value_max'] / 1e6))
PY
}

echo "# 3. --full --legs weak,shapes"
for r in 1 2; do
  full parent $A || exit 1
  full tree $ROOT || exit 1
done
rm -rf $tmp
