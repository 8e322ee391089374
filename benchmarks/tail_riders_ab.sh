#!/bin/bash
# Same-box A/B of the gather launch's riders (TTL_TAIL_RIDERS) against
# the parent checkout under _ab/<name> (built there), all runs alternating on one box,
# by the method of instep_ab.sh:
#   1. plain `python bench.py` (12 steps after 3 of warm-up) and `--steps 20 --warmup 5`:
#      the parent, this tree, and this tree with TTL_TAIL_RIDERS=0, in turn, ROUNDS times;
#   2. rocprofv3 --kernel-trace --stats of the headline leg: the parent, this tree at its
#      default, with the order scatter riding alone (TTL_TAIL_RIDERS=2) and with no rider;
#   3. `--full --legs weak,shapes` and `--legs hbm`, twice per tree;
#   4. the re-bucket period again, now that the scatter is off the chain: this tree at
#      TTL_ORDER_INSTEP = 1, 2, 3 in turn, ROUNDS times, at 12 and at 20 steps.
#   bash benchmarks/tail_riders_ab.sh parent 5 1234 > profiles/tail_riders_ab.log
# SECTIONS (third argument) picks among 1, 2, 3, 4.  With TTL_AB_SECONDS set, section 1
# starts no round that would not end inside that many seconds, and says so.
# Every GPU step runs under its own time limit; the script stops at the first step
# that does not end cleanly.
name=${1:-parent}
rounds=${2:-5}
sections=${3:-1234}
cd "$(dirname "$0")/.."
ROOT=$PWD
A=$ROOT/_ab/$name
tmp=$(mktemp -d)
export TMPDIR=/tmp
t0=$(date +%s)

one() { # tag dir riders bench-args...: one plain bench.py run, one line
  local tag=$1 dir=$2 R=$3; shift 3
  ( cd $dir; [ -n "$R" ] && export TTL_TAIL_RIDERS=$R; [ -n "$PERIOD" ] && export TTL_ORDER_INSTEP=$PERIOD
    timeout -k 10 200 python bench.py "$@" 2>/dev/null | tail -1 > $tmp/one.json )
  local rc=$?
  [ $rc = 0 ] || { echo "$tag: rc=$rc, stopping"; exit 1; }
  python3 -c "import json; d=json.load(open('$tmp/one.json')); print('%-10s %s  %7.1f M  %6.1f us/step' % ('$tag', '$*', d['value']/1e6, d['ms_per_step']*1e3))"
}

if [[ $sections == *1* ]]; then
  echo "# 1. parent / tree / tree with TTL_TAIL_RIDERS=0 ($rounds rounds, alternating)"
  for r in $(seq 1 $rounds); do
    r0=$(date +%s)
    for args in "--steps 12 --warmup 3" "--steps 20 --warmup 5"; do
      one parent $A "" $args || exit 1
      one tree $ROOT "" $args || exit 1
      one riders=0 $ROOT 0 $args || exit 1
    done
    now=$(date +%s)
    if [ -n "$TTL_AB_SECONDS" ] && [ $((now - t0 + now - r0)) -gt "$TTL_AB_SECONDS" ]; then
      echo "# stopped after round $r of $rounds: the next would not end inside $TTL_AB_SECONDS s"
      break
    fi
  done
fi

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

if [[ $sections == *2* ]]; then
  echo "# 2. kernel stats, headline leg"
  stats parent $A || exit 1
  stats tree_default $ROOT || exit 1
  stats tree_scatter_rider_only $ROOT TTL_TAIL_RIDERS=2 || exit 1
  stats tree_no_rider $ROOT TTL_TAIL_RIDERS=0 || exit 1
fi

full() { # tag dir legs
  local tag=$1 dir=$2 legs=$3
  ( cd $dir; timeout -k 10 600 python bench.py --full --no-cpu-baseline --legs $legs 2>/dev/null | tail -1 > $tmp/full.json )
  local rc=$?
  [ $rc = 0 ] || { echo "full $tag: rc=$rc, stopping"; exit 1; }
  python3 - $tmp/full.json $tag <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
w = d.get('windows') or {}
if w:
    print('%-8s headline %.1f M (windows %.1f .. %.1f)' % (sys.argv[2], d['value'] / 1e6, w['value_min'] / 1e6, w['value_max'] / 1e6))
we = d.get('whole_episode') or {}
if we:
    print('   whole_episode ' + '  '.join('%s %.1f M' % (k, v / 1e6) for k, v in we.items()
                                          if isinstance(v, float) and v > 1e6))
for k, v in (d.get('other_shapes') or {}).items():
    if isinstance(v, dict) and 'value' in v:
        print('   %-18s %8.1f M (windows %.1f .. %.1f)' % (k, v['value'] / 1e6, v['value_min'] / 1e6, v['value_max'] / 1e6))
h = d.get('roofline_hbm_regime') or {}
if 'ms_per_step' in h:
    print('%-8s hbm leg %.1f us/step' % (sys.argv[2], h['ms_per_step'] * 1e3))
PY
}

if [[ $sections == *3* ]]; then
  echo "# 3. --full --legs weak,shapes and --legs hbm"
  for r in 1 2; do
    for legs in weak,shapes hbm; do
      full parent $A $legs || exit 1
      full tree $ROOT $legs || exit 1
    done
  done
fi

if [[ $sections == *4* ]]; then
  echo "# 4. re-bucket period with the riders ($rounds rounds, alternating)"
  for args in "--steps 12 --warmup 3" "--steps 20 --warmup 5"; do
    for r in $(seq 1 $rounds); do
      for P in 1 2 3; do PERIOD=$P one P=$P $ROOT "" $args || exit 1; done
    done
  done
fi
rm -rf $tmp
