#!/usr/bin/env python3
"""Record tests/golden/state_rows_trace.json: SHA-256 digests of the state rows
the gather kernels of the library as built in this tree write, on the input sets
and the rig of tests/test_state_gather_reference.py.

    python tests/golden/make_golden_state_rows.py <commit of the library>

It needs the MI355X (and is therefore not among the generators
test_golden_reproducible.py runs).  The fixture pins the bits of the rows across
a restatement of the kernels: record it at the commit whose bits are to be kept,
not at the one under test.

  sweep     per width of WIDTHS and TTL_STATE_KERNEL 4, 3 and 0: the 203 rows
  edge      per (C, radius, shift) of edge_cases() x SHIFTS: the finite rows
            (all but the last 10, whose NaN payloads are not pinned)
  episodes  per C of STEP_C and launch configuration, K = 4: the per-step rows
            by streamline

and what that commit's own kernels agreed on: sweep_knob3_equals_knob4 per
width, episodes_equal_three_launch per C for the one-launch and free-running
tails.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_state_gather_reference as sg  # noqa: E402


def sweep_rows(C_, kernel):
    from tracktolearn_amd import _lib
    rig = sg._Rig(sg.volume(C_), _lib.SH_LINEAR, sg.N_SWEEP, sg.SWEEP_K)
    words = rig.gather(sg.sweep_seeds(C_), sg.SWEEP_R, 0.0, knobs=dict(TTL_STATE_KERNEL=kernel))
    return sg._contained(words, sg.N_SWEEP, 7 * C_ + 3 * sg.SWEEP_K)


def main():
    commit = sys.argv[1]
    out_dir = os.environ.get('TTL_GOLDEN_OUT', HERE)
    sweep = {str(C_): {str(k): sg.digest(sweep_rows(C_, k)) for k in (4, 3, 0)}
             for C_ in sg.WIDTHS}
    print('sweep:', len(sweep), 'widths', flush=True)
    edge = {sg.edge_name(C_, r, shift): sg.digest(sg._edge_output(C_, r, shift)[:-10])
            for C_, r in sg.edge_cases() for shift in sg.SHIFTS}
    print('edge:', len(edge), 'cases', flush=True)
    episodes, agree = {}, {}
    for C_ in sg.STEP_C:
        traces = {config: sg.episode_trace(C_, sg.TRACE_K, config) for config in sg.CONFIGS}
        episodes[str(C_)] = {config: sg.episode_digest(t) for config, t in traces.items()}
        agree[str(C_)] = {config: traces[config] == traces['three_launch']
                          for config in ('one_launch', 'free_running')}
        print('episodes: C =', C_, agree[str(C_)], flush=True)
    trace = dict(library_commit=commit, sweep=sweep,
                 sweep_knob3_equals_knob4={C_: d['3'] == d['4'] for C_, d in sweep.items()},
                 edge=edge, episodes=episodes, episodes_equal_three_launch=agree)
    with open(os.path.join(out_dir, 'state_rows_trace.json'), 'w') as f:
        f.write('{\n' + ',\n'.join(
            ' %s: %s' % (json.dumps(k), json.dumps(v) if not isinstance(v, dict) else
                         '{\n' + ',\n'.join('  %s: %s' % (json.dumps(kk), json.dumps(vv))
                                            for kk, vv in v.items()) + '\n }')
            for k, v in trace.items()) + '\n}\n')


if __name__ == '__main__':
    main()
