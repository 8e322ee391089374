#!/usr/bin/env python3
"""Record tests/golden/step_plan_trace.json: what every step of the episodes of
tests/test_hip_step_plan.py launches, on the library as built in this tree.

    python tests/golden/make_golden_step_plan.py <commit of the library>

It runs that file's own `run_episode` for each of its knob sets, so it needs the
MI355X (and is therefore not among the generators test_golden_reproducible.py
runs).  The fixture pins behaviour across a restatement of the host code: record
it at the commit whose choices are to be kept, not at the one under test.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_hip_step_plan as sp  # noqa: E402


def main():
    commit = sys.argv[1]
    out_dir = os.environ.get('TTL_GOLDEN_OUT', HERE)
    subject = sp.make_subject()
    episodes = {}
    for knobs in sp.knob_sets():
        with pytest.MonkeyPatch.context() as patch:
            episodes[sp.set_name(knobs)] = sp.run_episode(*subject, knobs, patch)
        print(sp.set_name(knobs), len(episodes[sp.set_name(knobs)]['steps']), 'steps', flush=True)
    trace = dict(library_commit=commit, step_fields=list(sp.STEP_FIELDS), episodes=episodes)
    with open(os.path.join(out_dir, 'step_plan_trace.json'), 'w') as f:
        f.write('{\n "library_commit": %s,\n "step_fields": %s,\n "episodes": {\n' %
                (json.dumps(commit), json.dumps(trace['step_fields'])))
        f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                           for k, v in episodes.items()))
        f.write('\n }\n}\n')


if __name__ == '__main__':
    main()
