"""What `ttl_env_step_end` decides, knob set by knob set, against a recording.

The host half of the library chooses every step's launches: the one-launch
small-batch tail, k_tail or k_prefix + k_proc_scatter; whether the processing
order is dropped, whether the step re-buckets it, whether the order scatter and
the row maps ride in the gather launch.  This file pins those choices as the
callers can see them, so that the code that makes them can be restated: every
knob set below runs one short episode and the record of each of its steps must
equal, entry for entry, `tests/golden/step_plan_trace.json`, which
`tests/golden/make_golden_step_plan.py` wrote by running this file's own
`run_episode` on the MI355X (the fixture names the commit of the library).

Per step: the rows active before it; the launches of each profile class
(advance, prefix, state, proc_scatter) between `profile_begin` and
`profile_end`; `last_step` of `ttl_env_tail_riders`; `(slots, instep)` of
`ttl_env_order_slots` after the harvest.  Per episode: a SHA-256 over the final
flags, lengths and streamline history.

Not seen from here: whether a stand-alone order scatter runs in front of the
gather or behind it (TTL_ORDER_INSTEP_AFTER): neither the launch counts nor the
ABI show it.

Shapes as in test_hip_tail_riders.py: a 24^3 volume, 700 streamlines (three row
blocks, the last partial; one scatter workgroup), TTL_ORDER_MIN_ROWS=1 and
TTL_FUSE_MAX_ROWS=256 so that the tails with a processing order run down to 257
rows; an episode goes on until at most 256 rows are active and two steps beyond,
so every kind of tail occurs.
"""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, synthetic_subject

D = 24
N = 700
FUSE_MAX = 256
FIXTURE = os.path.join(GOLDEN, 'step_plan_trace.json')
STEP_FIELDS = ('rows', 'advance', 'prefix', 'state', 'proc_scatter', 'last_riders', 'slots',
               'instep')

# every knob ttl_env_create reads: a set leaves the ones it does not name unset
LIBRARY_KNOBS = ('TTL_ORDER_MIN_ROWS', 'TTL_ORDER_INSTEP', 'TTL_ORDER_INSTEP_AFTER',
                 'TTL_TAIL_RIDERS', 'TTL_STATE_KERNEL', 'TTL_XCD_REMAP', 'TTL_XCD_ROTATE',
                 'TTL_STORE_FLAVOUR', 'TTL_FUSE_SMALL', 'TTL_FUSE_MAX_ROWS',
                 'TTL_GATHER_PERSIST_ROWS', 'TTL_TAIL_FUSED', 'TTL_TAIL_FUSED_MAX_ROWS',
                 'TTL_LOCAL_SORT', 'TTL_POLL_COUNTS')


def knob_sets():
    """The 39 sets: the product of the four knobs that choose tail, re-bucket and
    riders, then one departure from the defaults at a time."""
    sets = [dict(TTL_TAIL_FUSED=f, TTL_ORDER_INSTEP=i, TTL_TAIL_RIDERS=r, TTL_ORDER_INSTEP_AFTER=a)
            for f, i, r, a in itertools.product((0, 1), (0, 2), (0, 1, 2, 3), (0, 1))]
    sets += [{'TTL_FUSE_SMALL': 0}, {'TTL_POLL_COUNTS': 0}, {'TTL_LOCAL_SORT': 0},
             {'TTL_STATE_KERNEL': 0}, {'TTL_STATE_KERNEL': 2}, {'TTL_STATE_KERNEL': 3},
             {'TTL_GATHER_PERSIST_ROWS': 98304}]
    return sets


def set_name(knobs):
    return ' '.join(f'{k}={v}' for k, v in knobs.items())


def make_subject():
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    sh, mask, pk = synthetic_subject(D, C=45)
    aff = np.eye(4, dtype=np.float32)
    m = mask.astype(np.float32)
    return (Vol(sh, aff), Vol(m, aff), Vol(m, aff), Vol(pk, aff), None), mask


def run_episode(subject, mask, knobs, patch):
    """One episode under `knobs` (`patch`: a pytest MonkeyPatch); the record the
    fixture holds for it."""
    import torch
    from tracktolearn_amd.environments import TrackingEnvironment
    for k in LIBRARY_KNOBS:
        patch.delenv(k, raising=False)
    patch.setenv('TTL_ORDER_MIN_ROWS', '1')
    patch.setenv('TTL_FUSE_MAX_ROWS', str(FUSE_MAX))
    for k, v in knobs.items():
        patch.setenv(k, str(v))
    patch.setattr(TrackingEnvironment, 'SPATIAL_ORDER_MIN', 1)
    dto = dict(n_dirs=4, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=2.0, max_length=25.0, compute_reward=False,
               alignment_weighting=1.0, oracle_bonus=0.0, oracle_checkpoint=None,
               oracle_stopping_criterion=False, rng=np.random.RandomState(0),
               device=torch.device('cuda:0'), target_sh_order=None, noise=0.0, fa_map=None)
    env = TrackingEnvironment(subject, 'testing', dto)
    rng = np.random.RandomState(11)
    vox = np.argwhere(mask)
    env.seeds = vox[rng.randint(0, len(vox), N)] + rng.uniform(-0.5, 0.5, (N, 3))
    state = env.reset(0, N)
    lib, h = env._lib, env._handle         # (the reset creates the handle)
    steps, step, beyond = [], 0, 0
    while env._n_active and beyond < 2:
        rows = env._n_active
        beyond += rows <= FUSE_MAX
        a = env.scripted_actions(state, step, 9, 0.2)
        env.profile_begin(4, classes=env.PROFILE_CLASSES)
        env.step_device(a)
        kinds, last = C.c_int32(-1), C.c_int32(-1)
        assert lib.ttl_env_tail_riders(h, C.byref(kinds), C.byref(last), None) == 0
        state, _ = env.harvest()
        launches = {k: v[1] for k, v in env.profile_end().items()}
        slots, instep = C.c_int32(-1), C.c_int32(-1)
        assert lib.ttl_env_order_slots(h, C.byref(slots), C.byref(instep)) == 0
        steps.append([rows] + [launches[c] for c in env.PROFILE_CLASSES] +
                     [last.value, slots.value, instep.value])
        step += 1
    torch.cuda.synchronize()
    sha = hashlib.sha256()
    for a in (env.flags, env.lengths, env.streamlines):
        sha.update(np.ascontiguousarray(a).tobytes())
    return dict(steps=steps, sha256=sha.hexdigest())


@pytest.fixture(scope='module')
def subject():
    return make_subject()


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        trace = json.load(f)
    assert trace['step_fields'] == list(STEP_FIELDS)
    assert list(trace['episodes']) == [set_name(k) for k in knob_sets()]
    return trace['episodes']


@pytest.mark.gpu
@pytest.mark.parametrize('knobs', knob_sets(), ids=set_name)
def test_steps_take_the_recorded_launches(knobs, subject, recorded, monkeypatch):
    got = run_episode(*subject, knobs, monkeypatch)
    want = recorded[set_name(knobs)]
    assert len(got['steps']) == len(want['steps'])
    for s, (x, y) in enumerate(zip(got['steps'], want['steps'])):
        assert x == y, (s, dict(zip(STEP_FIELDS, x)), dict(zip(STEP_FIELDS, y)))
    assert got['sha256'] == want['sha256']


def test_the_recording_sees_every_kind_of_tail(recorded):
    """The fixture itself (no GPU): the default set's episode has k_tail steps
    with and without a re-bucket, riders of both kinds and the one-launch tail;
    TTL_TAIL_FUSED=0 has the two-kernel tail."""
    f = {k: i for i, k in enumerate(STEP_FIELDS)}
    persist = recorded['TTL_GATHER_PERSIST_ROWS=98304']['steps']       # (nothing rides there)
    assert all(s[f['last_riders']] == 0 for s in persist)
    default = recorded['TTL_TAIL_FUSED=1 TTL_ORDER_INSTEP=2 TTL_TAIL_RIDERS=1 '
                       'TTL_ORDER_INSTEP_AFTER=0']['steps']
    assert {s[f['last_riders']] for s in default} == {0, 2, 3}
    assert all(s[f['advance']] == 1 and s[f['state']] == 1 for s in default)
    assert [s[f['prefix']] for s in default if s[f['rows']] <= FUSE_MAX] == [0, 0]
    assert all(s[f['prefix']] == 1 for s in default if s[f['rows']] > FUSE_MAX)
    two = recorded['TTL_TAIL_FUSED=0 TTL_ORDER_INSTEP=2 TTL_TAIL_RIDERS=1 '
                   'TTL_ORDER_INSTEP_AFTER=0']['steps']
    assert any(s[f['proc_scatter']] == 1 for s in two)
    assert all(s[f['last_riders']] == 0 for s in two)
