"""The tissue-map criterion inside the step (``ttl_env_set_act``,
``env_dto['act_in_step']``, ``ttl_track.py --act_in_step``) against
the split path -- ``ttl_env_step_begin``, ``ttl_act_flags``, ``ttl_env_step_end``
-- which tests/test_act_reference.py and tests/test_act_tracking.py hold to
tests/ref_act.py.  Both sides run the same device code on the same inputs: every
comparison is exact.  The tube and the maps are those of tests/test_act_tracking.py."""
import ctypes as C
import re

import numpy as np
import pytest

import ref_act
import test_act_tracking as at
import test_odf_tracking as tube
from test_act_tracking import files  # noqa: F401  (the command's input files, a fixture)

DEV = tube.DEV
DIMS = tube.DIMS
F32 = np.float32
MASK, LENGTH, TARGET, EXCLUDE, ORACLE = 1, 2, ref_act.TARGET, ref_act.EXCLUDE, 64
TISSUE = TARGET | EXCLUDE
N = at.N
#: the wave boundaries and the block boundaries where the ranks are recomputed
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 1000)


def make_env(include=None, exclude=None, in_step=False, mode='act', act_seed=None,
             x=(8.0, 12.0), n=N, max_length=40.0, seeds=None, **more):
    import torch
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    sh, mask = tube.volumes()
    aff = np.eye(4, dtype=np.float32)
    dto = dict(n_dirs=tube.K, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=max_length, compute_reward=False,
               alignment_weighting=0.0, oracle_bonus=0.0, rng=np.random.RandomState(0),
               device=torch.device(DEV), target_sh_order=tube.ORDER)
    if include is not None:
        dto.update(act_include=include, act_exclude=exclude, act_mode=mode)
    if in_step:
        dto['act_in_step'] = True
    if act_seed is not None:
        dto['act_seed'] = act_seed
    dto.update(more)
    peaks = None
    if dto['compute_reward']:
        peaks = Vol(np.random.RandomState(1).standard_normal(DIMS + (15,)).astype(F32), aff)
    env = TrackingEnvironment((Vol(sh, aff), Vol(mask, aff), Vol(mask, aff), peaks, None),
                              'testing', dto)
    env.seeds = at.seeds(n, x) if seeds is None else seeds
    return env


def buffers(env):
    """Everything the handle keeps per streamline, downloaded."""
    n = env._n_total
    return dict(flags=env.flags, dones=env.dones, lengths=env.lengths,
                continue_idx=env.continue_idx,
                history=env.streamlines[:n].view(np.uint32))


def assert_same_buffers(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype.itemsize == 4 else np.uint8)


# ------------------------------------------------------------------ CPU part
def test_library_binding_names_the_entry_point():
    from tracktolearn_amd import _lib
    assert _lib.HAS_ACT_IN_STEP == 1
    res, args = _lib.SYMBOLS['ttl_env_set_act']
    assert res is C.c_int and args[1]._type_ is _lib.ActDesc
    header = open(tube.ROOT + '/include/ttl_hip.h').read()
    assert re.search(r'#define\s+TTL_HAS_ACT_IN_STEP\s+1\b', header)
    assert re.search(r'TTL_API\s+int\s+ttl_env_set_act\(ttl_env \*env, const ttl_act_desc \*desc\);',
                     header)
    assert re.search(r'#define\s+TTL_ABI_VERSION\s+13\b', header)
    assert hasattr(_lib.load(), 'ttl_env_set_act')


def test_option_parses_and_is_listed(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_track
    args = at._parse(['--odf_policy', 'prob', '--bidirectional', '--act_include', 'INC',
                      '--act_exclude', 'EXC', '--act_in_step'], tmp_path)
    assert args.act_in_step is True
    args = at._parse(['--odf_policy', 'det', '--act_include', 'INC', '--act_exclude', 'EXC'],
                     tmp_path)
    assert args.act_in_step is False
    with pytest.raises(SystemExit) as e:
        ttl_track.parse_args(['--help'])
    assert e.value.code == 0 and '--act_in_step' in capsys.readouterr().out


def test_option_needs_the_maps(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        at._parse(['--odf_policy', 'det', '--act_in_step'], tmp_path)
    assert e.value.code == 2
    assert '--act_in_step' in capsys.readouterr().err


def test_env_key_needs_the_maps():
    """Refused in BaseEnv.__init__ before anything touches a device."""
    from tracktolearn_amd.environments import TrackingEnvironment
    dto = dict(n_dirs=2, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=40.0, compute_reward=False, alignment_weighting=0.0,
               rng=np.random.RandomState(0), device='cpu', act_in_step=True)
    with pytest.raises(ValueError, match='act_in_step'):
        TrackingEnvironment(None, 'testing', dto)


# ------------------------------------------------------------------ GPU part
#: The C-level episodes run one way only, and which way the first step goes is
#: the policy's business: their inputs are symmetric about x = 11.5.  Seeds over
#: the tube's whole cross-section, the thick blob on either side of them (the
#: rows near the axis end there, EXCLUDE; the others pass it and reach a slab,
#: TARGET), and LENGTH at 15 points: include exceeds 0.5 from x = 20.5 (below
#: 2.5), so rows that set out from [10, 10.75) (from (12.25, 13]) reach it in
#: the step that LENGTH ends, and those from below 10 (above 13) never do.
SHORT = 15 * 0.75


def sym_seeds(n, seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(9.5, 13.5, n), rng.uniform(4.0, 7.0, n),
                     rng.uniform(4.0, 7.0, n)], axis=1)


def sym_maps(mode='act'):
    inc, exc = at.slabs(), at.thick_blob()
    exc[5:8, 5:7, 5:7] = 1.0
    if mode == 'cmc':
        inc[3:21] = 0.05
    return inc, exc


def _episode_side_by_side(n, mode, order):
    """Two handles stepped through one episode on the same actions: `a` with the
    criterion installed and plain ttl_env_step, `b` through begin -> ttl_act_flags
    -> end.  Returns the final flags."""
    import torch
    inc, exc = sym_maps(mode)
    more = dict(n=n, max_length=SHORT, seeds=sym_seeds(n), compute_reward=True,
                alignment_weighting=1.0)
    a = make_env(inc, exc, True, mode, 3, **more)
    b = make_env(inc, exc, False, mode, 3, **more)
    calls = []
    for env in (a, b):
        inner = env._lib

        class Spy:
            def __init__(self, lib, tag):
                self._lib, self._tag = lib, tag

            def __getattr__(self, name):
                if name in ('ttl_env_step', 'ttl_env_step_begin', 'ttl_act_flags',
                            'ttl_env_step_end'):
                    calls.append((self._tag, name))
                return getattr(self._lib, name)
        env._lib = Spy(inner, 'a' if env is a else 'b')
    agent = at.policy(a).agent
    sa, sb = a.reset(0, n), b.reset(0, n)
    assert np.array_equal(bits(sa), bits(sb))
    step = 0
    while a._n_active > 0:
        act = agent.select_action(sa)
        out_a = a._launch_step(act, order)
        out_b = b._launch_step(act, order)
        torch.cuda.synchronize()
        # the step's outputs: state rows (all of them, in the step's order), done, reward
        assert np.array_equal(bits(out_a[0]), bits(out_b[0])), (step, 'state rows')
        assert np.array_equal(bits(out_a[2]), bits(out_b[2])), (step, 'done_out')
        assert np.array_equal(out_a[1].cpu().numpy().view(np.uint64),
                              out_b[1].cpu().numpy().view(np.uint64)), (step, 'reward_out')
        assert np.array_equal(bits(a._row_dest_view(a._n_active)),
                              bits(b._row_dest_view(b._n_active))), (step, 'row_dest')
        sa, _ = a.harvest()
        sb, _ = b.harvest()
        assert np.array_equal(a._host_counts_np[:2], b._host_counts_np[:2]), (step, 'host_counts')
        assert np.array_equal(bits(sa), bits(sb)), (step, 'harvested rows')
        assert_same_buffers(buffers(a), buffers(b), step)
        step += 1
    assert b._n_active == 0 and step >= 2
    # the C calls each side made
    assert {c for c in calls if c[0] == 'a'} == {('a', 'ttl_env_step')}
    assert {c[1] for c in calls if c[0] == 'b'} == {'ttl_env_step_begin', 'ttl_act_flags',
                                                    'ttl_env_step_end'}
    return b.flags


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['act', 'cmc'])
@pytest.mark.parametrize('n', SIZES)
def test_step_with_the_criterion_equals_the_split_step(n, mode):
    from tracktolearn_amd import _lib
    for order in (_lib.ORDER_ACTIVE, _lib.ORDER_PARTITION):
        flags = _episode_side_by_side(n, mode, order)
        assert (flags & TISSUE).any() or n == 1
        if n >= 255:
            # the inputs hold every kind of stop, and rows that LENGTH stopped in
            # the step that gave them a tissue bit
            assert (flags == TARGET).any() and (flags == EXCLUDE).any()
            assert (flags == LENGTH).any()
            assert (flags == (LENGTH | TARGET)).any()


@pytest.mark.gpu
def test_bits_the_step_leaves_are_the_restatement_s():
    inc, exc = sym_maps()
    n = 257
    env = make_env(inc, exc, True, n=n, max_length=SHORT, seeds=sym_seeds(n))
    agent = at.policy(env).agent
    state = env.reset(0, n)
    seen = 0
    while env._n_active > 0:
        idx = env.continue_idx
        env.step_device(agent.select_action(state))
        state, _ = env.harvest()
        n_points = env.length
        want = ref_act.act_flags_ordered(inc, exc, env.streamlines[:n, :n_points], n_points,
                                         ref_act.THRESHOLD, ids=idx)
        assert np.array_equal(env.flags[idx] & TISSUE, want), n_points
        seen |= int(np.bitwise_or.reduce(want))
    assert seen == TISSUE


def _step_loop(env, agent, state, after=None):
    while state.shape[0] > 0:
        env.step_device(agent.select_action(state))
        state, _ = env.harvest()
        if after is not None:
            after()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['act', 'cmc'])
def test_backward_pass_equals_the_split_path(mode, monkeypatch):
    monkeypatch.setenv('TTL_GRAPH_EPISODE', '0')
    inc, exc = (at._cmc_maps() if mode == 'cmc' else (at.one_sided(), at.blob()))
    split = make_env(inc, exc, False, mode, 3)
    at.both_ways(split, at.policy(split))
    env = make_env(inc, exc, True, mode, 3)
    agent = at.policy(env).agent
    _step_loop(env, agent, env.reset(0, N))
    assert np.array_equal(env.flags, split.flags_forward.cpu().numpy())
    state = env.reset_backward()
    init_len = env._init_len.cpu().numpy()

    def replayed_rows_have_no_bit():
        # n_points <= init_len[g]: a replayed point or the seed, never judged
        flags = env.flags
        assert (flags[init_len >= env.length] & TISSUE == 0).all()
    _step_loop(env, agent, state, replayed_rows_have_no_bit)
    at.same(at.result(split), at.result(env))
    assert (env.flags & TISSUE).any()
    assert np.array_equal(env._init_len.cpu().numpy(), split._init_len.cpu().numpy())


@pytest.mark.gpu
def test_seeds_inside_the_include_map_still_grow_both_halves():
    inc, exc = at.slabs(), np.zeros(DIMS, F32)
    env = make_env(inc, exc, True, x=(21.0, 21.7))
    at.both_ways(env, at.policy(env))
    flags, lengths, hist = at.result(env)
    init_len = env._init_len.cpu().numpy()
    seed_at = env.seed_index.cpu().numpy()
    assert (at.include_along(inc, np.ascontiguousarray(env.initial_points, F32)) > 0.5).all()
    assert (init_len >= 2).all() and (lengths >= init_len + 1).all()
    assert ((flags & TARGET) != 0).all()
    for g in range(N):
        assert np.allclose(hist[g, seed_at[g]], env.initial_points[g], atol=1e-5)
    split = make_env(inc, exc, False, x=(21.0, 21.7))
    at.both_ways(split, at.policy(split))
    at.same(at.result(split), (flags, lengths, hist))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['act', 'cmc'])
def test_free_running_loops_equal_the_step_by_step_loop(mode, monkeypatch):
    inc, exc = (at._cmc_maps() if mode == 'cmc' else (at.one_sided(), at.blob()))
    split = make_env(inc, exc, False, mode, 3)
    state = split.reset(0, N)
    assert not split.freerun_supported()
    at.policy(split).validation_episode(state, split)
    want = at.result(split)
    assert (want[0] & TISSUE).any()
    # step by step, in the step
    env = make_env(inc, exc, True, mode, 3)
    alg = at.policy(env)
    monkeypatch.setenv('TTL_GRAPH_EPISODE', '0')
    alg.validation_episode(env.reset(0, N), env)
    assert len(env._free_runs) == 0
    at.same(want, at.result(env))
    monkeypatch.delenv('TTL_GRAPH_EPISODE')
    # the captured graph
    state = env.reset(0, N)
    assert env.freerun_supported()
    alg.validation_episode(state, env)
    assert len(env._free_runs) == 1
    at.same(want, at.result(env))
    # host-launched free-running steps
    state = env.reset(0, N)
    env.run_free_eager(alg.agent.select_action, state)
    at.same(want, at.result(env))
    # a backward pass stays step by step
    env.reset_backward()
    assert not env.freerun_supported()


@pytest.mark.gpu
def test_one_graph_serves_batches_with_other_id_bases_and_seeds():
    """A graph captured with a criterion installed reads seed and id base from
    the handle's record: replayed for the next batch it draws that batch's
    numbers (CMC), which are those of one batch holding both."""
    inc, exc = at._cmc_maps()
    env = make_env(inc, exc, True, 'cmc', 3)
    alg = at.policy(env)
    parts = []
    for lo, hi in ((0, N // 2), (N // 2, N)):
        alg.validation_episode(env.reset(lo, hi), env)
        parts.append(at.result(env))
    assert len(env._free_runs) == 1
    whole = make_env(inc, exc, False, 'cmc', 3)
    alg_w = at.policy(whole)
    alg_w.validation_episode(whole.reset(0, N), whole)
    at.same(at.result(whole), tuple(np.concatenate([p[k] for p in parts]) for k in range(3)))
    assert len(np.unique(at.result(whole)[1])) > 8            # the lengths are drawn
    # another seed, the same graph
    env.act_seed = 4
    alg.validation_episode(env.reset(0, N // 2), env)
    assert len(env._free_runs) == 1
    other = make_env(inc, exc, False, 'cmc', 4)
    at.policy(other).validation_episode(other.reset(0, N // 2), other)
    at.same(at.result(other), at.result(env))
    assert not np.array_equal(at.result(env)[1], parts[0][1])


@pytest.mark.gpu
def test_graph_captured_with_a_criterion_replays_after_it_was_switched_off():
    """The choice of the two the design allows: the hook of a captured step reads
    "off" from the handle's record and changes nothing; no new graph is needed."""
    inc, exc = at.one_sided(), at.blob()
    env = make_env(inc, exc, True)
    alg = at.policy(env)
    alg.validation_episode(env.reset(0, N), env)
    assert len(env._free_runs) == 1 and (env.flags & TISSUE).any()
    graph = next(iter(env._free_runs.values())).graph
    state = env.reset(0, N)
    from tracktolearn_amd import _lib
    _lib.check(env._lib.ttl_env_set_act(env._handle, None), 'ttl_env_set_act')
    alg.validation_episode(state, env)
    assert len(env._free_runs) == 1 and next(iter(env._free_runs.values())).graph is graph
    plain = make_env()
    at.policy(plain).validation_episode(plain.reset(0, N), plain)
    assert not (env.flags & TISSUE).any()
    at.same(at.result(plain), at.result(env))
    # ... and on again at the next reset
    alg.validation_episode(env.reset(0, N), env)
    assert next(iter(env._free_runs.values())).graph is graph
    split = make_env(inc, exc, False)
    at.policy(split).validation_episode(split.reset(0, N), split)
    at.same(at.result(split), at.result(env))


@pytest.mark.gpu
def test_free_running_step_for_too_few_rows_changes_nothing():
    import torch
    from tracktolearn_amd import _lib
    from tracktolearn_amd.environments.free_run import _FreeRunning
    inc = np.ones(DIMS, F32)                    # every judged point is a target
    env = make_env(inc, np.zeros(DIMS, F32), True)
    state = env.reset(0, N)
    agent = at.policy(env).agent
    act = agent.select_action(state)
    before = buffers(env)
    rows = env._new_state(N)
    done = torch.zeros(N, dtype=torch.uint8, device=env.device)
    with _FreeRunning.begin(env) as episode:
        _lib.check(env._lib.ttl_env_freerun_step(
            env._handle, act.data_ptr(), N - 1, rows.data_ptr(), env._state_pitch, None,
            done.data_ptr(), env._stream()), 'ttl_env_freerun_step')
        torch.cuda.synchronize()
        assert_same_buffers(before, buffers(env), 'skipped step')
        # the same step for all rows: every row reaches a target
        _lib.check(env._lib.ttl_env_freerun_step(
            env._handle, act.data_ptr(), N, rows.data_ptr(), env._state_pitch, None,
            done.data_ptr(), env._stream()), 'ttl_env_freerun_step')
    assert (episode.n_left, episode.length) == (0, 2)
    assert ((env.flags & TARGET) != 0).all() and done.cpu().numpy().all()


def _tracked(env, act_filter, mode):
    return at._tracked_seeds(env, at.policy(env, 'prob' if mode == 'cmc' else 'det'), act_filter,
                             at.seeds(N))


@pytest.mark.gpu
@pytest.mark.parametrize('act_filter', ['exclude', 'endpoints'])
@pytest.mark.parametrize('mode', ['act', 'cmc'])
def test_tracker_keeps_the_streamlines_of_the_split_run(mode, act_filter):
    inc, exc = (at._cmc_maps() if mode == 'cmc' else (at.one_sided(), at.blob()))
    want = _tracked(make_env(inc, exc, False, mode, 3), act_filter, mode)
    env = make_env(inc, exc, True, mode, 3)
    got = _tracked(env, act_filter, mode)
    assert len(env._free_runs) >= 1               # forward halves ran as a graph
    assert 0 < len(want) < N and set(got) == set(want)
    for k, s in want.items():
        assert np.array_equal(s.view(np.uint32), got[k].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('direct', [False, True])
def test_command_writes_the_bytes_of_the_run_without_the_option(files, capsys, direct):  # noqa: F811
    from tracktolearn_amd.runners import ttl_track
    act = ['--act_include', str(files / 'inc.nii.gz'), '--act_exclude', str(files / 'exc.nii.gz')]
    more = act + (['--direct_output'] if direct else [])
    names = ('split_direct.trk', 'instep_direct.trk') if direct else ('split.trk', 'instep.trk')
    ttl_track.main(at._argv(files, names[0], *more))
    n_split = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    ttl_track.main(at._argv(files, names[1], *(more + ['--act_in_step'])))
    n_in = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    assert 50 < n_split == n_in < 128
    assert open(str(files / names[0]), 'rb').read() == open(str(files / names[1]), 'rb').read()
    env, tracker, _ = at._in_memory(at._argv(files, 'never.trk', *(more + ['--act_in_step'])))
    assert env.act_in_step and env._act_desc is not None


@pytest.mark.gpu
def test_with_the_oracle_criterion_both_stop(tmp_path):
    """begin -> the oracle's bits -> end, the tissue maps applied by begin: the
    result of the split path with both criteria."""
    import torch
    from tracktolearn_amd.oracles.oracle import OracleSingleton
    from tracktolearn_amd.oracles.transformer_oracle import save_random_checkpoint
    ck = save_random_checkpoint(str(tmp_path / 'o.ckpt'), n_head=2, n_layers=1, seed=5)
    inc, exc = at.one_sided(), at.blob()
    n = 300

    def oracle_env(ckpt, *maps):
        OracleSingleton.reset()
        # (seeds within ten points of either slab, whichever way the first step goes)
        return make_env(*maps, n=n, x=(8.0, 15.5), oracle_checkpoint=ckpt,
                        oracle_stopping_criterion=True)

    # put the random network's scores below 0.5 where the criterion starts looking
    # (more than 5 * min_nb_steps = 10 points): the half that runs into the near
    # slab ends on the maps before that, the other half on the oracle
    probe = oracle_env(ck)
    agent = at.policy(probe).agent
    state = probe.reset(0, n)
    while probe.length < 10:
        probe.step_device(agent.select_action(state))
        state, _ = probe.harvest()
    p = probe._oracle.predict(probe._oracle_points(None, probe.length)).double()
    p = p.clamp(1e-6, 1 - 1e-6)
    blob = torch.load(ck, map_location='cpu', weights_only=True)
    blob['state_dict']['head.bias'] -= float(torch.log(p / (1 - p)).max()) + 0.5
    ck2 = str(tmp_path / 'o2.ckpt')
    torch.save(blob, ck2)

    results = []
    for in_step in (False, True):
        env = oracle_env(ck2, inc, exc, in_step)
        assert env._use_oracle_stopping
        alg = at.policy(env)
        state = env.reset(0, n)
        assert not env.freerun_supported()
        alg.validation_episode(state, env)
        alg.validation_episode(env.reset_backward(), env)
        results.append(at.result(env) + (env.flags_forward.cpu().numpy(),))
    OracleSingleton.reset()
    at.same(results[0][:3], results[1][:3])
    assert np.array_equal(results[0][3], results[1][3])
    flags = np.concatenate([results[0][0], results[0][3]])      # backward and forward halves
    assert (flags & ORACLE).any() and (flags & TISSUE).any()


def _desc(env, **change):
    from tracktolearn_amd import _lib
    src = env._act_desc_now()
    d = _lib.ActDesc()
    C.memmove(C.byref(d), C.byref(src), C.sizeof(d))
    for k, v in change.items():
        if k == 'dim':
            d.dim[:] = v
        else:
            setattr(d, k, v)
    return d


@pytest.mark.gpu
def test_refusals_leave_the_criterion_as_it_was():
    import torch
    from tracktolearn_amd import _lib
    from tracktolearn_amd.environments.free_run import _FreeRunning
    inc, exc = at._cmc_maps()
    env = make_env(inc, exc, True, 'cmc', 3)
    split = make_env(inc, exc, False, 'cmc', 3)
    agent = at.policy(env).agent
    state, state_s = env.reset(0, N), split.reset(0, N)
    set_act, h = env._lib.ttl_env_set_act, env._handle
    bad = [dict(include=None), dict(exclude=None), dict(dim=[24, 0, 12]), dict(dim=[24, 12, -1]),
           dict(mode=2), dict(mode=-1), dict(ids_base=-1), dict(exponent=0.0),
           dict(exponent=-1.0), dict(exponent=float('inf')), dict(exponent=float('nan'))]
    for change in bad:
        assert set_act(h, C.byref(_desc(env, **change))) == _lib.ERR_INVALID, change
    assert set_act(None, C.byref(_desc(env))) == _lib.ERR_INVALID
    # threshold mode does not read the exponent
    assert set_act(h, C.byref(_desc(env, mode=_lib.ACT_THRESHOLD, exponent=0.0))) == 0
    assert set_act(h, C.byref(_desc(env))) == 0

    def step_both():
        nonlocal state, state_s
        act = agent.select_action(state)
        env.step_device(act)
        split.step_device(act)
        # between a step and its harvest
        assert set_act(h, C.byref(_desc(env, seed=99))) == _lib.ERR_STATE
        assert set_act(h, None) == _lib.ERR_STATE
        state, _ = env.harvest()
        state_s, _ = split.harvest()
        assert_same_buffers(buffers(split), buffers(env), env.length)

    for _ in range(3):
        step_both()
    for change in bad:
        assert set_act(h, C.byref(_desc(env, **change))) == _lib.ERR_INVALID, change
    step_both()
    # while free-running
    with _FreeRunning.begin(env):
        assert set_act(h, C.byref(_desc(env, seed=99))) == _lib.ERR_STATE
        assert set_act(h, None) == _lib.ERR_STATE
    torch.cuda.synchronize()
    for _ in range(3):
        step_both()
    assert (env.flags & TISSUE).any() and env._n_active > 0
