"""Anatomically constrained tracking end to end (ttl_act_flags in the step,
``Tracker(act_filter=...)``, ``ttl_track.py --act_include / --act_exclude``;
DESIGN 3.14) on the tube of tests/test_odf_tracking.py: a lobe along x, an
include slab at either end of the tube, an exclude blob on its axis."""
import os
import re

import numpy as np
import pytest

import ref_act
import test_odf_tracking as tube

DEV = tube.DEV
DIMS = tube.DIMS
F32 = np.float32
MASK, LENGTH, CURVATURE, TARGET, EXCLUDE = 1, 2, 4, ref_act.TARGET, ref_act.EXCLUDE
N = 512
XOR = 0x9E3779B97F4A7C15


def slabs():
    """include = 1 for x < 3 and x >= 21."""
    inc = np.zeros(DIMS, F32)
    inc[:3] = 1.0
    inc[21:] = 1.0
    return inc


def blob():
    """exclude = 1 in three voxels beside the tube's axis: rows with y, z below
    5.5 read more than 0.5 there, the others less."""
    exc = np.zeros(DIMS, F32)
    exc[15:18, 5, 5] = 1.0
    return exc


def one_sided():
    """The low slab only where y < 6: a row with y > 5.5 runs on to the mask."""
    inc = slabs()
    inc[:3, 6:, :] = 0.0
    return inc


def seeds(n, x=(8.0, 12.0), seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(x[0], x[1], n), rng.uniform(4.5, 6.5, n),
                     rng.uniform(4.5, 6.5, n)], axis=1)


def make_env(include=None, exclude=None, mode='act', act_seed=None, x=(8.0, 12.0), n=N):
    import torch
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    sh, mask = tube.volumes()
    aff = np.eye(4, dtype=np.float32)
    dto = dict(n_dirs=tube.K, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=40.0, compute_reward=False, alignment_weighting=0.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=torch.device(DEV),
               target_sh_order=tube.ORDER)
    if include is not None:
        dto.update(act_include=include, act_exclude=exclude, act_mode=mode)
    if act_seed is not None:
        dto['act_seed'] = act_seed
    env = TrackingEnvironment((Vol(sh, aff), Vol(mask, aff), Vol(mask, aff), None, None),
                              'testing', dto)
    env.seeds = seeds(n, x)
    return env


def policy(env, mode='det'):
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    return OdfTracking(env, mode, seed=5)


def record_act(env):
    """Every ``env.act_flags`` call from here on: what it was given and returned."""
    records, inner = [], env.act_flags

    def recording(n, n_points):
        out = inner(n, n_points)
        backward = env._init_len is not None
        records.append(dict(
            idx=env.continue_idx.copy(), n=n, n_points=n_points, flags=out.cpu().numpy(),
            history=env._buf_streamlines[:env._n_total, :n_points].cpu().numpy(),
            init_len=env._init_len.cpu().numpy() if backward else None, backward=backward,
            ids_base=env.streamline_id_base()))
        return out
    env.act_flags = recording
    return records


def restated(rec, include, exclude, mode=ref_act.THRESHOLD, exponent=0.75, seed=0):
    return ref_act.act_flags_ordered(
        include, exclude, rec['history'], rec['n_points'], mode, ids=rec['idx'],
        init_len=rec['init_len'], exponent=exponent,
        seed=(seed ^ XOR if rec['backward'] else seed), ids_base=rec['ids_base'])


def both_ways(env, alg, start=0, end=N):
    alg.validation_episode(env.reset(start, end), env)
    alg.validation_episode(env.reset_backward(), env)


def result(env):
    n = env._n_total
    return env.flags.copy(), env.lengths.copy(), env.streamlines[:n].copy()


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for la, ra, rb in zip(a[1], a[2], b[2]):
        assert np.array_equal(ra[:la].view(np.uint32), rb[:la].view(np.uint32))


def key(seed):
    """A seed as a dictionary key (the file keeps seed - 0.5: rounded)."""
    return np.round(np.asarray(seed, np.float64), 5).tobytes()


def thick_blob():
    """The blob over the four voxel lines round the axis: a quarter of the seeds of
    the command's seed mask run into it."""
    exc = np.zeros(DIMS, F32)
    exc[15:18, 5:7, 5:7] = 1.0
    return exc


def include_along(inc, row):
    """include at every point of a history row (the restatement's values)."""
    return ref_act.act_values_ordered(inc, np.zeros_like(inc), row[:, None, :], 1)[:, 0]


# ------------------------------------------------------------------ CPU part
def _parse(argv, tmp_path, make=('inc', 'exc')):
    from tracktolearn_amd.runners import ttl_track
    files = []
    for name in ('fodf', 'seed', 'mask') + tuple(make):
        f = tmp_path / f'{name}.nii.gz'
        f.write_bytes(b'')
        files.append(str(f))
    argv = [a.replace('INC', str(tmp_path / 'inc.nii.gz')).replace(
        'EXC', str(tmp_path / 'exc.nii.gz')) for a in argv]
    return ttl_track.parse_args(files[:3] + [str(tmp_path / 'out.trk')] + argv)


def test_help_lists_the_options(capsys):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(SystemExit) as e:
        ttl_track.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--act_include FILE', '--act_exclude FILE', '--act_mode {act,cmc}',
                '--act_filter {none,exclude,endpoints}'):
        assert opt in text


def test_act_options_and_their_defaults(tmp_path):
    args = _parse(['--odf_policy', 'det', '--act_include', 'INC', '--act_exclude', 'EXC'], tmp_path)
    assert (args.act_mode, args.act_filter) == ('act', 'exclude')
    args = _parse(['--odf_policy', 'prob', '--bidirectional', '--compress', '0.1',
                   '--direct_output', '--npv', '3', '--act_include', 'INC', '--act_exclude', 'EXC',
                   '--act_mode', 'cmc', '--act_filter', 'endpoints'], tmp_path)
    assert (args.act_mode, args.act_filter) == ('cmc', 'endpoints')
    args = _parse(['--keyed_noise', '--noise', '0.1', '--act_include', 'INC', '--act_exclude',
                   'EXC', '--act_filter', 'none'], tmp_path)
    assert args.act_filter == 'none' and args.agent is not None
    args = _parse(['--odf_policy', 'det'], tmp_path)
    assert args.act_include is None and args.act_mode is None and args.act_filter is None


@pytest.mark.parametrize('argv,word', [
    (['--act_include', 'INC'], 'go together'),
    (['--act_exclude', 'EXC'], 'go together'),
    (['--act_mode', 'cmc'], '--act_mode'),
    (['--act_filter', 'endpoints'], '--act_filter'),
    (['--act_include', 'INC', '--act_exclude', 'EXC', '--act_mode', 'both'], 'invalid choice'),
    (['--act_include', 'INC', '--act_exclude', 'EXC', '--act_filter', 'all'], 'invalid choice'),
    (['--act_include', 'INC', '--act_exclude', 'nowhere.nii.gz'], 'does not exist'),
])
def test_argparse_errors(argv, word, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(['--odf_policy', 'det'] + argv, tmp_path)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_tracker_refuses_an_unknown_filter():
    from tracktolearn_amd.tracking.tracker import Tracker
    with pytest.raises(ValueError):
        Tracker(None, 1, act_filter='csf')
    assert Tracker(None, 1, act_filter='none').act_filter is None
    assert Tracker(None, 1).act_filter is None


# ------------------------------------------------------------------ GPU part
@pytest.mark.gpu
def test_env_refuses_half_a_pair_and_another_grid():
    with pytest.raises(ValueError):
        make_env(slabs(), None)
    with pytest.raises(ValueError):
        make_env(slabs(), np.zeros((24, 12, 11), F32))
    with pytest.raises(ValueError):
        make_env(slabs(), blob(), mode='threshold')
    with pytest.raises(RuntimeError):
        env = make_env()
        env.reset(0, 4)
        env.act_flags(4, 1)


@pytest.mark.gpu
def test_threshold_mode_ends_every_half_on_the_first_target_point():
    inc, exc = slabs(), np.zeros(DIMS, F32)
    env = make_env(inc, exc)
    records = record_act(env)
    alg = policy(env)
    state = env.reset(0, N)
    assert not env.freerun_supported()
    alg.validation_episode(state, env)
    assert len(env._free_runs) == 0               # the step-by-step loop ran
    n_forward = len(records)
    forward_flags = env.flags.copy()
    assert (forward_flags == TARGET).all()
    alg.validation_episode(env.reset_backward(), env)
    assert n_forward > 6 and len(records) > 2 * n_forward
    assert not any(r['backward'] for r in records[:n_forward])
    assert all(r['backward'] for r in records[n_forward:])
    for rec in records:
        assert np.array_equal(rec['flags'], restated(rec, inc, exc)), rec['n_points']
    flags, lengths, hist = result(env)
    assert (flags == TARGET).all() and np.array_equal(env.flags_forward.cpu().numpy(), forward_flags)
    seed_at = env.seed_index.cpu().numpy()
    assert (seed_at >= 6).all() and (lengths - 1 - seed_at >= 6).all()
    for g in range(N):
        s, L = seed_at[g], lengths[g]
        assert np.allclose(hist[g, s], env.initial_points[g], atol=1e-5)
        over = include_along(inc, hist[g, :L]) > 0.5
        # forward end .. seed .. backward end: only the two ends are in the slabs
        assert over[0] and over[L - 1] and not over[1:L - 1].any(), g
    # no replayed point and no seed was judged
    for rec in records[n_forward:]:
        replaying = rec['init_len'][rec['idx']] >= rec['n_points']
        assert (rec['flags'][replaying] == 0).all()


@pytest.mark.gpu
def test_seeds_inside_the_include_map_still_grow_both_halves():
    inc, exc = slabs(), np.zeros(DIMS, F32)
    env = make_env(inc, exc, x=(21.0, 21.7))
    records = record_act(env)
    both_ways(env, policy(env))
    flags, lengths, hist = result(env)
    init_len = env._init_len.cpu().numpy()
    seed_at = env.seed_index.cpu().numpy()
    assert (include_along(inc, np.ascontiguousarray(env.initial_points, F32)) > 0.5).all()
    assert (init_len >= 2).all()                  # the forward half left the seed
    assert (lengths >= init_len + 1).all()        # ... and so did the backward half
    assert ((flags & TARGET) != 0).all()
    for g in range(N):
        assert np.allclose(hist[g, seed_at[g]], env.initial_points[g], atol=1e-5)
    # the step that put the seed back was not judged although the seed is a target
    at_seed = [r for r in records if r['backward'] and
               (r['init_len'][r['idx']] == r['n_points']).any()]
    assert at_seed
    for rec in at_seed:
        here = rec['init_len'][rec['idx']] == rec['n_points']
        assert (rec['flags'][here] == 0).all()
        assert (restated(rec, inc, exc)[here] == 0).all()
    for rec in records:
        assert np.array_equal(rec['flags'], restated(rec, inc, exc))


def _tracked_seeds(env, alg, act_filter, all_seeds):
    """{seed as bytes: streamline} of ``Tracker.track`` over one batch."""
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env.seeds = all_seeds.copy()
    np.random.seed(11)
    tracker = Tracker(alg, N, min_length=2.0, max_length=60.0, save_seeds=True,
                      bidirectional=True, act_filter=act_filter)
    out = {}
    for item in tracker.track(env, TrkFile):
        out[key(np.asarray(item.data_for_streamline['seeds'], np.float64) + 0.5)] = \
            np.asarray(item.streamline)
    return out


@pytest.mark.gpu
def test_filters_drop_exactly_the_rows_the_restatement_marks():
    inc, exc = one_sided(), blob()
    env = make_env(inc, exc)
    alg = policy(env)
    all_seeds = seeds(N)
    kept_all = _tracked_seeds(env, alg, None, all_seeds)
    assert len(kept_all) == N
    records = record_act(env)
    kept_exclude = _tracked_seeds(env, alg, 'exclude', all_seeds)
    # the restatement's verdict per seed: the bits of the last judged step of each half
    ends = {}
    for rec in records:
        want = restated(rec, inc, exc)
        assert np.array_equal(rec['flags'], want)
        for g, f in zip(rec['idx'], want):
            if f:
                ends.setdefault(key(env.initial_points[g]), {})[rec['backward']] = int(f)
    excluded = {k for k, e in ends.items() if EXCLUDE in e.values()}
    targets = {k for k, e in ends.items() if e.get(False) == TARGET and e.get(True) == TARGET}
    assert 10 < len(excluded) < N // 2
    assert set(kept_all) - set(kept_exclude) == excluded
    assert set(kept_exclude) == set(kept_all) - excluded
    for k, s in kept_exclude.items():
        assert np.array_equal(s.view(np.uint32), kept_all[k].view(np.uint32))
    kept_ends = _tracked_seeds(env, alg, 'endpoints', all_seeds)
    assert set(kept_ends) == targets
    assert 40 < len(targets) < len(kept_exclude)          # the rows with y > 5.5 end on the mask
    assert not (targets & excluded)
    # the host output path drops the same rows
    from tracktolearn_amd.tracking.tracker import Tracker
    env.seeds = all_seeds.copy()
    both_ways(env, alg)
    for act_filter, want in (('exclude', set(kept_all) - excluded), ('endpoints', targets)):
        tracker = Tracker(alg, N, min_length=2.0, max_length=60.0, act_filter=act_filter)
        _, _, kept = tracker._batch_arrays_host(env, 2.0, 60.0)
        assert {key(s) for s in kept.cpu().numpy()} == want
        _, _, kept = tracker._batch_arrays(env, 2.0, 60.0)
        assert {key(s) for s in kept.cpu().numpy()} == want


def _cmc_maps():
    """A quarter of include everywhere between the slabs: every step may stop."""
    inc = slabs()
    inc[3:21] = 0.25
    return inc, blob()


@pytest.mark.gpu
def test_cmc_draws_do_not_depend_on_the_batching():
    inc, exc = _cmc_maps()
    env = make_env(inc, exc, mode='cmc', act_seed=3)
    records = record_act(env)
    alg = policy(env)
    both_ways(env, alg)
    whole = result(env)
    for rec in records:
        assert np.array_equal(rec['flags'], restated(rec, inc, exc, ref_act.CMC, 0.75, 3))
    assert any(((r['flags'] == TARGET).any() and (r['flags'] == 0).any()) for r in records)
    assert len(np.unique(whole[1])) > 8           # the lengths are drawn
    parts = []
    for lo, hi in ((0, N // 2), (N // 2, N)):
        both_ways(env, alg, lo, hi)
        parts.append(result(env))
    same(whole, tuple(np.concatenate([p[k] for p in parts]) for k in range(3)))
    other = make_env(inc, exc, mode='cmc', act_seed=4)
    both_ways(other, policy(other))
    assert not np.array_equal(result(other)[1], whole[1])


@pytest.mark.gpu
def test_without_the_keys_nothing_changes():
    """No ACT keys: the free-running path as before, and the same streamlines as
    with maps that never stop anything."""
    env = make_env()
    alg = policy(env)
    state = env.reset(0, N)
    assert env.freerun_supported() and env._act_desc is None
    alg.validation_episode(state, env)
    assert len(env._free_runs) == 1               # the graph ran
    alg.validation_episode(env.reset_backward(), env)
    plain = result(env)
    assert np.isin(plain[0], (MASK, LENGTH)).all()
    zeros = np.zeros(DIMS, F32)
    quiet = make_env(zeros, zeros)
    quiet.reset(0, N)
    assert not quiet.freerun_supported()
    both_ways(quiet, policy(quiet))
    same(plain, result(quiet))


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from tracktolearn_amd.io import nifti
    root = tmp_path_factory.mktemp('act_track')
    sh, mask = tube.volumes()
    seed_mask = np.zeros(DIMS, np.uint8)
    seed_mask[8:12, 4:8, 4:8] = 1
    aff = np.eye(4)
    for name, vol in (('fodf', sh), ('mask', mask), ('seed', seed_mask), ('inc', one_sided()),
                      ('exc', thick_blob()), ('other_grid', np.zeros((24, 12, 11), F32))):
        nifti.save(str(root / f'{name}.nii.gz'), vol, aff)
    return root


def _argv(files, out, *more):
    return [str(files / 'fodf.nii.gz'), str(files / 'seed.nii.gz'), str(files / 'mask.nii.gz'),
            str(files / out), '--odf_policy', 'det', '--bidirectional', '--npv', '2',
            '--min_length', '10', '--max_length', '60', '--n_actor', '100', '-f'] + list(more)


def _in_memory(argv):
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_track
    from tracktolearn_amd.tracking.tracker import Tracker
    exp = ttl_track.TrackToLearnTrack(vars(ttl_track.parse_args(argv)))
    env = exp.get_tracking_env()
    env.step_size_mm = exp.step_size
    alg = exp._load_policy(env)
    env.load_subject()
    tracker = Tracker(alg, exp.n_actor, min_length=exp.min_length, max_length=exp.max_length,
                      bidirectional=True, act_filter=exp.act_filter)
    ref_img = nifti.load(exp.reference_file)
    header = sio.create_tractogram_header(ref_img.affine, ref_img.shape[:3],
                                          ref_img.get_zooms()[:3])
    return env, tracker, header


@pytest.mark.gpu
@pytest.mark.parametrize('direct', [False, True])
def test_command_writes_the_file_of_the_in_memory_run(files, capsys, direct):
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_track
    from tracktolearn_amd.tracking.tracker import detect_format
    act = ['--act_include', str(files / 'inc.nii.gz'), '--act_exclude', str(files / 'exc.nii.gz')]
    more = act + (['--direct_output'] if direct else [])
    out = 'act_direct.trk' if direct else 'act.trk'
    ttl_track.main(_argv(files, out, *more))
    n_saved = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    ttl_track.main(_argv(files, 'all_' + out, *(more + ['--act_filter', 'none'])))
    n_all = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    assert 50 < n_saved < n_all == 128
    env, tracker, header = _in_memory(_argv(files, 'again_' + out, *more))
    assert env._act_desc is not None and env.act_seed == 1337 and tracker.act_filter == 'exclude'
    again = str(files / ('again_' + out))
    if direct:
        assert tracker.track_to_file(env, again, header) == n_saved
    else:
        assert sio.save(tracker.track(env, detect_format(again)), again, header=header) == n_saved
    assert open(again, 'rb').read() == open(str(files / out), 'rb').read()
    # no streamline of the file has a point the exclude map would have ended
    exc = thick_blob()
    for s in sio.load_trk(str(files / out))[0].streamlines:
        vox = np.ascontiguousarray(np.asarray(s, F32) - F32(0.5))
        assert (include_along(exc, vox) <= 0.5).all()
    assert any((include_along(exc, np.ascontiguousarray(np.asarray(s, F32) - F32(0.5))) > 0.5).any()
               for s in sio.load_trk(str(files / ('all_' + out)))[0].streamlines)


@pytest.mark.gpu
def test_command_without_the_options_is_the_earlier_run(files, capsys):
    """The command of test_odf_tracking's file test, no ACT option: no tissue
    maps reach the env, no filter the Tracker, the graphed loop runs, and the
    file is the in-memory run's."""
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_track
    from tracktolearn_amd.tracking.tracker import detect_format
    argv = _argv(files, 'plain.trk')
    ttl_track.main(argv)
    n_saved = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    env, tracker, header = _in_memory(_argv(files, 'plain_again.trk'))
    assert env._act_desc is None and tracker.act_filter is None
    again = str(files / 'plain_again.trk')
    assert sio.save(tracker.track(env, detect_format(again)), again, header=header) == n_saved == 128
    assert len(env._free_runs) >= 1               # forward halves ran as a graph
    assert open(again, 'rb').read() == open(str(files / 'plain.trk'), 'rb').read()


@pytest.mark.gpu
def test_command_checks_the_grid(files):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(ValueError, match='--act_exclude'):
        ttl_track.main(_argv(files, 'never.trk', '--act_include', str(files / 'inc.nii.gz'),
                             '--act_exclude', str(files / 'other_grid.nii.gz')))
    assert not os.path.exists(str(files / 'never.trk'))
