"""Classical tracking from the fODF end to end (tracking/odf_policy.py,
``ttl_track.py --odf_policy``): a tube of voxels that all hold one
sharp lobe along x, tracked step by step, through the graphed free-running
loop, both ways from the seed, in halves, under three affines and from the
command line into a file that the Tractometer scores."""
import functools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ref_odf_policy as ref
from tracktolearn_amd.reconst import peaks as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
DIMS = (24, 12, 12)
ORDER, C_SH, K = 6, 28, 2
TUBE = (slice(1, 23), slice(3, 9), slice(3, 9))
MASK, LENGTH, CURVATURE = 1, 2, 4

AFFINES = {
    'identity': np.eye(4),
    'las': np.diag([-1.0, 1.0, 1.0, 1.0]),
    'rot20z': np.array([[np.cos(np.deg2rad(20)), -np.sin(np.deg2rad(20)), 0, 0],
                        [np.sin(np.deg2rad(20)), np.cos(np.deg2rad(20)), 0, 0],
                        [0, 0, 1, 0], [0, 0, 0, 1.0]]),
}


@functools.lru_cache(maxsize=None)
def lobe_sh():
    """SH (order 6, least squares on the package's hemisphere) of the sharp
    lobe |d . x|^24 along world x."""
    verts, _ = pk.hemisphere(3)
    B = pk.sh_to_sf_matrix(verts, ORDER)
    target = np.abs(verts[:, 0]) ** 24
    return np.linalg.lstsq(B.T, target, rcond=None)[0].astype(F32)


def volumes():
    sh = np.broadcast_to(lobe_sh(), DIMS + (C_SH,)).copy()
    mask = np.zeros(DIMS, np.uint8)
    mask[TUBE] = 1
    return sh, mask


def tube_seeds(n, seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(10.0, 14.0, n), rng.uniform(4.5, 6.5, n),
                     rng.uniform(4.5, 6.5, n)], axis=1)


def make_env(n, affine=None, max_length=40.0):
    import torch
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    sh, mask = volumes()
    aff = np.asarray(AFFINES['identity'] if affine is None else affine, np.float32)
    dto = dict(n_dirs=K, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=max_length, compute_reward=False,
               alignment_weighting=0.0, oracle_bonus=0.0, rng=np.random.RandomState(0),
               device=torch.device(DEV), target_sh_order=ORDER)
    env = TrackingEnvironment((Vol(sh, aff), Vol(mask, aff), Vol(mask, aff), None, None),
                              'testing', dto)
    env.seeds = tube_seeds(n)
    return env


# ------------------------------------------------------------------ CPU part
def test_lobe_peaks_along_x():
    verts, _ = pk.hemisphere(3)
    sf = lobe_sh().astype(np.float64) @ pk.sh_to_sf_matrix(verts, ORDER)
    assert abs(verts[np.argmax(sf)][0]) == pytest.approx(1.0, abs=1e-12)
    assert np.sort(sf)[-2] < 0.9 * sf.max()


@pytest.mark.parametrize('name', sorted(AFFINES))
def test_directions_in_voxel_axes(name):
    """A step along dirs[v] in voxel space moves along vertex v in world space."""
    from tracktolearn_amd.tracking.odf_policy import voxel_directions
    verts, _ = pk.hemisphere(3)
    lin = AFFINES[name][:3, :3]
    d = voxel_directions(verts, AFFINES[name])
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-12)
    world = d @ lin.T
    world /= np.linalg.norm(world, axis=1, keepdims=True)
    assert np.allclose(world, verts, atol=1e-12)
    x = int(np.argmax(np.abs(verts[:, 0])))
    want = {'identity': (1, 0, 0), 'las': (-1, 0, 0),
            'rot20z': (np.cos(np.deg2rad(20)), -np.sin(np.deg2rad(20)), 0)}[name]
    assert np.allclose(d[x] * np.sign(verts[x, 0]), want, atol=1e-12)


def _parse(argv, tmp_path):
    from tracktolearn_amd.runners import ttl_track
    files = []
    for name in ('fodf', 'seed', 'mask'):
        f = tmp_path / f'{name}.nii.gz'
        f.write_bytes(b'')
        files.append(str(f))
    return ttl_track.parse_args(files + [str(tmp_path / 'out.trk')] + argv)


def test_help_lists_the_options(capsys):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(SystemExit) as e:
        ttl_track.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--odf_policy {det,prob}', '--theta DEG', '--sf_threshold R', '--step_size MM'):
        assert opt in text


def test_odf_policy_needs_no_agent(tmp_path):
    args = _parse(['--odf_policy', 'prob', '--bidirectional', '--compress', '0.1',
                   '--direct_output', '--save_seeds', '--npv', '3'], tmp_path)
    assert args.odf_policy == 'prob' and args.agent is None and args.hyperparameters is None
    assert args.theta is None and args.sf_threshold == 0.1 and args.step_size is None
    args = _parse(['--odf_policy', 'det', '--theta', '30', '--sf_threshold', '0.2',
                   '--step_size', '0.5'], tmp_path)
    assert (args.theta, args.sf_threshold, args.step_size) == (30.0, 0.2, 0.5)


@pytest.mark.parametrize('argv,word', [
    (['--odf_policy', 'det', '--noise', '0.1'], '--noise'),
    (['--odf_policy', 'det', '--agent', 'x', '--hyperparameters', 'y'], '--agent'),
    (['--odf_policy', 'both'], 'invalid choice'),
    (['--odf_policy', 'det', '--theta', '120'], '--theta'),
    (['--odf_policy', 'det', '--sf_threshold', '2'], '--sf_threshold'),
    (['--odf_policy', 'det', '--step_size', '0'], '--step_size'),
    (['--theta', '30'], '--odf_policy'),
    (['--step_size', '0.5'], '--odf_policy'),
    (['--sf_threshold', '0.5'], '--odf_policy'),
])
def test_argparse_errors(argv, word, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(argv, tmp_path)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_header_declares_the_entry_points(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'#define TTL_HAS_ODF_POLICY 1', text)
    body = text[text.index('#define TTL_HAS_ODF_POLICY 1'):]
    for name in ('ttl_odf_actions', 'ttl_env_freerun_odf_actions'):
        assert re.search(r'TTL_API int %s\(' % name, body)
    cc = shutil.which('gcc')
    assert cc is not None
    src = tmp_path / 'odf.c'
    src.write_text('#include "ttl_hip.h"\n#ifndef TTL_HAS_ODF_POLICY\n#error no policy\n#endif\n'
                   'int main(void) { return ttl_odf_actions(0, 0, 0, 0, 0, 0, 0, 0.f, 0.f, '
                   'TTL_ODF_PROB, 0, 0, 0, 0, 0, 0, 0, 0) + ttl_env_freerun_odf_actions(0, 0, 0, '
                   '0, 0, 0, 0, 0, 0.f, 0.f, TTL_ODF_DET, 0, 0, 0, 0, 0, 0); }\n')
    out = subprocess.run([cc, '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic',
                          '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_library_binding_names_the_entry_points():
    from tracktolearn_amd import _lib
    assert len(_lib.SYMBOLS['ttl_odf_actions'][1]) == 18
    assert len(_lib.SYMBOLS['ttl_env_freerun_odf_actions'][1]) == 17


# ------------------------------------------------------------------ GPU part
N_SMALL = 512


@pytest.fixture(scope='module')
def env():
    return make_env(4096)


def _policy(env, mode, seed=5):
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    return OdfTracking(env, mode, seed=seed)


def _result(env):
    """(flags, lengths, history rows) of the finished batch, host copies."""
    n = env._n_total
    return env.flags.copy(), env.lengths.copy(), env.streamlines[:n].copy()


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for la, ra, rb in zip(a[1], a[2], b[2]):
        assert np.array_equal(ra[:la].view(np.uint32), rb[:la].view(np.uint32))


def _step_loop(env, agent, state, records=None):
    while state.shape[0] > 0:
        a = agent.select_action(state)
        if records is not None:
            records.append((state.cpu().numpy(), env.continue_idx.copy(), env.length - 1,
                            a.cpu().numpy(), agent._seed_now()))
        env.step_device(a)
        state, _ = env.harvest()


def _check_records(env, agent, records, id_base):
    from tracktolearn_amd.tracking.odf_policy import MODES
    B, dirs = agent.sf_matrix.cpu().numpy(), agent.dirs.cpu().numpy()
    assert len(records) > 5
    for state, idx, step, action, seed in records:
        want, _ = ref.actions_ordered(
            state[:, :C_SH], state[:, 7 * C_SH:7 * C_SH + 3], B, dirs, agent.cos_theta,
            agent.rel_threshold, MODES[agent.mode], seed=seed, ids=id_base + idx, step=step)
        assert np.array_equal(action.view(np.uint32), want.view(np.uint32)), step


def _in_tube(env, slack=1.5):
    """``slack``: how far past the tube's faces the cubic-spline mask can still
    read 0.1 (1/6 one voxel past the last voxel centre, 0.02 at 1.5)."""
    tract = env.get_streamlines()
    flags = tract.data_per_streamline['flags'].astype(int).reshape(-1)
    assert (flags & CURVATURE == 0).all()
    assert ((flags == MASK) | (flags == LENGTH)).all() and (flags == MASK).mean() > 0.5
    pts = np.concatenate(tract.streamlines)
    lo = np.array([t.start for t in TUBE]) - 0.5 - slack
    hi = np.array([t.stop for t in TUBE]) - 0.5 + slack
    assert (pts >= lo).all() and (pts <= hi).all()
    return tract


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['det', 'prob'])
def test_step_by_step_tracking_follows_the_lobe(env, mode):
    """Every action equals the restatement of the state it saw; the streamlines
    stay in the tube and end on MASK or LENGTH; turned round, the two halves
    leave the seed in opposite directions."""
    agent = _policy(env, mode).agent
    start = 64
    records = []
    _step_loop(env, agent, env.reset(start, start + N_SMALL), records)
    _check_records(env, agent, records, start)
    tract = _in_tube(env)
    if mode == 'det':       # the lobe's maximum is the x vertex: y and z never move
        for s in tract.streamlines:
            assert np.ptp(s[:, 1]) == 0 and np.ptp(s[:, 2]) == 0 and len(s) > 8
    forward_len = env.lengths.copy()
    back = []
    _step_loop(env, agent, env.reset_backward(), back)
    assert back[0][4] == agent.seed ^ agent.BACKWARD_SEED_XOR != agent.seed
    _check_records(env, agent, back, start)
    _in_tube(env)
    hist, lengths = env.streamlines, env.lengths
    seed_at = env.seed_index.cpu().numpy()
    both = np.nonzero((seed_at >= 1) & (lengths > seed_at + 2))[0]
    assert len(both) > N_SMALL // 2
    for g in both:
        s = seed_at[g]
        assert np.allclose(hist[g, s], env.initial_points[g], atol=1e-5)
        assert np.dot(hist[g, s - 1] - hist[g, s], hist[g, s + 1] - hist[g, s]) < 0
    assert (lengths >= forward_len - 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [N_SMALL, 4096])
@pytest.mark.parametrize('mode', ['det', 'prob'])
def test_graphed_episode_equals_the_step_by_step_loop(env, mode, n):
    alg = _policy(env, mode)
    _step_loop(env, alg.agent, env.reset(0, n))
    eager = _result(env)
    env._free_runs.clear()
    state = env.reset(0, n)
    assert env.freerun_supported()
    alg.validation_episode(state, env)
    assert len(env._free_runs) == 1 and not env._free_running     # the graph ran
    _same(eager, _result(env))
    if mode == 'prob':
        other = _policy(env, mode, seed=6)
        other.validation_episode(env.reset(0, n), env)
        assert len(env._free_runs) == 2                           # another seed, another graph
        r = _result(env)
        assert not all(np.array_equal(a[:l], b[:l]) for l, a, b in zip(eager[1], eager[2], r[2]))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['det', 'prob'])
def test_halved_batch_gives_the_same_streamlines(env, mode):
    alg = _policy(env, mode)
    n = N_SMALL
    alg.validation_episode(env.reset(0, n), env)
    whole = _result(env)
    parts = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        alg.validation_episode(env.reset(lo, hi), env)
        parts.append(_result(env))
    halves = tuple(np.concatenate([a[k] for a in parts]) for k in range(3))
    _same(whole, halves)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(AFFINES))
def test_first_step_goes_along_world_x(name):
    """A lobe along world x: the first action, mapped to world space, is +-x,
    whichever voxel axes the affine gives the volume."""
    from tracktolearn_amd.tracking.odf_policy import OdfPolicy
    env = make_env(64, AFFINES[name])
    agent = OdfPolicy(env, 'det')
    a = agent.select_action(env.reset(0, 64)).cpu().numpy().astype(np.float64)
    world = a @ AFFINES[name][:3, :3].T
    world /= np.linalg.norm(world, axis=1, keepdims=True)
    assert np.allclose(np.abs(world[:, 0]), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(a, axis=1), 1.0, atol=1e-6)
    if name == 'rot20z':
        assert np.allclose(np.abs(a[:, 1]), np.sin(np.deg2rad(20)), atol=1e-6)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from tracktolearn_amd.io import nifti
    root = tmp_path_factory.mktemp('odf_track')
    sh, mask = volumes()
    seed_mask = np.zeros(DIMS, np.uint8)
    seed_mask[10:14, 4:8, 4:8] = 1
    aff = np.eye(4)
    nifti.save(str(root / 'fodf.nii.gz'), sh, aff)
    nifti.save(str(root / 'mask.nii.gz'), mask, aff)
    nifti.save(str(root / 'seed.nii.gz'), seed_mask, aff)
    scoring = root / 'scoring'
    scoring.mkdir()
    head, tail = np.zeros(DIMS, np.uint8), np.zeros(DIMS, np.uint8)
    head[1:4, 3:9, 3:9] = 1
    tail[20:23, 3:9, 3:9] = 1
    nifti.save(str(scoring / 'head.nii.gz'), head, aff)
    nifti.save(str(scoring / 'tail.nii.gz'), tail, aff)
    nifti.save(str(scoring / 'ref.nii.gz'), np.zeros(DIMS, np.uint8), aff)
    (scoring / 'scil_scoring_config.json').write_text(json.dumps(
        {'tube': {'head': 'head.nii.gz', 'tail': 'tail.nii.gz'}}))
    return root


@pytest.mark.gpu
def test_command_tracks_both_ways_into_a_file_the_tractometer_scores(files, capsys):
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_score_tractogram as score_cmd
    from tracktolearn_amd.runners import ttl_track
    from tracktolearn_amd.tracking.tracker import Tracker, detect_format
    out = str(files / 'tube.trk')
    argv = [str(files / 'fodf.nii.gz'), str(files / 'seed.nii.gz'), str(files / 'mask.nii.gz'), out,
            '--odf_policy', 'det', '--bidirectional', '--npv', '2', '--min_length', '10',
            '--max_length', '60', '--n_actor', '100', '-f']
    ttl_track.main(argv)
    n_saved = int(re.search(r'Saved (\d+) streamlines', capsys.readouterr().out).group(1))
    loaded = sio.load_trk(out)[0]
    assert n_saved == len(loaded.streamlines) > 100
    # the same experiment in memory
    exp = ttl_track.TrackToLearnTrack(vars(ttl_track.parse_args(argv)))
    env = exp.get_tracking_env()
    env.step_size_mm = exp.step_size
    alg = exp._load_policy(env)
    env.load_subject()
    tracker = Tracker(alg, exp.n_actor, min_length=exp.min_length, max_length=exp.max_length,
                      bidirectional=True)
    from tracktolearn_amd.io import nifti
    ref_img = nifti.load(exp.reference_file)
    header = sio.create_tractogram_header(ref_img.affine, ref_img.shape[:3],
                                          ref_img.get_zooms()[:3])
    again = str(files / 'again.trk')
    assert sio.save(tracker.track(env, detect_format(out)), again, header=header) == n_saved
    assert open(again, 'rb').read() == open(out, 'rb').read()
    lines = loaded.streamlines
    # whole streamlines run from one end of the tube to the other
    assert np.mean([np.ptp(s[:, 0]) > 17 for s in lines]) > 0.9
    result_dir = str(files / 'scored')
    score_cmd.main([out, str(files / 'scoring'), result_dir, '--reference',
                    str(files / 'scoring' / 'ref.nii.gz')])
    result = json.load(open(os.path.join(result_dir, 'results.json')))
    print('tractometer on the tracked tube:', {k: result[k] for k in ('VC', 'VB', 'n')
                                               if k in result})
    assert result['VC'] > 0 and result['VB'] == 1
