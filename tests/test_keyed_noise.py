"""Keyed action noise (ttl_env_set_noise / ttl_noise_normals): the
noise of a streamline at a step is a pure function of (seed, global seed index,
step), drawn inside the step's first kernel and optionally scaled by an FA map.

CPU: tests/ref_noise.py (the NumPy restatement) against the Random123 known
answers and against N(0, 1); the C ABI surface.  GPU: the library against the
restatement (1e-13), the in-kernel draw against the pointer path (bit for bit),
independence of the batching and of the loop flavour, the FA rule, the runners."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
SIGMA = 0.1
SEED = 1337
BIG = 2 ** 33 + 5


# --------------------------------------------------------------------------- #
# CPU: the restatement
def test_philox_reproduces_the_random123_known_answers():
    zero = ref_noise.philox(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert [int(w) for w in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = ref_noise.philox(np.full(4, 0xffffffff, np.uint32), np.full(2, 0xffffffff, np.uint32))
    assert [int(w) for w in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


@pytest.mark.parametrize('base', [0, BIG])
@pytest.mark.parametrize('step', [1, 2, 37])
def test_restated_normals_are_standard_normal(base, step):
    from scipy import stats
    z = ref_noise.normals(SEED, base + np.arange(65536, dtype=np.int64), step)
    assert z.shape == (65536, 3) and z.dtype == np.float64
    p = stats.kstest(z.ravel(), 'norm').pvalue
    corr = np.corrcoef(z.T)
    off = np.abs(corr - np.eye(3)).max()
    print(f'KS p={p:.3f} mean={z.mean():.5f} std={z.std():.5f} max off-diagonal corr={off:.5f}')
    assert p > 0.01
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert off < 0.02
    # the rows the FA test leaves out of its quotient (a component below 1e-3)
    assert np.mean(np.abs(z).min(axis=1) < 1e-3) <= 0.01


def test_restated_normals_do_not_repeat_across_steps_or_ids():
    ids = np.arange(4096, dtype=np.int64)
    a, b = ref_noise.normals(SEED, ids, 1), ref_noise.normals(SEED, ids, 2)
    across_steps = abs(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    neighbours = abs(np.corrcoef(a[:-1].ravel(), a[1:].ravel())[0, 1])
    print(f'corr step 1 / step 2: {across_steps:.5f}; neighbouring ids: {neighbours:.5f}')
    assert across_steps < 0.02 and neighbours < 0.02
    # other seed, other id half: other numbers
    assert not np.array_equal(a, ref_noise.normals(SEED + 1, ids, 1))
    assert not np.array_equal(a, ref_noise.normals(SEED, ids + 2 ** 32, 1))
    assert not np.array_equal(a, ref_noise.normals(SEED + 2 ** 32, ids, 1))


# --------------------------------------------------------------------------- #
# CPU: the C ABI surface
def test_header_and_binding_declare_the_entry_points():
    from tracktolearn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert '#define TTL_HAS_KEYED_NOISE' in header
    assert 'TTL_API int ttl_env_set_noise(ttl_env *env, const ttl_noise_desc *desc);' in header
    assert 'TTL_API int ttl_noise_normals(' in header
    assert '#define TTL_ABI_VERSION 13' in header
    for name in ('ttl_env_set_noise', 'ttl_noise_normals'):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    struct = header[header.index('typedef struct ttl_noise_desc {'):
                    header.index('} ttl_noise_desc;')]
    for field, _ in _lib.NoiseDesc._fields_:
        assert field in struct
    assert C.sizeof(_lib.NoiseDesc) == 56


def _host_only_handle(lib, mode):
    """A handle over addresses that are never dereferenced (ttl_env_create does
    no device work): enough for the calls that must fail on the host."""
    from tracktolearn_amd import _lib
    d = _lib.EnvDesc()
    d.abi_version, d.mode = _lib.ABI_VERSION, mode
    d.sh_dim[:] = d.mask_dim[:] = (4, 4, 4)
    d.n_coef, d.coef_pitch = 45, 48
    d.sh_packed = d.mask_coef = 4096
    d.n_dirs, d.max_nb_steps, d.step_size_vox, d.n_max = 4, 10, 0.75, 16
    d.streamlines = d.flags = d.lengths = d.dones = d.idx_a = d.idx_b = 4096
    d.workspace, d.workspace_bytes = 4096, lib.ttl_env_workspace_bytes(16)
    h = C.c_void_p()
    _lib.check(lib.ttl_env_create(C.byref(d), C.byref(h)), 'ttl_env_create')
    return h


def test_set_noise_and_normals_validate_on_the_host():
    from tracktolearn_amd import _lib
    lib = _lib.load()
    nd = _lib.NoiseDesc()
    nd.seed, nd.id_base, nd.sigma = SEED, 0, SIGMA
    assert lib.ttl_env_set_noise(None, C.byref(nd)) == _lib.ERR_INVALID
    assert b'null handle' in lib.ttl_last_error()
    h32 = _host_only_handle(lib, _lib.MODE_F32)
    assert lib.ttl_env_set_noise(h32, C.byref(nd)) == _lib.ERR_INVALID
    assert b'TTL_MODE_F64DIR' in lib.ttl_last_error()
    lib.ttl_env_destroy(h32)
    h = _host_only_handle(lib, _lib.MODE_F64DIR)
    try:
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == 0
        assert lib.ttl_env_set_noise(h, None) == 0            # off again
        for bad in (-0.1, float('nan'), float('inf')):
            nd.sigma = bad
            assert lib.ttl_env_set_noise(h, C.byref(nd)) == _lib.ERR_INVALID
            assert b'sigma' in lib.ttl_last_error()
        nd.sigma, nd.id_base = 0.0, -1
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == _lib.ERR_INVALID
        nd.id_base, nd.fa_coef = 0, 4100                       # not 8-byte aligned
        nd.fa_dim[:] = (4, 4, 4)
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == _lib.ERR_INVALID
        assert b'misaligned' in lib.ttl_last_error()
        nd.fa_coef = 4096
        nd.fa_dim[:] = (4, 0, 4)
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == _lib.ERR_INVALID
        nd.fa_dim[:] = (4, 4, 4)
        nd.noise_out = 4100
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == _lib.ERR_INVALID
        nd.noise_out = 0
        assert lib.ttl_env_set_noise(h, C.byref(nd)) == 0
    finally:
        lib.ttl_env_destroy(h)
    assert lib.ttl_noise_normals(SEED, None, 4, 1, 4096, None) == _lib.ERR_INVALID
    assert lib.ttl_noise_normals(SEED, 4096, 4, 1, None, None) == _lib.ERR_INVALID
    assert lib.ttl_noise_normals(SEED, 4096, -1, 1, 4096, None) == _lib.ERR_INVALID
    assert lib.ttl_noise_normals(SEED, 4096, 4, -1, 4096, None) == _lib.ERR_INVALID
    assert lib.ttl_noise_normals(SEED, 4100, 4, 1, 4096, None) == _lib.ERR_INVALID
    assert lib.ttl_noise_normals(SEED, 4096, 0, 1, 4096, None) == 0   # nothing to do


def test_fa_map_still_needs_keyed_noise():
    """Without device_noise='keyed' the FA branch stays what it was."""
    from tracktolearn_amd.environments.noisy_tracking_env import NoisyTrackingEnvironment
    with pytest.raises(NotImplementedError, match='FA-scaled noise is not supported'):
        NoisyTrackingEnvironment(None, 'testing', dict(noise=0.1, fa_map=np.zeros((4, 4, 4))))


@pytest.mark.parametrize('script', ['ttl_track.py', 'ttl_track_from_hdf5.py'])
def test_runners_offer_keyed_noise(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, script), '--help'],
                         capture_output=True, text=True)
    assert out.returncode == 0
    assert '--keyed_noise' in out.stdout and '--fa_map' in out.stdout
    assert 'unsupported' not in out.stdout.split('--fa_map')[1][:400]


# --------------------------------------------------------------------------- #
# GPU
def _keyed_env(N, K=4, *, D=20, reward=False, keyed=True, fa_map=None, export=False,
               id_offset=0, seeds=None, seed=3):
    import torch
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_subject
    subject = synthetic_subject(D, 45, seed=1234, peaks=True, affine_dtype=np.float32)
    dto = dict(n_dirs=K, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=2.0, max_length=30.0,
               compute_reward=reward, alignment_weighting=1.0, oracle_bonus=0.0,
               rng=np.random.RandomState(0), device=torch.device(DEV),
               target_sh_order=8, noise=SIGMA, fa_map=fa_map)
    if keyed:
        dto.update(device_noise='keyed', noise_seed=SEED, export_noise=export,
                   noise_id_offset=id_offset)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=seed) if seeds is None else seeds
    return env, subject


def _policy(K):
    from test_hip_freerun import _rowwise_policy
    return _rowwise_policy(K)


def _gpu_normals(seed, ids, step):
    import torch
    from tracktolearn_amd import _lib
    ids_dev = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=DEV)
    out = torch.empty((len(ids), 3), dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().ttl_noise_normals(
        seed & 0xffffffffffffffff, ids_dev.data_ptr(), len(ids), step, out.data_ptr(), None),
        'ttl_noise_normals')
    torch.cuda.synchronize()
    return out.cpu().numpy()


MIXED_IDS = np.concatenate([np.arange(100), 2 ** 32 - 1 + np.arange(3), 2 ** 31 + np.arange(-2, 3),
                            BIG + np.arange(150), 977 * np.arange(1, 43) ** 3]).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', [SEED, 2 ** 63 + 11])
@pytest.mark.parametrize('step', [1, 37])
def test_library_normals_equal_the_restatement(seed, step):
    assert len(MIXED_IDS) == 300
    got = _gpu_normals(seed, MIXED_IDS, step)
    want = ref_noise.normals(seed, MIXED_IDS, step)
    err = np.abs(got - want).max()
    print(f'max |library - restatement| = {err:.3e}')
    assert err <= 1e-13


def _snapshot(env):
    return env.flags.copy(), env.lengths.copy(), env.dones.copy(), env.streamlines.copy()


@pytest.mark.gpu
def test_in_kernel_draw_equals_the_pointer_path():
    """300 rows (a partial second workgroup) to exhaustion: a second handle on
    the host-noise path, fed with the exported noise, must do exactly the same;
    the exported noise is sigma times the restatement's normals."""
    import torch
    N, K = 300, 4
    keyed, _ = _keyed_env(N, K, reward=True, export=True, id_offset=BIG)
    plain, _ = _keyed_env(N, K, reward=True, keyed=False)
    fed = {}
    plain._noise_for = lambda actions: fed['noise']
    policy = _policy(K)
    s_k, s_p = keyed.reset(0, N), plain.reset(0, N)
    assert torch.equal(s_k, s_p)
    worst, steps = 0.0, 0
    while s_k.shape[0] > 0:
        L = keyed.length
        idx = keyed.continue_idx
        a = policy(s_k)
        st_k, r_k, d_k, _ = keyed.step_device(a)
        exported = keyed.noise_out[torch.as_tensor(idx, device=DEV)].clone()
        fed['noise'] = exported
        st_p, r_p, d_p, _ = plain.step_device(a.clone())
        assert torch.equal(d_k, d_p) and torch.equal(r_k, r_p)
        assert torch.equal(st_k, st_p)
        for x, y in zip(_snapshot(keyed), _snapshot(plain)):
            assert np.array_equal(x, y)
        want = SIGMA * ref_noise.normals(SEED, BIG + idx, L)
        worst = max(worst, float(np.abs(exported.cpu().numpy() - want).max()))
        s_k, _ = keyed.harvest()
        s_p, _ = plain.harvest()
        assert torch.equal(s_k, s_p)
        steps += 1
    print(f'{steps} steps, max |exported - sigma * restatement| = {worst:.3e}')
    assert steps > 5 and worst <= SIGMA * 1e-13
    # the step refuses noise rows while keyed noise is set
    from tracktolearn_amd import _lib
    keyed.reset(0, N)
    a = policy(keyed.reset(0, N)).contiguous()
    done = torch.empty(N, dtype=torch.uint8, device=DEV)
    rows = torch.zeros((N, 3), dtype=torch.float64, device=DEV)
    rc = keyed._lib.ttl_env_step_begin(keyed._handle, a.data_ptr(), rows.data_ptr(), N, None,
                                       done.data_ptr(), keyed._stream())
    assert rc == _lib.ERR_INVALID


@pytest.mark.gpu
def test_keyed_noise_counts_from_the_batchs_one_id_base():
    """``reset(start, end)`` on a shard whose seeds begin at ``noise_id_offset``:
    streamline g of the batch draws as seed ``streamline_id_base() + g`` of the
    run -- the one id base, which the fODF policy keys on as well."""
    import torch
    n_seeds, K, start, offset = 12, 4, 5, 1000
    env, _ = _keyed_env(n_seeds, K, export=True, id_offset=offset)
    state = env.reset(start, n_seeds)
    n = n_seeds - start
    assert env.streamline_id_base() == offset + start
    L = env.length
    env.step_device(_policy(K)(state))
    got = env.noise_out.cpu().numpy()
    want = SIGMA * _gpu_normals(SEED, env.streamline_id_base() + np.arange(n), L)
    print(f'max |exported - sigma * library normals| = {np.abs(got - want).max():.3e}')
    assert got.shape == (n, 3) and np.array_equal(got, want)
    env.harvest()
    # nreset counts from the offset alone
    env.nreset(3)
    assert env.streamline_id_base() == offset
    torch.cuda.synchronize()


def _track(env, policy, start, end):
    state = env.reset(start, end)
    while state.shape[0] > 0:
        env.step_device(policy(state))
        state, _ = env.harvest()
    t = env.get_streamlines()
    return list(t.streamlines), t.data_per_streamline['flags'].copy()


def _same_tracts(a, b):
    (lines_a, flags_a), (lines_b, flags_b) = a, b
    assert np.array_equal(flags_a, flags_b) and len(lines_a) == len(lines_b)
    for x, y in zip(lines_a, lines_b):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_tractogram_does_not_depend_on_the_batching():
    N, K = 3000, 4
    env, _ = _keyed_env(N, K)
    policy = _policy(K)
    whole = _track(env, policy, 0, N)
    assert np.mean([len(s) for s in whole[0]]) > 3
    for cuts in ((0, 1700, N), (0, 257, 1999, N)):
        lines, flags = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = _track(env, policy, lo, hi)
            lines += part[0]
            flags.append(part[1])
        _same_tracts(whole, (lines, np.concatenate(flags)))
    fresh, _ = _keyed_env(N, K)
    _same_tracts(whole, _track(fresh, policy, 0, N))
    # and it IS noisy: sigma = 0 tracks something else
    env.noise = 0.0
    quiet = _track(env, policy, 0, N)
    assert any(len(x) != len(y) or not np.array_equal(x, y) for x, y in zip(whole[0], quiet[0]))


@pytest.mark.gpu
def test_loop_flavours_agree_and_equal_the_oracle():
    """Graphed (captured, then replayed from the cache), eager free-running and
    step-by-step loops under keyed noise: the same flags, lengths and points;
    and the CPU oracle's noisy env, fed with float64(action) + exported noise,
    tracks the same."""
    import torch
    from test_hip_loops import _oracle
    N, K = 3000, 4
    env, subject = _keyed_env(N, K, export=True)
    policy = _policy(K)
    # step by step, recording what the oracle is fed
    state = env.reset(0, N)
    assert env.freerun_supported()
    fed = []
    while state.shape[0] > 0:
        idx = torch.as_tensor(env.continue_idx, device=DEV)
        a = policy(state)
        env.step_device(a)
        fed.append(a.double().cpu().numpy() + env.noise_out[idx].cpu().numpy())
        state, _ = env.harvest()
    want = _snapshot(env)
    ref = _oracle(env, subject, noisy=True, K=K, reward=False)
    ref.reset(0, N)
    for rows in fed:
        ref.step(rows)
        ref.harvest()
    assert len(ref.continue_idx) == 0
    assert np.array_equal(want[0], ref.flags) and np.array_equal(want[1], ref.lengths)
    assert np.array_equal(want[3], ref.streamlines)
    # graphed, twice
    for rep in range(2):
        state = env.reset(0, N)
        assert env.freerun_supported()
        _, n_steps = env.run_free(policy, state, key='rowwise')
        assert env._n_active == 0 and n_steps == len(fed)
        for x, y in zip(want, _snapshot(env)):
            assert np.array_equal(x, y)
    assert len(env._free_runs) == 1
    # eager free-running
    state = env.reset(0, N)
    _, n_steps = env.run_free_eager(policy, state)
    assert env._n_active == 0 and n_steps == len(fed)
    for x, y in zip(want, _snapshot(env)):
        assert np.array_equal(x, y)
    # set_noise is refused while free-running and between a step and its harvest
    from tracktolearn_amd import _lib
    state = env.reset(0, N)
    env.step_device(policy(state))
    assert env._lib.ttl_env_set_noise(env._handle, None) == _lib.ERR_STATE
    env.harvest()
    _lib.check(env._lib.ttl_env_freerun_begin(env._handle, None, env._stream()))
    assert env._lib.ttl_env_set_noise(env._handle, None) == _lib.ERR_STATE
    _lib.check(env._lib.ttl_env_freerun_end(env._handle, None, None, None, env._stream()))


def _fa_volume(D=20):
    """A smooth random field in [0, 1] plus a 3^3 block of 1.4 (FA > 1: the
    clamp)."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.RandomState(5)
    fa = gaussian_filter(rng.uniform(0.0, 1.0, (D, D, D)), 2.0)
    fa = (fa - fa.min()) / (fa.max() - fa.min())
    fa[9:12, 9:12, 9:12] = 1.4
    return fa


@pytest.mark.gpu
def test_fa_map_scales_the_noise():
    import torch
    from scipy.ndimage import map_coordinates, spline_filter
    D, K = 20, 4
    fa = _fa_volume(D)
    coef = spline_filter(fa, order=3, output=np.float64)
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_volumes
    mask = synthetic_volumes(D, 45, peaks=False)[1]
    rng = np.random.RandomState(9)
    inside = synthetic_seeds(mask, 500, seed=4)
    # voxels on and next to every face (the mirror-folded taps), the 1.4 block,
    # and points outside the volume
    g = np.array([0, 1, 18, 19])
    faces = np.array([(x, y, z) for x in g for y in (1, 7, 19) for z in (0, 12, 18)] +
                     [(y, x, z) for x in g for y in (1, 7, 19) for z in (0, 12, 18)] +
                     [(y, z, x) for x in g for y in (1, 7, 19) for z in (0, 12, 18)], float)
    faces = faces + rng.uniform(0.05, 0.95, faces.shape)
    # (FA is sampled at the cell's lower corner, trunc(p) - 0.5: the corners of
    # cells 10 and 11 have only block voxels next to them)
    block = np.array([(x, y, z) for x in (10, 11) for y in (10, 11) for z in (10, 11)] * 4,
                     float) + rng.uniform(0.05, 0.95, (32, 3))
    outside = np.array([[-2.3, 5.0, 5.0], [5.0, 21.5, 5.0], [5.0, 5.0, 20.2], [-0.5, -0.5, 30.0],
                        [0.4, 5.0, 5.0]])
    seeds = np.concatenate([inside, faces, block, outside])
    N = len(seeds)
    env, _ = _keyed_env(N, K, fa_map=fa, export=True, seeds=seeds)
    policy = _policy(K)
    state = env.reset(0, N)
    worst, rows_used, rows_skipped, block_rows, steps = 0.0, 0, 0, 0, 0
    while state.shape[0] > 0:
        L = env.length
        idx = env.continue_idx
        p = env._buf_streamlines[torch.as_tensor(idx, device=DEV), L - 1].cpu().numpy()
        env.step_device(policy(state))
        noise = env.noise_out[torch.as_tensor(idx, device=DEV)].cpu().numpy()
        z = ref_noise.normals(SEED, idx, L)
        cell = np.trunc(p).astype(np.int32)
        value = map_coordinates(coef, (cell - 0.5).T, order=3, mode='constant', prefilter=False)
        want = np.maximum(0.0, (1.0 - value) * SIGMA)
        # exactly 0.0 where the clamp bites (the 1.4 block)
        clamped = want == 0.0
        assert np.array_equal(noise[clamped], np.zeros((clamped.sum(), 3)))
        in_block = ((cell >= 10) & (cell <= 11)).all(axis=1)
        assert clamped[in_block].all()
        block_rows += int(in_block.sum())
        # outside the volume: the plain sigma
        out = ((cell - 0.5 < 0) | (cell - 0.5 > D - 1)).any(axis=1)
        assert np.array_equal(want[out], np.full(out.sum(), SIGMA))
        use = (np.abs(z).min(axis=1) >= 1e-3) & ~clamped
        rows_used += int(use.sum())
        rows_skipped += int((~use & ~clamped).sum())
        got = noise[use] / z[use]
        worst = max(worst, float(np.abs(got - want[use, None]).max()))
        if L == 1:
            assert out[-5:].all() and in_block[-37:-5].all() and not out[:500].any()
            folded = ((cell == 1) | (cell == 19)).any(axis=1) & ~out
            assert folded.sum() >= 20
        state, _ = env.harvest()
        steps += 1
    print(f'{steps} steps, {rows_used} rows in the quotient, {rows_skipped} left out, '
          f'{block_rows} in the block; max |sigma_kernel - sigma_scipy| = {worst:.3e} '
          f'(sigma = {SIGMA})')
    assert block_rows >= 32 and rows_used > 2000
    assert rows_skipped <= 0.01 * (rows_used + rows_skipped)
    assert worst <= 1e-12 * SIGMA


def _runner_inputs(tmp_path):
    from test_runners import _write_agent, _write_inputs
    paths, aff = _write_inputs(tmp_path, D=24)
    agent_dir, hp = _write_agent(tmp_path, 7 * 45 + 3 * 4)
    common = [paths['odf'], paths['seed'], paths['mask']]
    # no lower length limit: under noise a randomly initialised policy turns too
    # sharply within a step or two for most seeds, and every seed's streamline
    # should take part in the comparison (none can exceed the upper limit:
    # int(40 / 0.75) steps of 0.75 mm)
    opts = ['--agent', agent_dir, '--hyperparameters', hp, '--min_length', '0',
            '--max_length', '40', '--rng_seed', '5', '--noise', str(SIGMA)]
    return paths, aff, common, opts


@pytest.mark.gpu
def test_ttl_track_keyed_noise_does_not_depend_on_n_actor(tmp_path, monkeypatch):
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_track
    # fixed 512-row policy tiles: a row's action does not depend on its batch
    monkeypatch.setenv('TTL_POLICY_TILE_ROWS', '512')
    paths, aff, common, opts = _runner_inputs(tmp_path)
    small, large, scaled = (str(tmp_path / f'{k}.trk') for k in ('small', 'large', 'scaled'))
    ttl_track.main(common + [small] + opts + ['--keyed_noise', '--n_actor', '512'])
    ttl_track.main(common + [large] + opts + ['--keyed_noise', '--n_actor', '2000'])
    assert open(small, 'rb').read() == open(large, 'rb').read()
    tg, _ = sio.load_trk(small)
    n_seeds = int(nifti.load(paths['seed']).get_fdata().sum())     # npv 1
    print(f'{len(tg)} streamlines of {n_seeds} seeds, '
          f'{np.mean([len(x) for x in tg.streamlines]):.1f} points on average')
    assert n_seeds > 2000 and len(tg) == n_seeds        # several batches either way
    assert max(len(x) for x in tg.streamlines) > 3
    fa_path = str(tmp_path / 'fa.nii.gz')
    nifti.save(fa_path, _fa_volume(24).astype(np.float32), aff)
    ttl_track.main(common + [scaled] + opts + ['--fa_map', fa_path, '--n_actor', '2000'])
    tf, _ = sio.load_trk(scaled)
    assert len(tf) == n_seeds
    assert open(scaled, 'rb').read() != open(large, 'rb').read()
    # an FA map on another grid is refused
    nifti.save(fa_path, _fa_volume(20).astype(np.float32), aff)
    with pytest.raises(ValueError, match='grid'):
        ttl_track.main(common + [str(tmp_path / 'no.trk')] + opts + ['--fa_map', fa_path])
