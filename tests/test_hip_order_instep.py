"""The in-step re-bucket of the processing order (TTL_ORDER_INSTEP=P): k_tail
counts the survivors' bricks on every P-th step of an episode and
k_order_scatter writes the next step's order from the counts.

Scheduling only, so every output of every step must be BIT-identical to the
same episode with in-step off (same seeds, same actions): continue_idx,
row_dest, flags, dones, lengths, the reward, the state rows mapped by
streamline.  The state rows are written into buffers the test owns and has
filled with NaN: a slot the new order drops leaves its row NaN, and a
duplicated slot means another one is dropped (the order is as long as the
survivors), so either fails the comparison and the NaN check.

That the comparison catches it was proved once on a scratch build whose
k_order_scatter wrote `out[p + 1]` instead of `out[p]` for the first slot of
every bin (one slot lost and one overwritten per bin): all ten GPU cases this
file had then (every one but `late_order`) failed on it, the first at the NaN check of the step after a re-bucket.

Shapes (the smallest at which the kernels can still go wrong): a 24^3 volume
= 4 bricks per axis of the raster (3 hold voxels, the ball mask leaves the
corner bins empty), 700 streamlines = three 256-slot blocks with the last one
partial, not a multiple of the gather's 20-row blocks.  TTL_ORDER_MIN_ROWS=1
and TTL_FUSE_MAX_ROWS=256 keep the processing order -- and k_tail -- in use
down to 256 rows; SPATIAL_ORDER_MIN is patched as in test_hip_env_parity.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import synthetic_subject

D, N = 24, 700


def _env(monkeypatch, instep, *, n_dirs=4, f64=False, reward=False, seeds=None):
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import (NoisyTrackingEnvironment,
                                               TrackingEnvironment)
    monkeypatch.setenv('TTL_ORDER_INSTEP', str(instep))
    monkeypatch.setenv('TTL_ORDER_MIN_ROWS', '1')
    monkeypatch.setenv('TTL_FUSE_MAX_ROWS', '256')
    monkeypatch.setattr(TrackingEnvironment, 'SPATIAL_ORDER_MIN', 1)
    sh, mask, pk = synthetic_subject(D)
    aff = np.eye(4, dtype=np.float64 if f64 else np.float32)
    subject = (Vol(sh, aff), Vol(mask.astype(np.float32), aff),
               Vol(mask.astype(np.float32), aff), Vol(pk, aff), None)
    dto = dict(n_dirs=n_dirs, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=2.0, max_length=25.0, compute_reward=reward,
               alignment_weighting=1.0, oracle_bonus=0.0, oracle_checkpoint=None,
               oracle_stopping_criterion=False, rng=np.random.RandomState(0),
               device=torch.device('cuda:0'), target_sh_order=8, noise=0.0, fa_map=None)
    # float64-direction mode is the noisy environment's (sigma 0: no noise drawn)
    cls = NoisyTrackingEnvironment if f64 else TrackingEnvironment
    env = cls(subject, 'testing', dto)
    env.seeds = seeds
    return env


def _seeds(seed=11):
    _, mask, _ = synthetic_subject(D)
    rng = np.random.RandomState(seed)
    vox = np.argwhere(mask)
    return vox[rng.randint(0, len(vox), N)] + rng.uniform(-0.5, 0.5, (N, 3))


def _order_state(env):
    slots, period = C.c_int32(-1), C.c_int32(-1)
    assert env._lib.ttl_env_order_slots(env._handle, C.byref(slots), C.byref(period)) == 0
    return slots.value, period.value


def _own_state_buffers(env):
    """Every step's state rows go into a fresh NaN-filled tensor of the test."""
    def poisoned(n):
        return torch.full((n, env._state_pitch), float('nan'), dtype=torch.float32,
                          device=env.device)[:, :env._state_width]
    env._ring_state = poisoned
    env._new_state = poisoned


def _episode(monkeypatch, instep, *, wobble=0.2, refresh_at=(), restop=False, late_order=False,
             **kw):
    """One episode to exhaustion through step_device()/harvest(); returns the
    per-step records and the (slots, rows) pairs seen after each harvest while
    the order was in use."""
    env = _env(monkeypatch, instep, seeds=_seeds(), **kw)
    if late_order:
        # no order at reset; the forced refresh before step 1 installs the first one,
        # and the re-bucket steps must find their count buffers clear all the same
        env.spatial_order = False
        refresh_at = (1,)
    state = env.reset(0, N)
    _own_state_buffers(env)
    assert _order_state(env) == ((0, instep) if late_order else (N, instep))
    rng = np.random.RandomState(3)
    recs, fills, step = [], [], 0
    while env._n_active:
        n = env._n_active
        idx = env.continue_idx.copy()
        if step in refresh_at:
            env.spatial_order = True
            env._refresh_processing_order(force=True)     # the host refresh, in-step on or off
            assert _order_state(env)[0] == n
        a = env.scripted_actions(state, step, 9, wobble)
        if restop:
            # the oracle-stopping route: extra stop flags between step_begin and
            # step_end (k_restop): a seeded tenth of the rows from step 2 on, and
            # at step 3 every streamline in the lower half of the volume -- the
            # order is sorted by brick, x first, so whole 256-slot blocks of it
            # stop at once and half of the bins empty out
            extra = torch.from_numpy(
                (rng.random_sample(n) < 0.1).astype(np.uint8) * (step >= 2)).to(env.device)

            def flags(n_, n_points, e=extra, half=(step == 3)):
                if half:
                    g = env._idx_view(n_).long()
                    e = e | (env._buf_streamlines[g, n_points - 1, 0] < D / 2).to(torch.uint8)
                return e * 64           # the ORACLE bit
            env._use_oracle_stopping = True
            env._oracle_stopping_flags = flags
        full, rew, done, info = env.step_device(a)
        row_dest = info['row_dest'].cpu().numpy().copy()
        full = full.cpu().numpy()
        assert not np.isnan(full).any(), f'step {step}: a state row was never written'
        by_streamline = full[row_dest]      # row i: the state of streamline idx[i]
        state, _ = env.harvest()
        recs.append(dict(idx=idx, row_dest=row_dest, done=done.cpu().numpy().copy(),
                         reward=None if rew is None else rew.cpu().numpy().copy(),
                         flags=env.flags.copy(), lengths=env.lengths.copy(),
                         dones=env.dones.copy(), state=by_streamline,
                         harvested=state.cpu().numpy().copy()))
        slots, _ = _order_state(env)
        if slots:
            fills.append((step + 1, slots, env._n_active))
        step += 1
    recs.append(dict(streamlines=env.streamlines.copy()))
    return recs, fills


def _assert_same(a, b):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            if x[k] is None:
                assert y[k] is None
            else:
                # bit-identical: the bytes, not the values (NaN-safe)
                assert x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (s, k)


_OFF = {}


def _off(monkeypatch, **kw):
    """The in-step-off episode of a variant, computed once per module."""
    key = tuple(sorted(kw.items()))
    if key not in _OFF:
        _OFF[key] = _episode(monkeypatch, 0, **kw)
    return _OFF[key]


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 3])
def test_instep_is_bit_identical_to_off(P, monkeypatch):
    off, off_fills = _off(monkeypatch)
    on, fills = _episode(monkeypatch, P)
    _assert_same(on, off)
    # the episode is the kind the issue asks for: many streamlines stop early,
    # it runs for many steps, and the order stays in use while they do
    n_rows = [len(r['idx']) for r in off[:-1]]
    print('rows per step', n_rows, 'fills', fills, 'off', off_fills)
    # (the CPU oracle tracks 700 -> 272 rows over the first 11 steps with these actions)
    assert len(n_rows) >= 20 and len(fills) >= 10 and n_rows[10] < 0.5 * N
    assert sum(a > b for a, b in zip(n_rows[:len(fills)], n_rows[1:])) >= 10   # stops in 10+ steps
    # the re-bucket really ran: after a harvest that follows a re-bucket step the
    # order is dense (as many slots as rows); with in-step off it keeps holes
    # until the host's low-fill refresh
    for step, slots, rows in fills:
        if step % P == 0:
            assert slots == rows, (step, slots, rows)
    assert any(slots > rows for _, slots, rows in off_fills)
    if P > 1:
        assert any(slots > rows for step, slots, rows in fills if step % P)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['f64dir', 'reward', 'K100', 'restop', 'host_refresh',
                                     'late_order'])
def test_instep_variants_are_bit_identical_to_off(variant, monkeypatch):
    kw = dict(f64dir=dict(f64=True), reward=dict(reward=True), K100=dict(n_dirs=100),
              restop=dict(restop=True), host_refresh=dict(refresh_at=(3, 4)),
              late_order=dict(late_order=True))[variant]
    off, _ = _off(monkeypatch, **kw)
    on, fills = _episode(monkeypatch, 2, **kw)
    _assert_same(on, off)
    assert any(step % 2 == 0 and slots == rows for step, slots, rows in fills)
    if variant == 'reward':
        assert off[0]['reward'] is not None
    if variant == 'restop':      # the extra flags did stop rows the plain episode keeps
        plain, _ = _off(monkeypatch)
        assert [len(r['idx']) for r in off[:-1]] != [len(r['idx']) for r in plain[:-1]]


@pytest.mark.gpu
def test_instep_matches_the_cpu_oracle(monkeypatch):
    from oracle import env_oracle as orc
    seeds = _seeds()
    sh, mask, pk = synthetic_subject(D)
    env = _env(monkeypatch, 1, seeds=seeds)
    ref = orc.OracleTrackingEnv(sh, mask, seeds, n_dirs=4, theta=30.0, step_size=env.step_size,
                                max_nb_steps=env.max_nb_steps, mask_threshold=0.1, peaks=pk,
                                compute_reward=False, alignment_weighting=1.0)
    state, s_ref = env.reset(0, N), ref.reset(0, N)
    _own_state_buffers(env)
    assert np.abs(state.cpu().numpy() - s_ref).max() <= 1e-5
    step = 0
    while env._n_active:
        a = env.scripted_actions(state, step, 9, 0.2)
        full, _, done, info = env.step_device(a)
        ns_ref, _, d_ref, _ = ref.step(a.cpu().numpy().copy())
        assert np.array_equal(done.cpu().numpy().astype(bool), d_ref)
        got = full.cpu().numpy()[info['row_dest'].cpu().numpy()]
        assert np.abs(got - ns_ref).max() <= 1e-5           # NaN (a row never written) fails
        state, _ = env.harvest()
        ref.harvest()
        assert np.array_equal(env.continue_idx, ref.continue_idx)
        step += 1
    assert step >= 12
    assert np.array_equal(env.flags, ref.flags) and np.array_equal(env.lengths, ref.lengths)


@pytest.mark.gpu
def test_instep_through_the_c_abi_with_the_callers_buffers(monkeypatch):
    """ttl_env_step / ttl_env_harvest / ttl_env_wait_counts called directly, the
    state rows in a NaN-filled buffer of the caller, P = 1 against off."""
    def run(instep):
        env = _env(monkeypatch, instep, seeds=_seeds(5))
        state = env.reset(0, N)
        lib, h, W, stream = env._lib, env._handle, env._state_width, env._stream()
        counts = torch.zeros(4, dtype=torch.int32).pin_memory()
        n, step, out = N, 0, []
        while n >= 256 and step < 14:
            a = env.scripted_actions(state[:n], step, 9, 0.2).contiguous()
            buf = torch.full((n, W), float('nan'), dtype=torch.float32, device='cuda')
            done = torch.empty(n, dtype=torch.uint8, device='cuda')
            idx = env._buf_idx_rows[step & 1][:n].cpu().numpy().copy()
            assert lib.ttl_env_step(h, a.data_ptr(), None, n, 1, buf.data_ptr(), W, None,
                                    done.data_ptr(), counts.data_ptr(), stream) == 0
            assert lib.ttl_env_harvest(h, None, None, W, stream) == 0
            assert lib.ttl_env_wait_counts(h) == 0
            torch.cuda.synchronize()
            rows = buf.cpu().numpy()
            assert not np.isnan(rows).any()
            out.append((idx, done.cpu().numpy().copy(),
                        rows[env._row_dest_all[:n].cpu().numpy()]))
            slots, period = _order_state(env)
            n = int(counts[0])
            assert period == instep and (not instep or slots == n)
            env._n_active = n                # scripted_actions reads the current continue_idx
            env._cur ^= 1
            state = buf
            step += 1
        assert step >= 6
        return out
    off, on = run(0), run(1)
    assert len(off) == len(on)
    for s, (x, y) in enumerate(zip(off, on)):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes(), s


def _expected_refreshes(rows, every, k_tail):
    """Steps before which the host refreshes the order, from rows[k] = the active
    rows of step k alone.  The rule: periodically, when (length - 1) % every == 0
    (length = k + 1 points, never before step 0), or early, when fewer than 0.8 of
    the rows of the last refresh are left and the step tail keeps holes -- k_tail
    was asked for (TTL_TAIL_FUSED=1) and the step before ran over the order: the
    library drops the order at the first step of at most TTL_FUSE_MAX_ROWS = 256
    rows, which the one-launch tail takes, and a periodic refresh re-installs it
    for one such step at a time."""
    out, at_refresh, in_use = [], rows[0], True
    for k, n in enumerate(rows):
        periodic = bool(every) and k > 0 and k % every == 0
        early = bool(every) and k > 0 and k_tail and in_use and n < 0.8 * at_refresh
        if periodic or early:
            out.append(k)
            at_refresh, in_use = n, True
        if n <= 256:
            in_use = False
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('tail,every', [('1', 4), ('1', 0), ('0', 4)])
def test_host_refresh_schedule_follows_the_library(tail, every, monkeypatch):
    """With in-step off the host class decides when the order is rebuilt, from what
    the library reports (ttl_env_order_slots).  No output depends on it, so the
    calls themselves are recorded: k_tail (holes) refreshes periodically and early,
    never with TTL_ORDER_REFRESH=0, and the two-kernel tail, which compacts the
    order in every step, only periodically.

    Run once on the commit before the host class asked the library (it kept its own
    copy of the order's length and of the knobs that choose the tail): the second
    and third case gave the same schedules; the first gave [4, 7, 8, 11, 12] as
    here while the order was in use and then seven more early refreshes (before
    steps 14, 19, 23, 25, 27, 29, 30, at 172 rows and fewer) that its stale copy
    asked for after the library had dropped the order -- each rebuilt an order
    that the same step dropped again."""
    from tracktolearn_amd.environments import TrackingEnvironment
    monkeypatch.setenv('TTL_TAIL_FUSED', tail)
    monkeypatch.setattr(TrackingEnvironment, 'SPATIAL_ORDER_REFRESH', every)
    monkeypatch.setattr(TrackingEnvironment, 'ORDER_MIN_FILL', 0.8)
    env = _env(monkeypatch, 0, seeds=_seeds())
    refresh, called, rows = env._lib.ttl_env_refresh_processing_order, [], []

    def recorded(handle, stream):
        called.append(len(rows) - 1)
        return refresh(handle, stream)
    monkeypatch.setattr(env._lib, 'ttl_env_refresh_processing_order', recorded)
    state = env.reset(0, N)
    while env._n_active:
        rows.append(env._n_active)
        env.step_device(env.scripted_actions(state, len(rows) - 1, 9, 0.2))
        state, _ = env.harvest()
    want = _expected_refreshes(rows, every, tail == '1')
    print('rows per step', rows, 'refreshed before', called, 'expected', want)
    assert called == want
    periodic = [k for k in range(1, len(rows)) if every and k % every == 0]
    if tail == '1' and every:
        # (the CPU oracle: 557 -> 414 rows over steps 4..7, 376 -> 272 over 8..11)
        assert set(periodic) < set(called) and any(k % every for k in called)
    else:
        assert called == periodic and (every or not called)


def test_a_brick_grid_over_the_bin_cap_never_takes_the_instep_path(monkeypatch):
    """ttl_env_create does no device work: a descriptor with made-up (aligned,
    never dereferenced) addresses is enough to ask the handle which path it
    takes.  25 x 26 x 26 = 16 900 bricks > the cap; 13^3 (the 96^3 headline)
    is inside."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv('TTL_ORDER_INSTEP', '2')

    def period(dims):
        d = _lib.EnvDesc()
        d.abi_version, d.mode = _lib.ABI_VERSION, _lib.MODE_F32
        for a in range(3):
            d.sh_dim[a] = d.mask_dim[a] = d.peaks_dim[a] = dims[a]
        d.n_coef, d.coef_pitch, d.sh_layout = 45, 48, _lib.SH_LINEAR
        d.n_dirs, d.max_nb_steps, d.n_max = 4, 30, 1024
        d.step_size_vox, d.neigh_radius_vox = 0.75, 0.5
        fake = 1 << 20
        for f in ('sh_packed', 'mask_coef', 'streamlines', 'flags', 'lengths', 'dones',
                  'idx_a', 'idx_b', 'workspace'):
            setattr(d, f, fake)
        d.workspace_bytes = lib.ttl_env_workspace_bytes(1024)
        h = C.c_void_p()
        assert lib.ttl_env_create(C.byref(d), C.byref(h)) == 0, lib.ttl_last_error()
        slots, p = C.c_int32(-1), C.c_int32(-1)
        assert lib.ttl_env_order_slots(h, C.byref(slots), C.byref(p)) == 0
        lib.ttl_env_destroy(h)
        assert slots.value == 0           # no episode yet: no order in use
        return p.value
    assert period((96, 96, 96)) == 2
    assert period((185, 193, 193)) == 0 and period((8192, 24, 24)) == 0
    monkeypatch.setenv('TTL_ORDER_INSTEP', '0')
    assert period((96, 96, 96)) == 0
