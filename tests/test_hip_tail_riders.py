"""Riders of the gather launch (TTL_TAIL_RIDERS): on a step with the one-launch
tail (k_tail) the order scatter of an in-step re-bucket and the row maps
(continue_idx of the next step, row_dest, lengths, the stopped list) run as extra
workgroups behind the state gather's own instead of in front of it.

Scheduling only.  Every case runs the same episode on two handles,
TTL_TAIL_RIDERS=1 and =0 (same seeds, same scripted actions, state rows into
NaN-filled buffers of the test), and after every step compares bit for bit: the
state rows by streamline, continue_idx, row_dest, lengths, flags, dones, the
`ttl_env_stopped` list and the host counts.  The next processing order follows
the atomics inside a bin, so it is held to what must not change: the same
multiset of rows (every surviving row once), and after a re-bucket step dense in
front with nothing behind and bins non-decreasing along it.

`ttl_env_tail_riders` tells what rode in a step: with the knob at 1 the row maps
on every k_tail step and the scatter on every re-bucket step among them, nothing
with the knob at 0, and nothing (or the row maps alone) where a fallback applies.

Shapes: a 24^3 volume (4 x 4 x 4 bins), TTL_ORDER_MIN_ROWS=1 and
TTL_FUSE_MAX_ROWS=256 so that k_tail runs down to 257 rows; an episode goes on
until the batch has fallen to 256 rows or fewer (the order is dropped, the
one-launch small-batch tail takes over) and two steps beyond.  Streamline counts:
257 (two row blocks, one row in the second), 700 (last block partial, one scatter
workgroup), 1 024 (exactly one scatter chunk), 1 500 (two scatter workgroups, the
second partial).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import synthetic_subject

D = 24
FUSE_MAX = 256


def _subject(dims, n_coef):
    """synthetic_subject for the cube; for a long box (the fine raster) the same
    recipe with the ball mask in the middle of the long axis."""
    if dims == (D, D, D):
        return synthetic_subject(D, C=n_coef)
    rng = np.random.RandomState(1234)
    sh = (0.1 * rng.standard_normal(dims + (n_coef,))).astype(np.float32)
    sh[..., 0] = 1.0
    g = np.indices(dims).astype(np.float64)
    centre = np.array([(d - 1) / 2.0 for d in dims]).reshape(3, 1, 1, 1)
    mask = (np.sqrt(((g - centre) ** 2).sum(0)) < 0.42 * min(dims)).astype(np.uint8)
    return sh, mask, np.zeros(dims + (15,), dtype=np.float32)


def _env(monkeypatch, riders, *, n, seed, dims=(D, D, D), n_coef=45, instep=2, knobs=()):
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    for k in ('TTL_STATE_KERNEL', 'TTL_GATHER_PERSIST_ROWS', 'TTL_ORDER_INSTEP_AFTER'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('TTL_TAIL_RIDERS', str(riders))
    monkeypatch.setenv('TTL_ORDER_INSTEP', str(instep))
    monkeypatch.setenv('TTL_ORDER_MIN_ROWS', '1')
    monkeypatch.setenv('TTL_FUSE_MAX_ROWS', str(FUSE_MAX))
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(TrackingEnvironment, 'SPATIAL_ORDER_MIN', 1)
    sh, mask, pk = _subject(dims, n_coef)
    aff = np.eye(4, dtype=np.float32)
    subject = (Vol(sh, aff), Vol(mask.astype(np.float32), aff),
               Vol(mask.astype(np.float32), aff), Vol(pk, aff), None)
    dto = dict(n_dirs=4, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=2.0, max_length=25.0, compute_reward=False,
               alignment_weighting=1.0, oracle_bonus=0.0, oracle_checkpoint=None,
               oracle_stopping_criterion=False, rng=np.random.RandomState(0),
               device=torch.device('cuda:0'), target_sh_order=None, noise=0.0, fa_map=None)
    env = TrackingEnvironment(subject, 'testing', dto)
    rng = np.random.RandomState(seed)
    vox = np.argwhere(mask)
    env.seeds = vox[rng.randint(0, len(vox), n)] + rng.uniform(-0.5, 0.5, (n, 3))
    return env


def _ws_ints(env, ptr, n):
    """n int32 at a device address inside the workspace the env gave the library."""
    off = ptr - env._buf_ws.data_ptr()
    assert 0 <= off and off + 4 * n <= env._buf_ws.numel()
    return env._buf_ws[off:off + 4 * n].view(torch.int32).cpu().numpy().copy()


def _riders(env):
    kinds, last, order = C.c_int32(-1), C.c_int32(-1), C.c_void_p()
    assert env._lib.ttl_env_tail_riders(env._handle, C.byref(kinds), C.byref(last),
                                        C.byref(order)) == 0
    return kinds.value, last.value, order.value


def _slots(env):
    slots, period = C.c_int32(-1), C.c_int32(-1)
    assert env._lib.ttl_env_order_slots(env._handle, C.byref(slots), C.byref(period)) == 0
    return slots.value, period.value


def _bins(env, dims, rows_idx, n_points):
    """Brick of the newest point of the given streamlines in the re-bucket's raster."""
    p = env._buf_streamlines[torch.from_numpy(rows_idx).long().to(env.device), n_points - 1]
    v = np.clip(np.floor(p.cpu().numpy()), 0, 1023).astype(np.int64) >> 3
    nb = [(d + 7) // 8 + 1 for d in dims]
    v = np.minimum(v, np.array(nb) - 1)
    return (v[:, 0] * nb[1] + v[:, 1]) * nb[2] + v[:, 2]


def _episode(monkeypatch, riders, *, n, how='device', restop=False, dims=(D, D, D), **kw):
    """One episode; returns (per-step records that must be equal bit for bit,
    per-step (rows, k_tail ran, what rode))."""
    env = _env(monkeypatch, riders, n=n, seed=11, dims=dims, **kw)
    instep = kw.get('instep', 2)
    state = env.reset(0, n)

    def poisoned(rows):
        return torch.full((rows, env._state_pitch), float('nan'), dtype=torch.float32,
                          device=env.device)[:, :env._state_width]
    env._ring_state = poisoned
    env._new_state = poisoned
    if how == 'host':
        env.lazy_step_state = False     # step() in the reference's row order (ORDER_ACTIVE)
    kinds, _, _ = _riders(env)
    assert kinds == (3 if riders else 0)
    lib, rng = env._lib, np.random.RandomState(3)
    recs, ran, step, beyond = [], [], 0, 0
    while env._n_active and beyond < 2:
        rows = env._n_active
        beyond += rows <= FUSE_MAX
        idx = env.continue_idx.copy()
        slots_before, _ = _slots(env)
        a = env.scripted_actions(state, step, 9, 0.2)
        if restop:
            # extra stop flags between ttl_env_step_begin and ttl_env_step_end: k_restop
            # redoes the ranks and block counts the riders read
            extra = torch.from_numpy((rng.random_sample(rows) < 0.15).astype(np.uint8)
                                     * (step >= 1)).to(env.device) * 64
            env._use_oracle_stopping = True
            env._oracle_stopping_flags = lambda n_, n_points, e=extra: e
        if how == 'host':
            full, _, done, _ = env.step(a)
            full, done = full.cpu().numpy(), done.astype(np.uint8)
            row_dest = env._row_dest_view(rows).cpu().numpy().copy()
            by_streamline = full
            assert np.array_equal(row_dest, np.arange(rows))
        else:
            full, _, done, info = env.step_device(a)
            row_dest = info['row_dest'].cpu().numpy().copy()
            full, done = full.cpu().numpy(), done.cpu().numpy().copy()
            by_streamline = full[row_dest]
        assert not np.isnan(full).any(), f'step {step}: a state row was never written'
        lst, n_stop = C.c_void_p(), C.c_int32()
        assert lib.ttl_env_stopped(env._handle, C.byref(lst), C.byref(n_stop)) == 0
        stopped = _ws_ints(env, lst.value, 2 * n_stop.value) if n_stop.value else np.zeros(0, np.int32)
        _, last, _ = _riders(env)
        state, _ = env.harvest()
        if how == 'host':
            state = state.clone()
        torch.cuda.synchronize()
        nxt = env.continue_idx.copy()
        recs.append(dict(idx=idx, state=by_streamline, row_dest=row_dest, done=done,
                         stopped=stopped, counts=env._host_counts_np[:2].copy(),
                         continue_idx=nxt, harvested=state.cpu().numpy().copy(),
                         flags=env.flags.copy(), lengths=env.lengths.copy(),
                         dones=env.dones.copy()))
        assert int(recs[-1]['counts'][0]) == len(nxt) == env._n_active
        assert int(recs[-1]['counts'][1]) == rows - len(nxt) == n_stop.value
        # the next processing order
        slots, _ = _slots(env)
        k_tail = slots_before > 0 and rows > FUSE_MAX
        rebucket = k_tail and instep > 0 and (step + 1) % instep == 0 and _slots(env)[1] > 0
        if slots:
            _, _, order_ptr = _riders(env)
            order = _ws_ints(env, order_ptr, slots)
            live = order[order >= 0]
            assert np.array_equal(np.sort(live), np.arange(len(nxt))), (step, 'multiset of rows')
            if rebucket:
                assert slots == len(nxt) and (order >= 0).all(), (step, 'dense, nothing behind')
                b = _bins(env, dims, nxt[order], env.length)
                assert (np.diff(b) >= 0).all(), (step, 'bins along the order')
        ran.append((rows, k_tail, rebucket, last))
        step += 1
    return recs, ran


def _assert_same(a, b):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (s, k)


def _both(monkeypatch, **kw):
    on, ran_on = _episode(monkeypatch, 1, **kw)
    off, ran_off = _episode(monkeypatch, 0, **kw)
    _assert_same(on, off)
    assert [r[:3] for r in ran_on] == [r[:3] for r in ran_off]
    assert all(last == 0 for _, _, _, last in ran_off)
    print('rows, k_tail, re-bucket, rode:', ran_on)
    # two steps beyond the order's minimum
    assert sum(rows <= FUSE_MAX for rows, _, _, _ in ran_on) == 2 or ran_on[-1][0] <= FUSE_MAX
    return ran_on


def _assert_rode(ran, scatter=True, rows=True):
    assert any(k_tail for _, k_tail, _, _ in ran)
    for _, k_tail, rebucket, last in ran:
        assert last == ((1 if scatter and rebucket else 0) | (2 if rows and k_tail else 0))


@pytest.mark.gpu
@pytest.mark.parametrize('n,instep', [(257, 1), (700, 2), (1024, 1), (1500, 2)])
def test_riders_are_bit_identical_to_separate_launches(n, instep, monkeypatch):
    ran = _both(monkeypatch, n=n, instep=instep)
    _assert_rode(ran)
    assert any(rebucket for _, _, rebucket, _ in ran)
    if n >= 700:    # the episode is long enough to see holes, stops and a few re-buckets
        assert sum(k_tail for _, k_tail, _, _ in ran) >= 4


@pytest.mark.gpu
def test_riders_in_the_reference_row_order(monkeypatch):
    """step(): ORDER_ACTIVE rows through ttl_env_step_begin / ttl_env_step_end."""
    _assert_rode(_both(monkeypatch, n=700, how='host'))


@pytest.mark.gpu
def test_riders_with_another_lane_group(monkeypatch):
    """C = 28: records of 7 float4 columns, lane groups of 8 (C = 45 takes 12)."""
    _assert_rode(_both(monkeypatch, n=700, n_coef=28))


@pytest.mark.gpu
def test_riders_behind_extra_stop_flags(monkeypatch):
    ran = _both(monkeypatch, n=700, restop=True)
    _assert_rode(ran)
    plain, _ = _episode(monkeypatch, 1, n=700)
    assert [r[0] for r in ran] != [len(r['idx']) for r in plain]    # the flags did stop rows


@pytest.mark.gpu
@pytest.mark.parametrize('fallback', ['state_kernel_0', 'persist_rows', 'scatter_behind_gather'])
def test_fallbacks_take_the_separate_launches(fallback, monkeypatch):
    knobs, rows = dict(state_kernel_0=((('TTL_STATE_KERNEL', '0'),), False),
                       persist_rows=((('TTL_GATHER_PERSIST_ROWS', '1000000'),), False),
                       scatter_behind_gather=((('TTL_ORDER_INSTEP_AFTER', '1'),), True))[fallback]
    ran = _both(monkeypatch, n=700, knobs=knobs)
    if fallback == 'state_kernel_0':     # k_prefix + k_proc_scatter: no k_tail, nothing rides
        assert all(last == 0 for _, _, _, last in ran)
    else:
        _assert_rode(ran, scatter=False, rows=rows)
        assert any(rebucket for _, _, rebucket, _ in ran)


@pytest.mark.gpu
def test_a_fine_raster_keeps_the_scatter_launch(monkeypatch):
    """24 x 24 x 2040 voxels: 4 x 4 x 256 = 4 096 bins, whose scan needs 16 400
    bytes of LDS -- over the 16 KB the gather launch may carry, inside what the
    in-step re-bucket takes.  The scatter stays a launch, the row maps ride."""
    dims = (D, D, 2040)
    ran = _both(monkeypatch, n=700, dims=dims, n_coef=6)
    _assert_rode(ran, scatter=False)
    assert any(rebucket for _, _, rebucket, _ in ran)
