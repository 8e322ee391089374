"""The training episode against output recorded from the reference's own
``Tracker.track_and_train`` (tests/golden/make_golden_training.py;
TrackToLearn/tracking/tracker.py:152-202, algorithms/ddpg.py:141-232): one
episode of SACAuto, SAC (fixed alpha), TD3 and DDPG in which the learner's own
network drives the env, the 128-row ring wraps in mid-episode, the first
updates sample fewer rows than ``batch_size`` and -- TD3 -- the env adds
gaussian noise to the actions.

Every random draw of the reference's run is replayed: the gaussian draws in
call order (``torch.randn`` / ``torch.randn_like`` / ``noise_fn``), the rows of
every sampled batch (``torch.randperm``), the seeds ``nreset`` picked (numpy's
global generator) and the env's action noise (``env_dto['rng']``).

CPU: this project's ``Tracker.track_and_train`` / ``DDPG._episode`` over a thin
adapter that gives ``oracle/env_oracle.py`` the device-loop surface of the HIP
env (``step_device`` with partitioned rows and ``row_dest``), once with the
autograd update and once with the fused schedule on the ``TorchOps`` seam.
GPU: the product path (HIP env, fused policy head, ``ttl_replay_add``, fused
learner), and once more with ``TTL_FUSED_LEARNER=0``.

Exact: rows per step, every ``done``, ``t`` before every step, which steps
updated, ``total_it``, ring ``ptr`` / ``size`` / ``not_done``, stopping flags,
streamline lengths, ``episode_length``; the ring equals, bit for bit, the
candidate's own emissions written in the reference's row order.  Continuous
quantities: within ``max(4 * twin_spread/<name>, floor)`` -- ``twin_spread`` is
the spread the generator measured over 8 runs of the reference whose initial
weights differ by one float32 ulp; 4 because a twin perturbs only the initial
weights while another implementation differs in the summation order of every
GEMM and reduction; floor 2e-6 for learner quantities (actions, weights,
``log_alpha``, losses: tests/test_learner_golden.py) and 1e-5 for states,
rewards and streamline points (README parity statement).  Nothing is masked
out: every step, ring row and update is compared.
"""
import os

import numpy as np
import pytest
import torch

from helpers import load_trace, synthetic_subject, trace_noise, trace_step_size

ALGS = ['sac_auto', 'sac', 'td3', 'ddpg']
LEARNER, ENV = 2e-6, 1e-5
FACTOR = 4.0
NETS = ('actor', 'critic', 'target_actor', 'target_critic')


# --------------------------------------------------------------------------
# the candidate's run, with the reference's draws
# --------------------------------------------------------------------------
class _Tractogram:
    def __init__(self, streamlines, seeds, flags):
        self.streamlines = streamlines
        self.data_per_streamline = {'seeds': seeds, 'flags': flags}


class _OracleDeviceEnv:
    """The device-loop surface ``DDPG._episode`` calls, over the CPU oracle:
    ``step_device`` hands the state rows out survivors first (stable), then the
    rows that stopped (stable), with ``row_dest[i]`` the row of active row
    ``i`` -- the order the HIP env writes (tracking_env.py:step_device)."""

    def __init__(self, env):
        self.env = env

    def nreset(self, n):
        state = self.env.nreset(n)
        self.initial_points = self.env.initial_points
        return torch.from_numpy(np.ascontiguousarray(state))

    def step_device(self, action):
        assert action.dtype == torch.float32
        ns, reward, done, _ = self.env.step(action.numpy().copy())
        n = len(done)
        keep = torch.from_numpy(~done)
        self._n_keep = int(keep.sum())
        dest = torch.empty(n, dtype=torch.int32)
        dest[keep] = torch.arange(self._n_keep, dtype=torch.int32)
        dest[~keep] = torch.arange(self._n_keep, n, dtype=torch.int32)
        self._state = torch.empty((n, ns.shape[1]), dtype=torch.float32)
        self._state[dest.long()] = torch.from_numpy(np.ascontiguousarray(ns))
        return (self._state, torch.from_numpy(np.asarray(reward, np.float64)),
                torch.from_numpy(done.astype(np.uint8)),
                {'row_dest': dest, 'reward_info': {}})

    def harvest(self):
        self.env.harvest()
        return self._state[:self._n_keep], None

    def get_streamlines(self):
        lines, seeds, flags = self.env.get_streamlines()
        return _Tractogram(lines, seeds, flags)


def _cpu_env(z):
    from oracle import env_oracle as orc
    sh, mask, pk = synthetic_subject(int(z['D']))
    kw = dict(n_dirs=int(z['n_dirs']), theta=float(z['theta']),
              step_size=trace_step_size(z), max_nb_steps=int(z['max_nb_steps']),
              mask_threshold=0.1, peaks=pk, compute_reward=True, alignment_weighting=1.0)
    if bool(z['noisy']):
        sigma, rng = trace_noise(z)
        env = orc.OracleNoisyTrackingEnv(sh, mask, z['seeds'].copy(), noise=sigma, rng=rng, **kw)
    else:
        env = orc.OracleTrackingEnv(sh, mask, z['seeds'].copy(), **kw)
    return _OracleDeviceEnv(env)


def _gpu_env(z):
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import (NoisyTrackingEnvironment,
                                               TrackingEnvironment)
    sh, mask, pk = synthetic_subject(int(z['D']))
    aff = z['affine']
    sigma, rng = trace_noise(z)
    dto = dict(n_dirs=int(z['n_dirs']), theta=float(z['theta']), npv=1,
               binary_stopping_threshold=0.1, step_size=0.75, min_length=2.0,
               max_length=40.0, compute_reward=True, alignment_weighting=1.0,
               oracle_bonus=0.0, rng=np.random.RandomState(3),
               device=torch.device('cuda:0'), target_sh_order=8, noise=sigma, fa_map=None)
    cls = NoisyTrackingEnvironment if bool(z['noisy']) else TrackingEnvironment
    env = cls((Vol(sh, aff), Vol(mask.astype(np.float32), aff),
               Vol(mask.astype(np.float32), aff), Vol(pk, aff), None), 'testing', dto)
    assert float(env.step_size) == float(z['step_size'])
    assert env.max_nb_steps == int(z['max_nb_steps'])
    env.seeds = z['seeds'].copy()
    if rng is not None:     # building the env drew its own seeds from the generator
        env.rng.set_state(rng.get_state())
    return env


def _state_dict(z, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(z[k]) for k in z.files
            if k.startswith(prefix + '/')}


def _learner(z, device):
    from tracktolearn_amd.algorithms.ddpg import DDPG
    from tracktolearn_amd.algorithms.sac import SAC
    from tracktolearn_amd.algorithms.sac_auto import SACAuto
    from tracktolearn_amd.algorithms.td3 import TD3
    width = 7 * int(z['C']) + 3 * int(z['n_dirs'])
    kw = dict(lr=float(z['lr']), gamma=float(z['gamma']), n_actors=int(z['n_actor']),
              batch_size=int(z['batch_size']), replay_size=int(z['replay_size']), rng=None,
              device=device)
    name = str(z['alg'])
    if name in ('SACAuto', 'SAC'):
        alg = {'SACAuto': SACAuto, 'SAC': SAC}[name](width, 3, str(z['hidden']),
                                                     alpha=float(z['alpha']), **kw)
    else:
        alg = {'TD3': TD3, 'DDPG': DDPG}[name](width, 3, str(z['hidden']),
                                               action_std=float(z['action_std']), **kw)
    init = (_state_dict(z, 'init/actor'), _state_dict(z, 'init/critic'))
    alg.agent.load_state_dict(init)
    alg.target.load_state_dict(init)
    alg.start_timesteps = int(z['start_timesteps'])
    return alg


class _Replay:
    """The reference's draws, handed out in its call order."""

    def __init__(self, z, device):
        offs = np.concatenate(([0], np.cumsum(z['draw_rows'])))
        self.draws = [torch.from_numpy(z['draws'][offs[i]:offs[i + 1]]).to(device)
                      for i in range(len(offs) - 1)]
        offs = np.concatenate(([0], np.cumsum(z['sample_rows'])))
        self.samples = [torch.from_numpy(z['sample_idx'][offs[i]:offs[i + 1]]).to(device)
                        for i in range(len(offs) - 1)]
        self.i = self.j = 0
        # rows in the ring when the reference sampled: its permutation's length
        held = np.minimum(np.cumsum(z['step_rows']), int(z['replay_size']))
        self.held = [int(h) for h, u in zip(held, z['step_updated']) if u]
        self.batch = int(z['batch_size'])

    def gaussian(self, shape):
        e = self.draws[self.i]
        self.i += 1
        assert tuple(shape) == tuple(e.shape), 'a draw of another shape than the reference\'s'
        return e

    def randn(self, *size, **kw):
        assert kw.get('out') is None
        return self.gaussian(size[0] if len(size) == 1 and not isinstance(size[0], int)
                             else size)

    def randn_like(self, t, **kw):
        return self.gaussian(t.shape)

    def randperm(self, n, **kw):
        assert n == self.held[self.j], 'the ring holds other rows than the reference\'s'
        ind = self.samples[self.j]
        self.j += 1
        assert len(ind) == min(n, self.batch)
        return ind


def _run(z, device, monkeypatch, env, seam=None):
    """``track_and_train`` of this project with the reference's draws; returns
    everything the comparison needs, on the host."""
    from tracktolearn_amd.tracking.tracker import Tracker
    alg = _learner(z, device)
    if seam is not None:
        alg._fused_ops = seam
    rep = _Replay(z, device)
    monkeypatch.setattr(torch, 'randn', rep.randn)
    monkeypatch.setattr(torch, 'randn_like', rep.randn_like)
    monkeypatch.setattr(torch, 'randperm', rep.randperm)
    if hasattr(alg, 'noise_fn'):
        alg.noise_fn = lambda like: rep.gaussian(like.shape)

    # the recorded rows are forced through randperm + index_select for the
    # sampling only: the ring is still filled by add_partitioned's own path
    real_sample = alg.replay_buffer.sample

    def sample(batch_size):
        old = os.environ.get('TTL_REPLAY_RANDPERM')
        os.environ['TTL_REPLAY_RANDPERM'] = '1'
        try:
            return real_sample(batch_size)
        finally:
            if old is None:
                del os.environ['TTL_REPLAY_RANDPERM']
            else:
                os.environ['TTL_REPLAY_RANDPERM'] = old
    alg.replay_buffer.sample = sample

    steps = []
    real_step, real_harvest = env.step_device, env.harvest
    state_now = {}

    def step_device(action):
        res = real_step(action)
        ns, reward, done, info = res
        dest = info['row_dest'].long().clone()
        steps.append(dict(t=alg.t, it=alg.total_it, state=state_now['s'].clone(),
                          action=action.clone(), next_state=ns[dest].clone(),
                          reward=reward.clone(), done=done.clone()))
        return res

    def harvest():
        out = real_harvest()
        state_now['s'] = out[0]
        return out
    env.step_device, env.harvest = step_device, harvest
    real_nreset = env.nreset

    def nreset(n):
        state_now['s'] = real_nreset(n)
        return state_now['s']
    env.nreset = nreset

    tracker = Tracker(alg, n_actor=int(z['n_actor']), prob=0.0)
    np.random.seed(int(z['nreset_seed']))
    tg, mean_losses, reward, factors = tracker.track_and_train(env)
    assert rep.i == len(rep.draws) and rep.j == len(rep.samples)
    for s in steps:
        for k in ('state', 'action', 'next_state', 'reward', 'done'):
            s[k] = s[k].cpu().numpy()
    return dict(alg=alg, env=env, steps=steps, tg=tg, losses=mean_losses, reward=reward,
                factors=factors)


# --------------------------------------------------------------------------
# the comparison
# --------------------------------------------------------------------------
class _Report:
    def __init__(self, z, label):
        self.z, self.label, self.rows, self.bad = z, label, [], []

    def close(self, name, got, want, floor):
        bound = max(FACTOR * float(self.z[f'twin_spread/{name}']), floor)
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = float(np.abs(got - want).max()) if got.size else 0.0
        self.rows.append((name, err, bound))
        if not err <= bound:
            self.bad.append((name, err, bound))

    def finish(self):
        worst = {}
        for name, err, bound in self.rows:
            worst[name] = (max(err, worst.get(name, (0.0, bound))[0]), bound)
        print(f'\n{self.label}: measured maximum / bound')
        for name, (err, bound) in worst.items():
            print(f'    {name:16s} {err:.3e} / {bound:.3e}')
        assert not self.bad, self.bad


def _own_ring(z, steps):
    """The candidate's own emissions written as the reference writes its ring
    (replay.py:56-89): active-row order, modulo wrap."""
    size = int(z['replay_size'])
    width = steps[0]['state'].shape[1]
    ring = dict(state=np.zeros((size, width), np.float32), action=np.zeros((size, 3), np.float32),
                next_state=np.zeros((size, width), np.float32),
                reward=np.zeros((size, 1), np.float32), not_done=np.zeros((size, 1), np.float32))
    ptr = 0
    for s in steps:
        ind = (np.arange(len(s['action'])) + ptr) % size
        ring['state'][ind] = s['state']
        ring['action'][ind] = s['action']
        ring['next_state'][ind] = s['next_state']
        ring['reward'][ind] = s['reward'][..., None].astype(np.float32)
        ring['not_done'][ind] = 1. - s['done'][..., None].astype(np.float32)
        ptr = (ptr + len(ind)) % size
    return ring


def _compare(z, run, label):
    alg, steps, tg = run['alg'], run['steps'], run['tg']
    rep = _Report(z, label)
    # ---- exact: the schedule
    assert len(steps) == int(z['n_steps']) == int(z['episode_length'])
    assert [len(s['action']) for s in steps] == z['step_rows'].tolist()
    assert [s['t'] for s in steps] == z['step_t'].tolist()
    its = [s['it'] for s in steps] + [alg.total_it]
    assert [b > a for a, b in zip(its[:-1], its[1:])] == z['step_updated'].tolist()
    assert all(b - a <= 1 for a, b in zip(its[:-1], its[1:]))
    assert alg.total_it == int(z['total_it']) == int(z['n_updates'])
    assert alg.t == int(z['t'])
    assert np.array_equal(np.concatenate([s['done'] for s in steps]).astype(bool),
                          z['step_done'])
    # ---- exact: the ring
    buf = alg.replay_buffer
    assert (buf.ptr, buf.size) == (int(z['ring_ptr']), int(z['ring_size']))
    ring = {k: getattr(buf, k).cpu().numpy() for k in
            ('state', 'action', 'next_state', 'reward', 'not_done')}
    assert np.array_equal(ring['not_done'], z['ring_not_done'])
    own = _own_ring(z, steps)
    for k in ring:          # what the policy and the env emitted, row for row
        assert np.array_equal(ring[k], own[k]), f'ring {k} differs from the run\'s own rows'
    # ---- exact: the tractogram
    assert np.array_equal(np.asarray(run['env'].initial_points), z['initial_points'])
    assert np.array_equal(np.asarray(tg.data_per_streamline['flags']), z['tract_flags'])
    assert np.array_equal(np.asarray(tg.data_per_streamline['seeds']), z['tract_seeds'])
    assert [len(s) for s in tg.streamlines] == z['tract_lengths'].tolist()

    # ---- continuous
    rep.close('actions', np.concatenate([s['action'] for s in steps]), z['step_actions'],
              LEARNER)
    rep.close('reward', np.concatenate([s['reward'] for s in steps]), z['step_reward'], ENV)
    rep.close('ring_state', ring['state'], z['ring_state'], ENV)
    rep.close('ring_action', ring['action'], z['ring_action'], LEARNER)
    rep.close('ring_next_state', ring['next_state'], z['ring_next_state'], ENV)
    rep.close('ring_reward', ring['reward'], z['ring_reward'], ENV)
    rep.close('streamlines', np.concatenate([np.asarray(s).reshape(-1, 3) for s in tg.streamlines]),
              z['tract_points'], ENV)
    rep.close('running_reward', run['reward'], z['running_reward'], ENV)
    nets = dict(actor=alg.agent.actor, critic=alg.agent.critic,
                target_actor=alg.target.actor, target_critic=alg.target.critic)
    for net in NETS:
        want = _state_dict(z, f'final/{net}')
        got = nets[net].state_dict()
        assert set(got) == set(want)
        for k in want:
            rep.close(net, got[k].detach().cpu().numpy(), want[k].numpy(), LEARNER)
    if 'final/log_alpha' in z.files:
        rep.close('log_alpha', alg.log_alpha.detach().cpu().numpy(), z['final/log_alpha'],
                  LEARNER)
    # the reward-factor lists: one entry per step
    factors = run['factors']
    assert sorted(factors) == ['oracle_reward', 'peaks_reward']
    for k in factors:
        rep.close('reward_factors', np.asarray(factors[k], np.float64),
                  z[f'reward_factors/{k}'], ENV)
        rep.close('reward_factors', np.asarray(factors[k], np.float64), z[f'step_info/{k}'], ENV)
    # the losses of every update, and their mean as the trainer takes it
    from tracktolearn_amd.algorithms.shared.utils import mean_losses
    losses = run['losses']
    assert sorted(losses) == sorted(z['loss_keys'].tolist())
    for k in losses:
        got = np.array([float(v) for v in losses[k]])
        rep.close('losses', got, z[f'losses/{k}'], LEARNER)
    for k, v in (mean_losses(losses) if len(losses) else {}).items():
        rep.close('losses', float(v), z[f'losses/{k}'].astype(np.float32).mean(), LEARNER)
    rep.finish()


# --------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['autograd', 'torchops'])
@pytest.mark.parametrize('name', ALGS)
def test_training_episode_matches_the_reference_on_the_cpu(name, fused, monkeypatch):
    """Loop, ring and update schedule without a GPU: the oracle env behind the
    device-loop adapter, the autograd update or the fused schedule on the
    ``TorchOps`` seam."""
    from ref_learner_ops import TorchOps
    z = load_trace(f'training_{name}')
    run = _run(z, torch.device('cpu'), monkeypatch, _cpu_env(z),
               seam=TorchOps() if fused else None)
    assert (run['alg']._fused is not None) == fused
    _compare(z, run, f'{name} cpu {"torchops" if fused else "autograd"}')


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'TTL_FUSED_LEARNER=0'])
@pytest.mark.parametrize('name', ALGS)
def test_training_episode_matches_the_reference_on_the_gpu(name, fused, monkeypatch):
    """The product path: the HIP env through the C ABI, the fused policy head
    (SAC), ``add_partitioned`` -> ``ttl_replay_add`` into the HBM ring, the fused
    learner -- and once more with ``TTL_FUSED_LEARNER=0``, so that a failure can
    be placed on one side of that switch."""
    from tracktolearn_amd import _lib
    if not fused:
        monkeypatch.setenv('TTL_FUSED_LEARNER', '0')
    z = load_trace(f'training_{name}')
    lib = _lib.load()
    calls = {'add': 0}
    real_add = lib.ttl_replay_add

    def counted(*a):
        calls['add'] += 1
        return real_add(*a)
    monkeypatch.setattr(lib, 'ttl_replay_add', counted)
    run = _run(z, torch.device('cuda:0'), monkeypatch, _gpu_env(z))
    assert (run['alg']._fused is not None) == fused
    assert calls['add'] == int(z['n_steps'])          # every step took the kernel
    _compare(z, run, f'{name} gpu {"fused" if fused else "TTL_FUSED_LEARNER=0"}')


@pytest.mark.parametrize('cls_name', ['SAC', 'TD3', 'DDPG'])
def test_losses_kept_over_several_fused_updates_are_each_update_s_own(cls_name, monkeypatch):
    """Three updates through ``add_item_to_means`` + ``mean_losses``, as
    ``_episode`` and the trainer do: the fused schedule (``TorchOps`` seam) hands
    out each update's own values, not views of a buffer the next update
    rewrites -- entry by entry equal to the autograd path's."""
    from collections import defaultdict

    import tracktolearn_amd.algorithms.ddpg as ddpg
    import tracktolearn_amd.algorithms.sac as sac
    import tracktolearn_amd.algorithms.td3 as td3
    from ref_learner_ops import TorchOps
    from tracktolearn_amd.algorithms.shared.utils import (add_item_to_means,
                                                          mean_losses)
    cls = {'SAC': sac.SAC, 'TD3': td3.TD3, 'DDPG': ddpg.DDPG}[cls_name]
    W, B = 27, 48
    g = torch.Generator().manual_seed(7)
    batches = [[torch.randn(B, W, generator=g), torch.tanh(torch.randn(B, 3, generator=g)),
                torch.randn(B, W, generator=g), torch.rand(B, generator=g),
                (torch.rand(B, generator=g) > 0.2).float()] for _ in range(3)]
    eps = [torch.randn(B, 3, generator=g) for _ in range(6)]
    torch.manual_seed(11)
    plain = cls(W, 3, '32-32', n_actors=8, batch_size=B, replay_size=100, rng=None,
                device=torch.device('cpu'))
    seam = cls(W, 3, '32-32', n_actors=8, batch_size=B, replay_size=100, rng=None,
               device=torch.device('cpu'))
    seam.agent.load_state_dict(plain.agent.state_dict())
    seam.target.load_state_dict(plain.target.state_dict())
    seam._fused_ops = TorchOps()
    kept = []
    for alg in (plain, seam):
        it = iter(eps)
        monkeypatch.setattr(torch, 'randn_like', lambda t, **kw: next(it))
        alg.noise_fn = lambda like: next(it)
        running = defaultdict(list)
        for batch in batches:
            running = add_item_to_means(running, alg.update(batch))
        kept.append(running)
    assert seam._fused is not None and plain._fused is None
    assert sorted(kept[0]) == sorted(kept[1])
    means = [mean_losses(k) for k in kept]
    for k in kept[0]:
        want = np.array([float(v) for v in kept[0][k]])
        got = np.array([float(v) for v in kept[1][k]])
        assert len(set(want.tolist())) > 1 or k == 'actor_loss'
        assert np.abs(got - want).max() <= 2e-6, (k, got, want)
        assert abs(float(means[1][k]) - float(means[0][k])) <= 2e-6
