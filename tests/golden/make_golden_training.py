#!/usr/bin/env python3
"""Generate tests/golden/training_*.npz by running the REFERENCE's own,
unmodified ``Tracker.track_and_train`` (TrackToLearn/tracking/tracker.py:
152-202) with the ``_episode`` of its SACAuto / SAC / TD3 / DDPG learners
(TrackToLearn/algorithms/ddpg.py:141-232) over the reference's own
environment classes, on the CPU (same harness as make_golden_tracker.py).

    python tests/golden/make_golden_training.py

One training episode per learner: 32 random seeds tracked to exhaustion by the
learner's own (fresh) policy while it learns; small networks ('32-32'), a
128-row replay ring that wraps in mid-episode, updates that start after two
steps of pure collection and at first sample fewer rows than ``batch_size``.

Every random draw is an input that is recorded and replayed:

  * gaussian draws, in call order (``draws``, split by ``draw_rows``).  SAC:
    ``torch.distributions.normal._standard_normal`` (what ``Normal.rsample``
    draws).  DDPG: ``torch.normal(0, std, size)`` is given the body ``z *
    std`` with z ~ N(0, 1) recorded, ``torch.randn_like`` returns a recorded
    z.  TD3 explores with ``self.rng.normal(0, std, size)`` on the host: the
    ``rng`` constructor argument is a stand-in whose ``normal`` returns
    ``scale * z`` in float32 from a recorded float32 z (with a RandomState's
    float64 draws the action becomes float64 and the reference's own ring
    refuses it: ``index_put`` needs matching dtypes);
  * replay sampling: ``torch.randperm`` is replaced by a seeded permutation;
    ``sample_idx`` holds ``randperm(size)[:batch]`` of every update;
  * ``nreset`` draws from numpy's global generator: ``nreset_seed`` is set
    right before ``track_and_train``, the chosen seed points are stored;
  * ``NoisyTrackingEnvironment`` (the TD3 fixture, sigma = 0.05) draws from
    ``env_dto['rng']``: its state before the first step is stored as in
    ``trace_f64_K4_sigma``.

The initial weights are data (``init/*``): ``torch.manual_seed`` + the
reference's constructors, then -- for the two SAC fixtures -- the bias of the
log-std half of the actor's head set to -4 (a fresh policy with std = 1 stops
on curvature within three steps), then the twin's perturbation if any.

Robustness (asserted here): 8 "twins" per fixture repeat the run with every
initial weight scaled by 1 or 1 +- 2^-23 (one float32 ulp, seeded).  Every twin
must reproduce every discrete quantity of the main run bit for bit (rows per
step, dones, flags, streamline lengths, t, which steps updated, ring ptr /
size / not_done); the largest difference of each continuous quantity over the
twins is stored as ``twin_spread/<name>`` -- the only source of the continuous
tolerances of tests/test_training_golden.py.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden as mg  # noqa: E402
import make_golden_tracker as mgt  # noqa: E402

N_TWINS = 8
LOG_STD_BIAS = -4.0

# what the four fixtures share
COMMON = dict(D=14, K=4, theta=60.0, n_actor=32, hidden='32-32', batch_size=100,
              replay_size=128, start_timesteps=50, lr=3e-4, gamma=0.99,
              n_seeds=150)
FIXTURES = {
    'training_sac_auto': dict(alg='SACAuto', noisy=False, noise=0.0, seed_stream=1301,
                              weight_seed=31, nreset_seed=131, draw_seed=231),
    'training_sac': dict(alg='SAC', noisy=False, noise=0.0, seed_stream=1302,
                         weight_seed=32, nreset_seed=132, draw_seed=232),
    'training_td3': dict(alg='TD3', noisy=True, noise=0.05, seed_stream=1303,
                         weight_seed=33, nreset_seed=133, draw_seed=233),
    'training_ddpg': dict(alg='DDPG', noisy=False, noise=0.0, seed_stream=1304,
                          weight_seed=34, nreset_seed=134, draw_seed=234),
}
ACTION_STD = 0.05         # DDPG / TD3 exploration (the reference's default 0.35
#                           turns a fresh policy's streamlines back within 3 steps)


class Draws:
    """Seeded N(0, 1) float32 draws, recorded in call order."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.log = []

    def __call__(self, shape):
        z = self.rng.standard_normal(tuple(shape)).astype(np.float32)
        assert z.ndim == 2 and z.shape[1] == 3
        self.log.append(z)
        return z


class HostNormal:
    """Stand-in for the ``rng`` argument of TD3 (td3.py:111-128 calls
    ``rng.normal(0, std, size=...)``): ``scale * z`` in float32, z a recorded
    draw (float64 noise would make the action float64, which the reference's
    ring refuses)."""

    def __init__(self, draws):
        self.draws = draws

    def normal(self, loc, scale, size):
        assert loc == 0
        return np.float32(scale) * self.draws(size)


def build_env(ref, cfg):
    """The env of make_golden_tracker.build() with theta, reward and noise of
    this fixture."""
    mg._SEED_RNG.seed(cfg['seed_stream'])
    sh, mask, pk = mg.synthetic_subject(COMMON['D'])
    aff = mgt.rotated_affine()
    Vol = ref['MRIDataVolume']
    subject = (Vol(sh, aff), Vol(mask.astype(np.float32), aff),
               Vol(mask.astype(np.float32), aff), Vol(pk, aff), None)
    dto = dict(dataset_file=None, fa_map=None, n_dirs=COMMON['K'], step_size=0.75,
               theta=COMMON['theta'], min_length=2.0, max_length=40.0,
               noise=cfg['noise'], npv=1, rng=np.random.RandomState(3),
               alignment_weighting=1.0, oracle_bonus=0.0, oracle_validator=False,
               oracle_stopping_criterion=False, oracle_checkpoint=None,
               scoring_data=None, tractometer_validator=False,
               binary_stopping_threshold=0.1, compute_reward=True,
               device=torch.device('cpu'), target_sh_order=8)
    cls = ref['NoisyTrackingEnvironment' if cfg['noisy'] else 'TrackingEnvironment']
    env = cls(subject, 'testing', dto)
    pick = np.random.RandomState(11).permutation(len(env.seeds))[:COMMON['n_seeds']]
    env.seeds = env.seeds[pick]
    return env, sh, aff


def make_learner(cfg, width, draws):
    from TrackToLearn.algorithms.ddpg import DDPG
    from TrackToLearn.algorithms.sac import SAC
    from TrackToLearn.algorithms.sac_auto import SACAuto
    from TrackToLearn.algorithms.td3 import TD3
    kw = dict(lr=COMMON['lr'], gamma=COMMON['gamma'], n_actors=COMMON['n_actor'],
              batch_size=COMMON['batch_size'], replay_size=COMMON['replay_size'],
              rng=HostNormal(draws), device=torch.device('cpu'))
    torch.manual_seed(cfg['weight_seed'])
    name = cfg['alg']
    if name in ('SACAuto', 'SAC'):
        alg = (SACAuto if name == 'SACAuto' else SAC)(width, 3, COMMON['hidden'],
                                                      alpha=0.2, **kw)
        with torch.no_grad():
            list(alg.agent.actor.layers)[-1].bias[3:] = LOG_STD_BIAS
    else:
        alg = (TD3 if name == 'TD3' else DDPG)(width, 3, COMMON['hidden'],
                                               action_std=ACTION_STD, **kw)
    alg.start_timesteps = COMMON['start_timesteps']
    return alg


def perturb(alg, twin):
    """Every initial weight times 1, 1 - 2^-23 or 1 + 2^-23 (seeded)."""
    if twin is None:
        return
    rng = np.random.RandomState(9000 + twin)
    with torch.no_grad():
        for net in (alg.agent.actor, alg.agent.critic):
            for p in net.parameters():
                k = rng.randint(-1, 2, size=tuple(p.shape)).astype(np.float32)
                p.mul_(torch.from_numpy(np.float32(1) + k * np.float32(2.0 ** -23)))


def _flat(prefix, sd, out):
    for k, v in sd.items():
        out[f'{prefix}/{k}'] = v.detach().cpu().numpy().copy()


def run(ref, modules, cfg, twin=None):
    """One ``track_and_train`` of the reference; everything recorded."""
    import torch.distributions.normal as tdn
    env, sh, aff = build_env(ref, cfg)
    draws = Draws(cfg['draw_seed'])
    width = 7 * sh.shape[-1] + 3 * COMMON['K']
    alg = make_learner(cfg, width, draws)
    perturb(alg, twin)
    alg.target = copy.deepcopy(alg.agent)
    out = {}
    _flat('init/actor', alg.agent.actor.state_dict(), out)
    _flat('init/critic', alg.agent.critic.state_dict(), out)
    st = env.rng.get_state()
    out['rng_key'], out['rng_pos'] = st[1].copy(), np.int64(st[2])
    out['rng_has_gauss'], out['rng_cached'] = np.int64(st[3]), np.float64(st[4])

    steps = []
    real_step = env.step

    def step_spy(actions):
        rec = dict(t=alg.t, n=len(actions), actions=np.array(actions, copy=True),
                   it_before=alg.total_it)
        res = real_step(actions)
        _, reward, done, info = res
        rec['reward'] = np.array(reward, dtype=np.float64, copy=True)
        rec['done'] = np.array(done, copy=True)
        rec['info'] = {k: np.float64(v) for k, v in info['reward_info'].items()}
        steps.append(rec)
        return res
    env.step = step_spy

    updates, sample_idx = [], []
    real_update = alg.update

    def update_spy(batch):
        losses = real_update(batch)
        updates.append({k: np.float64(v) for k, v in losses.items()})
        return losses
    alg.update = update_spy

    perm_rng = np.random.RandomState(cfg['draw_seed'] + 500)

    def randperm(n, **kw):
        ind = perm_rng.permutation(n)
        sample_idx.append(ind[:COMMON['batch_size']].astype(np.int64))
        return torch.from_numpy(ind.astype(np.int64))

    def standard_normal(shape, dtype, device):
        return torch.from_numpy(draws(shape))

    def normal(mean, std, size, device=None):
        assert mean == 0
        return torch.from_numpy(draws(size)) * std

    def randn_like(t, **kw):
        return torch.from_numpy(draws(t.shape))

    saved = (tdn._standard_normal, torch.randperm, torch.normal, torch.randn_like)
    tdn._standard_normal, torch.randperm = standard_normal, randperm
    torch.normal, torch.randn_like = normal, randn_like
    try:
        tracker = modules['Tracker'](alg, n_actor=COMMON['n_actor'], prob=0.0)
        np.random.seed(cfg['nreset_seed'])
        tg, mean_losses, reward, factors = tracker.track_and_train(env)
    finally:
        tdn._standard_normal, torch.randperm, torch.normal, torch.randn_like = saved

    for i, s in enumerate(steps):
        s['updated'] = (steps[i + 1]['it_before'] if i + 1 < len(steps)
                        else alg.total_it) > s['it_before']
    out.update(
        alg=cfg['alg'], noisy=cfg['noisy'], noise=np.float64(cfg['noise']),
        D=COMMON['D'], C=sh.shape[-1], n_dirs=COMMON['K'], theta=COMMON['theta'],
        affine=aff, seeds=env.seeds.copy(), n_actor=COMMON['n_actor'],
        hidden=COMMON['hidden'], batch_size=COMMON['batch_size'],
        replay_size=COMMON['replay_size'], start_timesteps=COMMON['start_timesteps'],
        lr=COMMON['lr'], gamma=COMMON['gamma'], alpha=0.2, action_std=ACTION_STD,
        log_std_bias=LOG_STD_BIAS, nreset_seed=cfg['nreset_seed'],
        step_size=np.asarray(env.step_size),
        step_size_dtype=str(np.asarray(env.step_size).dtype),
        max_nb_steps=env.max_nb_steps, third_party_bodies=mgt.THIRD_PARTY,
        initial_points=np.asarray(env.initial_points).copy(),
        n_steps=len(steps),
        step_rows=np.array([s['n'] for s in steps], np.int64),
        step_t=np.array([s['t'] for s in steps], np.int64),
        step_updated=np.array([s['updated'] for s in steps], np.bool_),
        step_actions=np.concatenate([s['actions'] for s in steps]),
        step_actions_dtype=str(steps[0]['actions'].dtype),
        step_reward=np.concatenate([s['reward'] for s in steps]),
        step_done=np.concatenate([s['done'] for s in steps]).astype(np.bool_),
        n_updates=len(updates),
        sample_idx=(np.concatenate(sample_idx) if sample_idx
                    else np.zeros(0, np.int64)),
        sample_rows=np.array([len(i) for i in sample_idx], np.int64),
        draws=np.concatenate(draws.log),
        draw_rows=np.array([len(z) for z in draws.log], np.int64),
        ring_state=alg.replay_buffer.state.numpy().copy(),
        ring_action=alg.replay_buffer.action.numpy().copy(),
        ring_next_state=alg.replay_buffer.next_state.numpy().copy(),
        ring_reward=alg.replay_buffer.reward.numpy().copy(),
        ring_not_done=alg.replay_buffer.not_done.numpy().copy(),
        ring_ptr=np.int64(alg.replay_buffer.ptr),
        ring_size=np.int64(alg.replay_buffer.size),
        total_it=np.int64(alg.total_it), t=np.int64(alg.t),
        running_reward=np.float64(reward),
        episode_length=np.int64(len(steps)),
        tract_lengths=np.array([len(s) for s in tg.streamlines], np.int64),
        tract_points=np.concatenate(
            [np.asarray(s, np.float32).reshape(-1, 3) for s in tg.streamlines]),
        tract_flags=np.asarray(tg.data_per_streamline['flags']),
        tract_seeds=np.asarray(tg.data_per_streamline['seeds']))
    for k in steps[0]['info']:
        out[f'step_info/{k}'] = np.array([s['info'][k] for s in steps])
    for k in factors:
        out[f'reward_factors/{k}'] = np.asarray(factors[k], np.float64)
    # the losses dict of every update (empty for SACAuto, whose entries are
    # commented out upstream) and what track_and_train returned of them
    out['loss_keys'] = np.array(sorted(updates[0].keys()) if updates else [], dtype='U16')
    for k in out['loss_keys']:
        out[f'losses/{k}'] = np.array([u[k] for u in updates])
        got = np.array([np.float64(v) for v in mean_losses[k]])
        assert np.array_equal(got, out[f'losses/{k}'])
    assert sorted(mean_losses.keys()) == list(out['loss_keys'])
    _flat('final/actor', alg.agent.actor.state_dict(), out)
    _flat('final/critic', alg.agent.critic.state_dict(), out)
    _flat('final/target_actor', alg.target.actor.state_dict(), out)
    _flat('final/target_critic', alg.target.critic.state_dict(), out)
    if hasattr(alg, 'log_alpha'):
        out['final/log_alpha'] = alg.log_alpha.detach().numpy().copy()
    return out


DISCRETE = ('n_steps', 'step_rows', 'step_t', 'step_updated', 'step_done', 'n_updates',
            'sample_rows', 'draw_rows', 'ring_not_done', 'ring_ptr', 'ring_size',
            'total_it', 't', 'episode_length', 'tract_lengths', 'tract_flags',
            'tract_seeds', 'initial_points', 'sample_idx', 'draws')


def continuous_groups(out):
    """name of a tolerance -> the fixture's arrays it covers."""
    groups = {'actions': ['step_actions'], 'reward': ['step_reward'],
              'ring_state': ['ring_state'], 'ring_action': ['ring_action'],
              'ring_next_state': ['ring_next_state'], 'ring_reward': ['ring_reward'],
              'running_reward': ['running_reward'], 'streamlines': ['tract_points'],
              'reward_factors': [k for k in out if k.startswith(('reward_factors/',
                                                                 'step_info/'))],
              'losses': [k for k in out if k.startswith('losses/')]}
    for net in ('actor', 'critic', 'target_actor', 'target_critic'):
        groups[net] = [k for k in out if k.startswith(f'final/{net}/')]
    if 'final/log_alpha' in out:
        groups['log_alpha'] = ['final/log_alpha']
    return groups


def check_conditions(name, out):
    """What the issue asks of every fixture, asserted."""
    B, size = int(out['batch_size']), int(out['replay_size'])
    rows, upd = out['step_rows'], out['step_updated']
    assert out['n_steps'] >= 20 and out['n_updates'] >= 15, name
    assert not upd[:2].any(), f'{name}: fewer than 2 steps of pure collection'
    assert rows.sum() > size and out['ring_size'] == size, f'{name}: ring does not wrap'
    # the wrap happens in mid-episode: a step's rows straddle the end of the ring
    ends = np.cumsum(rows)
    assert np.any((ends - rows < size) & (ends > size)), name
    assert (out['sample_rows'] < B).any(), f'{name}: min(size, batch) never below batch'
    assert (out['sample_rows'] == B).any(), name
    assert np.array_equal(out['step_t'], 1 + np.concatenate(([0], ends[:-1])))
    assert np.array_equal(upd, out['step_t'] >= int(out['start_timesteps']))
    if out['alg'] == 'TD3':          # both delayed-actor phases
        assert out['n_updates'] >= 2
        al = out['losses/actor_loss']
        assert (al[0::2] == 0).all() and (al[1::2] != 0).all()
    assert out['step_done'].sum() == out['n_actor']


def record(ref, modules, name):
    cfg = FIXTURES[name]
    out = run(ref, modules, cfg)
    check_conditions(name, out)
    groups = continuous_groups(out)
    spread = {g: 0.0 for g in groups}
    for twin in range(N_TWINS):
        tw = run(ref, modules, cfg, twin=twin)
        for key in DISCRETE:
            a, b = np.asarray(out[key]), np.asarray(tw[key])
            assert a.dtype == b.dtype and a.shape == b.shape and \
                a.tobytes() == b.tobytes(), \
                f'{name}: twin {twin} differs in {key}; change the seeds'
        assert any(not np.array_equal(out[k], tw[k]) for k in out if k.startswith('init/'))
        for g, keys in groups.items():
            for k in keys:
                d = np.abs(np.asarray(out[k], np.float64) - np.asarray(tw[k], np.float64))
                spread[g] = max(spread[g], float(d.max()) if d.size else 0.0)
    for g, v in spread.items():
        out[f'twin_spread/{g}'] = np.float64(v)
    out['n_twins'] = N_TWINS
    mg._save(name, out)
    print(f'{name}: {out["n_steps"]} steps, rows {out["step_rows"].tolist()}, '
          f't={out["t"]}, {out["n_updates"]} updates (sampled '
          f'{sorted(set(out["sample_rows"].tolist()))}), ptr={out["ring_ptr"]} '
          f'size={out["ring_size"]}, reward {float(out["running_reward"]):.6f}')
    print('   twin spread: ' + ', '.join(f'{g} {v:.2e}' for g, v in spread.items()))


def main():
    if not os.path.isdir(mg.REFERENCE):
        sys.exit('reference tree not present; fixtures are committed')
    ref = mg.import_reference()
    sys.modules['nibabel.streamlines'].Tractogram = mgt.Holder
    sys.modules['dipy.io.stateful_tractogram'].Tractogram = mgt.Holder
    import TrackToLearn.environments.tracking_env as te
    te.Tractogram = mgt.Holder
    from TrackToLearn.tracking.tracker import Tracker
    modules = dict(Tracker=Tracker)
    for name in (sys.argv[1:] or FIXTURES):
        record(ref, modules, name)


if __name__ == '__main__':
    main()
