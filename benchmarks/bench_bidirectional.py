#!/usr/bin/env python3
"""Bidirectional tracking: `Tracker.track` forward-only against
`Tracker(bidirectional=True)` on one seed batch of n_actor 4 096 and 262 144
rows (32^3 volume, K = 4, no noise), with the scripted one-kernel policy and
with a SAC `1024-1024-1024` network.  Per run: wall time of the whole `track`
(output stage included), and per pass the time, the number of steps and the
row-steps.  For the backward pass also the share of its row-steps that were
replays: there the policy is evaluated and its action ignored, so that share
is what skipping the policy on replaying rows could save.  Best of `reps`
runs after one warm-up run.  One JSON line.

    python benchmarks/bench_bidirectional.py [D [reps]]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(D, N, K=4):
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import (synthetic_seeds,
                                                  synthetic_subject)
    subject = synthetic_subject(D, 45, seed=1234, peaks=False, affine_dtype=np.float64)
    dto = dict(n_dirs=K, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=20.0, max_length=200.0,
               compute_reward=False, alignment_weighting=1.0, oracle_bonus=0.0,
               rng=np.random.RandomState(0), device=torch.device('cuda:0'),
               target_sh_order=8, noise=0.0, fa_map=None)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=100)
    return env


class ScriptedAlg:
    """RLAlgorithm over `ttl_scripted_actions` (follows the newest segment)."""

    def __init__(self, env):
        from tracktolearn_amd.algorithms.rl import RLAlgorithm

        class Agent:
            def eval(self):
                pass

            def select_action(self, state, probabilistic=0.0):
                return env.scripted_actions(state, env.length - 1, 7, 0.05)
        self.agent = Agent()
        self.validation_episode = RLAlgorithm.validation_episode.__get__(self)


class PassTimer:
    """Wraps an algorithm's validation_episode: time, steps and row-steps of
    every pass of a batch, and the replay share of the backward one."""

    def __init__(self, alg, env):
        self.alg, self.env, self.passes = alg, env, []
        self._inner = alg.validation_episode
        alg.validation_episode = self

    def __call__(self, state, env, prob=1.):
        backward = env._init_len is not None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self._inner(state, env, prob)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = env._n_total
        row_steps = env._buf_lengths[:n].long() - 1
        rec = dict(ms=round(dt * 1e3, 3), steps=int(env.length - 1),
                   row_steps=int(row_steps.sum()))
        rec['us_per_step'] = round(dt / max(rec['steps'], 1) * 1e6, 2)
        if backward:
            replays = torch.minimum(env._init_len[:n].long() - 1, row_steps)
            rec['replay_row_steps'] = int(replays.sum())
            rec['replay_share'] = round(rec['replay_row_steps'] / max(rec['row_steps'], 1), 4)
        self.passes.append(rec)
        return out

    def close(self):
        self.alg.validation_episode = self._inner


def run(env, alg, N, bidirectional):
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    timer = PassTimer(alg, env)
    try:
        tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0,
                          bidirectional=bidirectional)
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        items = sum(1 for _ in tracker.track(env, TrkFile))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        timer.close()
    rec = dict(track_ms=round(dt * 1e3, 3), streamlines=items, forward=timer.passes[0])
    if bidirectional:
        rec['backward'] = timer.passes[1]
    return rec


def best_of(fn, reps):
    fn()
    return min((fn() for _ in range(reps)), key=lambda r: r['track_ms'])


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    from tracktolearn_amd.algorithms.sac_auto import SACAuto
    out = dict(workload=f'{D}^3 x 45 SH, K 4, one batch, min_length 20 mm', rows={})
    for N in (4096, 262144):
        env = make(D, N)
        seeds = env.seeds.copy()
        torch.manual_seed(0)
        net = SACAuto(env.get_state_size(), 3, '1024-1024-1024', n_actors=N, rng=None,
                      device=torch.device('cuda:0'))
        res = {}
        for name, alg in (('scripted', ScriptedAlg(env)), ('1024-1024-1024', net)):
            cols = {}
            for mode, both in (('forward_only', False), ('bidirectional', True)):
                def once():
                    env.seeds = seeds.copy()        # track() shuffles in place
                    return run(env, alg, N, both)
                cols[mode] = best_of(once, reps)
            res[name] = cols
        out['rows'][str(N)] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
