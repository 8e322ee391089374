#!/usr/bin/env python3
"""Probabilistic tracking (sigma = 0.1) of BASELINE config 1's shape (32^3
volume, K = 100) at n_actor 4 096 and 10 000: microseconds per step of

  host_step_by_step    the default: rng.normal on the host + upload every step;
  keyed_step_by_step   keyed noise drawn inside the step's first kernel
                       (device_noise='keyed'), same loop;
  keyed_free_running   keyed noise, policy + free-running step launched for the
                       newest reported survivor count (run_free_eager);
  keyed_graphed        keyed noise, policy + step in one replayed HIP graph,

with the scripted one-kernel policy and with a SAC `64-64` network.  Best of
five episodes after two warm-up episodes.  One JSON line.

    python benchmarks/bench_noisy_tracking.py [D]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA = 0.1


def make(D, N, keyed, K=100):
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import (synthetic_seeds,
                                                  synthetic_subject)
    subject = synthetic_subject(D, 45, seed=1234, peaks=False, affine_dtype=np.float64)
    dto = dict(n_dirs=K, theta=30.0, npv=1, binary_stopping_threshold=0.1,
               step_size=0.75, min_length=20.0, max_length=200.0,
               compute_reward=False, alignment_weighting=1.0, oracle_bonus=0.0,
               rng=np.random.RandomState(0), device=torch.device('cuda:0'),
               target_sh_order=8, noise=SIGMA, fa_map=None)
    if keyed:
        dto.update(device_noise='keyed', noise_seed=1337)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=100)
    return env


def scripted_episode(env, N, flavour):
    state = env.reset(0, N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if flavour == 'step_by_step':
        step = 0
        while state.shape[0] > 0:
            env.step_device(env.scripted_actions(state, step, 7, 0.05))
            state, _ = env.harvest()
            step += 1
    else:
        def policy(st):
            return env.scripted_actions_free(st, 7, 0.05)
        if flavour == 'free_running':
            env.run_free_eager(policy, state)
        else:
            env.run_free(policy, state, key='scripted')
    torch.cuda.synchronize()
    return time.perf_counter() - t0, env.length - 1


def network_episode(env, alg, N, flavour):
    os.environ['TTL_GRAPH_EPISODE'] = '0' if flavour == 'step_by_step' else '1'
    os.environ['TTL_FREE_RUNNING_EAGER'] = '1'
    type(alg).graph_policy_us = 1e9 if flavour == 'graphed' else 0.0
    state = env.reset(0, N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    alg.validation_episode(state, env, 0.0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, env.length - 1


def best_of(episode, warm=2, reps=5):
    for _ in range(warm):
        episode()
    dt, steps = min(episode() for _ in range(reps))
    return dict(us_per_step=round(dt / steps * 1e6, 2), steps=steps, ms=round(dt * 1e3, 3))


def main():
    D = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    from tracktolearn_amd.algorithms.sac_auto import SACAuto
    out = dict(workload=f'{D}^3 x 45 SH, K 100, sigma {SIGMA}', rows={})
    for N in (4096, 10000):
        torch.manual_seed(0)
        host, keyed = make(D, N, False), make(D, N, True)
        alg = SACAuto(keyed.get_state_size(), 3, '64-64', n_actors=N, rng=None,
                      device=torch.device('cuda:0'))
        alg.agent.eval()
        res = {}
        for policy in ('scripted', '64-64'):
            cols = {}
            for name, env, flavour in (('host_step_by_step', host, 'step_by_step'),
                                       ('keyed_step_by_step', keyed, 'step_by_step'),
                                       ('keyed_free_running', keyed, 'free_running'),
                                       ('keyed_graphed', keyed, 'graphed')):
                if policy == 'scripted':
                    cols[name] = best_of(lambda: scripted_episode(env, N, flavour))
                else:
                    cols[name] = best_of(lambda: network_episode(env, alg, N, flavour))
            res[policy] = cols
        out['rows'][str(N)] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
