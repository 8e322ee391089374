#!/usr/bin/env python3
"""ACT / CMC stopping: the kernel, and what it costs a tracking run.

    python benchmarks/bench_act.py [--rows 4096 262144] [--track_rows 4096] [--D 96]
                                   [--reps 20] [--track_reps 5]

One JSON line per measurement:

``act_kernel``  ``ttl_act_flags`` (threshold and CMC) on random points in two
    D^3 maps against the same definition composed of torch operators, in the
    same process, the two interleaved repetition by repetition; HIP-event time,
    median of ``--reps`` after two warm-up runs.  The flags of both are compared
    once (the composition rounds like the kernel except where torch contracts).
``act_tracking``  ``Tracker.track`` of one seed batch with ``OdfTracking('det')``
    and with a SAC ``64-64`` network of random weights (a policy cheap enough for
    the loop to be bound by its launches) on utils/synthetic.py's volume (D^3 x 45
    SH, step 0.75 mm), five ways, interleaved: without tissue maps and
    free-running (the graphed loop), without tissue maps step by step
    (``TTL_GRAPH_EPISODE=0``), with tissue maps between the two halves of the
    step (``ttl_act_flags``; step by step by necessity), with tissue maps in the
    step (``env_dto['act_in_step']``, ``ttl_env_set_act``) step by step, and with
    tissue maps in the step graphed.  Third minus second is what ACT itself
    costs outside the step, fourth minus second inside it; fifth against first is
    what the graphed loop pays for the maps, fifth against third what putting
    them into the step wins.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device('cuda:0')
TARGET, EXCLUDE = 8, 128


def torch_act(inc, exc, hist, ids, n_points, cmc, exponent, u1, u2):
    """``ttl_act_flags`` without suppression as torch operators (the uniforms
    are given: torch has no Philox keyed like the kernel's)."""
    dims = torch.tensor(inc.shape, device=inc.device, dtype=torch.float64)
    x = hist[ids.long(), n_points - 1].double()
    inside = ((x >= -0.5) & (x < dims - 0.5)).all(dim=1)
    x = torch.where(inside[:, None], x, torch.zeros_like(x))
    fl = torch.floor(x)
    f = x - fl
    i = fl.long()
    hi_max = torch.tensor(inc.shape, device=inc.device) - 1
    lo = torch.minimum(i.clamp(min=0), hi_max)
    hi = torch.minimum((i + 1).clamp(min=0), hi_max)

    def sample(v):
        v = v.double()
        c = [[None, None], [None, None]]
        for a, ix in enumerate((lo[:, 0], hi[:, 0])):
            for b, iy in enumerate((lo[:, 1], hi[:, 1])):
                c[a][b] = v[ix, iy, lo[:, 2]] * (1 - f[:, 2]) + v[ix, iy, hi[:, 2]] * f[:, 2]
        c0 = c[0][0] * (1 - f[:, 1]) + c[0][1] * f[:, 1]
        c1 = c[1][0] * (1 - f[:, 1]) + c[1][1] * f[:, 1]
        return torch.where(inside, c0 * (1 - f[:, 0]) + c1 * f[:, 0], torch.zeros_like(c0))

    vi, ve = sample(inc), sample(exc)
    if not cmc:
        out = torch.where(vi > 0.5, TARGET, torch.where(ve > 0.5, EXCLUDE, 0))
    else:
        s = vi + ve
        num = (1 - s).clamp(min=0)
        p = (num / (num + s)) ** exponent
        stop = (s > 0) & (u1 >= p)
        out = torch.where(stop, torch.where(u2 < vi / s, TARGET, EXCLUDE), 0)
    return out.to(torch.uint8)


def tissue_maps(D):
    """Maps for the synthetic ball of radius 0.42 D: a grey-matter shell under its
    surface (include, smooth ramp) and a ventricle at its centre (exclude)."""
    g = np.indices((D, D, D)).astype(np.float32)
    r = np.sqrt(((g - np.float32((D - 1) / 2.0)) ** 2).sum(0)) / np.float32(D)
    inc = np.clip((r - 0.34) / 0.04, 0.0, 1.0).astype(np.float32)
    exc = np.clip((0.08 - r) / 0.02, 0.0, 1.0).astype(np.float32)
    return inc, exc


def kernel_rows(rows, D, reps):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    inc_h, exc_h = tissue_maps(D)
    inc, exc = torch.from_numpy(inc_h).to(DEV), torch.from_numpy(exc_h).to(DEV)
    n_points, T = 40, 64
    for n in rows:
        gen = torch.Generator(device=DEV).manual_seed(n)
        hist = torch.rand((n, T, 3), device=DEV, generator=gen) * (D + 2) - 1.5
        ids = torch.randperm(n, device=DEV, generator=gen).to(torch.int32)
        out = torch.empty(n, dtype=torch.uint8, device=DEV)
        u1 = torch.rand(n, device=DEV, generator=gen, dtype=torch.float64)
        u2 = torch.rand(n, device=DEV, generator=gen, dtype=torch.float64)
        for mode, name in ((_lib.ACT_THRESHOLD, 'act'), (_lib.ACT_CMC, 'cmc')):
            d = _lib.ActDesc()
            d.include, d.exclude = inc.data_ptr(), exc.data_ptr()
            d.dim[:] = [D, D, D]
            d.mode, d.exponent, d.seed, d.ids_base = mode, 0.75, 7, 0

            def kernel():
                _lib.check(lib.ttl_act_flags(
                    C.byref(d), hist.data_ptr(), hist.stride(0), ids.data_ptr(), None, n,
                    n_points, out.data_ptr(), None, stream), 'ttl_act_flags')

            def composed():
                return torch_act(inc, exc, hist, ids, n_points, mode == _lib.ACT_CMC, 0.75,
                                 u1, u2)

            agree = None
            if mode == _lib.ACT_THRESHOLD:
                kernel()
                agree = float((composed() == out).double().mean())
            times = {'kernel': [], 'torch': []}
            for rep in range(reps + 2):
                for which, fn in (('kernel', kernel), ('torch', composed)):
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        times[which].append(e0.elapsed_time(e1))
            k, t = (float(np.median(times[x])) for x in ('kernel', 'torch'))
            print(json.dumps({
                'object': 'act_kernel', 'rows': n, 'maps': f'{D}^3', 'mode': name,
                'kernel_ms': round(k, 4), 'kernel_min_ms': round(min(times['kernel']), 4),
                'torch_ms': round(t, 4), 'torch_min_ms': round(min(times['torch']), 4),
                'torch_over_kernel': round(t / k, 2), 'flags_agree': agree, 'reps': reps,
                'device': torch.cuda.get_device_name(0)}), flush=True)


def make_env(D, N, maps=None, in_step=False):
    """bench_odf_policy.py's env, with tissue maps on request."""
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_subject
    subject = synthetic_subject(D, 45, seed=1234, peaks=False, affine_dtype=np.float64)
    dto = dict(n_dirs=4, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=20.0, max_length=200.0, compute_reward=False, alignment_weighting=1.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=DEV, target_sh_order=8,
               noise=0.0, fa_map=None)
    if maps is not None:
        dto.update(act_include=maps[0], act_exclude=maps[1], act_mode='act', act_seed=1,
                   act_in_step=in_step)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=100)
    return env


def track_once(env, alg, N, seeds, graph, act_filter=None):
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env.seeds = seeds.copy()            # track() shuffles in place
    tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0,
                      act_filter=act_filter)
    np.random.seed(0)
    os.environ['TTL_GRAPH_EPISODE'] = '1' if graph else '0'
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lines = [item.streamline for item in tracker.track(env, TrkFile)]
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), int(env.length - 1), len(lines)


def tracking_rows(D, track_rows, reps):
    from tracktolearn_amd.algorithms.sac_auto import SACAuto
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    maps = tissue_maps(D)
    for N in track_rows:
        plain, act, instep = make_env(D, N), make_env(D, N, maps), make_env(D, N, maps, True)
        seeds = plain.seeds.copy()
        torch.manual_seed(0)
        # the fODF policy, whose kernel bounds a step at this size, and a network
        # small enough for the loop to be bound by its launches (random weights)
        small = SACAuto(plain.get_state_size(), 3, '64-64', n_actors=N, rng=None, device=DEV)
        small.graph_policy_us = 1e9         # the graph whenever the env allows it
        for policy, on_plain, on_act, on_instep in (
                ('odf_det', OdfTracking(plain, 'det', seed=1), OdfTracking(act, 'det', seed=1),
                 OdfTracking(instep, 'det', seed=1)),
                ('64-64', small, small, small)):
            legs = [('plain_freerun', plain, on_plain, True, None),
                    ('plain_stepwise', plain, on_plain, False, None),
                    ('act_stepwise', act, on_act, True, 'exclude'),
                    ('act_instep_stepwise', instep, on_instep, False, 'exclude'),
                    ('act_instep_freerun', instep, on_instep, True, 'exclude')]
            runs = {name: [] for name, *_ in legs}
            for rep in range(reps + 1):         # interleaved; the first round warms up
                for name, env, alg, graph, act_filter in legs:
                    got = track_once(env, alg, N, seeds, graph, act_filter)
                    if rep:
                        runs[name].append(got)
            for name, got in runs.items():
                ms = [g[0] for g in got]
                steps, kept = got[0][1], got[0][2]
                print(json.dumps({
                    'object': 'act_tracking', 'policy': policy, 'leg': name, 'rows': N,
                    'volume': f'{D}^3 x 45', 'track_ms_median': round(float(np.median(ms)), 2),
                    'track_ms_min': round(min(ms), 2), 'track_ms_max': round(max(ms), 2),
                    'steps': steps,
                    'us_per_step_median': round(1e3 * float(np.median(ms)) / max(steps, 1), 1),
                    'streamlines_kept': kept, 'reps': reps,
                    'device': torch.cuda.get_device_name(0)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='*', default=[4096, 262144])
    ap.add_argument('--track_rows', type=int, nargs='*', default=[4096])
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--track_reps', type=int, default=5)
    args = ap.parse_args(argv)
    kernel_rows(args.rows, args.D, args.reps)
    if args.track_rows:
        tracking_rows(args.D, args.track_rows, args.track_reps)


if __name__ == '__main__':
    main()
