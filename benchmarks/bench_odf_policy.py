#!/usr/bin/env python3
"""The fODF policy: kernel, tracking end to end, Tractometer.

    python benchmarks/bench_odf_policy.py [--rows 4096 262144] [--track_rows 4096 65536]
                                          [--D 96] [--reps 20]

One JSON line per measurement:

``odf_policy_kernel``  ``ttl_odf_actions`` on fODF-like state rows (C = 28 and
    45, V = 321, theta 45 / 20 degrees) against the same quantity from plain
    torch -- ``state[:, :C] @ B``, masks, ``argmax`` or ``cumsum`` +
    ``searchsorted`` -- in the same process, the two interleaved repetition by
    repetition; HIP-event time, median of ``--reps`` after two warm-up runs.
``odf_policy_tracking``  ``Tracker.track`` of one seed batch on
    utils/synthetic.py's volume (D^3 x 45 SH, step 0.75 mm) with ``OdfTracking``
    (det and prob) and with a SAC ``1024-1024-1024`` network of random weights:
    wall time of the whole call, steps, streamlines kept.
``odf_policy_tractometer``  the Tractometer phases (classify, overlap, invalid;
    bench_tractometer.py's synthetic scoring set) on the tractogram the det
    policy tracked.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'benchmarks'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DEV = torch.device('cuda:0')


def torch_policy(state, C, dir_offset, B, dirs, cos_theta, rel, prob, u):
    """The kernel's quantity as a composition of torch operators."""
    sf = state[:, :C] @ B
    p = state[:, dir_offset:dir_offset + 3]
    dot = p @ dirs.T
    has_p = (p != 0).any(dim=1, keepdim=True)
    cone = (dot.abs() >= cos_theta * p.norm(dim=1, keepdim=True)) | ~has_p
    gmax = sf.max(dim=1, keepdim=True).values
    adm = cone & (sf > 0) & (sf >= rel * gmax)
    if prob:
        cdf = torch.where(adm, sf, torch.zeros_like(sf)).cumsum(dim=1)
        pick = torch.searchsorted(cdf, (u * cdf[:, -1])[:, None], right=True).squeeze(1)
        pick = pick.clamp_(max=sf.shape[1] - 1)
    else:
        pick = torch.where(adm, sf, torch.full_like(sf, -float('inf'))).argmax(dim=1)
    d = dirs[pick]
    sign = torch.where(dot.gather(1, pick[:, None]) < 0, -1.0, 1.0)
    return torch.where(adm.any(dim=1, keepdim=True), d * sign, torch.where(has_p, p, dirs[:1]))


def kernel_rows(rows, reps):
    import odf_cases as oc
    from tracktolearn_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for C, order in ((28, 6), (45, 8)):
        Bh, dh = oc.tables(order)
        B, dirs = torch.from_numpy(Bh).to(DEV), torch.from_numpy(dh).to(DEV)
        for n in rows:
            width = 7 * C + 12
            state = torch.randn((n, width), device=DEV) * 0.2
            state[:, 0] = 1.0 + torch.rand(n, device=DEV)
            p = torch.randn((n, 3), device=DEV)
            state[:, 7 * C:7 * C + 3] = p / p.norm(dim=1, keepdim=True)
            idx = torch.arange(n, dtype=torch.int32, device=DEV)
            out = torch.empty((n, 3), device=DEV)
            u = torch.rand(n, device=DEV)
            for mode, theta in ((_lib.ODF_DET, 45.0), (_lib.ODF_PROB, 20.0)):
                cos_t = oc.cos_deg(theta)

                def kernel():
                    _lib.check(lib.ttl_odf_actions(
                        state.data_ptr(), width, C, 7 * C, B.data_ptr(), dirs.data_ptr(),
                        dirs.shape[0], cos_t, 0.1, mode, 1, 0, idx.data_ptr(), n, 3,
                        out.data_ptr(), None, stream), 'ttl_odf_actions')

                def composed():
                    return torch_policy(state, C, 7 * C, B, dirs, cos_t, 0.1, mode, u)

                times = {'kernel': [], 'torch': []}
                for rep in range(reps + 2):
                    for name, fn in (('kernel', kernel), ('torch', composed)):
                        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        if rep >= 2:
                            times[name].append(e0.elapsed_time(e1))
                k, t = (float(np.median(times[x])) for x in ('kernel', 'torch'))
                print(json.dumps({
                    'object': 'odf_policy_kernel', 'rows': n, 'C': C, 'V': int(dirs.shape[0]),
                    'mode': 'prob' if mode else 'det', 'theta': theta,
                    'kernel_ms': round(k, 4), 'kernel_min_ms': round(min(times['kernel']), 4),
                    'torch_ms': round(t, 4), 'torch_min_ms': round(min(times['torch']), 4),
                    'torch_over_kernel': round(t / k, 2), 'reps': reps,
                    'device': torch.cuda.get_device_name(0)}), flush=True)


def make_env(D, N, K=4):
    """bench_bidirectional.py's env (bench.py's synthetic subject, step 0.75 mm,
    min_length 20 mm) with the curvature criterion 5 degrees wider than the det
    cone, as ``ttl_track.py --odf_policy`` sets it."""
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_subject
    subject = synthetic_subject(D, 45, seed=1234, peaks=False, affine_dtype=np.float64)
    dto = dict(n_dirs=K, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=20.0, max_length=200.0, compute_reward=False, alignment_weighting=1.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=DEV, target_sh_order=8,
               noise=0.0, fa_map=None)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=100)
    return env


def track_once(env, alg, N, seeds):
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env.seeds = seeds.copy()            # track() shuffles in place
    tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0)
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lines = [item.streamline for item in tracker.track(env, TrkFile)]
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), int(env.length - 1), lines


def tracking_rows(D, track_rows, reps):
    from tracktolearn_amd.algorithms.sac_auto import SACAuto
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    kept = None
    for N in track_rows:
        env = make_env(D, N)
        seeds = env.seeds.copy()
        torch.manual_seed(0)
        algs = [('odf_det', OdfTracking(env, 'det', seed=1)),
                ('odf_prob', OdfTracking(env, 'prob', seed=1)),
                ('1024-1024-1024', SACAuto(env.get_state_size(), 3, '1024-1024-1024', n_actors=N,
                                           rng=None, device=DEV))]
        best = {name: None for name, _ in algs}
        for rep in range(reps + 1):         # interleaved; the first round warms up
            for name, alg in algs:
                ms, steps, lines = track_once(env, alg, N, seeds)
                if rep and (best[name] is None or ms < best[name][0]):
                    best[name] = (ms, steps, lines)
        for name, (ms, steps, lines) in best.items():
            print(json.dumps({
                'object': 'odf_policy_tracking', 'policy': name, 'rows': N, 'volume': f'{D}^3 x 45',
                'track_ms': round(ms, 2), 'steps': steps, 'us_per_step': round(1e3 * ms / steps, 1),
                'streamlines_kept': len(lines),
                'mean_points': round(float(np.mean([len(s) for s in lines])), 1) if lines else 0,
                'reps': reps, 'device': torch.cuda.get_device_name(0)}), flush=True)
        kept = (env, best['odf_det'][2])
    return kept


def tractometer_row(env, lines, D):
    from bench_tractometer import N_BUNDLES, scoring_set
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels_from_tracker, pack
    from tracktolearn_amd.experiment.tractometer_validator import (ScoringData, Segmentation,
                                                                   classify, invalid,
                                                                   limits_table, metrics, overlap)
    aff = np.asarray(env.affine_vox2rasmm, np.float64)
    bundles = scoring_set(np.random.default_rng(0), D)
    cols = {k: [b[k] for b in bundles] for k in bundles[0]}
    R = 2 * N_BUNDLES
    valid = np.eye(R, dtype=bool)
    for b in range(N_BUNDLES):
        valid[b, N_BUNDLES + b] = valid[N_BUNDLES + b, b] = True
    data = ScoringData((D, D, D), cols['head'], cols['tail'], cols['all'], cols['any'],
                       cols['gt'], limits_table(cols['length'], cols['angle'], cols['dir'],
                                                cols['absdir']), DEV,
                       roi_masks=cols['head'] + cols['tail'], valid=valid)
    p, o = pack(lines)
    p = corner_voxels_from_tracker(p, aff, aff)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    visited = torch.zeros(D * D * D, dtype=torch.int64, device=DEV)
    ev[0].record()
    pd, od = torch.from_numpy(p).to(DEV), torch.from_numpy(o).to(DEV)
    ev[1].record()
    bundle, connected = classify(pd, od, data, aff[:3, :3])
    ev[2].record()
    counts, _ = overlap(pd, od, bundle, data, visited)
    ev[3].record()
    pair = invalid(pd, od, bundle, data)
    ev[4].record()
    ev[4].synchronize()
    s = Segmentation(data, bundle, connected, counts, pair).summary()
    n = len(lines)
    print(json.dumps({
        'object': 'odf_policy_tractometer', 'streamlines': n, 'points': int(len(p)),
        'bundles': N_BUNDLES, 'upload_ms': round(ev[0].elapsed_time(ev[1]), 3),
        'classify_ms': round(ev[1].elapsed_time(ev[2]), 3),
        'overlap_ms': round(ev[2].elapsed_time(ev[3]), 3),
        'invalid_ms': round(ev[3].elapsed_time(ev[4]), 3),
        'left_after_end_test': round(int((connected == 0).sum()) / max(n, 1), 4),
        'with_a_bundle': round(int(s.per_bundle.sum()) / max(n, 1), 4),
        'result': metrics(n, s.per_bundle, s.counts, data.gt_sizes, invalid=s.invalid),
        'device': torch.cuda.get_device_name(0)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='*', default=[4096, 262144])
    ap.add_argument('--track_rows', type=int, nargs='*', default=[4096, 65536])
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--track_reps', type=int, default=2)
    args = ap.parse_args(argv)
    kernel_rows(args.rows, args.reps)
    if args.track_rows:
        env, lines = tracking_rows(args.D, args.track_rows, args.track_reps)
        if lines:
            tractometer_row(env, lines, args.D)


if __name__ == '__main__':
    main()
