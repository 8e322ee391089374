#!/usr/bin/env python3
"""Structural connectome: the kernel pair, and what it costs a tracking run.

    python benchmarks/bench_connectome.py [--rows 262144] [--nodes 84] [--D 96] [--reps 20]
                                          [--track_rows 4096] [--track_reps 5]
                                          [--legs kernels tracking | plain]

One JSON line per measurement:

``connectome_kernels``  ``--rows`` synthetic streamlines of 64 points (random
    walks through a D^3 label image of ``--nodes`` nodes painted on the shell of
    the synthetic ball).  ``ttl_connectome_assign`` + ``ttl_connectome_accumulate``
    at radius 2 mm and at radius 0 (HIP-event time, median of ``--reps`` after two
    warm-up runs), interleaved with the torch composition of radius 0
    (``labels[floor(end)]`` gather + ``index_put_(accumulate=True)`` of the counts;
    it computes no length, the kernels do), and ``accumulate`` alone against the
    ``index_put_`` alone.  Once: download of the packed points + the same in NumPy
    (wall clock).  The counts of all three are compared.
``connectome_tracking``  ``Tracker.track`` of one seed batch with
    ``OdfTracking('det')`` on utils/synthetic.py's volume (D^3 x 45 SH, step
    0.75 mm), three ways, interleaved: without a connectome (``plain``: the code
    path of the commit before the feature), with one attached, and
    ``track_connectome`` (nothing cut into items or downloaded).
``--legs plain`` runs the first of the three alone and needs nothing of the
    feature: the same script measures the parent commit's tree with it.
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

DEV = torch.device('cuda:0')
POINTS = 64


def painted_labels(D, n_nodes):
    """``n_nodes`` patches on the outer shell (r > 0.3 D) of the ball of radius
    0.42 D: the node of a voxel is the nearest of n_nodes random directions."""
    g = np.indices((D, D, D)).astype(np.float32) - np.float32((D - 1) / 2.0)
    r = np.sqrt((g ** 2).sum(0))
    dirs = np.random.RandomState(84).standard_normal((n_nodes, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    node = 1 + np.argmax(np.tensordot(dirs, g, axes=(1, 0)), axis=0)
    return np.where((r > 0.3 * D) & (r < 0.42 * D), node, 0).astype(np.int32)


def timed(fn):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def kernel_rows(n, n_nodes, D, reps):
    from tracktolearn_amd import connectome as con
    labels_h = painted_labels(D, n_nodes)
    labels = torch.from_numpy(labels_h.reshape(-1)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(n)
    start = torch.rand((n, 1, 3), device=DEV, generator=gen) * D
    steps = torch.randn((n, POINTS, 3), device=DEV, generator=gen) * 0.5
    steps[:, 0] = 0
    points = (start + torch.cumsum(steps, 1)).to(torch.float32).reshape(-1, 3).contiguous()
    offsets = torch.arange(n + 1, device=DEV, dtype=torch.int64) * POINTS
    dims, lin, side = (D, D, D), np.eye(3), n_nodes + 1
    mats = [torch.zeros((side, side), dtype=torch.int64, device=DEV) for _ in range(2)]

    def pair(radius):
        def run():
            node, length = con.assign_nodes(points, offsets, labels, dims, lin, radius, n_nodes)
            for m in mats:
                m.zero_()
            con.accumulate(node, length, n_nodes, *mats)
            return node, length
        return run

    def torch_nodes():
        ends = points.view(n, POINTS, 3)[:, [0, POINTS - 1]]
        v = torch.floor(ends).long()
        inside = ((v >= 0) & (v < D)).all(dim=2)
        v = v.clamp(0, D - 1)
        lab = labels[(v[..., 0] * D + v[..., 1]) * D + v[..., 2]].long()
        return torch.where(inside & (lab >= 1) & (lab <= n_nodes), lab, torch.zeros_like(lab))

    def torch_count(node):
        count = torch.zeros((side, side), dtype=torch.int64, device=DEV)
        a, b = node.min(dim=1).values, node.max(dim=1).values
        count.index_put_((a, b), torch.ones_like(a), accumulate=True)
        return count

    node0, length0 = pair(0.0)()
    count0 = mats[0].clone()
    agree = bool(torch.equal(torch_count(torch_nodes()), count0))
    node0_long = node0.long()
    legs = {'pair_r2': pair(2.0), 'pair_r0': pair(0.0),
            'torch_r0': lambda: torch_count(torch_nodes()),
            'assign_r2': lambda: con.assign_nodes(points, offsets, labels, dims, lin, 2.0, n_nodes),
            'accumulate': lambda: con.accumulate(node0, length0, n_nodes, *mats),
            'index_put': lambda: torch_count(node0_long)}
    times = {k: [] for k in legs}
    for rep in range(reps + 2):
        for name, fn in legs.items():
            ms, _ = timed(fn)
            if rep >= 2:
                times[name].append(ms)
    # what a user without the kernels does: the points to the host, NumPy there
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = points.cpu().numpy().reshape(n, POINTS, 3)
    t1 = time.perf_counter()
    v = np.floor(host[:, [0, POINTS - 1]]).astype(np.int64)
    inside = ((v >= 0) & (v < D)).all(axis=2)
    v = np.clip(v, 0, D - 1)
    lab = labels_h[v[..., 0], v[..., 1], v[..., 2]].astype(np.int64)
    lab = np.where(inside & (lab >= 1), lab, 0)
    seg = np.diff(host.astype(np.float64), axis=1)
    length = np.sqrt((seg ** 2).sum(axis=2)).sum(axis=1)
    count = np.zeros((side, side), np.int64)
    np.add.at(count, (lab.min(axis=1), lab.max(axis=1)), 1)
    t2 = time.perf_counter()
    med = {k: round(float(np.median(t)), 4) for k, t in times.items()}
    print(json.dumps({
        'object': 'connectome_kernels', 'rows': n, 'points_per_row': POINTS, 'nodes': n_nodes,
        'labels': f'{D}^3', **{k + '_ms': v for k, v in med.items()},
        **{k + '_min_ms': round(min(t), 4) for k, t in times.items()},
        'torch_r0_over_pair_r0': round(med['torch_r0'] / med['pair_r0'], 2),
        'index_put_over_accumulate': round(med['index_put'] / med['accumulate'], 2),
        'download_ms': round(1e3 * (t1 - t0), 1), 'numpy_ms': round(1e3 * (t2 - t1), 1),
        'counts_agree_torch': agree,
        'counts_agree_numpy': bool(np.array_equal(count, count0.cpu().numpy())),
        'length_max_rel_diff_numpy': float(np.max(np.abs(length - length0.cpu().numpy())
                                                  / np.maximum(length, 1e-30))),
        'connected_rows': int(count0[1:, 1:].sum()), 'reps': reps,
        'device': torch.cuda.get_device_name(0)}), flush=True)


def make_env(D, N):
    """bench_odf_policy.py's env."""
    from tracktolearn_amd.environments import NoisyTrackingEnvironment
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_subject
    subject = synthetic_subject(D, 45, seed=1234, peaks=False, affine_dtype=np.float64)
    dto = dict(n_dirs=4, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=20.0, max_length=200.0, compute_reward=False, alignment_weighting=1.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=DEV, target_sh_order=8,
               noise=0.0, fa_map=None)
    env = NoisyTrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, N, seed=100)
    return env


def tracking_rows(D, track_rows, n_nodes, reps, plain_only):
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    for N in track_rows:
        env = make_env(D, N)
        seeds = env.seeds.copy()
        alg = OdfTracking(env, 'det', seed=1)
        connectome = None
        if not plain_only:
            from tracktolearn_amd.connectome import Connectome
            connectome = Connectome(painted_labels(D, n_nodes), np.eye(4), radius_mm=2.0,
                                    device=DEV)

        def run(leg):
            env.seeds = seeds.copy()            # track() shuffles in place
            options = {} if leg == 'plain' else {'connectome': connectome}
            tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0, **options)
            if connectome is not None:
                connectome.count.zero_()
                connectome.length_q.zero_()
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if leg == 'connectome_only':
                tracker.track_connectome(env)
                kept = int(connectome.count.sum().item())
            else:
                kept = len([item.streamline for item in tracker.track(env, TrkFile)])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), kept

        legs = ['plain'] if plain_only else ['plain', 'connectome_attached', 'connectome_only']
        runs = {leg: [] for leg in legs}
        for rep in range(reps + 1):             # interleaved; the first round warms up
            for leg in legs:
                got = run(leg)
                if rep:
                    runs[leg].append(got)
        for leg, got in runs.items():
            ms = [g[0] for g in got]
            print(json.dumps({
                'object': 'connectome_tracking', 'leg': leg, 'rows': N, 'volume': f'{D}^3 x 45',
                'nodes': n_nodes, 'track_ms_median': round(float(np.median(ms)), 2),
                'track_ms_min': round(min(ms), 2), 'track_ms_max': round(max(ms), 2),
                'streamlines_kept': got[0][1], 'reps': reps,
                'device': torch.cuda.get_device_name(0)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--nodes', type=int, default=84)
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--track_rows', type=int, nargs='*', default=[4096])
    ap.add_argument('--track_reps', type=int, default=5)
    ap.add_argument('--legs', nargs='*', default=['kernels', 'tracking'],
                    choices=['kernels', 'tracking', 'plain'])
    args = ap.parse_args(argv)
    if 'kernels' in args.legs:
        kernel_rows(args.rows, args.nodes, args.D, args.reps)
    if 'tracking' in args.legs or 'plain' in args.legs:
        tracking_rows(args.D, args.track_rows, args.nodes, args.track_reps,
                      'tracking' not in args.legs)


if __name__ == '__main__':
    main()
