#!/usr/bin/env python3
"""Weighted connectome edges: the sampling kernel, the whole pass with one
metric, and what a metric costs a tracking run.

    python benchmarks/bench_connectome_metric.py [--rows 262144] [--nodes 84] [--D 96]
                                                 [--reps 20] [--track_rows 4096]
                                                 [--track_reps 5] [--legs kernels tracking]

One JSON line per measurement, on the shapes of bench_connectome.py (its synthetic
streamlines of 64 points, its painted label image):

``connectome_metric_kernels``  HIP-event time, median of ``--reps`` after two warm-up
    runs, legs interleaved: ``ttl_tract_sample_mean`` alone; ``ttl_connectome_assign``
    alone; assign + accumulate (DESIGN 3.15's pair); assign + sample_mean + both
    accumulates (the pass with one metric); and a torch composition of the metric part
    (``grid_sample`` at the points, border padding, + the plain per-row mean +
    ``index_put_(accumulate=True)`` of sum and count: float32, uniform point weights, no
    dropped points -- what one writes without the kernel, not the same definition; how far
    its per-row means lie from the kernel's is reported for the rows inside the volume).
    The achieved bytes per second count what the kernel must move: the points, the
    offsets and its two outputs; the eight corner loads per point are counted apart.
``connectome_metric_tracking``  ``Tracker.track`` of one seed batch as
    bench_connectome.py runs it, interleaved: without a connectome, with one attached,
    and with one that carries one metric.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bench_connectome as base     # noqa: E402

DEV = base.DEV
POINTS = base.POINTS


def metric_volume(D):
    """A smooth positive map with noise, FA-like, (D, D, D) float32."""
    g = np.indices((D, D, D)).astype(np.float32) / np.float32(D)
    rng = np.random.RandomState(16)
    v = 0.4 + 0.3 * np.sin(6.0 * g[0]) * np.cos(5.0 * g[1]) + 0.1 * g[2]
    return (v + 0.05 * rng.standard_normal((D, D, D))).clip(0.0, 1.0).astype(np.float32)


def kernel_rows(n, n_nodes, D, reps):
    from tracktolearn_amd import connectome as con
    labels = torch.from_numpy(base.painted_labels(D, n_nodes).reshape(-1)).to(DEV)
    volume_h = metric_volume(D)
    volume = torch.from_numpy(volume_h).to(DEV)
    scale = con.metric_scale(volume_h)
    gen = torch.Generator(device=DEV).manual_seed(n)
    start = torch.rand((n, 1, 3), device=DEV, generator=gen) * D
    steps = torch.randn((n, POINTS, 3), device=DEV, generator=gen) * 0.5
    steps[:, 0] = 0
    points = (start + torch.cumsum(steps, 1)).to(torch.float32).reshape(-1, 3).contiguous()
    offsets = torch.arange(n + 1, device=DEV, dtype=torch.int64) * POINTS
    dims, lin, side = (D, D, D), np.eye(3), n_nodes + 1
    mats = [torch.zeros((side, side), dtype=torch.int64, device=DEV) for _ in range(4)]

    def full():
        node, length = con.assign_nodes(points, offsets, labels, dims, lin, 2.0, n_nodes)
        mean, _ = con.sample_mean(points, offsets, volume, lin)
        for m in mats:
            m.zero_()
        con.accumulate(node, length, n_nodes, mats[0], mats[1])
        con.accumulate_metric(node, mean, n_nodes, scale, mats[2], mats[3])
        return node, mean

    def pair():
        node, length = con.assign_nodes(points, offsets, labels, dims, lin, 2.0, n_nodes)
        for m in mats[:2]:
            m.zero_()
        con.accumulate(node, length, n_nodes, mats[0], mats[1])

    node0, mean0 = full()
    a0, b0 = node0.min(dim=1).values.long(), node0.max(dim=1).values.long()
    scored = node0[:, 0] >= 0
    # grid_sample: x is the fastest (last) axis of the input, coordinates in [-1, 1] from
    # edge to edge (align_corners=False puts voxel centres at v + 0.5)
    grid = (points.flip(1) * (2.0 / D) - 1.0).view(1, n, POINTS, 1, 3)
    vol5 = volume.view(1, 1, D, D, D)

    def torch_metric():
        s = torch.nn.functional.grid_sample(vol5, grid, mode='bilinear', padding_mode='border',
                                            align_corners=False)
        mean = s.view(n, POINTS).mean(dim=1).double()
        total = torch.zeros((side, side), dtype=torch.float64, device=DEV)
        count = torch.zeros((side, side), dtype=torch.int64, device=DEV)
        total.index_put_((a0[scored], b0[scored]), mean[scored], accumulate=True)
        count.index_put_((a0[scored], b0[scored]), torch.ones_like(a0[scored]), accumulate=True)
        return mean, total, count

    legs = {'sample_mean': lambda: con.sample_mean(points, offsets, volume, lin),
            'assign_r2': lambda: con.assign_nodes(points, offsets, labels, dims, lin, 2.0,
                                                  n_nodes),
            'pair_r2': pair, 'full_one_metric': full,
            'accumulate_metric': lambda: con.accumulate_metric(node0, mean0, n_nodes, scale,
                                                               mats[2], mats[3]),
            'torch_metric': torch_metric}
    times = {k: [] for k in legs}
    for rep in range(reps + 2):
        for name, fn in legs.items():
            ms, _ = base.timed(fn)
            if rep >= 2:
                times[name].append(ms)
    full()
    torch_mean, torch_total, torch_count = torch_metric()
    finite = torch.isfinite(mean0)
    # rows that never leave the volume: there the two differ by the point weights and float32
    inside = ((points >= 0) & (points <= D)).all(dim=1).view(n, POINTS).all(dim=1) & finite
    med = {k: round(float(np.median(t)), 4) for k, t in times.items()}
    moved = points.numel() * 4 + offsets.numel() * 8 + 2 * n * 8
    corners = points.shape[0] * 8 * 4
    print(json.dumps({
        'object': 'connectome_metric_kernels', 'rows': n, 'points_per_row': POINTS,
        'nodes': n_nodes, 'volume': f'{D}^3', **{k + '_ms': v for k, v in med.items()},
        **{k + '_min_ms': round(min(t), 4) for k, t in times.items()},
        'sample_mean_over_assign': round(med['sample_mean'] / med['assign_r2'], 2),
        'cost_per_extra_metric_ms': round(med['full_one_metric'] - med['pair_r2'], 4),
        'torch_metric_over_metric_part': round(
            med['torch_metric'] / (med['sample_mean'] + med['accumulate_metric']), 2),
        'sample_mean_moved_MB': round(moved / 1e6, 1),
        'sample_mean_moved_GB_per_s': round(moved / 1e6 / med['sample_mean'], 1),
        'sample_mean_corner_loads_MB': round(corners / 1e6, 1),
        'sample_mean_corner_loads_GB_per_s': round(corners / 1e6 / med['sample_mean'], 1),
        'rows_with_a_mean': int(finite.sum().item()),
        'metric_n_agrees_torch_count': bool(torch.equal(
            mats[3], torch.zeros_like(mats[3]).index_put_(
                (a0[scored & finite], b0[scored & finite]),
                torch.ones_like(a0[scored & finite]), accumulate=True))),
        'rows_inside': int(inside.sum().item()),
        'torch_uniform_mean_max_abs_diff_inside': float(
            (torch_mean[inside] - mean0[inside]).abs().max().item()),
        'torch_uniform_mean_mean_abs_diff_inside': float(
            (torch_mean[inside] - mean0[inside]).abs().mean().item()),
        'scale': scale, 'reps': reps, 'device': torch.cuda.get_device_name(0)}), flush=True)


def tracking_rows(D, track_rows, n_nodes, reps):
    from tracktolearn_amd.connectome import Connectome
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    for N in track_rows:
        env = base.make_env(D, N)
        seeds = env.seeds.copy()
        alg = OdfTracking(env, 'det', seed=1)
        labels = base.painted_labels(D, n_nodes)
        cons = {'plain': None,
                'connectome_attached': Connectome(labels, np.eye(4), radius_mm=2.0, device=DEV),
                'one_metric': Connectome(labels, np.eye(4), radius_mm=2.0, device=DEV,
                                         metrics={'fa': metric_volume(D)})}

        def run(leg):
            env.seeds = seeds.copy()            # track() shuffles in place
            options = {} if cons[leg] is None else {'connectome': cons[leg]}
            tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0, **options)
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = len([item.streamline for item in tracker.track(env, TrkFile)])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), kept

        runs = {leg: [] for leg in cons}
        for rep in range(reps + 1):             # interleaved; the first round warms up
            for leg in cons:
                got = run(leg)
                if rep:
                    runs[leg].append(got)
        for leg, got in runs.items():
            ms = [g[0] for g in got]
            print(json.dumps({
                'object': 'connectome_metric_tracking', 'leg': leg, 'rows': N,
                'volume': f'{D}^3 x 45', 'nodes': n_nodes,
                'track_ms_median': round(float(np.median(ms)), 2),
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
                    choices=['kernels', 'tracking'])
    args = ap.parse_args(argv)
    if 'kernels' in args.legs:
        kernel_rows(args.rows, args.nodes, args.D, args.reps)
    if 'tracking' in args.legs:
        tracking_rows(args.D, args.track_rows, args.nodes, args.track_reps)


if __name__ == '__main__':
    main()
