#!/usr/bin/env python3
"""Streamline registration: ttl_bundle_register_cost alone, against a torch
composition and against download + NumPy, and one whole ``register_atlas``.

    python benchmarks/bench_bundle_register.py [--shapes 600,600,20,25 4096,4096,20,25 ...]
                                               [--D 96] [--reps 5] [--torch_transforms 2]
                                               [--numpy_fixed 64] [--fit_lines 4096]
                                               [--numpy_fit_lines 32]

One JSON line.  Synthetic bundles: curved lines of a D^3 grid of 2 mm voxels, 64 lines to a
bundle, the fixed set the moving set under a planted affine with 0.5 mm of jitter and every second
line reversed.  HIP-event time, median of ``--reps`` after two warm-up runs, per shape (A, B, K,
T):

``kernel``  ``ttl_bundle_register_cost`` alone (the fill of col_min, the distances, the closing
    launch); ms, distances per second (A x B x K x 2 x T) and their share of the vector float64
    rate, counted as bench_bundle_recognize.py counts it: 36 float64 arithmetic instructions per
    distance against 39.3e12 float64 lane-instructions per second.
``torch``  the float64 composition on the device, chunked over the fixed lines so that the
    (lines, B, K, 3) intermediate stays under 2 GiB: transform, broadcast difference, ``@ lin.T``,
    norm, mean, minimum of both directions, the two minima, the means.  On the first
    ``--torch_transforms`` transforms, scaled to T by the count.
``download + NumPy``  both sets copied to the host (timed once) and the same composition in
    NumPy on the first ``--numpy_fixed`` fixed lines and one transform, scaled by lines and T.
``register_atlas``  one affine, progressive fit of ``--fit_lines`` lines a side from a .trk: wall
    time, evaluations, the share of the wall that is the launches, and the distance of the
    result from the planted transform; against the same driver on the NumPy ``evaluate`` at
    ``--numpy_fit_lines`` lines a side, its time per evaluation scaled by the table's size
    (labelled so).
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import bench_connectome as base                 # noqa: E402

DEV = base.DEV
LIN = np.diag([2.0, 2.0, 2.0])
FP64_LANE_INSTRUCTIONS_PER_S = 39.3e12
FP64_ARITHMETIC_PER_DISTANCE = 36.0
TEMP_DOUBLES = 2 ** 28                          # 2 GiB of float64 per intermediate
PLANTED = [6.0, -4.0, 3.0, 8.0, -5.0, 10.0, 1.08, 0.95, 1.03, 0.05, -0.04, 0.03]


def make_sets(n, K, D, seed=3):
    """(moving_mm, fixed_mm, planted): ``n`` lines of K stations in n / 64 curved bundles inside
    the middle of a D^3 grid of 2 mm voxels, and their planted, jittered, half reversed copy."""
    from tracktolearn_amd.bundle_register import compose
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 1.0, 200)[:, None]
    size = 2.0 * D
    lines = []
    for b in range((n + 63) // 64):
        a, e = rng.uniform(0.3 * size, 0.7 * size, (2, 3))
        bend = rng.normal(0.0, 0.06 * size, 3)
        core = a + s * (e - a) + np.sin(np.pi * s) * bend
        for _ in range(64):
            fine = core + rng.normal(0.0, 1.5, 3) + rng.normal(0.0, 0.6, 3) * (2 * s - 1)
            # K stations equidistant in arc length, as the resampler leaves a line
            cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(fine, axis=0), axis=1))])
            at = np.linspace(0.0, cum[-1], K)
            lines.append(np.stack([np.interp(at, cum, fine[:, c]) for c in range(3)], 1))
    moving = np.stack(lines[:n])
    planted = compose(PLANTED, 'affine', moving.reshape(-1, 3).mean(0))
    fixed = moving @ planted[:3, :3].T + planted[:3, 3] + rng.normal(0.0, 0.5, moving.shape)
    fixed[1::2] = fixed[1::2, ::-1]
    return moving, fixed, planted


def to_vox(mm):
    return (np.asarray(mm) / 2.0 + 0.5).astype(np.float32)     # the grid's affine is diag(2)


def torch_cost(fixed, moving, xf, lin):
    """(T,) costs, float64 on the device."""
    f, m = fixed.double(), moving.double()
    A, (B, K) = f.shape[0], m.shape[:2]
    chunk = max(1, TEMP_DOUBLES // (B * K * 3))
    lin_t = torch.from_numpy(lin).to(DEV)
    out = []
    for x in xf:
        mt = (m @ x[:, :3].T + x[:, 3])[None]
        rows, cols = [], []
        for lo in range(0, A, chunk):
            a = f[lo:lo + chunk]
            d = ((a[:, None] - mt) @ lin_t.T).norm(dim=3).mean(2)
            r = ((a.flip(1)[:, None] - mt) @ lin_t.T).norm(dim=3).mean(2)
            delta = torch.minimum(d, r)
            rows.append(delta.min(1).values)
            cols.append(delta.min(0).values)
        s = torch.cat(rows).mean() + torch.stack(cols).min(0).values.mean()
        out.append(0.25 * s * s)
    return torch.stack(out)


def numpy_evaluate(fixed, moving, lin):
    la = fixed.astype(np.float64) @ lin.T
    moving = moving.astype(np.float64)

    def run(mats):
        out = np.empty(len(mats))
        for t, x in enumerate(np.asarray(mats, np.float64)):
            lm = (moving @ x[:, :3].T + x[:, 3]) @ lin.T
            d = np.sqrt(((la[:, None] - lm[None]) ** 2).sum(-1)).mean(-1)
            r = np.sqrt(((la[:, None, ::-1] - lm[None]) ** 2).sum(-1)).mean(-1)
            delta = np.minimum(d, r)
            s = delta.min(1).mean() + delta.min(0).mean()
            out[t] = s * s / 4
        return out
    return run


def transforms(T, seed=5):
    rng = np.random.default_rng(seed)
    xf = np.zeros((T, 3, 4))
    xf[:, :, :3] = np.eye(3) + rng.normal(0.0, 0.02, (T, 3, 3))
    xf[:, :, 3] = rng.normal(0.0, 1.0, (T, 3))
    xf[0] = np.eye(4)[:3]
    return xf


def displacement(points_mm, a, b):
    p = points_mm.reshape(-1, 3)
    return float(np.sqrt((((p @ a[:3, :3].T + a[:3, 3]) - (p @ b[:3, :3].T + b[:3, 3])) ** 2)
                         .sum(1)).max())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['600,600,20,25', '4096,4096,20,25',
                                                    '4096,4096,100,25', '4096,4096,20,1'])
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch_transforms', type=int, default=2)
    ap.add_argument('--numpy_fixed', type=int, default=64)
    ap.add_argument('--fit_lines', type=int, default=4096)
    ap.add_argument('--numpy_fit_lines', type=int, default=32)
    args = ap.parse_args(argv)
    from tracktolearn_amd import _lib
    from tracktolearn_amd.bundle_recognize import BundleAtlas
    from tracktolearn_amd.bundle_register import (fixed_stations, gpu_evaluate, register,
                                                  register_atlas, to_voxel)
    lib = _lib.load()
    D = args.D
    lin_c = (C.c_double * 9)(*LIN.reshape(9))
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    shapes = []
    for shape in args.shapes:
        A, B, K, T = (int(v) for v in shape.split(','))
        moving_mm, fixed_mm, _ = make_sets(max(A, B), K, D)
        fixed = torch.from_numpy(to_vox(fixed_mm[:A])).to(DEV)
        moving = torch.from_numpy(to_vox(moving_mm[:B])).to(DEV)
        xf = torch.from_numpy(transforms(T)).to(DEV)
        row_min = torch.empty((T, A), dtype=torch.float64, device=DEV)
        col_min = torch.empty((T, B), dtype=torch.float64, device=DEV)
        cost = torch.empty(T, dtype=torch.float64, device=DEV)

        def kernel():
            _lib.check(lib.ttl_bundle_register_cost(
                fixed.data_ptr(), A, moving.data_ptr(), B, K, xf.data_ptr(), T, lin_c,
                row_min.data_ptr(), col_min.data_ptr(), cost.data_ptr(), stream),
                'ttl_bundle_register_cost')
        n_torch = min(args.torch_transforms, T)
        legs = {'kernel': kernel, 'torch': lambda: torch_cost(fixed, moving, xf[:n_torch], LIN)}
        times = {k: [] for k in legs}
        for rep in range(args.reps + 2):
            for name, fn in legs.items():
                ms, _ = base.timed(fn)
                if rep >= 2:
                    times[name].append(ms)
        t_cost = torch_cost(fixed, moving, xf[:n_torch], LIN)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_fixed, host_moving = fixed.cpu().numpy(), moving.cpu().numpy()
        download_ms = 1e3 * (time.perf_counter() - t0)
        n_numpy = min(args.numpy_fixed, A)
        t0 = time.perf_counter()
        numpy_evaluate(host_fixed[:n_numpy], host_moving, LIN)(xf[:1].cpu().numpy())
        numpy_ms = 1e3 * (time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        rate = 2.0 * A * B * K * T / (med['kernel'] * 1e-3)
        torch_all = med['torch'] * T / n_torch
        numpy_all = download_ms + numpy_ms * (A / n_numpy) * T
        shapes.append({
            'A': A, 'B': B, 'K': K, 'T': T, 'kernel_ms': round(med['kernel'], 3),
            'kernel_min_ms': round(min(times['kernel']), 3),
            'kernel_max_ms': round(max(times['kernel']), 3),
            'distances_per_s': round(rate, -6),
            'share_of_fp64_vector_rate': round(
                rate * FP64_ARITHMETIC_PER_DISTANCE / FP64_LANE_INSTRUCTIONS_PER_S, 4),
            'torch_transforms': n_torch, 'torch_ms_measured': round(med['torch'], 3),
            'torch_ms_scaled_to_T': round(torch_all, 1),
            'torch_over_kernel': round(torch_all / med['kernel'], 1),
            'cost_max_rel_difference_from_torch': float(
                ((t_cost - cost[:n_torch]).abs() / t_cost).max().item()),
            'numpy_fixed': n_numpy, 'numpy_ms_measured': round(numpy_ms, 1),
            'download_numpy_ms_scaled': round(numpy_all, 1),
            'numpy_over_kernel': round(numpy_all / med['kernel'], 1)})
    # one whole fit from a file, and the same driver on NumPy at a smaller size
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    n, K = args.fit_lines, 20
    affine = np.diag([2.0, 2.0, 2.0, 1.0])
    moving_mm, fixed_mm, planted = make_sets(n, K, D)
    atlas = BundleAtlas((D, D, D), affine, to_vox(moving_mm),
                        [f'bundle_{b}' for b in range((n + 63) // 64)],
                        label=np.arange(n) // 64, device=DEV)
    with tempfile.TemporaryDirectory() as tmp:
        trk = os.path.join(tmp, 'subject.trk')
        sio.save(Tractogram([line.astype(np.float32) for line in fixed_mm],
                            affine_to_rasmm=np.eye(4)), trk,
                 sio.create_tractogram_header(affine, (D, D, D), (2.0, 2.0, 2.0)))
        walls = []
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = register_atlas(atlas, trk, kind='affine', max_fixed=n)
            walls.append(1e3 * (time.perf_counter() - t0))
        stations = fixed_stations(trk, affine, K, max_fixed=n, device=DEV)
    at_planted = float(gpu_evaluate(stations, atlas.models_vox, LIN, DEV)(
        to_voxel(planted, affine)[None])[0])
    k = min(args.numpy_fit_lines, n)
    small_m, small_f, small_planted = make_sets(k, K, D)
    t0 = time.perf_counter()
    small = register(to_vox(small_f), to_vox(small_m), affine, kind='affine',
                     evaluate=numpy_evaluate(to_vox(small_f), to_vox(small_m), LIN))
    small_ms = 1e3 * (time.perf_counter() - t0)
    kernel_2020 = [s for s in shapes if (s['A'], s['B'], s['K'], s['T']) == (n, n, K, 25)]
    print(json.dumps({
        'object': 'bundle_register', 'grid': f'{D}^3',
        'fp64_arithmetic_per_distance': FP64_ARITHMETIC_PER_DISTANCE,
        'fp64_lane_instructions_per_s': FP64_LANE_INSTRUCTIONS_PER_S, 'shapes': shapes,
        'register_atlas': {
            'lines': n, 'K': K, 'kind': 'affine', 'wall_ms': round(walls[1], 1),
            'first_wall_ms': round(walls[0], 1), 'evaluations': fit['evaluations'],
            'ms_per_evaluation': round(walls[1] / fit['evaluations'], 3),
            'kernel_ms_at_25_transforms': kernel_2020[0]['kernel_ms'] if kernel_2020 else None,
            'cost_before': fit['cost_before'], 'cost_after': fit['cost_after'],
            'cost_at_planted': at_planted,
            'displacement_from_planted_mm': displacement(moving_mm, fit['matrix'], planted)},
        'numpy_driver': {
            'lines': k, 'wall_ms': round(small_ms, 1), 'evaluations': small['evaluations'],
            'ms_per_evaluation': round(small_ms / small['evaluations'], 1),
            'displacement_from_planted_mm': displacement(small_m, small['matrix'], small_planted),
            'wall_ms_scaled_to_the_fit_by_table_size_and_evaluations': round(
                small_ms / small['evaluations'] * (n / k) ** 2 * fit['evaluations'], 0)},
        'reps': args.reps, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
