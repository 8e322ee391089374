#!/usr/bin/env python3
"""Bundle recognition: ttl_bundle_recognize alone, against a torch
composition and against download + NumPy, and ``BundleAtlas.recognize`` on a file.

    python benchmarks/bench_bundle_recognize.py [--rows 262144] [--models 21 256 2048]
                                                [--K 20 100] [--D 96] [--reps 5]
                                                [--torch_rows 32768] [--numpy_rows 128]
                                                [--file_rows 32768]

One JSON line.  Synthetic streamlines of the Tracker's lengths (bench_density.py's rows: 27 ..
267 points); the models are random straight lines of the grid, 4 to a label.  HIP-event time,
median of ``--reps`` after two warm-up runs, per shape (M, K):

``kernel``  ``ttl_bundle_recognize`` alone with labels and runner_up; ms, distances per second
    (rows x M x K x 2) and their share of the vector float64 rate.  The microarchitecture guide
    lists the vector FP32 peak, 157.3 TFLOP/s = 78.6e12 lane-instructions per second; a float64
    instruction issues at half that rate (AMD's 78.6 TFLOP/s vector FP64), 39.3e12.  The inner loop
    is, in the disassembly (--save-temps, the loop behind the second barrier), 194 VALU
    instructions per model station for 4 distances: 144 float64 arithmetic (56 mul, 48 add, 28
    fma of the square root's refinement, 8 ldexp, 4 rsq), 15 float32 -> float64 conversions, 8
    compares, 27 integer or select.  share = distances/s x 36 / 39.3e12: the float64 arithmetic
    alone, the least time the definition's operations could take with this square root.
``torch``  the float64 composition on the device, chunked over rows so that the (rows, M, K, 3)
    intermediate stays under 2 GiB: resampling as bench_bundle_profile.py, broadcast difference,
    ``@ lin.T``, norm, mean, minimum of both directions, argmin.  On the first ``--torch_rows``
    rows, scaled to all rows by the row count; rows on which its winner differs from the kernel's
    are counted.
``download + NumPy``  the points copied to the host (all of them, timed once) and the same
    composition per streamline in NumPy on the first ``--numpy_rows`` rows, scaled by the rows.
``recognize_file``  ``BundleAtlas.recognize`` on a .trk of the first ``--file_rows`` rows at the
    middle shape (M = 256, K = 20 when they are among the shapes): wall time from the file name to
    the host arrays, and the share of it that is the kernel.
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

import bench_bundle_profile as profile_bench    # noqa: E402
import bench_connectome as base                 # noqa: E402
import bench_density as rows_of                 # noqa: E402

DEV = base.DEV
LIN = np.diag([2.0, 2.0, 2.0])
FP64_LANE_INSTRUCTIONS_PER_S = 39.3e12
FP64_ARITHMETIC_PER_DISTANCE = 36.0
VALU_PER_DISTANCE = 48.5
TEMP_DOUBLES = 2 ** 28                          # 2 GiB of float64 per intermediate


def make_models(M, K, D, gen):
    ends = torch.rand((M, 2, 3), device=DEV, generator=gen) * D
    t = torch.linspace(0.0, 1.0, K, device=DEV)[None, :, None]
    models = (ends[:, :1] + t * (ends[:, 1:] - ends[:, :1])).float().contiguous()
    label = (torch.arange(M, device=DEV) // 4).to(torch.int32).contiguous()
    return models, label


def torch_recognize(points, offsets, n, models, lin):
    """(best, mdf) of the first n rows, float64 on the device."""
    M, K = models.shape[:2]
    chunk = max(1, min(16384, TEMP_DOUBLES // (M * K * 3)))
    m, lin_t = models.double()[None], torch.from_numpy(lin).to(DEV)
    best, mdf = [], []
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        r = profile_bench.resample_padded(points, offsets, lo, hi, K)
        d = ((r[:, None] - m) @ lin_t.T).norm(dim=3).mean(2)
        f = ((r.flip(1)[:, None] - m) @ lin_t.T).norm(dim=3).mean(2)
        low, arg = torch.minimum(d, f).min(1)
        best.append(arg)
        mdf.append(low)
    return torch.cat(best), torch.cat(mdf)


def numpy_recognize(points, offsets, models, lin):
    K = models.shape[1]
    t = np.linspace(0.0, 1.0, K)
    best = np.empty(len(offsets) - 1, np.int64)
    for s in range(len(offsets) - 1):
        p = points[offsets[s]:offsets[s + 1]].astype(np.float64)
        cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(p, axis=0), axis=1))])
        r = np.stack([np.interp(t * cum[-1], cum, p[:, k]) for k in range(3)], 1)
        d = np.linalg.norm((r[None] - models) @ lin.T, axis=2).mean(1)
        f = np.linalg.norm((r[::-1][None] - models) @ lin.T, axis=2).mean(1)
        best[s] = np.argmin(np.minimum(d, f))
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--models', type=int, nargs='+', default=[21, 256, 2048])
    ap.add_argument('--K', type=int, nargs='+', default=[20, 100])
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch_rows', type=int, default=32768)
    ap.add_argument('--numpy_rows', type=int, default=128)
    ap.add_argument('--file_rows', type=int, default=32768)
    args = ap.parse_args(argv)
    from tracktolearn_amd import _lib
    from tracktolearn_amd.bundle_recognize import BundleAtlas
    lib = _lib.load()
    n, D = args.rows, args.D
    points, offsets = rows_of.synthetic_rows(n, D)
    gen = torch.Generator(device=DEV).manual_seed(11)
    lin_c = (C.c_double * 9)(*LIN.reshape(9))
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    best = torch.zeros(n, dtype=torch.int32, device=DEV)
    flip = torch.zeros(n, dtype=torch.int32, device=DEV)
    mdf = torch.zeros(n, dtype=torch.float64, device=DEV)
    second = torch.zeros(n, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_points, host_offsets = points.cpu().numpy(), offsets.cpu().numpy()
    download_ms = 1e3 * (time.perf_counter() - t0)
    n_torch, n_numpy = min(args.torch_rows, n), min(args.numpy_rows, n)
    shapes = []
    for K in args.K:
        for M in args.models:
            models, label = make_models(M, K, D, gen)

            def kernel():
                _lib.check(lib.ttl_bundle_recognize(
                    points.data_ptr(), offsets.data_ptr(), n, models.data_ptr(), label.data_ptr(),
                    M, K, lin_c, best.data_ptr(), flip.data_ptr(), mdf.data_ptr(),
                    second.data_ptr(), stream), 'ttl_bundle_recognize')
            legs = {'kernel': kernel,
                    'torch': lambda: torch_recognize(points, offsets, n_torch, models, LIN)}
            times = {k: [] for k in legs}
            for rep in range(args.reps + 2):
                for name, fn in legs.items():
                    ms, _ = base.timed(fn)
                    if rep >= 2:
                        times[name].append(ms)
            t_best, t_mdf = torch_recognize(points, offsets, n_torch, models, LIN)
            t0 = time.perf_counter()
            numpy_recognize(host_points, host_offsets[:n_numpy + 1], models.double().cpu().numpy(),
                            LIN)
            numpy_ms = 1e3 * (time.perf_counter() - t0)
            med = {k: float(np.median(v)) for k, v in times.items()}
            distances = 2.0 * n * M * K
            rate = distances / (med['kernel'] * 1e-3)
            torch_all = med['torch'] * n / n_torch
            numpy_all = download_ms + numpy_ms * n / n_numpy
            shapes.append({
                'M': M, 'K': K, 'kernel_ms': round(med['kernel'], 3),
                'kernel_min_ms': round(min(times['kernel']), 3),
                'kernel_max_ms': round(max(times['kernel']), 3),
                'distances_per_s': round(rate, -6),
                'share_of_fp64_vector_rate': round(
                    rate * FP64_ARITHMETIC_PER_DISTANCE / FP64_LANE_INSTRUCTIONS_PER_S, 4),
                'torch_rows': n_torch, 'torch_ms_measured': round(med['torch'], 3),
                'torch_ms_scaled_to_all_rows': round(torch_all, 1),
                'torch_over_kernel': round(torch_all / med['kernel'], 1),
                'winners_differing_from_torch': int(
                    (t_best != best[:n_torch].long()).sum().item()),
                'mdf_max_abs_difference_from_torch_mm': float(
                    (t_mdf - mdf[:n_torch]).abs().max().item()),
                'numpy_rows': n_numpy, 'numpy_ms_measured': round(numpy_ms, 1),
                'download_numpy_ms_scaled_to_all_rows': round(numpy_all, 1),
                'numpy_over_kernel': round(numpy_all / med['kernel'], 1)})
    # BundleAtlas.recognize on a file, at the middle shape
    M = 256 if 256 in args.models else args.models[len(args.models) // 2]
    K = 20 if 20 in args.K else args.K[0]
    models, label = make_models(M, K, D, gen)
    k = min(args.file_rows, n)
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    affine = np.diag([2.0, 2.0, 2.0, 1.0])
    lines = [((host_points[host_offsets[s]:host_offsets[s + 1]] - 0.5) * 2.0).astype(np.float32)
             for s in range(k)]
    atlas = BundleAtlas((D, D, D), affine, models.cpu().numpy(),
                        [f'bundle_{b}' for b in range((M + 3) // 4)],
                        label=label.cpu().numpy(), device=DEV)
    with tempfile.TemporaryDirectory() as tmp:
        trk = os.path.join(tmp, 'rows.trk')
        sio.save(Tractogram(lines, affine_to_rasmm=np.eye(4)), trk,
                 sio.create_tractogram_header(affine, (D, D, D), (2.0, 2.0, 2.0)))
        file_bytes = os.path.getsize(trk)
        walls = []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = atlas.recognize(trk)
            walls.append(1e3 * (time.perf_counter() - t0))
    sub_off = offsets[:k + 1].contiguous()
    sub_times = []
    for rep in range(args.reps + 2):
        ms, _ = base.timed(lambda: _lib.check(lib.ttl_bundle_recognize(
            points.data_ptr(), sub_off.data_ptr(), k, models.data_ptr(), label.data_ptr(), M, K,
            lin_c, best.data_ptr(), flip.data_ptr(), mdf.data_ptr(), second.data_ptr(), stream),
            'ttl_bundle_recognize'))
        if rep >= 2:
            sub_times.append(ms)
    wall = float(np.median(walls[1:]))
    print(json.dumps({
        'object': 'bundle_recognize', 'rows': n, 'points': int(points.shape[0]), 'grid': f'{D}^3',
        'fp64_arithmetic_per_distance': FP64_ARITHMETIC_PER_DISTANCE,
        'valu_per_distance': VALU_PER_DISTANCE,
        'fp64_lane_instructions_per_s': FP64_LANE_INSTRUCTIONS_PER_S,
        'download_all_points_ms': round(download_ms, 1), 'shapes': shapes,
        'recognize_file': {'rows': k, 'M': M, 'K': K, 'file_bytes': file_bytes,
                           'wall_ms': round(wall, 1), 'first_wall_ms': round(walls[0], 1),
                           'kernel_ms': round(float(np.median(sub_times)), 3),
                           'kernel_share_of_wall': round(float(np.median(sub_times)) / wall, 4),
                           'recognised': int((got['bundle'] >= 0).sum())},
        'reps': args.reps, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
