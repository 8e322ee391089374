#!/usr/bin/env python3
"""Track density maps: the kernel against what one writes without it, and
what a map costs a tracking run.

    python benchmarks/bench_density.py [--rows 262144] [--D 96] [--zooms 1 4] [--reps 10]
                                       [--wave_slots 0] [--numpy_rows 16384]
                                       [--track_rows 4096] [--track_reps 5]
                                       [--legs kernels tracking]

One JSON line per measurement.

``density_kernels``  per zoom, on synthetic streamlines of the Tracker's lengths (27 .. 267
    points: 20 .. 200 mm at steps of 0.75 mm in 2 mm voxels; smooth random directions, starts
    uniform in the volume): HIP-event time, median of ``--reps`` after two warm-up runs, legs
    interleaved: ``ttl_tract_density`` with all four maps (count, length, dec, ends);
    with count alone; with every map but count (no set); and a torch composition of the same
    maps -- the voxel of every point, ``torch.unique`` over (row, voxel) pairs + ``bincount``
    for the count, ``index_add_`` of every segment's length and |components| at the voxel of
    its midpoint, ``bincount`` of the end voxels: float64, no walk, so a segment that crosses
    a voxel without a point in it is missed and no length is split between voxels; how far
    its count lies from the kernel's is reported.  ``download + NumPy``: the same composition
    in NumPy (``np.unique``, ``np.add.at``) after copying the points to the host, on the first
    ``--numpy_rows`` rows, scaled to all rows by the number of points.  Also the share of rows
    per status (the tiers) and the largest and mean number of voxels of a row.
``density_tracking``  ``Tracker.track`` of one seed batch as bench_connectome.py runs it,
    interleaved: without a map, with one at zoom 1, with one at zoom 4 (``--wave_slots`` sets
    the wave set of both legs too).
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
MIN_POINTS, MAX_POINTS = 27, 267
STEP_VOX = 0.375
LIN = np.diag([2.0, 2.0, 2.0])


def synthetic_rows(n, D):
    """(points (M, 3) float32, offsets (n + 1,) int64) on the device: corner-origin voxel
    coordinates of the D^3 reference grid."""
    gen = torch.Generator(device=DEV).manual_seed(n)
    lens = torch.randint(MIN_POINTS, MAX_POINTS + 1, (n,), device=DEV, generator=gen)
    start = torch.rand((n, 1, 3), device=DEV, generator=gen) * D
    chunks = []
    for lo in range(0, n, 32768):           # a chunk of padded rows at a time
        hi = min(lo + 32768, n)
        turn = torch.randn((hi - lo, MAX_POINTS, 3), device=DEV, generator=gen) * 0.15
        turn[:, 0] = torch.randn((hi - lo, 3), device=DEV, generator=gen)
        heading = torch.nn.functional.normalize(torch.cumsum(turn, 1), dim=2) * STEP_VOX
        heading[:, 0] = 0
        padded = start[lo:hi] + torch.cumsum(heading, 1)
        keep = torch.arange(MAX_POINTS, device=DEV)[None, :] < lens[lo:hi, None]
        chunks.append(padded[keep].to(torch.float32))
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(lens, 0, out=offsets[1:])
    return torch.cat(chunks).contiguous(), offsets


def composition_torch(points, offsets, dims, lin):
    """The maps without the walk, in torch: (count, length, dec, ends)."""
    dev = points.device
    n, words = offsets.shape[0] - 1, dims[0] * dims[1] * dims[2]
    p = points.double()
    dims_t, lin_t = torch.tensor(dims, device=dev), torch.from_numpy(lin).to(dev)

    def voxel(q):
        v = torch.floor(q)
        inside = ((v >= 0) & (v < dims_t)).all(1)
        v = v.long()
        return (v[:, 0] * dims[1] + v[:, 1]) * dims[2] + v[:, 2], inside
    row = torch.repeat_interleave(torch.arange(n, device=dev), offsets[1:] - offsets[:-1])
    idx, inside = voxel(p)
    pairs = torch.unique(row[inside] * words + idx[inside])
    count = torch.bincount(pairs % words, minlength=words)
    first, last = offsets[:-1], offsets[1:] - 1
    seg = torch.ones(p.shape[0], dtype=torch.bool, device=dev)
    seg[last] = False
    a, b = p[seg], p[1:][seg[:-1]]
    v = (b - a) @ lin_t.T
    mid, mid_in = voxel((a + b) * 0.5)
    length = torch.zeros(words, dtype=torch.float64, device=dev)
    length.index_add_(0, mid[mid_in], torch.sqrt((v * v).sum(1))[mid_in])
    dec = torch.zeros((words, 3), dtype=torch.float64, device=dev)
    dec.index_add_(0, mid[mid_in], v[mid_in].abs())
    end_idx, end_in = torch.cat([idx[first], idx[last]]), torch.cat([inside[first], inside[last]])
    return count, length, dec, torch.bincount(end_idx[end_in], minlength=words)


def composition_numpy(points, offsets, dims, lin):
    """The same in NumPy, on host arrays."""
    n, words = offsets.shape[0] - 1, dims[0] * dims[1] * dims[2]
    p = points.astype(np.float64)
    dims_a = np.array(dims)

    def voxel(q):
        v = np.floor(q)
        inside = ((v >= 0) & (v < dims_a)).all(1)
        v = v.astype(np.int64)
        return (v[:, 0] * dims[1] + v[:, 1]) * dims[2] + v[:, 2], inside
    row = np.repeat(np.arange(n), offsets[1:] - offsets[:-1])
    idx, inside = voxel(p)
    pairs = np.unique(row[inside] * words + idx[inside])
    count = np.bincount(pairs % words, minlength=words)
    first, last = offsets[:-1], offsets[1:] - 1
    seg = np.ones(p.shape[0], dtype=bool)
    seg[last] = False
    a, b = p[seg], p[1:][seg[:-1]]
    v = (b - a) @ lin.T
    mid, mid_in = voxel((a + b) * 0.5)
    length = np.zeros(words)
    np.add.at(length, mid[mid_in], np.sqrt((v * v).sum(1))[mid_in])
    dec = np.zeros((words, 3))
    np.add.at(dec, mid[mid_in], np.abs(v[mid_in]))
    end_idx, end_in = np.concatenate([idx[first], idx[last]]), np.concatenate([inside[first], inside[last]])
    return count, length, dec, np.bincount(end_idx[end_in], minlength=words)


def kernel_rows(n, D, zooms, reps, wave_slots, numpy_rows):
    from tracktolearn_amd import density
    ref_points, offsets = synthetic_rows(n, D)
    for zoom in zooms:
        dims, affine = density.zoom_grid((D, D, D), np.vstack([np.c_[LIN, [0, 0, 0]], [0, 0, 0, 1]]),
                                         zoom)
        lin = np.ascontiguousarray(affine[:3, :3])
        points = (ref_points * float(zoom)).contiguous()
        words = dims[0] * dims[1] * dims[2]
        maps = {'count': torch.zeros(words, dtype=torch.int32, device=DEV),
                'length_q': torch.zeros(words, dtype=torch.int64, device=DEV),
                'dec_q': torch.zeros((words, 3), dtype=torch.int64, device=DEV),
                'ends': torch.zeros(words, dtype=torch.int32, device=DEV)}
        spill = density.DEFAULT_SPILL_SLOTS
        ws = torch.zeros(density.workspace_bytes(spill, n), dtype=torch.uint8, device=DEV)

        def run(**given):            # the maps are added to: nothing is zeroed between runs
            return density.tract_density(points, offsets, dims, lin, wave_slots=wave_slots,
                                         spill_slots=spill, workspace=ws, **given)
        legs = {'all_maps': lambda: run(**maps),
                'count_only': lambda: run(count=maps['count']),
                'no_count': lambda: run(**{k: v for k, v in maps.items() if k != 'count'}),
                'torch_composition': lambda: composition_torch(points, offsets, dims, lin)}
        times = {k: [] for k in legs}
        for rep in range(reps + 2):
            for name, fn in legs.items():
                ms, _ = base.timed(fn)
                if rep >= 2:
                    times[name].append(ms)
        for t in maps.values():
            t.zero_()
        status = run(**maps)
        count = maps['count'].clone()
        t_count = composition_torch(points, offsets, dims, lin)[0]
        tiers = torch.bincount((status + 1).long(), minlength=4).cpu().tolist()
        per_row = torch.zeros(n, dtype=torch.int64, device=DEV)      # voxels per row: the torch pairs
        idx = torch.floor(points.double())
        inside = ((idx >= 0) & (idx < torch.tensor(dims, device=DEV))).all(1)
        lin_idx = ((idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]).long()
        row = torch.repeat_interleave(torch.arange(n, device=DEV), offsets[1:] - offsets[:-1])
        pairs = torch.unique(row[inside] * words + lin_idx[inside])
        per_row.index_add_(0, pairs // words, torch.ones_like(pairs))
        # download + NumPy on the first rows
        k = min(numpy_rows, n)
        m = int(offsets[k].item())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_points, host_offsets = points[:m].cpu().numpy(), offsets[:k + 1].cpu().numpy()
        composition_numpy(host_points, host_offsets, dims, lin)
        numpy_ms = 1e3 * (time.perf_counter() - t0)
        med = {k_: round(float(np.median(t)), 3) for k_, t in times.items()}
        print(json.dumps({
            'object': 'density_kernels', 'rows': n, 'points': int(points.shape[0]), 'zoom': zoom,
            'grid': 'x'.join(str(d) for d in dims), 'wave_slots': wave_slots or
            density.DEFAULT_WAVE_SLOTS, 'spill_slots': spill,
            **{k_ + '_ms': v for k_, v in med.items()},
            **{k_ + '_min_ms': round(min(t), 3) for k_, t in times.items()},
            'torch_over_kernel': round(med['torch_composition'] / med['all_maps'], 2),
            'numpy_rows': k, 'download_numpy_ms_measured': round(numpy_ms, 1),
            'download_numpy_ms_scaled_to_all_rows': round(numpy_ms * points.shape[0] / m, 1),
            'rows_not_added': tiers[0], 'rows_wave': tiers[1], 'rows_spill': tiers[2],
            'rows_left_out': tiers[3], 'voxels_per_row_points_only_max': int(per_row.max().item()),
            'voxels_per_row_points_only_mean': round(float(per_row.double().mean().item()), 1),
            'count_sum_kernel': int(count.sum().item()), 'count_sum_torch': int(t_count.sum().item()),
            'voxels_where_torch_count_differs': int((t_count != count).sum().item()),
            'reps': reps, 'device': torch.cuda.get_device_name(0)}), flush=True)
        del maps, ws, count, t_count, pairs, row, lin_idx, idx, inside, per_row
        torch.cuda.empty_cache()


def tracking_rows(D, track_rows, zooms, reps, wave_slots):
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    for N in track_rows:
        env = base.make_env(D, N)
        seeds = env.seeds.copy()
        alg = OdfTracking(env, 'det', seed=1)
        dims = tuple(int(v) for v in tuple(env.tracking_mask.data.shape)[:3])
        maps = {'plain': None}
        for zoom in zooms:
            maps[f'density_zoom{zoom}'] = DensityMap(dims, np.asarray(env.affine_vox2rasmm),
                                                     zoom=zoom, device=DEV, dec=True,
                                                     wave_slots=wave_slots)

        def run(leg):
            env.seeds = seeds.copy()            # track() shuffles in place
            options = {} if maps[leg] is None else {'density': maps[leg]}
            tracker = Tracker(alg, N, prob=0.0, min_length=20.0, max_length=200.0, **options)
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = len([item.streamline for item in tracker.track(env, TrkFile)])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), kept

        runs = {leg: [] for leg in maps}
        for rep in range(reps + 1):             # interleaved; the first round warms up
            for leg in maps:
                got = run(leg)
                if rep:
                    runs[leg].append(got)
        for leg, got in runs.items():
            ms = [g[0] for g in got]
            row = {'object': 'density_tracking', 'leg': leg, 'rows': N, 'volume': f'{D}^3 x 45',
                   'track_ms_median': round(float(np.median(ms)), 2),
                   'track_ms_min': round(min(ms), 2), 'track_ms_max': round(max(ms), 2),
                   'streamlines_kept': got[0][1], 'reps': reps,
                   'device': torch.cuda.get_device_name(0)}
            if maps[leg] is not None:
                row['wave_slots'] = wave_slots or maps[leg].totals()['wave_slots']
                row['tiers'] = maps[leg].tiers()
            print(json.dumps(row), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--zooms', type=int, nargs='*', default=[1, 4])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--wave_slots', type=int, default=0)
    ap.add_argument('--numpy_rows', type=int, default=16384)
    ap.add_argument('--track_rows', type=int, nargs='*', default=[4096])
    ap.add_argument('--track_reps', type=int, default=5)
    ap.add_argument('--legs', nargs='*', default=['kernels', 'tracking'],
                    choices=['kernels', 'tracking'])
    args = ap.parse_args(argv)
    if 'kernels' in args.legs:
        kernel_rows(args.rows, args.D, args.zooms, args.reps, args.wave_slots, args.numpy_rows)
    if 'tracking' in args.legs:
        tracking_rows(args.D, args.track_rows, args.zooms, args.track_reps, args.wave_slots)


if __name__ == '__main__':
    main()
