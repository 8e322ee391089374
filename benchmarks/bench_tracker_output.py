#!/usr/bin/env python3
"""The tracker's output stage on one finished batch.

    python benchmarks/bench_tracker_output.py [--n 262144] [--reps 3] [--host-rows 4096]

bench.py's synthetic subject and scripted policy (96^3 x 45 SH, step 0.75 mm,
max_length 200 mm) tracked once to exhaustion at n_actor = 262 144; then
``Tracker.batch_output`` (.trk, min_length 20 mm) on that same batch, in this
process, wall time from call to the last yielded item, ``--reps`` times each:

  host_c0      device_output=False, compress 0      (the earlier filter + pack)
  host_c02     device_output=False, compress 0.2 mm, on the first --host-rows
               rows only; ``host_c02_extrapolated_ms`` scales its best time by
               n / host-rows -- an extrapolation, labelled as such (the full
               run is tens of minutes of per-streamline Python)
  device_c02   device_output=True,  compress 0.2 mm
  device_c0    device_output=True,  compress 0

``to_host_arrays_ms`` is the same stage up to the downloaded arrays (for
host_c02: before the host compresses), without the per-streamline Python loop
that cuts them into items and dominates the wall time of every path;
plus, per path, the peak of torch.cuda.max_memory_allocated over the stage
(above what was allocated before it), the bytes downloaded, points in / out,
and the HIP-event times of ``ttl_tract_select`` and ``ttl_tract_emit`` beside
their bytes-moved bounds (select: every kept point of every row read once +
lengths, flags, counts, mask; emit: survivors read and written + mask, scans,
counts, rows).  One JSON line.
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
import bench  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, the spec figure DESIGN.md quotes fractions of


def stage(tracker, env, fmt):
    """One output stage: (ms, items, peak bytes above the starting level)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    items = list(tracker.batch_output(env, fmt))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, items, torch.cuda.max_memory_allocated() - base


def arrays(tracker, env, lo, hi, tol):
    """The stage up to host arrays (filter [+ compression] + pack + download), without
    the per-streamline Python loop that cuts them into items: ms."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if tracker._device_output(env):
        got = tracker._batch_arrays(env, lo, hi, tol)
    else:
        got = tracker._batch_arrays_host(env, lo, hi)
    got = [g.cpu().numpy() for g in got]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_times(env, n, lo, hi, tol, reps):
    """HIP-event ms of the two kernels (best of reps) and their compulsory bytes."""
    from tracktolearn_amd import _lib
    from tracktolearn_amd.environments.env import _raw_stream
    from tracktolearn_amd.parallel import kept_lengths, tract_survivors
    lib = _lib.load()
    stream = C.c_void_p(_raw_stream(0))
    h, ln, fl = env._buf_streamlines[:n], env._buf_lengths[:n], env._buf_flags[:n]
    best = [None, None]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(reps + 1):           # the first pass warms up
        ev[0].record()
        hist, sel, mask = tract_survivors(h, ln, fl, lo, hi, tol)
        ev[1].record()
        ends = (torch.cumsum(sel[0], 0, dtype=torch.int64),
                torch.cumsum(sel[1], 0, dtype=torch.int64))
        total, k = torch.stack((ends[0][-1], ends[1][-1])).tolist()
        points = torch.empty((total, 3), dtype=torch.float32, device=h.device)
        counts = torch.empty(k, dtype=torch.int64, device=h.device)
        rows = torch.empty(k, dtype=torch.int32, device=h.device)
        ev[2].record()
        _lib.check(lib.ttl_tract_emit(
            hist.data_ptr(), hist.stride(0), n, sel[0].data_ptr(), sel[1].data_ptr(),
            ends[0].data_ptr(), ends[1].data_ptr(), mask.data_ptr(), points.data_ptr(),
            counts.data_ptr(), rows.data_ptr(), stream), 'ttl_tract_emit')
        ev[3].record()
        ev[3].synchronize()
        for j, (a, b) in enumerate(((0, 1), (2, 3))):
            ms = ev[a].elapsed_time(ev[b])
            best[j] = ms if best[j] is None else min(best[j], ms)
    kept_in = int(kept_lengths(ln, fl).sum().item())
    words = mask.shape[1]
    select_bytes = 12 * kept_in + n * (4 + 4 + 8 + 8 * words)
    emit_bytes = 24 * total + n * (8 + 16) + k * (8 * words + 12)
    return {'select_ms': round(best[0], 4), 'emit_ms': round(best[1], 4),
            'select_bound_MB': round(select_bytes / 1e6, 1),
            'emit_bound_MB': round(emit_bytes / 1e6, 1),
            'select_TBps': round(select_bytes / best[0] / 1e9, 3),
            'emit_TBps': round(emit_bytes / best[1] / 1e9, 3),
            'select_fraction_of_hbm_peak': round(select_bytes / best[0] / 1e-3 / HBM_PEAK, 3),
            'emit_fraction_of_hbm_peak': round(emit_bytes / best[1] / 1e-3 / HBM_PEAK, 3),
            'points_kept_in': kept_in, 'points_out': total, 'streamlines_out': k}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=bench.N_ACTOR)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-rows', type=int, default=4096)
    ap.add_argument('--compress', type=float, default=0.2)
    args = ap.parse_args(argv)
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile

    n, seed = args.n, 7
    subject = bench.make_subject('c2')
    env = bench.make_env(subject, 'cuda:0', 'c2')
    env.seeds = bench.shard_seeds(subject[1].data, n, 0, 1)
    t0 = time.perf_counter()
    state = env.reset(0, n)
    steps, _ = bench.track_to_exhaustion(env, state, seed, True)
    torch.cuda.synchronize()
    track_ms = (time.perf_counter() - t0) * 1e3
    assert env._n_total == n

    def tracker(compress, device_output):
        return Tracker(None, n, compress=compress, min_length=20.0,
                       max_length=bench.MAX_LENGTH, device_output=device_output)

    out = {'object': 'tracker_output', 'n_actor': n, 'row_points': int(env._buf_streamlines.shape[1]),
           'track_ms': round(track_ms, 1), 'track_steps': steps, 'compress_mm': args.compress,
           'reps': args.reps, 'device': torch.cuda.get_device_name(0)}
    sub = min(args.host_rows, n)
    runs = (('host_c0', 0.0, False, n), ('host_c02', args.compress, False, sub),
            ('device_c02', args.compress, True, n), ('device_c0', 0.0, True, n))
    kept = {}
    for name, compress, on_device, rows in runs:
        trk = tracker(compress, on_device)
        env._n_total = rows
        times, peak, items = [], 0, None
        for _ in range(args.reps if name != 'host_c02' else 1):
            ms, items, pk = stage(trk, env, TrkFile)
            times.append(round(ms, 2))
            peak = max(peak, pk)
        vox = float(np.mean(np.abs(env.affine_vox2rasmm)[np.diag_indices(4)][:3]))
        arr = [round(arrays(trk, env, 20.0 / vox, bench.MAX_LENGTH / vox, compress / vox), 2)
               for _ in range(args.reps)]
        env._n_total = n
        pts = sum(len(it.streamline) for it in items)
        kept[name] = (len(items), pts)
        # what the stage copies to the host: the points, a count per streamline, and the
        # seeds (host path, float64) or the row indices (device path, int64)
        down = 12 * pts + len(items) * (8 + (8 if on_device else 24))
        if not on_device and compress:  # the host path downloads before it compresses
            down = None
        out[name] = {'rows': rows, 'ms': times, 'best_ms': min(times),
                     'median_ms': float(np.median(times)),
                     'to_host_arrays_ms': arr, 'to_host_arrays_best_ms': min(arr),
                     'peak_alloc_MB': round(peak / 1e6, 1), 'streamlines_out': len(items),
                     'points_out': pts, 'downloaded_MB': None if down is None else round(down / 1e6, 1)}
        del items
    out['host_c02']['downloaded_MB'] = round(
        out['host_c0']['downloaded_MB'] * sub / n, 1) if sub < n else out['host_c0']['downloaded_MB']
    out['host_c02_extrapolated_ms'] = round(out['host_c02']['best_ms'] * n / sub, 1)
    out['host_c02_note'] = (f'measured on the first {sub} rows; the extrapolated figure scales it '
                            f'by {n}/{sub} and is not a measurement')
    out['host_c02_ms_per_streamline_out'] = round(
        out['host_c02']['best_ms'] / max(out['host_c02']['streamlines_out'], 1), 3)
    out['kept_fraction'] = round(kept['device_c02'][1] / max(kept['device_c0'][1], 1), 4)
    out['speedup_c02_extrapolated'] = round(
        out['host_c02_extrapolated_ms'] / out['device_c02']['best_ms'], 1)
    out['device_c0_over_host_c0'] = round(out['device_c0']['best_ms'] / out['host_c0']['best_ms'], 3)
    out['device_c0_over_host_c0_to_host_arrays'] = round(
        out['device_c0']['to_host_arrays_best_ms'] / out['host_c0']['to_host_arrays_best_ms'], 3)

    affine = env.affine_vox2rasmm
    vox = float(np.mean(np.abs(affine)[np.diag_indices(4)][:3]))
    lo, hi = 20.0 / vox, bench.MAX_LENGTH / vox
    out['kernels_c02'] = kernel_times(env, n, lo, hi, args.compress / vox, args.reps)
    out['kernels_c0'] = kernel_times(env, n, lo, hi, 0.0, args.reps)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
