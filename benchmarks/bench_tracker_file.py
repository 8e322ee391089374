#!/usr/bin/env python3
"""From a finished batch to a closed tractogram file.

    python benchmarks/bench_tracker_file.py [--n 262144] [--rounds 5] [--dir DIR]

bench_tracker_output.py's batch (bench.py's synthetic subject and scripted
policy, tracked once to exhaustion at n_actor = 262 144), then, for .trk with
seeds and .tck, without compression and at --compress mm, ``--rounds`` rounds
of two paths in this process, alternating, wall time from the call to the file
closed:

  save      ``io.streamlines.save`` over ``Tracker.batch_output``'s items
            (what ``Tracker.track`` + ``save`` do with the batch)
  direct    ``Tracker.batch_body`` + ``PackedWriter`` (what
            ``Tracker.track_to_file`` does with it)

Files go to --dir (default: the system's temporary directory; named in the
output, with its filesystem type when /proc/mounts tells).  After the last
round the two files are compared: length, header bytes, the share of 4-byte
words that differ.  ``kernels`` gives the HIP-event times (best of rounds) of
``ttl_tract_emit`` and ``ttl_tract_emit_file`` on the same survivors beside
the bytes each must move.  One JSON line.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def filesystem_of(path):
    best, kind = '', None
    try:
        with open('/proc/mounts') as f:
            for line in f:
                _, mount, fstype = line.split()[:3]
                if os.path.realpath(path).startswith(mount) and len(mount) > len(best):
                    best, kind = mount, fstype
    except OSError:
        pass
    return kind


def save_path(tracker, env, fmt, path, header):
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import LazyTractogram
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tractogram = LazyTractogram.from_data_func(lambda: tracker.batch_output(env, fmt))
    tractogram.affine_to_rasmm = env.affine_vox2rasmm
    count = sio.save(tractogram, path, header=header)
    return (time.perf_counter() - t0) * 1e3, count


def direct_path(tracker, env, fmt, path, header):
    from tracktolearn_amd.io import streamlines as sio
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    desc = tracker.file_desc(env, fmt, header)
    writer = sio.PackedWriter(path, fmt.EXT, header, desc.n_props)
    words, k = tracker.batch_body(env, desc)
    writer.append(words, k)
    count = writer.close()
    return (time.perf_counter() - t0) * 1e3, count


def compare(a_path, b_path, header_bytes):
    a, b = np.fromfile(a_path, np.uint8), np.fromfile(b_path, np.uint8)
    out = {'bytes': int(len(b)), 'same_length': len(a) == len(b)}
    if len(a) == len(b):
        out['same_header'] = bool(np.array_equal(a[:header_bytes], b[:header_bytes]))
        wa, wb = a[header_bytes:].view('<u4'), b[header_bytes:].view('<u4')
        out['words'] = int(len(wa))
        out['words_differing'] = int((wa != wb).sum())
    return out


def kernel_times(env, n, lo, hi, tol, desc, rounds):
    """HIP-event ms of the two packs (best of rounds) and the bytes each must move."""
    from tracktolearn_amd import _lib
    from tracktolearn_amd.environments.env import _raw_stream
    from tracktolearn_amd.parallel import tract_survivors
    lib = _lib.load()
    stream = C.c_void_p(_raw_stream(0))
    h, ln, fl = env._buf_streamlines[:n], env._buf_lengths[:n], env._buf_flags[:n]
    dev = h.device
    seeds = torch.from_numpy(np.ascontiguousarray(
        np.asarray(env.initial_points)[:n], dtype=np.float64)).to(dev)
    hist, sel, mask = tract_survivors(h, ln, fl, lo, hi, tol)
    ends = (torch.cumsum(sel[0], 0, dtype=torch.int64), torch.cumsum(sel[1], 0, dtype=torch.int64))
    total, k = torch.stack((ends[0][-1], ends[1][-1])).tolist()
    c_desc = desc.to_c()
    size = lib.ttl_tract_file_words(c_desc.format, c_desc.n_props, k, total)
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    rows = torch.empty(k, dtype=torch.int32, device=dev)
    words = torch.empty(size, dtype=torch.int32, device=dev)
    best = [None, None]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(rounds + 1):         # the first pass warms up
        ev[0].record()
        _lib.check(lib.ttl_tract_emit(
            hist.data_ptr(), hist.stride(0), n, sel[0].data_ptr(), sel[1].data_ptr(),
            ends[0].data_ptr(), ends[1].data_ptr(), mask.data_ptr(), points.data_ptr(),
            counts.data_ptr(), rows.data_ptr(), stream), 'ttl_tract_emit')
        ev[1].record()
        _lib.check(lib.ttl_tract_emit_file(
            hist.data_ptr(), hist.stride(0), n, sel[0].data_ptr(), sel[1].data_ptr(),
            ends[0].data_ptr(), ends[1].data_ptr(), mask.data_ptr(), seeds.data_ptr(),
            C.byref(c_desc), words.data_ptr(), stream), 'ttl_tract_emit_file')
        ev[2].record()
        ev[2].synchronize()
        for j in range(2):
            ms = ev[j].elapsed_time(ev[j + 1])
            best[j] = ms if best[j] is None else min(best[j], ms)
    nw = mask.shape[1]
    # both: survivors read, counts / accepted / two scan ends per row, the mask of accepted rows
    common = 12 * total + n * (8 + 16) + k * 8 * nw
    emit_bytes = common + 12 * total + k * 12
    file_bytes = common + 4 * size + (24 * k if c_desc.n_props else 0)
    return {'emit_ms': round(best[0], 4), 'emit_file_ms': round(best[1], 4),
            'emit_MB': round(emit_bytes / 1e6, 1), 'emit_file_MB': round(file_bytes / 1e6, 1),
            'emit_TBps': round(emit_bytes / best[0] / 1e9, 3),
            'emit_file_TBps': round(file_bytes / best[1] / 1e9, 3),
            'streamlines_out': k, 'points_out': total, 'body_words': int(size)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=bench.N_ACTOR)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--compress', type=float, default=0.2)
    ap.add_argument('--dir', default=None)
    args = ap.parse_args(argv)
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tracking.tracker import TckFile, Tracker, TrkFile

    n, seed = args.n, 7
    subject = bench.make_subject('c2')
    env = bench.make_env(subject, 'cuda:0', 'c2')
    env.seeds = bench.shard_seeds(subject[1].data, n, 0, 1)
    state = env.reset(0, n)
    steps, _ = bench.track_to_exhaustion(env, state, seed, True)
    torch.cuda.synchronize()
    assert env._n_total == n
    affine = np.asarray(env.affine_vox2rasmm, dtype=np.float64)
    vox = float(np.mean(np.abs(affine)[np.diag_indices(4)][:3]))
    header = sio.create_tractogram_header(affine, subject[1].data.shape[:3], (vox,) * 3)

    out = {'object': 'tracker_file', 'n_actor': n, 'row_points': int(env._buf_streamlines.shape[1]),
           'track_steps': steps, 'compress_mm': args.compress, 'rounds': args.rounds,
           'affine_is_axis_aligned': bool(np.count_nonzero(affine[:3, :3]) == 3),
           'device': torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        out['dir'] = os.path.dirname(tmp)
        out['filesystem'] = filesystem_of(tmp)
        for fmt in (TrkFile, TckFile):
            for compress in (0.0, args.compress):
                tracker = Tracker(None, n, compress=compress, min_length=20.0,
                                  max_length=bench.MAX_LENGTH, save_seeds=True)
                paths = [os.path.join(tmp, name + fmt.EXT) for name in ('save', 'direct')]
                ms = {'save': [], 'direct': []}
                for _ in range(args.rounds):
                    a, count_a = save_path(tracker, env, fmt, paths[0], header)
                    b, count_b = direct_path(tracker, env, fmt, paths[1], header)
                    assert count_a == count_b
                    ms['save'].append(round(a, 2))
                    ms['direct'].append(round(b, 2))
                head = sio.TRK_HEADER_SIZE if fmt is TrkFile else len(sio._tck_header(0))
                name = '{}_c{}'.format(fmt.EXT[1:], ('%g' % compress).replace('.', ''))
                out[name] = {
                    'save_ms': ms['save'], 'direct_ms': ms['direct'], 'streamlines': count_b,
                    'direct_below_save_in_every_round': all(
                        b < a for a, b in zip(ms['save'], ms['direct'])),
                    'best_save_over_best_direct': round(min(ms['save']) / min(ms['direct']), 1),
                    'files': compare(paths[0], paths[1], head),
                    'kernels': kernel_times(env, n, 20.0 / vox, bench.MAX_LENGTH / vox,
                                            compress / vox, tracker.file_desc(env, fmt, header),
                                            args.rounds)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
