"""The oracle validator's phases on one GPU.

    python benchmarks/bench_oracle_validator.py [--sizes 65536 1048576] [--reps 3]

Synthetic ragged tractograms: random walks of 50-400 points at steps of
0.5-0.75 voxel in a 145^3 volume, starting in its middle 60 % (tracking
mask: the central 105^3 cube).  Per size one JSON line with the HIP-event time
of the three device phases -- ``segments`` (ttl_oracle_segments_packed, every
chunk), ``network`` (the fused TractOracle-Net on a random checkpoint) and
``coverage`` (ttl_tract_coverage) -- the host time of packing and upload, the
whole ``OracleValidator.__call__`` wall time, streamlines/s, and the achieved
GB/s of the two new kernels on their compulsory bytes (segments: the points
and offsets read once + the 127 x 3 floats written per streamline; coverage:
the points and offsets of the accepted streamlines read once + one byte per
distinct voxel written).  Best of ``--reps``.  A last line times the NumPy
restatement on 4 096 streamlines on the CPU (the padded resampler of
tests/ref_resample.py, the coverage map of tests/ref_oracle_validator.py),
labelled as such: the reference itself (dipy + scilpy) cannot run here.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tractogram(n, rng, D=145, chunk=65536):
    """n random walks (tracker voxel coordinates) as one packed float32 array
    and their lengths; the running sums in float64, chunk by chunk."""
    lens = rng.integers(50, 401, n)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    pts = np.empty((int(offsets[-1]), 3), np.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        a, b = offsets[lo], offsets[hi]
        d = rng.standard_normal((b - a, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d *= rng.uniform(0.5, 0.75, (b - a, 1))
        first = offsets[lo:hi] - a
        d[first] = rng.uniform(0.2 * D, 0.8 * D, (hi - lo, 3))   # the start points
        c = np.cumsum(d, 0)
        c -= np.repeat(c[first] - d[first], lens[lo:hi], axis=0)
        pts[a:b] = c
    return pts, lens


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[65536, 1048576])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--restatement', type=int, default=4096)
    args = ap.parse_args(argv)

    from tracktolearn_amd.datasets.utils import MRIDataVolume
    from tracktolearn_amd.experiment.oracle_validator import (
        OracleValidator, corner_voxels_from_tracker, pack, tract_coverage)
    from tracktolearn_amd.oracles.oracle import oracle_segments_packed
    from tracktolearn_amd.oracles.transformer_oracle import save_random_checkpoint
    from tracktolearn_amd.tractogram import Tractogram

    dev = torch.device('cuda:0')
    D = 145
    mask = np.zeros((D, D, D), np.uint8)
    mask[20:125, 20:125, 20:125] = 1
    aff = np.eye(4)
    env = type('Env', (), {})()
    env.tracking_mask = MRIDataVolume(mask, aff)
    env.affine_vox2rasmm = aff
    env.reference = {'affine': aff, 'shape': (D, D, D)}
    ck = os.path.join(tempfile.mkdtemp(), 'oracle.ckpt')
    save_random_checkpoint(ck, n_head=4, n_layers=4)
    val = OracleValidator(ck, dev)
    net = val.model.net
    rng = np.random.default_rng(0)

    for n in args.sizes:
        pts, lens = tractogram(n, rng, D)
        lines = np.split(pts, np.cumsum(lens)[:-1])
        tract = Tractogram(lines)
        best = None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, o = pack([s for s in lines if len(s) >= 2])
            p = corner_voxels_from_tracker(p, aff, aff)
            t1 = time.perf_counter()
            pd, od = torch.from_numpy(p).to(dev), torch.from_numpy(o).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            chunk = val.model.packed_chunk
            dirs = torch.empty((min(n, chunk), 127, 3), dtype=torch.float32, device=dev)
            scores = torch.empty(n, dtype=torch.float32, device=dev)
            seg_ms = net_ms = 0.0
            for lo in range(0, n, chunk):
                rows = min(chunk, n - lo)
                ev[0].record()
                oracle_segments_packed(pd, od[lo:lo + rows + 1], 128, dirs[:rows])
                ev[1].record()
                scores[lo:lo + rows] = net(dirs[:rows])
                ev[2].record()
                ev[2].synchronize()
                seg_ms += ev[0].elapsed_time(ev[1])
                net_ms += ev[1].elapsed_time(ev[2])
            visited = torch.zeros(D * D * D, dtype=torch.uint8, device=dev)
            ev[0].record()
            tract_coverage(pd, od, (D, D, D), scores, 0.5, visited)
            ev[3].record()
            ev[3].synchronize()
            cov_ms = ev[0].elapsed_time(ev[3])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            out = val(tract, env)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            row = {'segments_ms': seg_ms, 'network_ms': net_ms, 'coverage_ms': cov_ms,
                   'pack_host_ms': 1e3 * (t1 - t0), 'upload_ms': 1e3 * (t2 - t1),
                   'validator_call_ms': 1e3 * (t4 - t3)}
            if best is None or row['validator_call_ms'] < best[0]['validator_call_ms']:
                acc = (scores > 0.5).cpu().numpy()
                accepted_points = int(lens[acc].sum())
                n_visited = int(torch.count_nonzero(visited))
                best = (row, out, accepted_points, n_visited)
        row, out, accepted_points, n_visited = best
        M = int(lens.sum())
        seg_bytes = 12 * M + 8 * (n + 1) + 127 * 12 * n
        cov_bytes = 12 * accepted_points + 8 * (n + 1) + 4 * n + n_visited
        print(json.dumps({
            'object': 'oracle_validator', 'streamlines': n, 'points': M,
            'mean_points': M / n, **{k: round(v, 3) for k, v in row.items()},
            'streamlines_per_s': round(n / (row['validator_call_ms'] / 1e3)),
            'segments_GBps': round(seg_bytes / (row['segments_ms'] * 1e6), 1),
            'coverage_GBps': round(cov_bytes / (row['coverage_ms'] * 1e6), 1),
            'segments_compulsory_MB': round(seg_bytes / 1e6, 1),
            'coverage_compulsory_MB': round(cov_bytes / 1e6, 1),
            'result': out, 'reps': args.reps,
            'device': torch.cuda.get_device_name(0)}), flush=True)

    if args.restatement:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import ref_oracle_validator as ref
        from ref_resample import resample_streamlines
        n = args.restatement
        pts, lens = tractogram(n, rng, D)
        p, o = pack(np.split(pts + np.float32(0.5), np.cumsum(lens)[:-1]))
        L = int(lens.max())
        pad = np.zeros((n, L, 3), np.float32)
        for i in range(n):
            pad[i, :lens[i]] = p[o[i]:o[i + 1]]
        t0 = time.perf_counter()
        r = resample_streamlines(torch.from_numpy(pad), torch.from_numpy(lens), 128)
        _ = (r[:, 1:] - r[:, :-1]).numpy()
        t1 = time.perf_counter()
        ref.coverage_map(p, o, (D, D, D))
        t2 = time.perf_counter()
        print(json.dumps({
            'object': 'oracle_validator_numpy_restatement', 'streamlines': n,
            'note': 'CPU restatement (tests/), not the reference; network not included',
            'resample_ms': round(1e3 * (t1 - t0), 1),
            'coverage_ms': round(1e3 * (t2 - t1), 1)}), flush=True)


if __name__ == '__main__':
    main()
