"""The Tractometer validator's phases on one GPU.

    python benchmarks/bench_tractometer.py [--sizes 65536 1048576] [--reps 3]

The tractograms of benchmarks/bench_oracle_validator.py (random walks of 50-400
points at steps of 0.5-0.75 voxel in a 145^3 volume) against a synthetic
scoring set of 21 bundles: head and tail ROIs are cubes of edge 14 about 12
voxels apart, a third of the bundles have an all_mask, a third an any_mask,
all have a length limit, a third an angle, all a gt_mask.  Per size one JSON
line with the HIP-event time of ``upload`` (points and offsets, pageable host
memory), ``classify`` (ttl_tractometer_classify), ``overlap``
(ttl_tractometer_overlap: memset, mark, count) and ``invalid``
(ttl_tractometer_invalid against the 42 head / tail ROIs of the 21 bundles, each
bundle's own pair valid), the host time of packing, the share of rows that
leave after the end test, the share that reach the walk's result with a bundle,
the share that reach the invalid kernel's end test (no bundle) and that leave
it with a pair, and the metrics (compute_ic).  ``device_ms``, which picks the
best repetition, is classify + overlap as before.  Best of ``--reps``.  A last
line times the NumPy definition (tests/ref_tractometer.py) on a subsample on
the CPU and scales it to the first size, labelled as such: the reference itself
(scilpy) cannot run here.
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

N_BUNDLES = 21


def scoring_set(rng, D=145):
    """21 bundle dicts in the layout of tests/ref_tractometer.py."""
    import ref_tractometer as ref

    def cube(centre, half):
        m = np.zeros((D, D, D), bool)
        lo = np.maximum(np.round(centre - half).astype(int), 0)
        hi = np.minimum(np.round(centre + half).astype(int), D)
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        return m

    bundles = []
    for b in range(N_BUNDLES):
        c0 = rng.uniform(0.3 * D, 0.7 * D, 3)
        step = rng.standard_normal(3)
        c1 = c0 + 12.0 * step / np.linalg.norm(step)
        mid = 0.5 * (c0 + c1)
        bundles.append(ref.bundle(
            cube(c0, 7), cube(c1, 7), gt=cube(mid, 12),
            all=cube(mid, 30) if b % 3 == 0 else None,
            any=cube(mid, 4) if b % 3 == 1 else None,
            length=[20.0, 200.0], angle=330.0 if b % 3 == 2 else None))
    return bundles


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[65536, 1048576])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--definition', type=int, default=2048,
                    help='rows of the NumPy definition on the CPU (0: skip)')
    args = ap.parse_args(argv)

    from bench_oracle_validator import tractogram
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels_from_tracker, pack
    from tracktolearn_amd.experiment.tractometer_validator import (ScoringData, Segmentation,
                                                                   classify, invalid,
                                                                   limits_table, metrics, overlap)

    dev = torch.device('cuda:0')
    D = 145
    aff = np.eye(4)
    rng = np.random.default_rng(0)
    bundles = scoring_set(rng, D)
    cols = {k: [b[k] for b in bundles] for k in bundles[0]}
    # the ROIs: every head, then every tail; bundle b joins b and N_BUNDLES + b
    R = 2 * N_BUNDLES
    valid = np.eye(R, dtype=bool)
    for b in range(N_BUNDLES):
        valid[b, N_BUNDLES + b] = valid[N_BUNDLES + b, b] = True
    t0 = time.perf_counter()
    data = ScoringData((D, D, D), cols['head'], cols['tail'], cols['all'], cols['any'],
                       cols['gt'], limits_table(cols['length'], cols['angle'], cols['dir'],
                                                cols['absdir']), dev,
                       roi_masks=cols['head'] + cols['tail'], valid=valid)
    torch.cuda.synchronize()
    setup_ms = 1e3 * (time.perf_counter() - t0)
    lin = aff[:3, :3]
    first = None

    for n in args.sizes:
        pts, lens = tractogram(n, rng, D)
        lines = np.split(pts, np.cumsum(lens)[:-1])
        best = None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, o = pack(lines)
            p = corner_voxels_from_tracker(p, aff, aff)
            t1 = time.perf_counter()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            visited = torch.zeros(D * D * D, dtype=torch.int64, device=dev)
            ev[0].record()
            pd, od = torch.from_numpy(p).to(dev), torch.from_numpy(o).to(dev)
            ev[1].record()
            bundle, connected = classify(pd, od, data, lin)
            ev[2].record()
            counts, _ = overlap(pd, od, bundle, data, visited)
            ev[3].record()
            pair = invalid(pd, od, bundle, data)
            ev[4].record()
            ev[4].synchronize()
            row = {'pack_host_ms': 1e3 * (t1 - t0), 'upload_ms': ev[0].elapsed_time(ev[1]),
                   'classify_ms': ev[1].elapsed_time(ev[2]),
                   'overlap_ms': ev[2].elapsed_time(ev[3]),
                   'invalid_ms': ev[3].elapsed_time(ev[4])}
            row['device_ms'] = row['classify_ms'] + row['overlap_ms']
            if best is None or row['device_ms'] < best[0]['device_ms']:
                best = (row, Segmentation(data, bundle, connected, counts, pair).summary(),
                        int((connected == 0).sum()))
        row, s, unconnected = best
        M = int(lens.sum())
        result = metrics(n, s.per_bundle, s.counts, data.gt_sizes, invalid=s.invalid)
        print(json.dumps({
            'object': 'tractometer_validator', 'streamlines': n, 'points': M,
            'bundles': N_BUNDLES, 'rois': R, 'scoring_setup_ms': round(setup_ms, 1),
            **{k: round(v, 3) for k, v in row.items()},
            'left_after_end_test': round(unconnected / n, 4),
            'with_a_bundle': round(int(s.per_bundle.sum()) / n, 4),
            'reach_invalid': round(1 - int(s.per_bundle.sum()) / n, 4),
            'with_a_pair': round(int(s.invalid[0]) / n, 4),
            'result': result, 'reps': args.reps,
            'device': torch.cuda.get_device_name(0)}), flush=True)
        if first is None:
            first = (n, p, o)

    if args.definition and first is not None:
        import ref_tractometer as ref
        n, p, o = first
        k = min(args.definition, n)
        sub_o = o[:k + 1]
        t0 = time.perf_counter()
        got = ref.score(p[:sub_o[-1]], sub_o, (D, D, D), bundles, lin)
        ms = 1e3 * (time.perf_counter() - t0)
        print(json.dumps({
            'object': 'tractometer_numpy_definition', 'streamlines': k,
            'note': 'CPU definition (tests/ref_tractometer.py), not the reference (scilpy)',
            'definition_ms': round(ms, 1),
            'scaled_to': n, 'scaled_ms': round(ms * n / k, 1),
            'with_a_bundle': round(float((got['bundle'] >= 0).mean()), 4)}), flush=True)


if __name__ == '__main__':
    main()
