#!/usr/bin/env python3
"""Bundle profiles: the two kernels each alone, with and without their
register runs, against what one writes without them.

    python benchmarks/bench_bundle_profile.py [--rows 262144] [--bundles 21] [--K 100] [--D 96]
                                              [--reps 10] [--numpy_rows 4096]
                                              [--variant benchmarks/micro/_exp/libttl_hip_noruns.so]

One JSON line.  Synthetic streamlines of the Tracker's lengths (bench_density.py's rows: 27 ..
267 points) in ``--bundles`` random bundles, a random model line per bundle, a random volume.
HIP-event time, median of ``--reps`` after two warm-up runs, legs interleaved:

``orient`` / ``profile``  ``ttl_bundle_orient`` and ``ttl_bundle_profile`` each alone, on the rows
    sorted by bundle (what ``BundleProfiles.fit`` passes) and on the rows as they arrive; ms, and
    the bytes of the point array per second against the 8 TB/s peak (a pass reads every point
    once, plus the prefix replays of the resampler).
``*_no_runs``  the same kernels from the variant library, built with the benchmark's switch
    ``-DTTL_BUNDLE_PROFILE_NO_RUNS`` (benchmarks/micro/build_variant.py noruns ...): every row
    flushes its sums with atomics, the naive form.  Skipped when the variant is not built.
``torch_*``  a torch composition on the device: rows padded in chunks, cumulative lengths,
    ``searchsorted``, linear interpolation, distances, ``index_add_`` into float64 sums; the
    profile gathers the eight corners itself.  Not the kernels' bits; how far its sums lie from
    theirs is reported.
``download + NumPy``  the host loop a dipy user writes (per streamline: ``np.interp`` over the
    cumulative length, distances, a flip, sums) after copying the points to the host, on the
    first ``--numpy_rows`` rows, scaled to all rows by the number of points.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import bench_connectome as base     # noqa: E402
import bench_density as rows_of     # noqa: E402

DEV = base.DEV
LIN = np.diag([2.0, 2.0, 2.0])
PEAK = 8e12


def entry_points(path):
    """(ttl_bundle_orient, ttl_bundle_profile) of the library at ``path``."""
    from tracktolearn_amd import _lib
    lib = C.CDLL(path)
    out = []
    for name in ('ttl_bundle_orient', 'ttl_bundle_profile'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
        out.append(fn)
    return out


def resample_padded(points, offsets, lo, hi, K):
    """(hi - lo, K, 3) float64: rows lo .. hi resampled at equal arc length, in torch."""
    lens = offsets[lo + 1:hi + 1] - offsets[lo:hi]
    longest = int(lens.max().item())
    col = torch.arange(longest, device=DEV)
    src = (offsets[lo:hi, None] + torch.minimum(col[None, :], lens[:, None] - 1))
    p = points[src].double()                                # the last point repeated
    seg = (p[:, 1:] - p[:, :-1]).norm(dim=2)
    cum = torch.nn.functional.pad(torch.cumsum(seg, 1), (1, 0))
    target = cum[:, -1:] * torch.linspace(0.0, 1.0, K, device=DEV, dtype=torch.float64)[None, :]
    j = (torch.searchsorted(cum, target, right=True) - 1).clamp(0, longest - 2)
    c0, c1 = cum.gather(1, j), cum.gather(1, j + 1)
    r = torch.where(c1 > c0, (target - c0) / (c1 - c0), torch.zeros_like(c0)).clamp(0.0, 1.0)
    a = p.gather(1, j[:, :, None].expand(-1, -1, 3))
    b = p.gather(1, (j + 1)[:, :, None].expand(-1, -1, 3))
    return a + r[:, :, None] * (b - a)


def torch_orient(points, offsets, bundle, B, K, model, lin, chunk=16384):
    n = bundle.shape[0]
    sums = torch.zeros((B, K, 3), dtype=torch.float64, device=DEV)
    count = torch.zeros(B, dtype=torch.float64, device=DEV)
    flips = []
    m, lin_t = model.double(), torch.from_numpy(lin).to(DEV)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        r = resample_padded(points, offsets, lo, hi, K)
        b = bundle[lo:hi].long()
        d = ((r - m[b]) @ lin_t.T).norm(dim=2).mean(1)
        f = ((r.flip(1) - m[b]) @ lin_t.T).norm(dim=2).mean(1)
        flip = f < d
        flips.append(flip)
        sums.index_add_(0, b, torch.where(flip[:, None, None], r.flip(1), r))
        count.index_add_(0, b, torch.ones_like(d))
    return torch.cat(flips), sums, count


def torch_profile(points, offsets, bundle, flip, B, K, volume, chunk=16384):
    n = bundle.shape[0]
    D = volume.shape
    flat = volume.reshape(-1).double()
    sums = torch.zeros((3, B * K), dtype=torch.float64, device=DEV)
    station = torch.arange(K, device=DEV)
    hi_idx = torch.tensor(D, device=DEV) - 1
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        r = resample_padded(points, offsets, lo, hi, K)
        r = torch.where(flip[lo:hi, None, None] != 0, r.flip(1), r)
        inside = ((r >= 0) & (r <= torch.tensor(D, device=DEV))).all(2)
        u = r - 0.5
        i = torch.floor(u)
        f = u - i
        i0 = torch.minimum(i.long().clamp(min=0), hi_idx)
        i1 = torch.minimum((i.long() + 1).clamp(min=0), hi_idx)
        v = torch.zeros(r.shape[:2], dtype=torch.float64, device=DEV)
        for corner in range(8):
            pick = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
            idx = [i1[..., k] if pick[k] else i0[..., k] for k in range(3)]
            w = 1.0
            for k in range(3):
                w = w * (f[..., k] if pick[k] else 1.0 - f[..., k])
            v += w * flat[(idx[0] * D[1] + idx[1]) * D[2] + idx[2]]
        cell = (bundle[lo:hi, None].long() * K + station[None, :])[inside]
        sums[0].index_add_(0, cell, v[inside])
        sums[1].index_add_(0, cell, (v * v)[inside])
        sums[2].index_add_(0, cell, torch.ones_like(v[inside]))
    return sums.reshape(3, B, K)


def numpy_loop(points, offsets, bundle, B, K, model, lin, volume):
    """The host loop: per streamline np.interp over the cumulative length, the two
    distances, the flip, the sums, nearest-voxel profile aside (trilinear by hand)."""
    sums = np.zeros((B, K, 3))
    prof = np.zeros((3, B, K))
    dims = np.array(volume.shape)
    t = np.linspace(0.0, 1.0, K)
    for s in range(len(offsets) - 1):
        p = points[offsets[s]:offsets[s + 1]].astype(np.float64)
        cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(p, axis=0), axis=1))])
        r = np.stack([np.interp(t * cum[-1], cum, p[:, k]) for k in range(3)], 1)
        b = bundle[s]
        d = np.linalg.norm((r - model[b]) @ lin.T, axis=1).mean()
        f = np.linalg.norm((r[::-1] - model[b]) @ lin.T, axis=1).mean()
        if f < d:
            r = r[::-1]
        sums[b] += r
        inside = ((r >= 0) & (r <= dims)).all(1)
        u = r - 0.5
        i = np.floor(u)
        fr = u - i
        i0 = np.clip(i.astype(np.int64), 0, dims - 1)
        i1 = np.clip(i.astype(np.int64) + 1, 0, dims - 1)
        v = np.zeros(K)
        for corner in range(8):
            pick = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
            idx = [np.where(pick[k], i1[:, k], i0[:, k]) for k in range(3)]
            w = np.prod([fr[:, k] if pick[k] else 1.0 - fr[:, k] for k in range(3)], axis=0)
            v += w * volume[idx[0], idx[1], idx[2]]
        prof[0, b, inside] += v[inside]
        prof[1, b, inside] += (v * v)[inside]
        prof[2, b, inside] += 1
    return sums, prof


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=262144)
    ap.add_argument('--bundles', type=int, default=21)
    ap.add_argument('--K', type=int, default=100)
    ap.add_argument('--D', type=int, default=96)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--numpy_rows', type=int, default=4096)
    ap.add_argument('--variant', default=os.path.join(HERE, 'micro', '_exp',
                                                      'libttl_hip_noruns.so'))
    args = ap.parse_args(argv)
    from tracktolearn_amd import _lib, bundle_profile as bp
    from tracktolearn_amd.density import gather_rows
    n, B, K, D = args.rows, args.bundles, args.K, args.D
    points, offsets = rows_of.synthetic_rows(n, D)
    gen = torch.Generator(device=DEV).manual_seed(7)
    bundle = torch.randint(0, B, (n,), device=DEV, generator=gen, dtype=torch.int32)
    order = torch.argsort(bundle, stable=True)
    s_points, s_offsets = gather_rows(points, offsets, order)
    s_points, s_bundle = s_points.contiguous(), bundle[order].contiguous()
    ends = torch.rand((B, 2, 3), device=DEV, generator=gen) * D
    t = torch.linspace(0.0, 1.0, K, device=DEV)[None, :, None]
    model = (ends[:, :1] + t * (ends[:, 1:] - ends[:, :1])).float().contiguous()
    volume = torch.rand((D, D, D), device=DEV, generator=gen).float().contiguous()
    scale = bp.coordinate_scale((D, D, D))
    scale_v, scale_sq = bp.metric_scales(volume.cpu().numpy())
    lin_c = (C.c_double * 9)(*LIN.reshape(9))
    dims_c = (C.c_int32 * 3)(D, D, D)
    flip = torch.zeros(n, dtype=torch.int32, device=DEV)
    mdf = torch.zeros(n, dtype=torch.float64, device=DEV)
    sum_q = torch.zeros((B, K, 3), dtype=torch.int64, device=DEV)
    sum_n = torch.zeros(B, dtype=torch.int64, device=DEV)
    prof = [torch.zeros((B, K), dtype=torch.int64, device=DEV) for _ in range(3)]
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    libs = {'': entry_points(_lib.LIB_PATH)}
    _lib.load()
    if os.path.exists(args.variant):
        libs['_no_runs'] = entry_points(args.variant)

    def orient(fn, pts, off, bun):      # the sums are added to: nothing is zeroed between runs
        _lib.check(fn(pts.data_ptr(), off.data_ptr(), n, bun.data_ptr(), B, K, model.data_ptr(),
                      lin_c, scale, flip.data_ptr(), mdf.data_ptr(), sum_q.data_ptr(),
                      sum_n.data_ptr(), stream), 'ttl_bundle_orient')

    def profile(fn, pts, off, bun):
        _lib.check(fn(pts.data_ptr(), off.data_ptr(), n, bun.data_ptr(), flip.data_ptr(), B, K,
                      volume.data_ptr(), dims_c, scale_v, scale_sq, prof[0].data_ptr(),
                      prof[1].data_ptr(), prof[2].data_ptr(), None, stream),
                   'ttl_bundle_profile')
    legs = {}
    for tag, (fo, fp) in libs.items():
        legs['orient_sorted' + tag] = lambda fo=fo: orient(fo, s_points, s_offsets, s_bundle)
        legs['orient_unsorted' + tag] = lambda fo=fo: orient(fo, points, offsets, bundle)
        legs['profile_sorted' + tag] = lambda fp=fp: profile(fp, s_points, s_offsets, s_bundle)
        legs['profile_unsorted' + tag] = lambda fp=fp: profile(fp, points, offsets, bundle)
    legs['torch_orient'] = lambda: torch_orient(s_points, s_offsets, s_bundle, B, K, model, LIN)
    legs['torch_profile'] = lambda: torch_profile(s_points, s_offsets, s_bundle, flip, B, K,
                                                  volume)
    times = {k: [] for k in legs}
    for rep in range(args.reps + 2):
        for name, fn in legs.items():
            ms, _ = base.timed(fn)
            if rep >= 2:
                times[name].append(ms)
    # how far the torch composition lies from the kernels
    sum_q.zero_()
    sum_n.zero_()
    for p in prof:
        p.zero_()
    orient(libs[''][0], s_points, s_offsets, s_bundle)
    profile(libs[''][1], s_points, s_offsets, s_bundle)
    k_flip = flip.clone()
    t_flip, t_sums, t_count = torch_orient(s_points, s_offsets, s_bundle, B, K, model, LIN)
    centroid = sum_q.double() / scale / sum_n[:, None, None]
    t_prof = torch_profile(s_points, s_offsets, s_bundle, k_flip, B, K, volume)
    mean = prof[0].double() / scale_v / prof[2]
    # download + NumPy on the first rows of the sorted input
    k = min(args.numpy_rows, n)
    m = int(s_offsets[k].item())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    numpy_loop(s_points[:m].cpu().numpy(), s_offsets[:k + 1].cpu().numpy(),
               s_bundle[:k].cpu().numpy(), B, K, model.double().cpu().numpy(), LIN,
               volume.cpu().numpy())
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    med = {k_: round(float(np.median(v)), 3) for k_, v in times.items()}
    nbytes = points.shape[0] * 12
    print(json.dumps({
        'object': 'bundle_profile_kernels', 'rows': n, 'points': int(points.shape[0]),
        'bundles': B, 'K': K, 'grid': f'{D}^3',
        **{k_ + '_ms': v for k_, v in med.items()},
        **{k_ + '_min_ms': round(min(v), 3) for k_, v in times.items()},
        **{k_ + '_point_bytes_per_s': round(nbytes / (v * 1e-3), -6) for k_, v in med.items()
           if not k_.startswith('torch')},
        **{k_ + '_share_of_8TBs': round(nbytes / (v * 1e-3) / PEAK, 4) for k_, v in med.items()
           if not k_.startswith('torch')},
        'variant_built': '_no_runs' in libs,
        'numpy_rows': k, 'download_numpy_ms_measured': round(numpy_ms, 1),
        'download_numpy_ms_scaled_to_all_rows': round(numpy_ms * points.shape[0] / m, 1),
        'rows_taking_part': int(sum_n.sum().item()),
        'flips_kernel': int(k_flip.sum().item()),
        'flips_differing_from_torch': int((t_flip != (k_flip != 0)).sum().item()),
        'centroid_max_abs_difference_from_torch_vox': float(
            (centroid - t_sums / t_count[:, None, None]).abs().max().item()),
        'profile_mean_max_abs_difference_from_torch': float(
            (mean - t_prof[0] / t_prof[2]).abs().nan_to_num(0.0).max().item()),
        'reps': args.reps, 'device': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
