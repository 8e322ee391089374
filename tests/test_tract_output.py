"""The tracker's output stage: `parallel.select_tracts` --
`ttl_tract_select` + `ttl_tract_emit` on the GPU -- against its
specification, the float64 arc filter followed by
`tractogram.compress_streamline`.

CPU: the host branch of `select_tracts` equals that composition bit for bit;
the new symbols are bound and the ABI numbers agree.  GPU: equivalence on
20 480 generated rows for every tolerance / segment bound, hand-built dyadic
rows with hand-written answers, rows beyond the LDS staging limit, the Tracker
with and without the device stage, and the stage's peak memory.

All inputs come from the seeded generators below.  The host reference of the
large comparison runs in freshly spawned worker processes that never open the
GPU.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = 1 | 4                       # STOPPING_MASK | STOPPING_CURVATURE
T_ROW = 267
N_ROWS = 20480
TOLS = (0.0, 0.005, 0.1, 0.4)
# (max_segment_length, min_arc, max_arc) in voxels: 1.0 makes the segment bound
# bind (steps are 0.375); the arc bounds avoid the multiples of 0.375 the
# straight rows hit exactly, and reject rows at both ends
BOUNDS = ((10.0, 0.25, 88.1), (1.0, 7.3, 60.2))
KNIFE = 1e-12


# --------------------------------------------------------------------------
# generators
# --------------------------------------------------------------------------
def make_rows(n, T, seed, step=0.375):
    """(history (n, T, 3) f32, lengths i32, flags i32): random walks with
    turning noise from {0.02, 0.15, 0.4}, exactly straight rows on a dyadic
    grid, rows with repeated points and exact back-tracks; junk after the
    true length."""
    rng = np.random.RandomState(seed)
    sigma = rng.choice([0.02, 0.15, 0.4], size=n)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    steps = np.empty((n, T, 3))
    steps[:, 0] = rng.uniform(5.0, 90.0, (n, 3))
    for k in range(1, T):
        d = d + sigma[:, None] * rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        steps[:, k] = step * d
    kind = rng.randint(0, 10, n)        # 0: straight, 1: stutter, 2: back-track
    stutter = np.nonzero(kind == 1)[0]
    zero = rng.uniform(size=(len(stutter), T)) < 0.15
    zero[:, 0] = False
    steps[stutter] = np.where(zero[:, :, None], 0.0, steps[stutter])
    hist = np.cumsum(steps, axis=1).astype(np.float32)
    straight = np.nonzero(kind == 0)[0]
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 0], [1, -1, 1]], np.float64)
    start = np.round(rng.uniform(5.0, 90.0, (len(straight), 3)) * 8) / 8
    dirs = axes[rng.randint(0, len(axes), len(straight))] * step
    hist[straight] = (start[:, None] + np.arange(T)[None, :, None] * dirs[:, None]
                      ).astype(np.float32)
    for i in np.nonzero(kind == 2)[0]:  # p[j + 2] == p[j] at point 0 and elsewhere
        for j in np.concatenate(([0], rng.randint(0, T - 2, 6))):
            hist[i, j + 2] = hist[i, j]
    lengths = rng.randint(1, T + 1, n).astype(np.int32)
    lengths[:8] = [1, 2, 3, T, 1, 2, 3, T]
    flags = rng.choice([0, 1, 2, 4, 5, 64, 66, 68], size=n).astype(np.int32)
    flags[:4] = 0
    flags[4:8] = [1, 4, 5, 1]
    junk = np.arange(T)[None, :] >= lengths[:, None]
    hist[junk] = rng.uniform(-1e3, 1e3, (int(junk.sum()), 3)).astype(np.float32)
    return hist, lengths, flags


def kept_length(lengths, flags):
    return lengths.astype(np.int64) - ((flags & CUT) != 0)


# --------------------------------------------------------------------------
# the specification on the host
# --------------------------------------------------------------------------
def _rel(x, thr):
    return abs(x - thr) / abs(thr) if thr != 0 else (np.inf if x != 0 else 0.0)


def spec_compress(s, tol, msl):
    """`compress_streamline` restated to return the kept indices, the
    smallest relative distance of any tested quantity to its threshold, the
    longest look-back and the number of zero-length chords."""
    n = len(s)
    if n <= 2:
        return list(range(n)), np.inf, 0, 0
    keep, prev, margin, look, zeros = [0], 0, np.inf, 0, 0
    for nxt in range(2, n):
        a, b = s[prev].astype(np.float64), s[nxt].astype(np.float64)
        ab = b - a
        L = np.linalg.norm(ab)
        margin = min(margin, _rel(L, msl))
        ok = L <= msl
        if ok:
            mid = s[prev + 1:nxt].astype(np.float64) - a
            if L > 0:
                t = np.clip(mid @ ab / (L ** 2), 0.0, 1.0)
                dist = np.linalg.norm(mid - t[:, None] * ab, axis=1)
            else:
                zeros += 1
                dist = np.linalg.norm(mid, axis=1)
            margin = min(margin, np.abs(dist - tol).min() / tol)
            ok = bool((dist <= tol).all())
            if ok:
                look = max(look, nxt - prev)
        if not ok:
            keep.append(nxt - 1)
            prev = nxt - 1
    keep.append(n - 1)
    return keep, margin, look, zeros


def spec_arc(s):
    """The arc filter's quantity as tests/test_tracker_golden.py computes it."""
    if len(s) < 2:
        return 0.0
    d = (s[1:] - s[:-1]).astype(np.float64)
    return float(np.sqrt((d * d).sum(axis=1)).sum())


def reference_rows(job):
    """Worker: for rows (hist, keep) and every (tol, bounds) case, the accepted
    flag, the kept indices and the knife-edge margin of each row.  The kept
    indices are checked against `compress_streamline`'s points here."""
    from tracktolearn_amd.tractogram import compress_streamline
    hist, keep_len, cases = job
    out = []
    for tol, (msl, lo, hi) in cases:
        rows = []
        for r in range(len(hist)):
            s = hist[r, :keep_len[r]]
            arc = spec_arc(s)
            margin = min(_rel(arc, lo), _rel(arc, hi))
            ok = lo <= arc <= hi
            idx, look, zeros = None, 0, 0
            if ok:
                if tol > 0:
                    idx, m, look, zeros = spec_compress(s, tol, msl)
                    margin = min(margin, m)
                    want = compress_streamline(s, tol, msl)
                    assert want.dtype == np.float32 and np.array_equal(
                        s[idx].view(np.uint32), want.view(np.uint32))
                else:
                    idx = list(range(len(s)))
            rows.append((ok, idx, margin, look, zeros))
        out.append(rows)
    return out


def reference(hist, keep_len, cases, workers=None):
    """`reference_rows` over all rows, in spawned processes (fresh
    interpreters: nothing of this process's GPU state is inherited)."""
    import multiprocessing as mp
    workers = workers or min(16, os.cpu_count() or 1)
    chunk = 256
    jobs = [(hist[a:a + chunk], keep_len[a:a + chunk], cases)
            for a in range(0, len(hist), chunk)]
    if workers > 1 and len(jobs) > 1:
        with mp.get_context('spawn').Pool(workers) as pool:
            parts = pool.map(reference_rows, jobs)
    else:
        parts = [reference_rows(j) for j in jobs]
    return [[row for p in parts for row in p[c]] for c in range(len(cases))]


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_host_select_tracts_is_the_arc_filter_then_compress_streamline():
    import torch
    from tracktolearn_amd.parallel import select_tracts
    hist, lengths, flags = make_rows(384, 120, seed=5)
    keep_len = kept_length(lengths, flags)
    cases = [(0.0, (10.0, 0.25, 30.1)), (0.1, (10.0, 3.1, 40.1)), (0.4, (1.0, 0.25, 30.1))]
    ref = reference(hist, keep_len, cases, workers=1)
    for (tol, (msl, lo, hi)), rows in zip(cases, ref):
        pts, counts, sel = select_tracts(torch.from_numpy(hist), torch.from_numpy(lengths),
                                         torch.from_numpy(flags), lo, hi, tol, msl)
        assert pts.dtype == torch.float32 and counts.dtype == torch.int64
        assert sel.dtype == torch.int64 and pts.shape[1:] == (3,)
        want_rows = [r for r, row in enumerate(rows) if row[0]]
        assert 0 < len(want_rows) < len(rows)
        assert sel.tolist() == want_rows
        assert counts.tolist() == [len(rows[r][1]) for r in want_rows]
        want = np.concatenate([hist[r][rows[r][1]] for r in want_rows])
        assert np.array_equal(pts.numpy().view(np.uint32), want.view(np.uint32))
        assert min(row[2] for row in rows) > KNIFE
    empty = select_tracts(torch.zeros((0, 120, 3)), torch.zeros(0, dtype=torch.int32),
                          torch.zeros(0, dtype=torch.int32), 0.0, 1.0, 0.1)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0,), (0,)]


def test_the_output_stage_is_bound_and_the_abi_numbers_agree():
    from tracktolearn_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ttl_hip.h')) as f:
        header = f.read()
    assert int(re.search(r'#define TTL_ABI_VERSION (\d+)', header).group(1)) == 13
    assert _lib.ABI_VERSION == 13
    lib = _lib.load()
    assert lib.ttl_abi_version() == 13
    for name in ('ttl_tract_select', 'ttl_tract_emit', 'ttl_tract_mask_words',
                 'ttl_tract_stage_points'):
        assert name in _lib.SYMBOLS and re.search(r'\b%s\(' % name, header)
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert lib.ttl_tract_mask_words(3 * 267) == 5
    assert lib.ttl_tract_mask_words(3 * 64) == 1 and lib.ttl_tract_mask_words(3 * 65) == 2


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
def _device_rows(hist, lengths, flags, lo, hi, tol, msl):
    """(rows, counts, packed points, survivor indices per row from the mask)."""
    import torch
    from tracktolearn_amd.parallel import select_tracts, tract_survivors
    dev = torch.device('cuda:0')
    h, ln, fl = (torch.from_numpy(a).to(dev) for a in (hist, lengths, flags))
    pts, counts, rows = select_tracts(h, ln, fl, lo, hi, tol, msl)
    _, sel, mask = tract_survivors(h, ln, fl, lo, hi, tol, msl)
    assert pts.dtype == torch.float32 and pts.is_cuda and pts.shape[1:] == (3,)
    assert counts.dtype == torch.int64 and rows.dtype == torch.int64
    sel = sel.cpu().numpy()
    bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), axis=1, bitorder='little')
    assert np.array_equal(np.nonzero(sel[1])[0], rows.cpu().numpy())
    assert np.array_equal(sel[0][sel[1] != 0], counts.cpu().numpy())
    assert np.array_equal(bits.sum(axis=1), sel[0])
    return rows.cpu().numpy(), counts.cpu().numpy(), pts.cpu().numpy(), bits


def _compare(hist, lengths, flags, cases, ref, max_excluded):
    worst, excluded_total, look, zeros = np.inf, 0, 0, 0
    for (tol, (msl, lo, hi)), want in zip(cases, ref):
        rows, counts, pts, bits = _device_rows(hist, lengths, flags, lo, hi, tol, msl)
        margins = np.array([w[2] for w in want])
        excluded = margins <= KNIFE
        worst = min(worst, margins.min())
        excluded_total += int(excluded.sum())
        look = max(look, max(w[3] for w in want))
        zeros += sum(w[4] for w in want)
        offs = np.concatenate(([0], np.cumsum(counts)))
        assert offs[-1] == len(pts)
        where = {int(r): k for k, r in enumerate(rows)}
        assert list(rows) == sorted(where)                       # row order
        n_ok = 0
        for r, (ok, idx, _, _, _) in enumerate(want):
            if excluded[r]:
                continue
            assert ok == (r in where), (tol, msl, r)
            if not ok:
                assert not bits[r].any()
                continue
            n_ok += 1
            k = where[r]
            assert np.array_equal(np.nonzero(bits[r])[0], idx), (tol, msl, r)
            got = pts[offs[k]:offs[k + 1]]
            assert np.array_equal(got.view(np.uint32), hist[r][idx].view(np.uint32)), (tol, msl, r)
        assert 0 < n_ok < len(want)
        print(f'tol {tol} max_segment_length {msl}: {n_ok} of {len(want)} rows accepted, '
              f'{int(counts.sum())} points kept, smallest margin {margins.min():.3e}, '
              f'{int(excluded.sum())} rows excluded')
    print(f'smallest margin over all cases {worst:.3e}; excluded {excluded_total}; '
          f'longest look-back {look}; zero-length chords {zeros}')
    assert excluded_total <= max_excluded
    return worst, look, zeros


@pytest.mark.gpu
def test_select_tracts_equals_the_specification_on_generated_rows():
    """Accepted rows, their order, the kept indices and the packed bits for
    every tolerance and segment bound.  Rows the host finds within relative
    1e-12 of a threshold would be left out; with these seeds there are none."""
    hist, lengths, flags = make_rows(N_ROWS, T_ROW, seed=20250)
    assert set(lengths[:8]) == {1, 2, 3, T_ROW}
    keep_len = kept_length(lengths, flags)
    cases = [(tol, b) for b in BOUNDS for tol in TOLS]
    ref = reference(hist, keep_len, cases)
    worst, look, zeros = _compare(hist, lengths, flags, cases, ref, max_excluded=0)
    assert worst > KNIFE
    assert zeros > 0                    # the L == 0 branch was exercised


def _exact(points, tol, msl=10.0):
    lengths = np.array([len(p) for p in points], np.int32)
    hist = np.full((len(points), 8, 3), 777.0, np.float32)
    for i, p in enumerate(points):
        hist[i, :len(p)] = p
    flags = np.zeros(len(points), np.int32)
    rows, counts, pts, bits = _device_rows(hist, lengths, flags, 0.0, 1e9, tol, msl)
    assert list(rows) == list(range(len(points)))
    offs = np.concatenate(([0], np.cumsum(counts)))
    out = []
    for i in range(len(points)):
        idx = list(np.nonzero(bits[i])[0])
        assert np.array_equal(pts[offs[i]:offs[i + 1]], hist[i][idx])
        out.append(idx)
    return out


@pytest.mark.gpu
def test_exactly_representable_rows_give_the_hand_written_indices():
    """Dyadic rows: every intermediate of the specification is exact, so the
    expected indices below are written by hand, not computed."""
    bump = [(0, 0, 0), (2, 0.5, 0), (4, 0, 0)]           # distance exactly 0.5
    beyond = [(0, 0, 0), (3, 0, 0), (1, 0, 0)]           # t = 3 -> 1: 2 from the end, 0 from the line
    before = [(0, 0, 0), (-2, 0, 0), (1, 0, 0)]          # t = -2 -> 0: 2 from the start
    line = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)]
    # chord 0 -> 2: point 1 is 2 from its end (kept out at tol 2); chord 0 -> 3: point 2 is
    # 0.5 from its end, point 1 is 2.5 -- the OLDER interior point breaks it
    earlier = [(0, 0, 0), (3, 0, 0), (1, 0, 0), (0.5, 0, 0)]
    assert _exact([bump], 0.5) == [[0, 2]]                       # <=, not <
    assert _exact([bump], 0.5 - 2.0 ** -30) == [[0, 1, 2]]
    assert _exact([beyond, before], 1.0) == [[0, 1, 2], [0, 1, 2]]   # the clamp decides
    assert _exact([beyond, before], 2.0) == [[0, 2], [0, 2]]
    assert _exact([line], 0.5, msl=10.0) == [[0, 4]]
    assert _exact([line], 0.5, msl=2.0) == [[0, 2, 4]]           # only the segment bound
    assert _exact([earlier], 2.0) == [[0, 2, 3]]
    assert _exact([earlier], 2.5) == [[0, 3]]
    assert _exact([bump, line, earlier], 0.0) == [[0, 1, 2], [0, 1, 2, 3, 4], [0, 1, 2, 3]]


@pytest.mark.gpu
def test_rows_beyond_the_staging_limit_and_look_backs_beyond_a_wave():
    """Rows longer than the LDS staging limit read global memory; near-straight
    rows with a generous segment bound make the look-back exceed 64 points."""
    from tracktolearn_amd import _lib
    T = 2304
    assert T > _lib.load().ttl_tract_stage_points() and T >= 2048
    hist, lengths, flags = make_rows(96, T, seed=77)
    rng = np.random.RandomState(78)
    for i in range(8, 72):              # near-straight: a line plus 2e-3 of jitter
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        line = rng.uniform(20, 60, 3) + 0.375 * np.arange(T)[:, None] * d
        hist[i] = (line + 2e-3 * rng.standard_normal((T, 3))).astype(np.float32)
    lengths[8:] = rng.randint(400, T + 1, 88)
    lengths[8:12] = T
    keep_len = kept_length(lengths, flags)
    cases = [(0.05, (200.0, 0.25, 1e4)), (0.0, (200.0, 100.0, 700.0)), (0.4, (31.0, 0.25, 601.3))]
    ref = reference(hist, keep_len, cases, workers=min(8, os.cpu_count() or 1))
    worst, look, _ = _compare(hist, lengths, flags, cases, ref, max_excluded=0)
    assert worst > KNIFE
    assert look > 64


def _track(name, fmt_name, compress, device_output, min_length=None):
    import torch
    from test_tracker_golden import ReplayAgent, _Alg, _gpu_env
    from helpers import load_trace
    from tracktolearn_amd.tracking import tracker as trk
    z = load_trace(name)
    env = _gpu_env(z, noisy=True, reward=False)
    env.seeds = z['seeds_before_shuffle'].copy()
    agent = ReplayAgent(z, torch.device('cuda:0'))
    tracker = trk.Tracker(_Alg(agent), n_actor=int(z['n_actor']), prob=0.0, compress=compress,
                          min_length=float(z['min_length']) if min_length is None else min_length,
                          max_length=float(z['max_length']), save_seeds=True,
                          device_output=device_output)
    np.random.seed(int(z['shuffle_seed']))
    items = list(tracker.track(env, getattr(trk, fmt_name)))
    assert agent.i == len(agent.batches)
    return items, tracker, env


@pytest.mark.gpu
@pytest.mark.parametrize('fmt_name', ['TrkFile', 'TckFile'])
@pytest.mark.parametrize('compress', [0.0, 0.2])
def test_tracker_items_are_the_same_with_and_without_the_device_stage(fmt_name, compress):
    name = 'tracker_trk' if fmt_name == 'TrkFile' else 'tracker_tck'
    new, tracker, _ = _track(name, fmt_name, compress, True)
    old, _, _ = _track(name, fmt_name, compress, False)
    assert tracker.device_output is True and len(new) == len(old) > 0
    for a, b in zip(new, old):
        assert a.streamline.dtype == b.streamline.dtype
        assert a.streamline.shape == b.streamline.shape
        assert a.streamline.tobytes() == b.streamline.tobytes()
        assert a.data_for_streamline['seeds'].dtype == b.data_for_streamline['seeds'].dtype
        assert np.array_equal(a.data_for_streamline['seeds'], b.data_for_streamline['seeds'])
    if compress:
        plain, _, _ = _track(name, fmt_name, 0.0, None)
        assert sum(len(i.streamline) for i in new) < sum(len(i.streamline) for i in plain)


@pytest.mark.gpu
def test_tracker_with_an_empty_batch_and_with_every_row_rejected():
    import torch
    from tracktolearn_amd.parallel import select_tracts
    items, tracker, env = _track('tracker_trk', 'TrkFile', 0.2, None, min_length=1e6)
    assert items == [] and tracker._device_output(env)
    n = env._n_total
    assert n > 0
    pts, counts, rows = select_tracts(env._buf_streamlines[:n], env._buf_lengths[:n],
                                      env._buf_flags[:n], 1e6, 2e6, 0.1)
    assert (pts.shape, counts.shape, rows.shape) == ((0, 3), (0,), (0,)) and pts.is_cuda
    env._n_total = 0                    # an empty shard of a sharded batch
    assert list(tracker._batch_items(env, 0.0, 1e6, tol_vox=0.1)) == []
    pts, counts, rows = select_tracts(env._buf_streamlines[:0], env._buf_lengths[:0],
                                      env._buf_flags[:0], 0.0, 1e6, 0.1)
    assert (pts.shape, counts.shape, rows.shape) == ((0, 3), (0,), (0,))
    assert pts.dtype == torch.float32 and counts.dtype == rows.dtype == torch.int64


@pytest.mark.gpu
def test_the_stage_allocates_less_than_one_float64_segment_tensor():
    """65 536 x 267: the torch filter it replaces allocates several (n, T-1, 3)
    float64 tensors; everything the device stage allocates, outputs included,
    stays below one."""
    import torch
    from tracktolearn_amd.parallel import select_tracts
    dev = torch.device('cuda:0')
    n, T = 65536, T_ROW
    g = torch.Generator(device=dev).manual_seed(3)
    steps = torch.randn((n, T, 3), device=dev, generator=g)
    steps *= 0.375 / steps.norm(dim=2, keepdim=True)
    hist = torch.cumsum(steps, dim=1)
    del steps
    lengths = torch.randint(1, T + 1, (n,), device=dev, generator=g, dtype=torch.int32)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    one = n * (T - 1) * 3 * 8
    for tol in (0.0, 0.1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = select_tracts(hist, lengths, flags, 5.0, 95.0, tol)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        print(f'tol {tol}: peak {peak / 1e6:.1f} MB over the stage, one float64 segment '
              f'tensor {one / 1e6:.1f} MB, {out[1].numel()} rows, {out[0].shape[0]} points')
        assert out[1].numel() > 0
        assert peak < one
        del out
