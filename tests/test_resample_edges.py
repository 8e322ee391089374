"""The resampler family at the shapes the rest of the suite never runs:
``ttl_resample_streamlines``, ``ttl_oracle_segments`` and
``ttl_oracle_segments_packed`` with other point counts than 128, rows of one
point, rows of one repeated point, rows above the 64 KB LDS path, clamped
lengths and wide pitches -- bit for bit against the blocked-order float64
restatement (tests/ref_oracle_validator.py) and within the suite's 1e-5 of
the plain float64 resampler (tests/ref_resample.py)."""
import functools

import numpy as np
import pytest
import torch

import ref_oracle_validator as ref
from ref_resample import resample_streamlines as plain_resample

NB_POINTS = (2, 3, 64, 65, 100, 129, 257)
ROW_LENGTHS = (1, 2, 64, 65, 66, 129, 1000, 3000, 5120)


def _walk(L, seed):
    """A smooth random walk of L points with coordinates in [0, 100]."""
    rng = np.random.RandomState(seed)
    p = rng.uniform(10, 90, 3) + np.cumsum(rng.standard_normal((L, 3)) * 0.5, axis=0)
    return np.clip(p, 0.0, 100.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rows():
    """(points (L, 3) float32, stated length): one walk per length, a row of
    one repeated point, leading and trailing runs of a repeated point, a
    stated length of 0 (read as 1) and one above max_len (read as max_len)."""
    rows = [(_walk(L, L), L) for L in ROW_LENGTHS]
    rows.append((np.repeat(_walk(1, 7), 65, axis=0), 65))            # total arc length 0
    runs = _walk(129, 8)
    runs[:20] = runs[20]
    runs[-30:] = runs[-31]
    rows.append((runs, 129))
    rows.append((_walk(40, 9), 0))
    return rows


def _batches():
    """Two padded batches: max_len 1000 (32 KB of LDS) with the clamped
    lengths, max_len 5120 (exactly the 160 KB) with the long rows."""
    rows = _rows()
    small = [r for r in rows if len(r[0]) <= 1000] + [(_walk(1000, 10), 1003)]
    large = [r for r in rows if len(r[0]) > 1000 or len(r[0]) in (1, 65)]
    return {1000: small, 5120: large}


def _padded(rows, max_len, extra):
    pts = np.full((len(rows), max_len + extra, 3), np.nan, np.float32)
    for i, (p, _) in enumerate(rows):
        pts[i, :len(p)] = p
    lengths = np.array([L for _, L in rows], np.int64)
    return pts, lengths


def _read_length(stated, max_len):
    return min(max(int(stated), 1), max_len)


def test_blocked_restatement_handles_one_point():
    """L = 1: the output is the single point, the differences zero vectors."""
    p = _walk(1, 3)
    for nb in (2, 3, 128):
        assert np.array_equal(ref.resample_blocked(p, nb), np.repeat(p, nb, axis=0))
        assert np.array_equal(ref.segments_blocked(p, nb), np.zeros((nb - 1, 3), np.float32))


@pytest.mark.parametrize('nb', (2, 65, 257))
def test_blocked_restatement_matches_the_plain_resampler_at_the_edges(nb):
    for p, stated in _rows():
        L = _read_length(stated, 5120)
        np.testing.assert_allclose(ref.resample_blocked(p[:L], nb), _plain(p[:L], nb), atol=1e-5,
                                   rtol=0)


def _plain(p, nb):
    """tests/ref_resample.py on one row (L, 3); one point is its own resampling."""
    if len(p) == 1:
        return np.repeat(p, nb, axis=0)
    return plain_resample(torch.from_numpy(p[None]), torch.tensor([len(p)]), nb)[0].numpy()


def _stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize('lengths_dtype', ('int32', 'int64'))
@pytest.mark.parametrize('nb', NB_POINTS)
def test_hip_resampler_equals_the_blocked_restatement(nb, lengths_dtype):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    for max_len, rows in _batches().items():
        pts, lengths = _padded(rows, max_len, extra=7)            # pitch wider than 3 max_len
        d_pts = torch.from_numpy(pts).cuda()
        d_len = torch.from_numpy(lengths.astype(lengths_dtype)).cuda()
        out = torch.full((len(rows), nb, 3), float('nan'), dtype=torch.float32, device='cuda')
        l32 = d_len.data_ptr() if lengths_dtype == 'int32' else None
        l64 = d_len.data_ptr() if lengths_dtype == 'int64' else None
        _lib.check(lib.ttl_resample_streamlines(d_pts.data_ptr(), d_pts.stride(0), l32, l64,
                                                len(rows), max_len, nb, out.data_ptr(),
                                                _stream()), 'resample')
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i, (p, stated) in enumerate(rows):
            L = _read_length(stated, max_len)
            want = ref.resample_blocked(pts[i, :L], nb)
            assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (max_len, i, L)
            np.testing.assert_allclose(got[i], _plain(pts[i, :L], nb), atol=1e-5, rtol=0)


@pytest.mark.gpu
def test_hip_resampler_refuses_rows_above_the_lds():
    from tracktolearn_amd import _lib
    lib = _lib.load()
    pts = torch.zeros((1, 5121, 3), dtype=torch.float32, device='cuda')
    lengths = torch.tensor([5121], dtype=torch.int32, device='cuda')
    out = torch.full((1, 128, 3), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.ttl_resample_streamlines(pts.data_ptr(), pts.stride(0), lengths.data_ptr(), None, 1,
                                      5121, 128, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and bool(torch.isnan(out).all())


def _history(L):
    """Six history rows of at least L points behind a wide pitch: walks, one
    repeated point, leading and trailing repeated runs."""
    hist = np.stack([_walk(L + 5, 100 + L + r) for r in range(6)])
    hist[3, :L] = hist[3, 0]
    if L >= 3:
        hist[4, :L // 3] = hist[4, L // 3]
        hist[4, L - L // 3:L] = hist[4, L - L // 3 - 1]
    return hist


@pytest.mark.gpu
@pytest.mark.parametrize('nb', NB_POINTS)
def test_hip_oracle_segments_equal_the_blocked_restatement(nb):
    """Every row has n_points points here.  The kernel keeps cum, the points
    and the result of four waves in LDS (20 B per point per wave), so rows of
    up to 1000 points run and rows of 3000 and 5120 points are refused."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    ids = np.array([5, 3, 0, 4, 1], np.int32)                     # rows gathered by id
    for L in ROW_LENGTHS:
        hist = _history(L)
        d_hist = torch.from_numpy(hist).cuda()
        d_ids = torch.from_numpy(np.stack([ids, -np.ones_like(ids)], 1).copy()).cuda()
        out = torch.full((len(ids), nb - 1, 3), float('nan'), dtype=torch.float32, device='cuda')
        rc = lib.ttl_oracle_segments(d_hist.data_ptr(), d_hist.stride(0), d_ids.data_ptr(), 2,
                                     len(ids), L, None, nb, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        if L in (3000, 5120):
            assert rc == _lib.ERR_INVALID and bool(torch.isnan(out).all()), (L, rc)
            continue
        assert rc == 0, (L, rc)
        got = out.cpu().numpy()
        for q, g in enumerate(ids):
            want = ref.segments_blocked(hist[g, :L], nb)
            assert np.array_equal(got[q].view(np.uint32), want.view(np.uint32)), (L, q)
            plain = _plain(hist[g, :L], nb)
            np.testing.assert_allclose(got[q], plain[1:] - plain[:-1], atol=1e-5, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize('nb', NB_POINTS + (1400,))
def test_hip_packed_segments_equal_the_blocked_restatement(nb):
    """Ragged input of any length, an empty streamline included (zero
    vectors); 1400 output points take the kernel above 64 KB of LDS."""
    from tracktolearn_amd.oracles.oracle import oracle_segments_packed
    lines = [p[:_read_length(stated, 5120)] for p, stated in _rows()]
    lines.insert(3, np.zeros((0, 3), np.float32))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in lines])]).astype(np.int64)
    points = torch.from_numpy(np.concatenate(lines)).cuda()
    got = oracle_segments_packed(points, torch.from_numpy(offsets).cuda(), nb).cpu().numpy()
    assert got.shape == (len(lines), nb - 1, 3)
    for i, s in enumerate(lines):
        if len(s) == 0:
            assert np.array_equal(got[i].view(np.uint32), np.zeros((nb - 1, 3), np.uint32))
            continue
        want = ref.segments_blocked(s, nb)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, len(s))
        plain = _plain(s, nb)
        np.testing.assert_allclose(got[i], plain[1:] - plain[:-1], atol=1e-5, rtol=0)


# ------------------------------------------------- the 3x3 map of ttl_oracle_segments
# (row-major, out = p @ m: the matrix of tests/test_oracle_net.py::test_oracle_segments_kernel)
LIN = np.array([[0.9, 0.05, 0.0], [-0.03, 1.1, 0.02], [0.01, 0.0, 0.8]], np.float32)
MAP_LENGTHS = (1, 2, 65, 129)


@functools.lru_cache(maxsize=None)
def _mapped_history(L):
    """(_history(L), its six rows' first L points through the exact-fma map)."""
    hist = _history(L)
    return hist, np.stack([ref.map_points_fma(hist[g, :L], LIN) for g in range(len(hist))])


def _ordered(x):
    """float32 -> int64 that counts representable values (-0 and +0 coincide)."""
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def test_exact_fma_map_is_within_an_ulp_of_the_float64_product():
    """The restatement itself, without a GPU.  The three float32 roundings of
    the fma chain (at most half an ulp each) leave it less than 1.5 ulp from
    the exact value and the float64 product rounded to float32 lies within
    half an ulp of it, so the two float32 values are equal or neighbours."""
    for L in MAP_LENGTHS:
        hist, mapped = _mapped_history(L)
        want = (hist[:, :L].astype(np.float64) @ LIN.astype(np.float64)).astype(np.float32)
        assert np.abs(_ordered(mapped) - _ordered(want)).max() <= 1, L
    # the identity keeps every bit
    assert np.array_equal(ref.map_points_fma(_history(65)[0], np.eye(3)).view(np.uint32),
                          _history(65)[0].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('nb', (2, 65, 128))
def test_hip_oracle_segments_map_equals_the_exact_fma_restatement(nb):
    """The mapped path bit for bit: the points through the exact-fma map,
    rounded to float32, then the blocked restatement; ids with stride 2."""
    import ctypes as C

    from tracktolearn_amd import _lib
    lib = _lib.load()
    ids = np.array([5, 3, 0, 4, 1, 2], np.int32)
    lin = (C.c_float * 9)(*[float(v) for v in LIN.ravel()])
    for L in MAP_LENGTHS:
        hist, mapped = _mapped_history(L)
        d_hist = torch.from_numpy(hist).cuda()
        d_ids = torch.from_numpy(np.stack([ids, -np.ones_like(ids)], 1).copy()).cuda()
        out = torch.full((len(ids), nb - 1, 3), float('nan'), dtype=torch.float32, device='cuda')
        _lib.check(lib.ttl_oracle_segments(d_hist.data_ptr(), d_hist.stride(0), d_ids.data_ptr(),
                                           2, len(ids), L, lin, nb, out.data_ptr(), _stream()),
                   'segments')
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for q, g in enumerate(ids):
            want = ref.segments_blocked(mapped[g], nb)
            assert np.array_equal(got[q].view(np.uint32), want.view(np.uint32)), (L, q)


# ------------------------------------------------- more rows than waves in the grid
# Grids are capped at 4096 (k_resample) and 8192 (the segment kernels) workgroups of four
# waves; beyond 4 cap rows a wave takes a second row and reuses its LDS.  Seven distinct
# short rows repeated with period 7 (which divides neither 16 384 nor 32 768): a wave's
# successive rows differ, so values left in the LDS would show.
WRAP_NB = 3


@functools.lru_cache(maxsize=None)
def _short_rows(first_len):
    """Seven rows of first_len .. first_len + 6 points."""
    return [_walk(first_len + r, 300 + r) for r in range(7)]


@pytest.mark.gpu
def test_hip_resampler_when_a_wave_takes_a_second_row():
    from tracktolearn_amd import _lib
    lib = _lib.load()
    n, rows = 4 * 4096 + 3, _short_rows(1)
    pts7, len7 = _padded([(p, len(p)) for p in rows], 7, extra=0)
    want7 = np.stack([ref.resample_blocked(p, WRAP_NB) for p in rows])
    which = np.arange(n) % 7
    d_pts = torch.from_numpy(pts7[which]).cuda()
    d_len = torch.from_numpy(len7[which].astype(np.int32)).cuda()
    out = torch.full((n, WRAP_NB, 3), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.ttl_resample_streamlines(d_pts.data_ptr(), d_pts.stride(0), d_len.data_ptr(),
                                            None, n, 7, WRAP_NB, out.data_ptr(), _stream()),
               'resample')
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want7[which].view(np.uint32))


@pytest.mark.gpu
def test_hip_oracle_segments_when_a_wave_takes_a_second_row():
    """Every row has five points; the rows are gathered through a permutation."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    n, L = 4 * 8192 + 3, 5
    rows = [p[:L] for p in _short_rows(5)]
    want7 = np.stack([ref.segments_blocked(p, WRAP_NB) for p in rows])
    ids = np.random.RandomState(11).permutation(n).astype(np.int32)
    d_hist = torch.from_numpy(np.stack(rows)[np.arange(n) % 7]).cuda()
    d_ids = torch.from_numpy(ids).cuda()
    out = torch.full((n, WRAP_NB - 1, 3), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.ttl_oracle_segments(d_hist.data_ptr(), d_hist.stride(0), d_ids.data_ptr(), 1,
                                       n, L, None, WRAP_NB, out.data_ptr(), _stream()),
               'segments')
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want7[ids % 7].view(np.uint32))


@pytest.mark.gpu
def test_hip_packed_segments_when_a_wave_takes_a_second_row():
    """Lengths 0 .. 6: an empty streamline (zero vectors) sits inside the loop."""
    from tracktolearn_amd.oracles.oracle import oracle_segments_packed
    n = 4 * 8192 + 3
    rows = [np.zeros((0, 3), np.float32)] + _short_rows(1)[:6]
    want7 = np.stack([ref.segments_blocked(p, WRAP_NB) if len(p) else
                      np.zeros((WRAP_NB - 1, 3), np.float32) for p in rows])
    which = np.arange(n) % 7
    offsets = np.concatenate([[0], np.cumsum([len(rows[w]) for w in which])]).astype(np.int64)
    points = torch.from_numpy(np.concatenate([rows[w] for w in which])).cuda()
    got = oracle_segments_packed(points, torch.from_numpy(offsets).cuda(), WRAP_NB).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want7[which].view(np.uint32))
