"""Deterministic case generators for tests/test_bundle_profile.py: nothing is
committed as data.  A case is a dict of NumPy arrays: points (M, 3) float32,
offsets (n + 1,) int64, bundle (n,) int32, model (B, K, 3) float32, lin (3, 3),
scale, volume (X, Y, Z) float32, scale_v / scale_sq, and B, K."""
import functools

import numpy as np

import ref_bundle_profile as ref

F32 = np.float32
KS = (2, 3, 63, 64, 65, 100, 128, 256)
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 129, 4099)
BS = (1, 2, 21, 64)
DIMS = (7, 6, 5)
LINS = {
    'axis': np.diag([2.0, 2.0, 2.0]),
    'anisotropic': np.diag([-1.25, 0.75, 3.0]),
    'oblique': np.array([[1.5, 0.25, -0.5], [-0.375, 1.25, 0.5], [0.25, -0.75, 2.0]]),
}
#: workgroups of the launch at most (ttl_bundle_profile.hip) x waves of a workgroup
GRID_WAVES = 1024 * 4
COORD_SCALE = 2.0 ** 34                      # bundle_profile.coordinate_scale(DIMS)


def pack(rows):
    offsets = np.zeros(len(rows) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    points = np.concatenate([np.asarray(r, F32).reshape(-1, 3) for r in rows] +
                            [np.zeros((0, 3), F32)])
    return np.ascontiguousarray(points, F32), offsets


def walk(rng, length, dims=DIMS, step=0.3):
    """A random walk of ``length`` points that starts inside the volume and may
    leave it."""
    if length == 0:
        return np.zeros((0, 3), F32)
    start = rng.uniform(0.5, np.asarray(dims) - 0.5)
    steps = rng.normal(0.0, step, (length - 1, 3)) + rng.normal(0.0, step / 4, 3)
    return np.concatenate([[start], start + np.cumsum(steps, 0)]).astype(F32)


def volume(rng, dims=DIMS):
    v = rng.uniform(-1.0, 3.0, dims).astype(F32)
    if v.size > 20:
        v[2, 3, 1] = np.nan                  # a non-finite corner: its stations are not sampled
        v[5, 1, 3] = np.inf
    return v


def volume_scales(v):
    """(scale, scale_sq) as bundle_profile.metric_scales chooses them."""
    import math
    a = np.abs(v[np.isfinite(v)].astype(np.float64))
    e = math.frexp(float(a.max()) if a.size and a.max() > 0 else 1.0)[1]
    return 2.0 ** (39 - e), 2.0 ** (39 - 2 * e)


def tie_rows(K):
    """(row, model line) built as an exact tie when K - 1 is a power of two: a
    straight row of K points along x at unit spacing (its stations are its
    points, exactly) against the model line that sits at the row's middle, 2
    voxels off in y: d(r_k, m) and d(r_{K-1-k}, m) are the same bits under an
    axis-aligned lin, station by station, so D == F in the kernel and in exact
    arithmetic."""
    if (K - 1) & (K - 2):
        return None
    row = np.zeros((K, 3), F32)
    row[:, 0] = np.arange(K) * (4.0 / (K - 1)) + 1.0       # dyadic spacing inside the volume
    row[:, 1:] = (2.5, 2.5)
    model = np.zeros((K, 3), F32)
    model[:] = (3.0, 4.5, 2.5)
    return row, model


@functools.lru_cache(maxsize=None)
def case(K, B, lin_name='oblique', seed=0, dims=DIMS, lengths=LENGTHS, repeat=2):
    """Rows of every length in ``lengths`` (``repeat`` of each) in random bundles,
    numbers -1 and B among them, plus the special rows: a NaN and an Inf at the
    LAST point, a row at 1e30, a row of identical points, a row whose last point
    alone fails the range gate (|r * scale| is exactly 2^40 there and below it before), and (axis-aligned lin, K - 1 a power of two) an
    exact tie in a bundle of its own model line.  The row of identical points is
    an exact tie as well: its D and F are the same terms in the same places."""
    rng = np.random.default_rng(1000 * K + 10 * B + seed)
    rows, bundle = [], []
    for length in lengths:
        for _ in range(repeat):
            rows.append(walk(rng, length, dims))
            bundle.append(int(rng.integers(0, B)))
    for bad in (-1, B):
        rows.append(walk(rng, 9, dims))
        bundle.append(bad)
    special = {}
    for name, value in (('nan', np.nan), ('inf', np.inf), ('gate', 2.0 ** 40 / COORD_SCALE)):
        r = walk(rng, 70, dims)
        r[-1, 2] = value
        special[name] = len(rows)
        rows.append(r)
        bundle.append(int(rng.integers(0, B)))
    special['far'] = len(rows)
    rows.append((walk(rng, 5, dims) + F32(1e30)).astype(F32))
    bundle.append(0)
    special['same'] = len(rows)
    rows.append(np.repeat(walk(rng, 1, dims), 4, 0))
    bundle.append(B - 1)
    model = np.stack([ref.resample_blocked(walk(rng, 40, dims, 0.5), K) for _ in range(B)])
    tie = tie_rows(K) if lin_name == 'axis' and B >= 2 else None
    if tie is not None:
        # bundle B - 1 becomes the tie's alone: against a model line that is one point,
        # every row would be a tie
        bundle = [0 if b == B - 1 else b for b in bundle]
        special['tie'] = len(rows)
        rows.append(tie[0])
        bundle.append(B - 1)
        model[B - 1] = tie[1]
    points, offsets = pack(rows)
    v = volume(rng, dims)
    scale_v, scale_sq = volume_scales(v)
    return {'points': points, 'offsets': offsets, 'bundle': np.asarray(bundle, np.int32),
            'model': model.astype(F32), 'lin': LINS[lin_name], 'scale': COORD_SCALE, 'volume': v,
            'scale_v': scale_v, 'scale_sq': scale_sq, 'B': B, 'K': K, 'special': special}


GPU_CASES = [(2, 1, 'axis'), (3, 2, 'axis'), (63, 2, 'anisotropic'), (64, 21, 'oblique'),
             (65, 64, 'axis'), (100, 21, 'anisotropic'), (128, 2, 'oblique'), (256, 21, 'oblique')]


@functools.lru_cache(maxsize=None)
def tiny_volume_case():
    """The 1 x 1 x 2 volume: every index clamps on x and y."""
    return case(65, 2, 'axis', seed=3, dims=(1, 1, 2), lengths=(2, 3, 65), repeat=3)


@functools.lru_cache(maxsize=None)
def reference(key):
    """orient and, with its flips, profile of a case, computed once."""
    c = tiny_volume_case() if key == 'tiny' else case(*key)
    o = ref.orient(c['points'], c['offsets'], c['bundle'], c['B'], c['K'], c['model'], c['lin'],
                   c['scale'])
    p = ref.profile(c['points'], c['offsets'], c['bundle'], o['flip'], c['B'], c['K'],
                    c['volume'], c['scale_v'], c['scale_sq'])
    return o, p


def periodic_case(K=65, B=3):
    """4 * GRID_WAVES + 3 rows of period 7: every wave takes several rows, reuses
    its LDS and carries its register sums across bundle changes (and across rows
    that take no part).  Returns (the 7 template rows' case, the full case)."""
    rng = np.random.default_rng(77)
    rows = [walk(rng, length) for length in (5, 2, 70, 9, 3, 130, 12)]
    rows[3][-1, 0] = np.nan
    bundle = np.array([0, 0, 1, 1, 1, -1, 2], np.int32)
    model = np.stack([ref.resample_blocked(walk(rng, 40, DIMS, 0.5), K) for _ in range(B)])
    v = volume(rng)
    scale_v, scale_sq = volume_scales(v)
    n = 4 * GRID_WAVES + 3
    pick = np.arange(n) % 7
    shared = {'model': model.astype(F32), 'lin': LINS['oblique'], 'scale': COORD_SCALE,
              'volume': v, 'scale_v': scale_v, 'scale_sq': scale_sq, 'B': B, 'K': K}
    p7, o7 = pack(rows)
    pn, on = pack([rows[i] for i in pick])
    return (dict(shared, points=p7, offsets=o7, bundle=bundle),
            dict(shared, points=pn, offsets=on, bundle=bundle[pick]), pick)


def witness():
    """The witness set of the named mutants: half-integer coordinates at scale 1
    and odd values at scale 1/2 (halves to round), an anisotropic lin under which a row is nearer
    the model reversed in mm but not in voxels, a tie, a row whose last station
    fails the gate, stations outside the volume, and a coarse metric scale."""
    K, B = 3, 3
    rows = [
        np.array([(1.5, 1.5, 1.5), (3.5, 1.5, 1.5), (5.5, 3.5, 1.5)], F32),  # 0: flips
        np.array([(5.5, 3.5, 1.5), (3.5, 1.5, 1.5), (1.5, 1.5, 1.5)], F32),  # 0: stays
        tie_rows(3)[0],                                                      # 1: the tie
        np.array([(1.5, 1.5, 1.5), (3.5, 1.5, 1.5), (5.5, 1.5, 2.0 ** 42)], F32),  # 0: the gate
        np.array([(0.5, 0.5, 0.5), (4.5, 0.5, 0.5), (4.5, 0.5, 1.5)], F32),  # 2: mm against voxels
        np.array([(1.5, 1.5, 1.5), (3.5, 3.5, 3.5), (9.5, 9.5, 9.5)], F32),  # 0: leaves the volume
    ]
    bundle = np.array([0, 0, 1, 0, 2, 0], np.int32)
    model = np.zeros((B, K, 3), F32)
    model[0] = rows[1]
    model[1] = tie_rows(3)[1]
    model[2] = [(3.9, 0, 1), (2, 0, 0.5), (0.1, 0, 0.1)]
    points, offsets = pack(rows)
    v = (2.0 * np.arange(7 * 6 * 5) + 1.0).astype(F32).reshape(DIMS)        # odd: halves at 1/2
    return {'points': points, 'offsets': offsets, 'bundle': bundle, 'model': model,
            'lin': np.diag([0.1, 1.0, 10.0]), 'scale': 1.0, 'volume': v, 'scale_v': 0.5,
            'scale_sq': 2.0 ** -3, 'B': B, 'K': K}
