"""Case sets of tests/test_connectome_metric.py: a scalar volume, a ``lin`` and
ragged rows whose points stand where ttl_tract_sample_mean can go wrong (voxel
centres, the faces of the volume and one ulp beyond them, -0.3, 1e30, NaN), at
the row lengths where its rounds of 64 lanes begin and end."""
import functools

import numpy as np

import ref_connectome_metric as ref

F32 = np.float32
ROW_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 1000)

LINS = {
    'axis': np.array([[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.5]]),
    # a rotation about (1, 2, 3) times the voxel sizes (1.25, 1, 2), sheared a little
    'oblique': np.array([[1.1204, -0.4357, 0.6169], [0.5411, 0.8820, -0.1083],
                         [-0.3042, 0.1794, 1.8943]]),
}
BOX, ONE, SLAB = (5, 6, 7), (1, 1, 1), (4, 1, 3)
LINEAR = (0.5, -0.25, 2.0)              # a x + b y + c z: exact in float32 on the box

# name: (dims, what the volume holds)
VOLUMES = {
    'constant': (BOX, 'constant'),
    'linear': (BOX, 'linear'),
    'normal': (BOX, 'normal'),
    'holes': (BOX, 'holes'),
    'small': (BOX, 'small'),
    'large': (BOX, 'large'),
    'one': (ONE, 'normal'),
    'slab': (SLAB, 'normal'),
}
SETS = {f'{v}_{lin}': (v, lin) for v in VOLUMES for lin in LINS}
CONSTANT = 0.7


def volume_of(name):
    dims, kind = VOLUMES[name]
    rng = np.random.RandomState(sorted(VOLUMES).index(name))
    if kind == 'constant':
        return np.full(dims, CONSTANT, F32)
    if kind == 'linear':
        x, y, z = np.indices(dims).astype(np.float64)
        v = LINEAR[0] * x + LINEAR[1] * y + LINEAR[2] * z
        assert np.array_equal(v.astype(F32), v)
        return v.astype(F32)
    v = rng.standard_normal(dims).astype(F32)
    if kind == 'holes':                 # a NaN block and a +Inf voxel
        v[3:, 4:, 5:] = np.nan
        v[0, 0, 3] = np.inf
    if kind == 'small':
        v *= F32(1e-3)
    if kind == 'large':
        v *= F32(1e4)
    return v


def special_points(dims):
    """Where the definition decides: voxel centres (f = 0), the faces 0 and
    dims_k (inside), one ulp beyond them (outside), -0.3, 1e30."""
    d = np.array(dims, F32)
    beyond_hi = np.nextafter(d, F32(np.inf))
    beyond_lo = np.nextafter(F32(0), F32(-1))
    mid = (d / 2).astype(F32)
    pts = [np.floor(mid) + F32(0.5),                        # a voxel centre
           np.array([0.5, 0.5, 0.5], F32), d - F32(0.5),    # the first and last centres
           np.zeros(3, F32), d.copy(),                      # the corners of the closed volume
           np.array([0.0, mid[1], mid[2]], F32), np.array([mid[0], d[1], mid[2]], F32),
           np.array([mid[0], mid[1], d[2]], F32),
           np.array([0.25, 0.25, 0.25], F32), d - F32(0.125),   # inside the border half voxel
           np.array([beyond_lo, mid[1], mid[2]], F32),
           np.array([mid[0], beyond_hi[1], mid[2]], F32),
           np.array([mid[0], mid[1], beyond_hi[2]], F32),
           np.array([-0.3, mid[1], mid[2]], F32), np.array([mid[0], mid[1], -0.3], F32),
           np.array([1e30, mid[1], mid[2]], F32), np.array([mid[0], -1e30, mid[2]], F32)]
    return [p.astype(F32) for p in pts]


def _inside(rng, dims, L, margin=0.0):
    return np.stack([rng.uniform(margin, d - margin, L) for d in dims], axis=1).astype(F32)


def _rows(dims, seed):
    rng = np.random.RandomState(seed)
    special = special_points(dims)
    rows = [_inside(rng, dims, L) for L in ROW_LENGTHS]
    # the special points, spread over rows that cross a round of 64 lanes
    for L in (3, 66, 129):
        row = _inside(rng, dims, L)
        for k, p in enumerate(special):
            row[(7 * k + 1) % L] = p
        rows.append(row)
    # a NaN (an Inf) in the first, a middle and the last position
    for L, at, bad in ((5, 0, np.nan), (5, 2, np.nan), (5, 4, np.nan), (130, 0, np.nan),
                       (130, 64, np.inf), (130, 63, np.nan), (130, 129, np.nan),
                       (2, 0, np.nan), (2, 1, -np.inf)):
        row = _inside(rng, dims, L)
        row[at, at % 3] = bad
        rows.append(row)
    rows.append(np.tile(_inside(rng, dims, 1), (4, 1)))             # identical points
    rows.append(np.tile(_inside(rng, dims, 1), (70, 1)))
    outside = np.array(dims, F32) + F32(2.0)
    # one sampled point between outside ones: in 'holes' it touches the NaN block
    touch = (np.array(dims, F32) - F32(1.25)).astype(F32)
    rows.append(np.stack([outside, touch, -outside]))
    rows.append(np.stack([outside, outside + F32(1.0), outside]))   # nothing sampled
    rows.append(np.stack([special[0], np.array([1e30, 1.0, 1.0], F32), special[1]]))
    rows.append(np.stack([special[3], special[4]]))                 # corner to corner
    return rows


class Case:
    """One set: volume (X, Y, Z) float32, lin, the ragged rows."""


@functools.lru_cache(maxsize=None)
def case(name):
    vol, lin = SETS[name]
    c = Case()
    c.name, c.volume_name, c.volume, c.lin = name, vol, volume_of(vol), LINS[lin].copy()
    c.dims = c.volume.shape
    c.rows = _rows(c.dims, 300 + sorted(VOLUMES).index(vol))
    c.offsets = np.zeros(len(c.rows) + 1, np.int64)
    np.cumsum([len(r) for r in c.rows], out=c.offsets[1:])
    c.points = np.concatenate(c.rows).astype(F32)
    c.volume.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name, mutant=None):
    """(mean, weight, bound_mean, bound_weight) of the definition, longdouble,
    once per set and mutant."""
    c = case(name)
    out = ref.sample_mean(c.points, c.offsets, c.volume, c.lin, mutant)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def interior_rows(name):
    """Rows whose points lie half a voxel and more inside the box, where the
    trilinear sample of 'linear' is a (x - 0.5) + b (y - 0.5) + c (z - 0.5)."""
    c = case(name)
    rng = np.random.RandomState(77)
    rows = [_inside(rng, c.dims, L, margin=0.5) for L in (2, 3, 64, 65, 200)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.concatenate(rows), offsets


def analytic_means(name):
    """The longdouble means of ``interior_rows`` from the analytic value."""
    c = case(name)
    points, offsets = interior_rows(name)
    out = []
    for s in range(len(offsets) - 1):
        row = points[offsets[s]:offsets[s + 1]]
        p = row.astype(ref.LD) - ref.LD(0.5)
        values = LINEAR[0] * p[:, 0] + LINEAR[1] * p[:, 1] + LINEAR[2] * p[:, 2]
        out.append(ref.weighted_mean(ref.point_weights(row, c.lin), values,
                                     np.ones(len(row), bool))[0])
    return np.array(out, ref.LD)


def many_rows(name, n):
    """n two- and three-point rows that cycle through a pool of 97 (more rows than
    one launch has wavefronts): (points, offsets, mean, weight, bounds) with the
    definition evaluated once per pool row."""
    c = case(name)
    rng = np.random.RandomState(5)
    pool = [_inside(rng, c.dims, 2 + k % 2) for k in range(97)]
    pool[3][1] = np.array(c.dims, F32) + F32(1.0)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in pool])]).astype(np.int64)
    want = ref.sample_mean(np.concatenate(pool), offsets, c.volume, c.lin)
    pick = np.arange(n) % len(pool)
    rows = [pool[k] for k in pick]
    all_offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return (np.concatenate(rows), all_offsets) + tuple(w[pick] for w in want)


def differs(name, mutant):
    """The rows of the set on which ``mutant`` is told from the definition: the
    NaN decision differs, or the mean (the weight) lies further from the
    definition's than twice the bound a kernel is held to."""
    mean, weight, b_mean, b_weight = expected(name)
    m_mean, m_weight, _, _ = expected(name, mutant)
    nan, m_nan = np.isnan(mean), np.isnan(m_mean)
    both = ~nan & ~m_nan
    far = np.zeros(len(mean), bool)
    far[both] = (np.abs(m_mean[both] - mean[both]) > 2 * b_mean[both]) | \
        (np.abs(m_weight[both] - weight[both]) > 2 * b_weight[both])
    return np.flatnonzero((nan != m_nan) | far)
