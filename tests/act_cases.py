"""Cases of the ACT / CMC stopping criterion (ttl_act_flags; tests/ref_act.py),
small on purpose: three grids, dyadic map values, points on voxel centres, on
the faces of the sampled region and their float32 neighbours, non-finite and
huge points, permuted ids above 2^32, init_len around n_points -- and, for the
comparisons of the CMC draw, ids found by search whose u1 equals P exactly."""
import functools

import numpy as np

import ref_act

F32 = np.float32
GRIDS = ((1, 1, 1), (2, 3, 7), (5, 4, 3))
IDS_BASE = 2 ** 32 + 12345
N_SIZES = (0, 1, 63, 64, 65, 257, 1000)
HALF_UP = float(np.nextafter(F32(0.5), F32(1.0)))
#: what the maps hold: dyadic, so that sums and products on voxel centres are
#: exact; 0.5 and its float32 successor decide `>` against `>=`
LEVELS = np.array([0.0, 0.0, 0.125, 0.25, 0.5, HALF_UP, 0.75, 1.0], dtype=F32)


def _maps(dims, rng):
    inc = rng.choice(LEVELS, size=dims).astype(F32)
    exc = rng.choice(LEVELS, size=dims).astype(F32)
    flat_i, flat_e = inc.reshape(-1), exc.reshape(-1)
    if flat_i.size >= 8:
        # the rows the definition names: s = 0, s >= 1, include = 0, exclude = 0,
        # include == 0.5 exactly (under an exclude above 0.5), both above 0.5
        forced = [(0.0, 0.0), (1.0, 0.5), (0.0, 0.75), (0.75, 0.0), (0.5, HALF_UP),
                  (HALF_UP, 0.5), (0.75, 0.75), (0.25, 0.125)]
        at = rng.permutation(flat_i.size)[:len(forced)]
        for k, (a, b) in zip(at, forced):
            flat_i[k], flat_e[k] = a, b
    else:
        flat_i[:], flat_e[:] = 0.5, HALF_UP
    return inc, exc


def _neighbours(v):
    v = F32(v)
    return [float(np.nextafter(v, F32(-np.inf))), float(v), float(np.nextafter(v, F32(np.inf)))]


def _points(dims, shift, rng):
    """float32 points; ``shift`` (dyadic) is taken off so that x + shift lands
    where the case wants it."""
    dims = np.asarray(dims)
    pts = [np.array(c, dtype=np.float64) for c in np.ndindex(*dims)]        # voxel centres
    inner = lambda: rng.uniform(-0.5, dims - 0.5)                           # noqa: E731
    for c in range(3):
        for face in (-0.5, dims[c] - 0.5):
            for v in _neighbours(face):
                p = inner()
                p[c] = v
                pts.append(p)
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            p = inner()
            p[c] = v
            pts.append(p)
    pts += [inner() for _ in range(40)]
    pts = np.array(pts)
    # corners: every coordinate on a face at once
    pts = np.concatenate([pts, [np.full(3, -0.5), dims - 0.5, [-0.5, dims[1] - 0.5, -0.5]]])
    return (pts - shift).astype(F32)


def _case(name, dims, rng_seed, n_points=3, shift=0.0, exponent=0.75, seed=7):
    rng = np.random.RandomState(rng_seed)
    inc, exc = _maps(dims, rng)
    pts = _points(dims, shift, rng)
    rows = len(pts)
    # earlier points of a row are other rows' points: reading the wrong point shows
    history = np.empty((rows, n_points + 1, 3), dtype=F32)
    for j in range(n_points + 1):
        history[:, j] = np.roll(pts, n_points - 1 - j, axis=0)
    history[:, n_points - 1] = pts
    ids = rng.permutation(rows).astype(np.int32)
    init_len = (n_points - 1 + np.arange(rows) % 3).astype(np.int32)        # below, equal, above
    return dict(name=name, include=inc, exclude=exc, history=history, n_points=n_points,
                ids=ids, init_len=init_len, coord_shift=float(shift), exponent=float(exponent),
                seed=int(seed), ids_base=IDS_BASE)


@functools.lru_cache(maxsize=None)
def knife_ids(seed=7, n_points=3, want=3, span=1 << 19):
    """ids >= IDS_BASE + 8 whose u1 at (seed, n_points) is k / 256, 0 < k < 256:
    P = 1 - s takes such a value for dyadic maps with exponent 1."""
    ids = IDS_BASE + 8 + np.arange(span, dtype=np.int64)
    u1, _ = ref_act.uniforms(seed, ids, n_points)
    k = u1 * 256.0
    hit = np.nonzero((k == np.floor(k)) & (u1 > 0))[0][:want]
    return tuple((int(ids[h]), float(u1[h])) for h in hit)


def _knife_case(k, the_id, u1):
    """Eight rows on one voxel centre of a (2, 3, 7) grid whose maps make
    P = rho = u1 of row 3 exactly (exponent 1): include = exclude = (1 - u1) / 2."""
    dims, voxel, n_points, rows = (2, 3, 7), (1, 2, 4), 3, 8
    half = F32((1.0 - u1) / 2.0)
    assert float(half) * 2.0 == 1.0 - u1
    inc, exc = np.zeros(dims, F32), np.zeros(dims, F32)
    inc[voxel] = exc[voxel] = half
    history = np.zeros((rows, n_points + 1, 3), dtype=F32)
    history[:, n_points - 1] = voxel
    return dict(name=f'knife{k}', include=inc, exclude=exc, history=history, n_points=n_points,
                ids=np.arange(rows, dtype=np.int32), init_len=np.zeros(rows, np.int32),
                coord_shift=0.0, exponent=1.0, seed=7, ids_base=the_id - 3, knife_row=3)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_case('g111', GRIDS[0], 1), _case('g237', GRIDS[1], 2, n_points=4),
           _case('g543', GRIDS[2], 3, exponent=1.5, seed=2 ** 63 + 11),
           _case('g237_shift', GRIDS[1], 4, shift=0.25),
           _case('g543_exp1', GRIDS[2], 5, exponent=1.0, n_points=1)]
    found = knife_ids()
    assert len(found) >= 2, 'the id search found no u1 on a multiple of 1/256'
    out += [_knife_case(k, i, u) for k, (i, u) in enumerate(found)]
    return tuple(out)


def flags_of(case, mode, n=None, use_ids=True, use_init_len=True, mutate=None, **kw):
    """``ref_act.act_flags_ordered`` on a case; ``n`` rows, the ids repeated."""
    ids = case['ids'] if use_ids else None
    if n is not None:
        ids = np.resize(case['ids'] if use_ids else np.arange(len(case['history']), dtype=np.int32),
                        n).astype(np.int32)
    return ref_act.act_flags_ordered(
        case['include'], case['exclude'], case['history'], case['n_points'], mode, ids=ids,
        init_len=case['init_len'] if use_init_len else None, coord_shift=case['coord_shift'],
        exponent=case['exponent'], seed=case['seed'], ids_base=case['ids_base'], mutate=mutate,
        **kw)


# hand cases: literal flags -------------------------------------------------
def hand_cases():
    """(case dict, mode, expected flags) with the expectation worked out by hand."""
    nan = np.nan
    one = dict(include=np.full((1, 1, 1), 0.5, F32), exclude=np.full((1, 1, 1), HALF_UP, F32),
               n_points=1, ids=None, init_len=None, coord_shift=0.0, exponent=1.0, seed=0,
               ids_base=0)
    # one voxel, include exactly 0.5 (not a target), exclude just above: the whole
    # region [-0.5, 0.5) reads the voxel's value, its far face is outside
    pts = np.array([[0, 0, 0], [-0.5, 0, 0], [0.25, -0.5, 0.49], [0.5, 0, 0], [0, 0, -0.51],
                    [nan, 0, 0], [0, np.inf, 0]], dtype=F32)
    a = dict(one, name='hand_one_voxel', history=pts[:, None, :].copy())
    want_a = np.array([128, 128, 128, 0, 0, 0, 0], np.uint8)
    # two voxels along x: include (1, 0), exclude (0, 1); third point of each row
    inc = np.array([1, 0], F32).reshape(2, 1, 1)
    exc = np.array([0, 1], F32).reshape(2, 1, 1)
    xs = [0.0, 1.0, 0.5, 0.25, 0.75, 0.0, 0.0]
    hist = np.zeros((len(xs), 3, 3), F32)
    hist[:, 0, 0] = 1.0              # an older point that would read EXCLUDE
    hist[:, 2, 0] = xs
    init_len = np.array([0, 0, 0, 0, 0, 3, 4], np.int32)      # rows 5, 6: not judged
    b = dict(one, name='hand_two_voxels', include=inc, exclude=exc, history=hist, n_points=3,
             init_len=init_len)
    want_b = np.array([8, 128, 0, 8, 128, 0, 0], np.uint8)
    # CMC on the same maps: s = 1 everywhere between the centres, so every judged
    # row stops; include / s = 1 at x = 0 (u2 < 1: TARGET), 0 at x = 1 (EXCLUDE)
    c = dict(b, name='hand_cmc', history=hist[[0, 1, 5]].copy(), init_len=init_len[[0, 1, 5]])
    want_c = np.array([8, 128, 0], np.uint8)
    return ((a, ref_act.THRESHOLD, want_a), (b, ref_act.THRESHOLD, want_b),
            (c, ref_act.CMC, want_c))
