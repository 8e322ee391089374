"""The case set of tests/test_coverage_reference.py (test infrastructure only),
shared by its CPU and GPU tests: seeded, deterministic, float32 before
anything looks at it.

Segment cases: ``segment_cases(dims)`` -> {class: (A, B)} with A, B (n, 3)
float32, for each volume of VOLUMES (the per-segment GPU launches) and for
RAGGED_VOLUME (each class once more as one ragged tractogram).  Row cases:
``row_cases()`` (streamline lengths, empty rows, non-finite points, the score
gate) and ``grid_batch()`` (40 000 short rows, a handful accepted)."""
import functools

import numpy as np

import ref_oracle_validator as ref

VOLUMES = ((5, 6, 7), (1, 1, 9), (2, 3, 1), (8, 1, 8))
RAGGED_VOLUME = (23, 9, 40)
ROW_VOLUME = (16, 17, 18)
GRID_VOLUME = (9, 17, 33)
PER_CLASS = 240                 # x 10 classes = 2 400 launches per volume
CLASSES = ('inside', 'through', 'far_near', 'far_far', 'lattice', 'diagonal', 'axis', 'faces',
           'grazing', 'huge')


# ------------------------------------------------------------ segment classes
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _chord(rng, D, n):
    """Per case two points of the volume (the second the farthest, in voxels,
    of three uniform candidates) and the unit vector from the first to the
    second: a line aimed through the volume along a long chord."""
    q1 = rng.uniform(0, D, (n, 3))
    cand = rng.uniform(0, D, (3, n, 3))
    dist = np.abs(np.floor(cand) - np.floor(q1)).sum(-1)
    q2 = cand[dist.argmax(0), np.arange(n)]
    v = q2 - q1
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return q1, q2, v


def _inside(rng, D, n):
    q1, q2, _ = _chord(rng, D, n)
    return q1, q2


def _through(rng, D, n):
    """Ends uniform in [-6, dim + 6); every other case aimed along a chord of
    the volume, its ends up to 6 voxels beyond the chord's."""
    a, b = rng.uniform(-6, D + 6, (n, 3)), rng.uniform(-6, D + 6, (n, 3))
    q1, q2, v = _chord(rng, D, n)
    aim = np.arange(n) % 2 == 0
    a[aim] = (q1 - v * rng.uniform(0, 6, (n, 1)))[aim]
    b[aim] = (q2 + v * rng.uniform(0, 6, (n, 1)))[aim]
    return a, b


def _far_near(rng, D, n):
    """One end 50-300 voxels out on a random non-empty subset of axes, the
    other within 2 voxels of the volume; every other case along a chord."""
    b = rng.uniform(-2, D + 2, (n, 3))
    a = rng.uniform(-2, D + 2, (n, 3))
    subset = rng.random((n, 3)) < 0.5
    subset[np.arange(n), rng.integers(0, 3, n)] = True
    out = rng.uniform(50, 300, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    a = np.where(subset, np.where(out > 0, D + out, out), a)
    q1, q2, v = _chord(rng, D, n)
    aim = np.arange(n) % 2 == 0
    a[aim] = (q1 - v * rng.uniform(50, 300, (n, 1)))[aim]
    b[aim] = (q2 + v * rng.uniform(0, 2, (n, 1)))[aim]
    return a, b


def _far_far(rng, D, n):
    """Through a point of the volume with 50-300 voxels on each side: any
    direction, every other case along a chord."""
    q1, q2, v = _chord(rng, D, n)
    free = np.arange(n) % 2 == 1
    v[free] = _unit(rng, n)[free]
    q2[free] = q1[free]
    return q1 - v * rng.uniform(50, 300, (n, 1)), q2 + v * rng.uniform(50, 300, (n, 1))


def _lattice(rng, D, n):
    a, b = _through(rng, D, n)
    return (np.floor(a) + rng.choice([0.0, 0.5], (n, 3)),
            np.floor(b) + rng.choice([0.0, 0.5], (n, 3)))


def _diagonal(rng, D, n):
    """a on the lattice within one voxel of the volume, b = a + s k with s in
    {-1, 0, 1}^3 (not all zero), k in 1 .. 8.  s_i = 0 with probability
    max(1/3, 1 - dim_i / 4): a diagonal that moves along an axis of extent 1
    or 2 leaves the volume at once.  A moving axis starts just outside on the
    side it enters from (index -1 ascending, dim descending) in three cases of
    four where dim_i < 4 and one of four elsewhere -- a short axis is crossed
    whole only from outside -- and otherwise, like a fixed axis, inside in
    three cases of four and anywhere in [-1, dim + 1] in the fourth."""
    s = rng.choice([-1.0, 1.0], (n, 3)) * (rng.random((n, 3)) >= np.maximum(1 / 3, 1 - D / 4))
    zero = ~s.any(1)
    s[zero, D.argmax()] = 1.0
    a = np.floor(np.where(rng.random((n, 3)) < 0.75, rng.uniform(0, D, (n, 3)),
                          rng.uniform(-1, D + 2, (n, 3))))
    enter = (s != 0) & (rng.random((n, 3)) < np.where(D < 4, 0.75, 0.25))
    a = np.where(enter, np.where(s > 0, -1.0, D), a)
    return a, a + s * rng.integers(1, 9, (n, 1))


def _axis(rng, D, n):
    """Axis-aligned.  The moving axis is drawn with weights dim_i (a longer
    axis has more planes to order).  In two cases of three the moving
    coordinate starts up to one voxel outside and runs inwards over dim / 2 to
    dim + 2 voxels, since a short axis is crossed whole only from outside; in
    the third it starts anywhere within one voxel of the volume and runs 0.5
    to dim + 2 voxels either way.  The fixed coordinates lie inside in three
    of four cases, on the (half-)lattice in one of four."""
    ax = rng.choice(3, n, p=D / D.sum())
    a = rng.uniform(-1, D + 1, (n, 3))
    ins = rng.uniform(0, D, (n, 3))
    keep = rng.random((n, 3)) < 0.75
    a = np.where(keep, ins, a)
    snap = np.floor(a) + rng.choice([0.0, 0.5], (n, 3))
    a = np.where(rng.random((n, 1)) < 0.25, snap, a)
    rows = np.arange(n)
    Da = D[ax]
    side = rng.choice([-1.0, 1.0], n)                 # -1: from below 0, +1: from above dim
    out = np.where(side < 0, -rng.uniform(0, 1, n), Da + rng.uniform(0, 1, n))
    enter = rng.random(n) < 2 / 3
    a[rows, ax] = np.where(enter, out, rng.uniform(-1, Da + 1))
    b = a.copy()
    b[rows, ax] += np.where(enter, -side * rng.uniform(Da / 2, Da + 2),
                            rng.uniform(0.5, Da + 2) * rng.choice([-1.0, 1.0], n))
    return a, b


def _faces(rng, D, n):
    """One end on a face x_i in {0, dim_i} (a second coordinate there too in
    one case of sixteen); the other end inside or uniform in [-6, dim + 6)."""
    a = rng.uniform(0, D, (n, 3))
    rows = np.arange(n)
    ax = rng.integers(0, 3, n)
    a[rows, ax] = rng.choice([0.0, 1.0], n) * D[ax]
    ax2 = (ax + rng.integers(1, 3, n)) % 3            # one of the two axes that remain
    sel = rng.random(n) < 1 / 16
    a[rows[sel], ax2[sel]] = (rng.choice([0.0, 1.0], n) * D[ax2])[sel]
    b = np.where(rng.random((n, 1)) < 0.5, rng.uniform(0, D, (n, 3)),
                 rng.uniform(-6, D + 6, (n, 3)))
    return a, b


def _grazing(rng, D, n):
    """Past a lattice point P of [0, dim]^3 from 9-300 voxels away on both
    sides (one component of the direction zero in every other case),
    displaced by a few float32 ulps of the largest extent: the crossings of
    two axes near P sit ~1e-9 apart in t, which float64 orders and float32
    does not."""
    P = np.floor(rng.uniform(0, D + 1, (n, 3)))
    v = rng.normal(size=(n, 3)) * D       # the volume's aspect: stays inside over several voxels
    zero = rng.random(n) < 0.5
    v[zero, rng.integers(0, 3, zero.sum())] = 0.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = rng.uniform(30, 300, (n, 1))
    delta = rng.integers(-2, 3, (n, 3)) * float(np.spacing(np.float32(D.max())))
    return (P - v * f * rng.uniform(0.3, 1, (n, 1)) + delta,
            P + v * f * rng.uniform(0.3, 1, (n, 1)) + delta)


def _huge(rng, D, n):
    """Ends inside, then one end (two cases of three) or both offset by
    +-10^[3, 38] on a non-empty subset of axes.  One axis, drawn with weights
    dim_i, is always in the subset, and alone in it in every other case (two
    offsets of unlike size make an axis-aligned segment anyway; along a long
    axis it has the most planes to order); the others join with probability
    1/2.  In three cases of four every offset points to the side of the volume
    opposite the other end, so the segment crosses the volume whole between
    them."""
    a, b = _inside(rng, D, n)
    a0, b0 = a.copy(), b.copy()
    for end, other, sel in ((a, b0, np.arange(n) % 3 != 1), (b, a0, np.arange(n) % 3 == 1),
                            (b, a0, np.arange(n) % 3 == 2)):
        subset = (rng.random((n, 3)) < 0.5) & (rng.random((n, 1)) < 0.5)
        subset[np.arange(n), rng.choice(3, n, p=D / D.sum())] = True
        across = np.where(other < D / 2, 1.0, -1.0)   # beyond the face farther from the other end
        sign = np.where(rng.random((n, 1)) < 0.75, across, rng.choice([-1.0, 1.0], (n, 3)))
        off = 10.0 ** rng.uniform(3, 38, (n, 3)) * sign
        end += np.where(subset & sel[:, None], off, 0.0)
    return a, b


_GENERATORS = {'inside': _inside, 'through': _through, 'far_near': _far_near,
               'far_far': _far_far, 'lattice': _lattice, 'diagonal': _diagonal, 'axis': _axis,
               'faces': _faces, 'grazing': _grazing, 'huge': _huge}


@functools.lru_cache(maxsize=None)
def segment_cases(dims, n=PER_CLASS):
    """{class: (A, B)}: n segments of every class for the volume ``dims``,
    either end first with equal chance."""
    D = np.array(dims, np.float64)
    out = {}
    for k, name in enumerate(CLASSES):
        rng = np.random.default_rng([20, k, *dims])
        a, b = _GENERATORS[name](rng, D, n)
        swap = rng.random((n, 1)) < 0.5
        a, b = np.where(swap, b, a), np.where(swap, a, b)
        out[name] = (a.astype(np.float32), b.astype(np.float32))
    return out


def first_voxel(p, dims):
    """What the first point of a streamline marks: {floor(p)} when finite and
    inside, else nothing."""
    p = np.asarray(p, np.float32).astype(np.float64)
    if not np.isfinite(p).all():
        return set()
    v = tuple(int(x) for x in np.floor(p))
    return {v} if all(0 <= v[i] < dims[i] for i in range(3)) else set()


@functools.lru_cache(maxsize=None)
def segment_walks(dims):
    """{class: [voxel list of every segment]} by ``walk_segment_planes``, the
    definition that holds at any magnitude."""
    return {name: [ref.walk_segment_planes(a, b, dims) for a, b in zip(A, B)]
            for name, (A, B) in segment_cases(dims).items()}


def ragged_from_segments(A, B, seed):
    """One ragged tractogram from the segments of a class: runs of 1-130
    segments concatenated into streamlines (a0 b0 a1 b1 ...), so the jump from
    one case to the next is one more segment."""
    rng = np.random.default_rng([21, seed])
    lines, k = [], 0
    while k < len(A):
        run = int(rng.integers(1, 131))
        lines.append(np.stack([A[k:k + run], B[k:k + run]], 1).reshape(-1, 3))
        k += run
    return lines


# ------------------------------------------------------------------ row cases
def _walk(rng, L, dims, step=(0.2, 2.5)):
    """A random walk of L points starting in the middle half of the volume,
    steps of 0.2-2.5 voxels, folded back at one voxel outside the volume so
    that long rows keep marking."""
    D = np.array(dims, np.float64)
    if L == 0:
        return np.zeros((0, 3), np.float32)
    d = _unit(rng, L - 1) * rng.uniform(step[0], step[1], (L - 1, 1)) if L > 1 else \
        np.zeros((0, 3))
    p = np.concatenate([rng.uniform(D / 4, 3 * D / 4, (1, 3)), d]).cumsum(0)
    period = 2 * (D + 2)
    p = np.abs((p + 1) % period - (D + 2)) * -1 + (D + 2) - 1    # triangle wave in [-1, D + 1]
    return p.astype(np.float32)


def pack(lines):
    offsets = np.zeros(len(lines) + 1, np.int64)
    np.cumsum([len(s) for s in lines], out=offsets[1:])
    points = np.concatenate([np.zeros((0, 3), np.float32)] + list(lines)).astype(np.float32)
    return points.reshape(-1, 3), offsets


LENGTHS = (0, 1, 2, 3, 64, 65, 66, 129, 130)


@functools.lru_cache(maxsize=None)
def row_cases():
    """[(name, dims, points, offsets, scores or None, threshold)].  The seed
    and value counts below are sized by the floor of 5 witnesses per row
    mutant (test_every_mutant_has_witnesses): one launch per seed or value
    witnesses score_ge, nan_score_accepted, first_point_clamped and
    nonfinite_point_ends_row, six each; trimming them trips that test."""
    dims = ROW_VOLUME
    D = np.array(dims, np.float64)
    out = []
    empty = np.zeros((0, 3), np.float32)
    # every length, empty rows between full ones, one-point rows outside the volume
    for seed in range(6):
        rng = np.random.default_rng([22, seed])
        lines = []
        for L in rng.permutation(LENGTHS):
            lines += [_walk(rng, int(L), dims), empty]
        for _ in range(3):
            p = rng.uniform(-3, D + 3, (1, 3))
            ax = rng.integers(0, 3)
            p[0, ax] = rng.choice([-0.5, D[ax] + 0.5])
            lines.append(p.astype(np.float32))
        out.append((f'lengths{seed}', dims, *pack(lines), None, 0.5))
    # NaN, +Inf, -Inf as the first, a middle and the last point
    for vi, val in enumerate((np.nan, np.inf, -np.inf)):
        for where in ('first', 'middle', 'last'):
            rng = np.random.default_rng([23, vi, len(where)])
            lines = [_walk(rng, int(L), dims) for L in (9, 2, 3, 70, 12)]
            for ln in lines:
                j = {'first': 0, 'middle': len(ln) // 2, 'last': len(ln) - 1}[where]
                ln[j, rng.integers(0, 3)] = val
            lines[-1][{'first': 0, 'middle': 6, 'last': 11}[where]] = val   # all three
            out.append((f'{where}_{val}', dims, *pack(lines), None, 0.5))
    # the score gate: threshold, its neighbours, NaN, +-Inf, -0.0
    for thr in (0.5, 0.0):
        for seed in range(3):
            rng = np.random.default_rng([24, seed])
            t = np.float32(thr)
            up, down = np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))
            scores = np.array([t, up, down, np.nan, np.inf, -np.inf, -0.0, 1.0, t, np.nan, 0.25,
                               up, down], np.float32)
            lines = [_walk(rng, int(rng.integers(1, 9)), dims, step=(0.2, 1.0))
                     for _ in scores]
            order = rng.permutation(len(scores))
            out.append((f'scores{seed}_thr{thr}', dims, *pack(lines), scores[order], thr))
            out.append((f'noscores{seed}_thr{thr}', dims, *pack(lines), None, thr))
    return out


GRID_ACCEPTED = (0, 1, 4095, 32767, 32768, 32769, 33000, 35001, 36864, 38002, 39998, 39999)


@functools.lru_cache(maxsize=None)
def grid_batch():
    """40 000 rows of 2-4 points in GRID_VOLUME, of which only GRID_ACCEPTED
    score above 0.5: rows on both sides of the largest grid's 32 768 waves,
    and a union sparse enough that a lost row shows.
    (dims, points, offsets, scores)."""
    rng = np.random.default_rng(25)
    n = 40000
    D = np.array(GRID_VOLUME, np.float64)
    lens = rng.integers(2, 5, n)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    start = rng.uniform(0, D, (n, 3))
    pts = np.repeat(start, lens, 0)
    pts += rng.uniform(-1.5, 1.5, pts.shape)
    scores = rng.uniform(0.0, 0.5, n).astype(np.float32)
    scores[list(GRID_ACCEPTED)] = rng.uniform(0.6, 1.0, len(GRID_ACCEPTED))
    return GRID_VOLUME, pts.astype(np.float32), offsets, scores
