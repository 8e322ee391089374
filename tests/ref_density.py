"""The track density maps' definition (include/ttl_hip.h, ttl_tract_density),
three ways (test infrastructure only):

(a) ``segment_pieces_planes``: the definition as events over the planes
    0 .. dims_i, the style of ``walk_segment_planes``: sorted crossings cut
    [0, 1] into pieces, a piece exists when the voxel occupied is inside;
(b) ``segment_pieces``: an ordered float64 restatement of the kernel's bounded
    walk (entry E, exit X, binary search), which the kernel must equal bit for
    bit: Python floats are IEEE float64, every expression is in the header's
    order, and the library is built with -ffp-contract=off;
(c) ``segment_pieces_exact``: the pieces in exact arithmetic
    (``fractions.Fraction``), the yardstick of the header's derived bound.

``density`` adds the rows of a ragged tractogram into the four maps and
predicts every row's status.  ``mutant`` names one deliberate misreading; the
tests show witnesses for each inside the sets the GPU tests launch."""
import collections
import math
from fractions import Fraction

import numpy as np

import ref_oracle_validator as walk

LENGTH_SCALE = 1048576.0
MAX_LENGTH = 2.0 ** 40
U = 2.0 ** -53

MUTANTS = ('no_dedupe', 'dedupe_consecutive_only', 'chord_to_entered_voxel',
           'last_piece_dropped', 'first_piece_from_0_when_outside', 'exit_piece_to_1',
           'length_in_voxels', 'ends_first_only', 'nonfinite_row_partly_added',
           'count_partial_on_overflow')


def _f64(p):
    """Three Python floats (IEEE float64) of a float32 point; a list is one already."""
    if type(p) is list:
        return p
    return np.asarray(p, np.float32).astype(np.float64).tolist()


def _inside(v, dims):
    return all(0 <= v[i] < dims[i] for i in range(3))


def _floor_voxel(p):
    return tuple(int(math.floor(v)) for v in p)


# ------------------------------------------------------------- (a) the planes
def segment_pieces_planes(a, b, dims):
    """[(voxel, t_lo, t_hi)] of segment a -> b (finite ends), in order."""
    a, b = _f64(a), _f64(b)
    d = [b[i] - a[i] for i in range(3)]
    idx = list(_floor_voxel(a))
    vb = _floor_voxel(b)
    events = []
    for i in range(3):
        if vb[i] > idx[i]:
            planes = range(max(idx[i] + 1, 0), min(vb[i], dims[i]) + 1)
            events += [((float(beta) - a[i]) / d[i], i, k, beta) for k, beta in enumerate(planes)]
        elif vb[i] < idx[i]:
            planes = range(min(idx[i], dims[i]), max(vb[i] + 1, 0) - 1, -1)
            events += [((float(beta) - a[i]) / d[i], i, k, beta - 1)
                       for k, beta in enumerate(planes)]
    events.sort()
    out, t_lo = [], 0.0
    for t, i, _, after in events:
        if _inside(idx, dims):
            out.append((tuple(idx), t_lo, t))
        idx[i] = after
        t_lo = t
    if _inside(idx, dims):
        out.append((tuple(idx), t_lo, 1.0))
    return out


# ------------------------------------------------------- (b) the bounded walk
def _bounded_walk(a, b, dims):
    """The kernel's walk (walk_segment_pieces, ttl_internal.h), statement for
    statement: ([(voxel, t of the crossing that enters it)], t at which the
    last one is left: X's, or 1)."""
    before = walk._before
    d = [b[i] - a[i] for i in range(3)]

    def tof(plane, i):
        return (float(plane) - a[i]) / d[i]
    idx, cur, left, step = [0] * 3, [0] * 3, [0] * 3, [0] * 3
    et, eax, xt, xax = -math.inf, -1, math.inf, 3
    for i in range(3):
        dim = dims[i]
        va = int(min(max(math.floor(a[i]), -1.0), float(dim)))
        vb = int(min(max(math.floor(b[i]), -1.0), float(dim)))
        inside = 0 <= va < dim
        idx[i] = va
        if va == vb:
            if not inside:
                return [], 1.0
            continue
        exit_plane = None
        if vb > va:
            step[i], first, last = 1, max(va + 1, 0), min(vb, dim - 1)
            if vb >= dim:
                exit_plane = dim
        else:
            step[i], first, last = -1, min(va, dim), max(vb + 1, 1)
            if vb < 0:
                exit_plane = 0
        left[i] = max((last - first) * step[i] + 1, 0)
        cur[i] = first
        if not inside:
            if left[i] == 0:
                return [], 1.0
            t = tof(first, i)
            if before(et, eax, t, i):
                et, eax = t, i
        if exit_plane is not None:
            t = tof(exit_plane, i)
            if before(t, i, xt, xax):
                xt, xax = t, i
    if eax >= 0:
        for i in range(3):
            if left[i] == 0:
                continue
            lo, hi = 0, left[i]
            while lo < hi:
                mid = (lo + hi) >> 1
                if before(tof(cur[i] + mid * step[i], i), i, et, eax):
                    lo = mid + 1
                else:
                    hi = mid
            if lo > 0:
                plane = cur[i] + (lo - 1) * step[i]
                idx[i] = plane if step[i] > 0 else plane - 1
                cur[i] += lo * step[i]
                left[i] -= lo
    tn = [tof(cur[i], i) if left[i] else 0.0 for i in range(3)]
    visits = []
    while True:
        m = -1
        for i in range(3):
            if left[i] and (m < 0 or before(tn[i], i, tn[m], m)):
                m = i
        if m < 0 or before(xt, xax, tn[m], m):
            break
        idx[m] = cur[m] if step[m] > 0 else cur[m] - 1
        if _inside(idx, dims):
            visits.append((tuple(idx), tn[m]))
        cur[m] += step[m]
        left[m] -= 1
        if left[m]:
            tn[m] = tof(cur[m], m)
    return visits, (xt if xax < 3 else 1.0)


def segment_pieces(a, b, dims, mutant=None, walked=None):
    """[(voxel, t_lo, t_hi)] as the kernel forms them: floor(a)'s piece from 0
    when a lies inside, every visited voxel from its crossing's t to the next
    visit's, the last to X's t or 1.  ``walked``: ``_bounded_walk``'s result,
    when the caller has it."""
    a, b = _f64(a), _f64(b)
    visits, t_end = walked or _bounded_walk(a, b, dims)
    if mutant == 'exit_piece_to_1':
        t_end = 1.0
    out = []
    first = _floor_voxel(a)
    opened = [(first, 0.0)] if _inside(first, dims) else []
    if mutant == 'first_piece_from_0_when_outside' and not opened and visits:
        visits = [(visits[0][0], 0.0)] + visits[1:]
    opened += visits
    for k, (vox, t_lo) in enumerate(opened):
        last = k + 1 == len(opened)
        t_hi = t_end if last else opened[k + 1][1]
        if last and mutant == 'last_piece_dropped':
            break
        if mutant == 'chord_to_entered_voxel' and not last:
            vox = opened[k + 1][0]
        out.append((vox, t_lo, t_hi))
    return out


# ------------------------------------------------------- (c) exact arithmetic
def segment_pieces_exact(a, b, dims):
    """[(voxel, exact t_hi - t_lo as a Fraction)]: the events of (a) with every
    t an exact rational, ties to the lower axis."""
    a = [Fraction(v) for v in _f64(a)]
    b = [Fraction(v) for v in _f64(b)]
    d = [b[i] - a[i] for i in range(3)]
    idx = [math.floor(v) for v in a]
    vb = [math.floor(v) for v in b]
    events = []
    for i in range(3):
        if vb[i] > idx[i]:
            planes = range(max(idx[i] + 1, 0), min(vb[i], dims[i]) + 1)
            events += [((beta - a[i]) / d[i], i, k, beta) for k, beta in enumerate(planes)]
        elif vb[i] < idx[i]:
            planes = range(min(idx[i], dims[i]), max(vb[i] + 1, 0) - 1, -1)
            events += [((beta - a[i]) / d[i], i, k, beta - 1) for k, beta in enumerate(planes)]
    events.sort()
    out, t_lo = [], Fraction(0)
    for t, i, _, after in events:
        if _inside(idx, dims):
            out.append((tuple(idx), t - t_lo))
        idx[i] = after
        t_lo = t
    if _inside(idx, dims):
        out.append((tuple(idx), 1 - t_lo))
    return out


# ------------------------------------------------------------------- the rows
def _apply(m, d):
    """lin d, each row ((m0 x + m1 y) + m2 z)."""
    return [(m[3 * r] * d[0] + m[3 * r + 1] * d[1]) + m[3 * r + 2] * d[2] for r in range(3)]


def segment_vector(a, b, m):
    """(|v_j|, [|v_jx|, |v_jy|, |v_jz|]) of segment a -> b, the header's expressions."""
    a, b = _f64(a), _f64(b)
    v = _apply(m, [b[i] - a[i] for i in range(3)])
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), [abs(c) for c in v]


def kernel_length(row, m):
    """sum_j |v_j| in the kernel's order: lane l of 64 adds its segments j = l,
    l + 64, ... in that order to 0.0, then the butterfly v += v[lane ^ off] for
    off = 32, 16, .. 1 (a + b == b + a, so every lane ends with the same bits)."""
    pts = np.asarray(row, np.float32).astype(np.float64).tolist()
    lanes = [0.0] * 64
    for j in range(len(pts) - 1):           # increasing j: lane j % 64 meets them in order
        lanes[j % 64] += segment_vector(pts[j], pts[j + 1], m)[0]
    off = 32
    while off:
        lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
        off >>= 1
    return lanes[0]


def streamline_order_length(row, m):
    """The same sum in streamline order: what the kernel does NOT compute."""
    pts = np.asarray(row, np.float32).astype(np.float64).tolist()
    total = 0.0
    for j in range(len(pts) - 1):
        total += segment_vector(pts[j], pts[j + 1], m)[0]
    return total


def row_is_added(row, m):
    """L >= 2, every point finite, and the length in the kernel's order
    (``kernel_length``) < 2^40 mm."""
    if len(row) < 2 or not np.isfinite(row).all():
        return False
    return kernel_length(row, m) < MAX_LENGTH


def _rint(x):
    """llrint in the default mode: half to even."""
    return int(np.rint(x))


def row_voxels(row, dims):
    """The voxels a row visits, in walk order and with repeats: floor(c_0) when
    inside, then every voxel entered."""
    out = []
    first = _floor_voxel(_f64(row[0]))
    if _inside(first, dims):
        out.append(first)
    for j in range(len(row) - 1):
        out += [v for v, _ in _bounded_walk(_f64(row[j]), _f64(row[j + 1]), dims)[0]]
    return out


def tier(n_voxels, wave_slots, spill_slots):
    """The status of an added row with ``n_voxels`` distinct voxels; spill_slots
    None or 0: no workspace."""
    if n_voxels <= wave_slots // 2:
        return 0
    if spill_slots and n_voxels <= spill_slots // 2:
        return 1
    return 2


def density(points, offsets, dims, lin, wave_slots=2048, spill_slots=None, mutant=None,
            maps=None, only_count=False):
    """The four maps ((X, Y, Z) count / ends int64, length_q int64, dec_q
    (X, Y, Z, 3) int64), ``status`` and ``n_voxels`` per row, of one call of
    ttl_tract_density (a status-2 row adds nothing to count).  ``maps``: added
    to when given.  ``only_count``: the re-add call of the status-2 rows."""
    assert mutant is None or mutant in MUTANTS, mutant
    points = np.asarray(points, np.float32).reshape(-1, 3)
    m = [float(v) for v in np.asarray(lin, np.float64).reshape(9)]
    if mutant == 'length_in_voxels':
        m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    n = len(offsets) - 1
    if maps is None:
        maps = {'count': np.zeros(dims, np.int64), 'ends': np.zeros(dims, np.int64),
                'length_q': np.zeros(dims, np.int64), 'dec_q': np.zeros(tuple(dims) + (3,), np.int64)}
    status = np.full(n, -1, np.int32)
    n_voxels = np.zeros(n, np.int64)
    for s in range(n):
        row = points[offsets[s]:offsets[s + 1]]
        partly = mutant == 'nonfinite_row_partly_added' and len(row) >= 2 and \
            not np.isfinite(row).all()
        if not row_is_added(row, m) and not partly:
            continue
        finite = np.isfinite(row).all(axis=1)
        row = row.astype(np.float64).tolist()
        visited = []
        if finite[0]:
            visited += row_voxels(row[:1], dims)
        if not only_count:
            ends = [row[0]] if mutant == 'ends_first_only' else [row[0], row[-1]]
            for p in ends:
                if all(math.isfinite(c) for c in p):
                    v = _floor_voxel(_f64(p))
                    if _inside(v, dims):
                        maps['ends'][v] += 1
        for j in range(len(row) - 1):
            if not (finite[j] and finite[j + 1]):
                continue
            walked = _bounded_walk(_f64(row[j]), _f64(row[j + 1]), dims)
            visited += [v for v, _ in walked[0]]
            if only_count:
                continue
            pieces = segment_pieces(row[j], row[j + 1], dims, mutant, walked)
            length, comps = segment_vector(row[j], row[j + 1], m)
            for vox, t_lo, t_hi in pieces:
                w = t_hi - t_lo
                maps['length_q'][vox] += _rint((w * length) * LENGTH_SCALE)
                for k in range(3):
                    maps['dec_q'][vox + (k,)] += _rint((w * comps[k]) * LENGTH_SCALE)
        distinct = list(dict.fromkeys(visited))
        n_voxels[s] = len(distinct)
        status[s] = tier(len(distinct), wave_slots, spill_slots)
        if mutant == 'no_dedupe':
            counted = visited
        elif mutant == 'dedupe_consecutive_only':
            counted = [v for k, v in enumerate(visited) if k == 0 or visited[k - 1] != v]
        else:
            counted = distinct
        if status[s] == 2:
            limit = spill_slots // 2 if spill_slots else wave_slots // 2
            counted = distinct[:limit] if mutant == 'count_partial_on_overflow' else []
        for v in counted:
            maps['count'][v] += 1
    return dict(maps, status=status, n_voxels=n_voxels)


def density_final(points, offsets, dims, lin, mutant=None):
    """The maps once every row is counted (what ``DensityMap.add`` leaves)."""
    return density(points, offsets, dims, lin, wave_slots=1 << 30, mutant=mutant)


def _sqrt(x):
    """The square root of a Fraction to 2^-100."""
    return Fraction(math.isqrt((x.numerator << 200) // x.denominator), 1 << 100)


def bounds(points, offsets, dims, lin):
    """(exact length_q, length bound, exact dec_q, dec bound), all (X, Y, Z[, 3])
    float64 in units of 2^-20 mm: per piece of statement (c), rounded half to
    even like the kernel's, and the header's tolerance 1 + 17 u B_j 2^20 (13 u
    B_jk for a component) summed once over a voxel's pieces.  (b) and (c) share
    every piece unless two crossings closer than the rounding of their t swap;
    then a voxel may hold a piece on one side only, so per segment and voxel the
    larger of the two piece counts is taken (a multiset union)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    m = [float(v) for v in np.asarray(lin, np.float64).reshape(9)]
    exact_m = [Fraction(v) for v in m]
    abs_m = [abs(v) for v in exact_m]
    shape = tuple(dims)
    q = np.zeros(shape, np.float64)
    qb = np.zeros(shape, np.float64)
    dq = np.zeros(shape + (3,), np.float64)
    dqb = np.zeros(shape + (3,), np.float64)
    scale = Fraction(2) ** 20
    for s in range(len(offsets) - 1):
        row = points[offsets[s]:offsets[s + 1]]
        if not row_is_added(row, m):
            continue
        for j in range(len(row) - 1):
            a = [Fraction(v) for v in _f64(row[j])]
            b = [Fraction(v) for v in _f64(row[j + 1])]
            d = [b[i] - a[i] for i in range(3)]
            v = [sum(exact_m[3 * r + i] * d[i] for i in range(3)) for r in range(3)]
            B = [sum(abs_m[3 * r + i] * abs(d[i]) for i in range(3)) for r in range(3)]
            norm = _sqrt(sum(c * c for c in v))
            Bn = float(np.sqrt(np.longdouble(float(sum(c * c for c in B)))))
            for vox, w in segment_pieces_exact(row[j], row[j + 1], dims):
                q[vox] += float(round(w * norm * scale))
                for k in range(3):
                    dq[vox + (k,)] += float(round(w * abs(v[k]) * scale))
            pieces = collections.Counter(
                p[0] for p in segment_pieces_exact(row[j], row[j + 1], dims)) | \
                collections.Counter(p[0] for p in segment_pieces(row[j], row[j + 1], dims))
            for vox, times in pieces.items():
                qb[vox] += times * (1.0 + 17.0 * U * Bn * LENGTH_SCALE)
                for k in range(3):
                    dqb[vox + (k,)] += times * (1.0 + 13.0 * U * float(B[k]) * LENGTH_SCALE)
    return q, qb, dq, dqb
