"""NumPy restatement of the oracle validator's device work (test
infrastructure only): the coverage walk of ``ttl_tract_coverage`` exactly as
include/ttl_hip.h defines it, the blocked-order float64 resampler of
``k_resample`` (which ``ttl_oracle_segments_packed`` reproduces bit for bit),
and the two numbers ``Oracle`` / ``Coverage``.  The library is built with
-ffp-contract=off -fno-fast-math, so the same float64 operations here give
the same bits."""
import math
from fractions import Fraction

import numpy as np


# ---------------------------------------------------------------- coverage
def _inside(v, dims):
    return all(0 <= int(v[i]) < dims[i] for i in range(3))


def walk_segment_naive(a, b, dims):
    """The definition, crossing by crossing: the voxels (in volume) entered by
    segment a -> b, in order.  Axis i has |vb_i - va_i| crossings; crossing m
    lies on the plane va_i + m (d_i > 0) or va_i - m + 1 (d_i < 0), at
    t = (plane - a_i) / d_i; increasing t, the lower axis first on ties."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return []
    d = b - a
    va, vb = np.floor(a), np.floor(b)
    events = []
    for i in range(3):
        n = int(abs(vb[i] - va[i]))
        for m in range(1, n + 1):
            beta = va[i] + m if d[i] > 0 else va[i] - m + 1
            events.append(((beta - a[i]) / d[i], i, m))
    events.sort()
    idx = [int(v) for v in va]
    out = []
    for _, i, _ in events:
        idx[i] += 1 if d[i] > 0 else -1
        if _inside(idx, dims):
            out.append(tuple(idx))
    return out


def _before(t0, ax0, t1, ax1):
    return t0 < t1 or (t0 == t1 and ax0 < ax1)


# Named deviations of the bounded walk that a plausible kernel bug would
# produce (``walk_segment(..., mutant=name)``), each one statement of the walk:
SEGMENT_MUTANTS = (
    'tie_higher_axis',        # the merge takes the higher axis on equal t
    'exit_never_stops',       # X does not end the walk
    'exit_on_t_only',         # X ends the walk on t alone (axis ignored on ties)
    'entry_skips_E',          # the entry search also skips E itself
    'desc_first_dim_minus_1',  # descending run starts at plane dim - 1
    'desc_index_is_plane',    # descending index after = plane (no - 1)
    't_not_refreshed',        # t of the stepped axis is not recomputed
    'exit_plane_dim_minus_1',  # ascending exit plane dim - 1
    't_float32',              # every t rounded to float32
    'd_float32',              # d = b - a formed in float32
)


def walk_segment(a, b, dims, mutant=None):
    """The same voxels with the work bounded by the marked voxels plus
    O(log dims), statement for statement as ``walk_segment`` in
    csrc/ttl_coverage.hip (per axis: the run of planes whose crossing keeps
    that index inside; start every run at the last axis entering, stop at the
    first axis leaving).

    ``mutant`` (one of SEGMENT_MUTANTS) plants one deviation; the tests show
    that each changes the marked set of cases the GPU test launches.  Three
    further candidates change no marked set and are therefore not listed:
    descending ``last = max(vb + 1, 0)`` (the extra crossing of plane 0 gives
    index -1, which the in-volume test of the mark drops); ascending
    ``first = max(va, 0)`` (the extra crossing re-marks the voxel the segment
    starts in, which the previous segment or the first point has marked); and
    E chosen on t alone (the other axis's tied crossing is then not skipped,
    but the index of the axis entering later is still outside when it is
    taken, so nothing is marked)."""
    assert mutant is None or mutant in SEGMENT_MUTANTS, mutant
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return []
    d = b - a
    if mutant == 'd_float32':
        with np.errstate(over='ignore'):
            d = (b32 - a32).astype(np.float64)
        if not np.isfinite(d).all():
            return []
    if mutant == 't_float32':
        def tof(plane, i):
            with np.errstate(over='ignore'):
                return float(np.float32((float(plane) - a[i]) / d[i]))
    else:
        def tof(plane, i):
            return (float(plane) - a[i]) / d[i]
    idx, cur, left, step = [0] * 3, [0] * 3, [0] * 3, [0] * 3
    et, eax, xt, xax = -np.inf, -1, np.inf, 3
    for i in range(3):
        dim = dims[i]
        va = int(min(max(np.floor(a[i]), -1.0), float(dim)))
        vb = int(min(max(np.floor(b[i]), -1.0), float(dim)))
        inside = 0 <= va < dim
        idx[i] = va
        if va == vb:
            if not inside:
                return []
            continue
        exit_plane = None
        if vb > va:
            step[i], first, last = 1, max(va + 1, 0), min(vb, dim - 1)
            if vb >= dim:
                exit_plane = dim - 1 if mutant == 'exit_plane_dim_minus_1' else dim
        else:
            step[i], first, last = -1, min(va, dim), max(vb + 1, 1)
            if mutant == 'desc_first_dim_minus_1':
                first = min(va, dim - 1)
            if vb < 0:
                exit_plane = 0
        left[i] = max((last - first) * step[i] + 1, 0)
        cur[i] = first
        if not inside:
            if left[i] == 0:
                return []
            t = tof(first, i)
            if _before(et, eax, t, i):
                et, eax = t, i
        if exit_plane is not None:
            t = tof(exit_plane, i)
            if _before(t, i, xt, xax):
                xt, xax = t, i
    if eax >= 0:
        for i in range(3):
            if left[i] == 0:
                continue
            lo, hi = 0, left[i]
            while lo < hi:
                mid = (lo + hi) >> 1
                t = tof(cur[i] + mid * step[i], i)
                skip = _before(t, i, et, eax)
                if mutant == 'entry_skips_E':
                    skip = not _before(et, eax, t, i)
                if skip:
                    lo = mid + 1
                else:
                    hi = mid
            if lo > 0:
                plane = cur[i] + (lo - 1) * step[i]
                idx[i] = plane if step[i] > 0 else plane - 1
                cur[i] += lo * step[i]
                left[i] -= lo
    tn = [tof(cur[i], i) if left[i] else 0.0 for i in range(3)]
    out = []
    while True:
        m = -1
        for i in range(3):
            if not left[i]:
                continue
            if mutant == 'tie_higher_axis':
                if m < 0 or tn[i] <= tn[m]:
                    m = i
            elif m < 0 or _before(tn[i], i, tn[m], m):
                m = i
        if m < 0:
            break
        if mutant == 'exit_never_stops':
            pass
        elif mutant == 'exit_on_t_only':
            if xt < tn[m]:
                break
        elif _before(xt, xax, tn[m], m):
            break
        idx[m] = cur[m] if step[m] > 0 or mutant == 'desc_index_is_plane' else cur[m] - 1
        if _inside(idx, dims):
            out.append(tuple(idx))
        cur[m] += step[m]
        left[m] -= 1
        if left[m] and mutant != 't_not_refreshed':
            tn[m] = tof(cur[m], m)
    return out


def walk_segment_planes(a, b, dims):
    """A third statement of the same voxels, valid at any magnitude and
    independent of the bounded walk's structure (no entry, no exit, no search,
    no clamped floor): floors as exact Python integers; on every axis whose
    index changes, the planes 0 .. dims_i that lie between the two floors are
    events (t, axis, order along the run, index after: the plane ascending,
    the plane - 1 descending); sorted, each sets its axis's index, and the
    voxel is marked when all three indices are inside.  Planes outside
    0 .. dims_i move an index from outside to outside, so they never mark and
    are left out: O(sum of dims) events wherever the ends lie."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return []
    d = b - a
    idx = [int(math.floor(v)) for v in a]
    vb = [int(math.floor(v)) for v in b]
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
    out = []
    for _, i, _, after in events:
        idx[i] = after
        if _inside(idx, dims):
            out.append(tuple(idx))
    return out


def streamline_voxels(points, dims, walk=walk_segment):
    """The set of voxels one streamline marks (floor of its first point, then
    every segment's walk)."""
    p = np.asarray(points, np.float32)
    out = set()
    if len(p) == 0:
        return out
    if np.isfinite(p[0]).all():
        v = np.floor(p[0].astype(np.float64))
        if all(0 <= v[i] < dims[i] for i in range(3)):
            out.add(tuple(int(x) for x in v))
    for j in range(len(p) - 1):
        out.update(walk(p[j], p[j + 1], dims))
    return out


def coverage_map(points, offsets, dims, accept=None, max_crossings=64):
    """visited (X, Y, Z) uint8 for the ragged tractogram (points (M, 3)
    float32, offsets (n + 1,)): the naive definition vectorised over segments
    (every crossing an event, sorted by (segment, t, axis, m)); segments with
    more than ``max_crossings`` crossings or a non-finite end go through
    ``walk_segment_planes``, so nothing here leans on the bounded walk."""
    X, Y, Z = (int(v) for v in dims)
    visited = np.zeros((X, Y, Z), np.uint8)
    pts = np.asarray(points, np.float32)
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    rows = np.arange(n) if accept is None else np.flatnonzero(np.asarray(accept))
    rows = rows[offsets[rows + 1] > offsets[rows]]
    if len(rows) == 0:
        return visited
    # first points
    first = pts[offsets[rows]].astype(np.float64)
    ok = np.isfinite(first).all(1)
    v = np.floor(first[ok]).astype(np.float64)
    inb = ((v >= 0) & (v < np.array([X, Y, Z]))).all(1)
    vi = v[inb].astype(np.int64)
    visited[vi[:, 0], vi[:, 1], vi[:, 2]] = 1
    # segments of the accepted streamlines
    lens = offsets[rows + 1] - offsets[rows]
    nseg = np.maximum(lens - 1, 0)
    seg_start = np.repeat(offsets[rows], nseg) + (
        np.arange(nseg.sum()) - np.repeat(np.cumsum(nseg) - nseg, nseg))
    A = pts[seg_start].astype(np.float64)
    B = pts[seg_start + 1].astype(np.float64)
    fin = np.isfinite(A).all(1) & np.isfinite(B).all(1)
    with np.errstate(invalid='ignore'):
        va, vb = np.floor(A), np.floor(B)
        ncross = np.where(fin[:, None], np.abs(vb - va), 0)
    big = fin & (ncross.sum(1) > max_crossings)
    for s in np.flatnonzero(big | ~fin):
        for vox in walk_segment_planes(pts[seg_start[s]], pts[seg_start[s] + 1], (X, Y, Z)):
            visited[vox] = 1
    small = np.flatnonzero(fin & ~big)
    A, B, va, ncross = A[small], B[small], va[small], ncross[small].astype(np.int64)
    D = B - A
    segs, axes, ms, ts = [], [], [], []
    for i in range(3):
        c = ncross[:, i]
        s_ = np.repeat(np.arange(len(small)), c)
        m_ = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c) + 1
        pos = D[s_, i] > 0
        beta = np.where(pos, va[s_, i] + m_, va[s_, i] - m_ + 1)
        ts.append((beta - A[s_, i]) / D[s_, i])
        segs.append(s_)
        axes.append(np.full(len(s_), i))
        ms.append(m_)
    seg, ax, m, t = (np.concatenate(x) for x in (segs, axes, ms, ts))
    order = np.lexsort((m, ax, t, seg))
    seg, ax = seg[order], ax[order]
    if len(seg) == 0:
        return visited
    start = np.searchsorted(seg, seg)            # first event of each event's segment
    idx = np.empty((len(seg), 3), np.int64)
    for i in range(3):
        hit = (ax == i).astype(np.int64)
        cum = np.cumsum(hit)
        cnt = cum - (cum[start] - hit[start])
        sign = np.sign(D[seg, i]).astype(np.int64)
        idx[:, i] = va[seg, i].astype(np.int64) + sign * cnt
    inb = ((idx >= 0) & (idx < np.array([X, Y, Z]))).all(1)
    idx = idx[inb]
    visited[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    return visited


WAVE, GRID_WAVES = 64, 4 * 8192     # lanes of a wave; waves of the largest grid

# Named deviations of the kernel's outer loop (``coverage_rows(..., mutant=name)``)
ROW_MUTANTS = (
    'segments_past_64_dropped',   # the lane stride stops after one pass
    'rows_past_grid_dropped',     # rows >= 4 * 8192 are never visited
    'score_ge',                   # scores >= threshold accepted
    'nan_score_accepted',         # the gate is `scores <= threshold -> skip`
    'first_point_unmarked',
    'first_point_clamped',        # floor of the first point clamped into the volume
    'nonfinite_point_ends_row',   # a non-finite point drops the rest of the row
)


def coverage_rows(points, offsets, dims, scores=None, threshold=0.5, mutant=None):
    """``k_tract_coverage`` row by row (its outer loop, restated): visited
    (X, Y, Z) uint8.  The score gate compares float32 with float32; an empty
    row marks nothing; the first point is marked when it is finite and inside;
    every segment goes through the bounded walk.  ``mutant``: one of
    ROW_MUTANTS, or one of SEGMENT_MUTANTS (handed to the walk)."""
    assert mutant is None or mutant in ROW_MUTANTS + SEGMENT_MUTANTS, mutant
    seg_mutant = mutant if mutant in SEGMENT_MUTANTS else None
    dims = tuple(int(v) for v in dims)
    visited = np.zeros(dims, np.uint8)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    thr = np.float32(threshold)
    sc = None if scores is None else np.asarray(scores, np.float32)
    for row in range(len(offsets) - 1):
        if mutant == 'rows_past_grid_dropped' and row >= GRID_WAVES:
            break
        if sc is not None:
            if mutant == 'score_ge':
                skip = not (sc[row] >= thr)
            elif mutant == 'nan_score_accepted':
                skip = bool(sc[row] <= thr)
            else:
                skip = not (sc[row] > thr)
            if skip:
                continue
        p = pts[offsets[row]:offsets[row + 1]]
        L = len(p)
        if L < 1:
            continue
        first = p[0].astype(np.float64)
        if mutant != 'first_point_unmarked' and np.isfinite(first).all():
            v = np.floor(first)
            if mutant == 'first_point_clamped':
                v = np.clip(v, 0, np.array(dims) - 1)
            if _inside(v, dims):
                visited[tuple(int(x) for x in v)] = 1
        nseg = L - 1
        if mutant == 'segments_past_64_dropped':
            nseg = min(nseg, WAVE)
        for j in range(nseg):
            if mutant == 'nonfinite_point_ends_row' and not np.isfinite(p[j:j + 2]).all():
                break
            for vox in walk_segment(p[j], p[j + 1], dims, seg_mutant):
                visited[vox] = 1
    return visited


def oracle_and_coverage(scores, visited, mask):
    """{'Oracle', 'Coverage'} from scores (n,), the visited map and the
    tracking mask (oracle_validator.py:48-56)."""
    scores = np.asarray(scores)
    return {'Oracle': float(np.mean(scores > 0.5)),
            'Coverage': float(np.count_nonzero(visited) / np.count_nonzero(mask))}


# ------------------------------------------------------- shared test inputs
def random_walks(rng, n, lo, hi, box, step=(0.5, 0.75), start=None):
    """n random-walk streamlines of lo..hi points, steps of 0.5-0.75 voxel,
    starting uniformly in [0, box)^3 (or in ``start``)."""
    lines = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        d = rng.normal(size=(L - 1, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d *= rng.uniform(step[0], step[1], (L - 1, 1))
        p0 = rng.uniform(0, box, 3) if start is None else rng.uniform(*start, 3)
        lines.append(np.concatenate([p0[None], p0 + np.cumsum(d, 0)]).astype(np.float32))
    return lines


HAND = [   # (a, b, dims, voxels the segment enters)
    # axis-aligned run
    ((0.5, 0.5, 0.5), (3.5, 0.5, 0.5), (5, 5, 5), [(1, 0, 0), (2, 0, 0), (3, 0, 0)]),
    # diagonal through an edge: the tie goes to the lower axis
    ((0.5, 0.5, 0.5), (1.5, 1.5, 0.5), (4, 4, 4), [(1, 0, 0), (1, 1, 0)]),
    ((2.5, 2.5, 0.5), (0.5, 0.5, 0.5), (4, 4, 4), [(1, 2, 0), (1, 1, 0), (0, 1, 0), (0, 0, 0)]),
    # points exactly on a face
    ((1.0, 0.5, 0.5), (2.5, 0.5, 0.5), (4, 4, 4), [(2, 0, 0)]),
    ((0.5, 0.5, 0.5), (1.0, 0.5, 0.5), (4, 4, 4), [(1, 0, 0)]),
    ((1.0, 0.5, 0.5), (0.5, 0.5, 0.5), (4, 4, 4), [(0, 0, 0)]),
    # negative coordinates: outside voxels are skipped, not clamped
    ((-1.5, 0.5, 0.5), (1.5, 0.5, 0.5), (4, 4, 4), [(0, 0, 0), (1, 0, 0)]),
    ((0.5, -0.25, 0.5), (0.5, -2.5, 0.5), (4, 4, 4), []),
    # leaving the volume
    ((3.5, 0.5, 0.5), (6.5, 0.5, 0.5), (5, 5, 5), [(4, 0, 0)]),
    ((3.5, 3.5, 0.5), (5.5, 6.5, 0.5), (5, 5, 5), [(3, 4, 0), (4, 4, 0)]),
    # zero length
    ((1.25, 1.25, 1.25), (1.25, 1.25, 1.25), (4, 4, 4), []),
    # a point 10^6 voxels away (both ends of the run outside on one side)
    ((2.5, 2.5, 2.5), (2.5 + 1e6, 2.5 + 1e6, 2.5), (5, 5, 5),
     [(3, 2, 2), (3, 3, 2), (4, 3, 2), (4, 4, 2)]),
    ((-1e6, 2.5, 2.5), (3.5, 2.5, 2.5), (5, 5, 5),
     [(0, 2, 2), (1, 2, 2), (2, 2, 2), (3, 2, 2)]),
]



# ---------------------------------------------------------------- resampler
def resample_blocked(points, nb_points=128):
    """k_resample on one streamline (L, 3) float32, L >= 1 (one point: the
    output is that point, every difference a zero vector), in its own order:
    lane l of 64 sums the float64 segment lengths [l per, (l + 1) per)
    sequentially, a Hillis-Steele scan over the lanes gives the inclusive
    prefix, the exclusive one is that minus the lane's sum, cum[j + 1] =
    local_j + exclusive; then k_resample's binary search and interpolation."""
    p = np.asarray(points, np.float32)
    L = len(p)
    nseg = L - 1
    pd = p.astype(np.float64)
    dx, dy, dz = (pd[1:, i] - pd[:-1, i] for i in range(3))
    seg = np.sqrt((dx * dx + dy * dy) + dz * dz)
    per = (nseg + 63) >> 6
    cum = np.zeros(L, np.float64)
    local_cum = []
    local = np.zeros(64, np.float64)
    for lane in range(64):
        lo = min(lane * per, nseg)
        hi = min(lo + per, nseg)
        c = np.add.accumulate(seg[lo:hi]) if hi > lo else np.zeros(0)
        local_cum.append((lo, c))
        local[lane] = c[-1] if len(c) else 0.0
    before = local.copy()
    off = 1
    while off < 64:
        nxt = before.copy()
        nxt[off:] = before[off:] + before[:-off]
        before = nxt
        off <<= 1
    excl = before - local
    for lane, (lo, c) in enumerate(local_cum):
        cum[lo + 1:lo + 1 + len(c)] = c + excl[lane]
    total = cum[nseg]
    out = np.empty((nb_points, 3), np.float32)
    for k in range(nb_points):
        if k == nb_points - 1 or nseg == 0:
            out[k] = p[nseg]
            continue
        target = total * (float(k) / float(nb_points - 1))
        a, b = 0, nseg
        while a < b:
            mid = (a + b) >> 1
            if cum[mid + 1] <= target:
                a = mid + 1
            else:
                b = mid
        j = min(a, nseg - 1)
        c0, c1 = cum[j], cum[j + 1]
        den = c1 - c0
        r = (target - c0) / den if den > 0.0 else 0.0
        out[k] = (pd[j] + r * (pd[j + 1] - pd[j])).astype(np.float32)
    return out


def segments_blocked(points, nb_points=128):
    """The network's input of one streamline: the float32 differences of
    ``resample_blocked``."""
    r = resample_blocked(points, nb_points)
    return r[1:] - r[:-1]


# ---------------------------------------------------------------- 3x3 map
def _round_f32(q):
    """The float32 nearest to the rational q, ties to even, rounded once
    (normal range and zero; coordinates never leave it)."""
    if q == 0:
        return np.float32(0.0)
    n, d = abs(q.numerator), q.denominator
    e = n.bit_length() - d.bit_length()          # 2^(e - 1) < |q| < 2^(e + 1)
    if Fraction(n, d) < Fraction(2) ** e:
        e -= 1
    e = max(e, -126)
    m = round(abs(q) / Fraction(2) ** (e - 23))  # round(Fraction): half to even
    v = np.float32(np.ldexp(float(m), e - 23))   # m <= 2^24: exact
    return -v if q < 0 else v


def _fma_f32(a, b, c):
    """fmaf(a, b, c): the exact a b + c rounded to float32 once."""
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def map_points_fma(points, m):
    """The 3x3 map of ``k_oracle_segments`` (out = p @ m, m row-major) on
    (L, 3) float32 points as the kernel states it, in float32:
    out_c = fma(z, m[6 + c], fma(y, m[3 + c], x * m[c])), every operation
    rounded exactly once (exact rational arithmetic, then one rounding)."""
    p = np.asarray(points, np.float32)
    m = np.asarray(m, np.float32).reshape(9)
    out = np.empty_like(p)
    for j, (x, y, z) in enumerate(p):
        for c in range(3):
            t = _round_f32(Fraction(float(x)) * Fraction(float(m[c])))
            out[j, c] = _fma_f32(z, m[6 + c], _fma_f32(y, m[3 + c], t))
    return out
