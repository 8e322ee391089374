"""NumPy restatement of the oracle validator's device work (test
infrastructure only): the coverage walk of ``ttl_tract_coverage`` exactly as
include/ttl_hip.h defines it, the blocked-order float64 resampler of
``k_resample`` (which ``ttl_oracle_segments_packed`` reproduces bit for bit),
and the two numbers ``Oracle`` / ``Coverage``.  The library is built with
-ffp-contract=off -fno-fast-math, so the same float64 operations here give
the same bits."""
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


def walk_segment(a, b, dims):
    """The same voxels with the work bounded by the marked voxels plus
    O(log dims), statement for statement as ``walk_segment`` in
    csrc/ttl_coverage.hip (per axis: the run of planes whose crossing keeps
    that index inside; start every run at the last axis entering, stop at the
    first axis leaving)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return []
    d = b - a
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
                exit_plane = dim
        else:
            step[i], first, last = -1, min(va, dim), max(vb + 1, 1)
            if vb < 0:
                exit_plane = 0
        left[i] = max((last - first) * step[i] + 1, 0)
        cur[i] = first
        if not inside:
            if left[i] == 0:
                return []
            t = (float(first) - a[i]) / d[i]
            if _before(et, eax, t, i):
                et, eax = t, i
        if exit_plane is not None:
            t = (float(exit_plane) - a[i]) / d[i]
            if _before(t, i, xt, xax):
                xt, xax = t, i
    if eax >= 0:
        for i in range(3):
            if left[i] == 0:
                continue
            lo, hi = 0, left[i]
            while lo < hi:
                mid = (lo + hi) >> 1
                t = (float(cur[i] + mid * step[i]) - a[i]) / d[i]
                if _before(t, i, et, eax):
                    lo = mid + 1
                else:
                    hi = mid
            if lo > 0:
                plane = cur[i] + (lo - 1) * step[i]
                idx[i] = plane if step[i] > 0 else plane - 1
                cur[i] += lo * step[i]
                left[i] -= lo
    tn = [(float(cur[i]) - a[i]) / d[i] if left[i] else 0.0 for i in range(3)]
    out = []
    while True:
        m = -1
        for i in range(3):
            if left[i] and (m < 0 or _before(tn[i], i, tn[m], m)):
                m = i
        if m < 0 or _before(xt, xax, tn[m], m):
            break
        idx[m] = cur[m] if step[m] > 0 else cur[m] - 1
        if _inside(idx, dims):
            out.append(tuple(idx))
        cur[m] += step[m]
        left[m] -= 1
        if left[m]:
            tn[m] = (float(cur[m]) - a[m]) / d[m]
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
    more than ``max_crossings`` crossings or a non-finite end go through the
    bounded scalar walk."""
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
        for vox in walk_segment(pts[seg_start[s]], pts[seg_start[s] + 1], (X, Y, Z)):
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


def oracle_and_coverage(scores, visited, mask):
    """{'Oracle', 'Coverage'} from scores (n,), the visited map and the
    tracking mask (oracle_validator.py:48-56)."""
    scores = np.asarray(scores)
    return {'Oracle': float(np.mean(scores > 0.5)),
            'Coverage': float(np.count_nonzero(visited) / np.count_nonzero(mask))}


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
