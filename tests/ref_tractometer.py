"""NumPy float64 statement of the Tractometer validator's definitions
(include/ttl_hip.h, ttl_tractometer_classify / ttl_tractometer_overlap; test
infrastructure only).  Voxels come from ``walk_segment_planes`` of
tests/ref_oracle_validator.py, eigenvectors from ``numpy.linalg.eigh``, the
metrics from Python sets.  ``mutant`` plants one named deviation; the tests
show that each changes what the GPU tests compare.

A scoring set is a list of bundles, each a dict:
    head, tail        bool (X, Y, Z)
    all, any, gt      bool (X, Y, Z) or None
    length            [lo, hi] or None          (mm)
    dir, absdir       [[lo, hi]] * 3 or None    (length_x/y/z, length_x/y/z_abs)
    angle             degrees or None
"""
import math

import numpy as np

from ref_oracle_validator import streamline_voxels, walk_segment_planes

MUTANTS = (
    'trunc_ends',        # int cast for floor
    'one_order',         # only head -> tail
    'points_only',       # all / any tested at the points' voxels instead of the walk
    'strict_bounds',     # exclusive limits
    'first_connected',   # the lowest connected bundle instead of the lowest valid one
    'shift32',           # bits >= 32 lost
)


def bundle(head, tail, all=None, any=None, gt=None, length=None, dir=None, absdir=None,
           angle=None):
    return {'head': head, 'tail': tail, 'all': all, 'any': any, 'gt': gt, 'length': length,
            'dir': dir, 'absdir': absdir, 'angle': angle}


# ------------------------------------------------------------- per streamline
def end_voxel(c, dims, mutant=None):
    """floor(c) as a voxel, or None when c is non-finite or outside."""
    c = np.asarray(c, np.float32).astype(np.float64)
    if not np.isfinite(c).all():
        return None
    v = [int(x) if mutant == 'trunc_ends' else int(math.floor(x)) for x in c]
    return tuple(v) if all(0 <= v[i] < dims[i] for i in range(3)) else None


def connected_set(points, dims, bundles, mutant=None):
    """[b with connects(b)]: ends from a row of >= 2 points."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if len(p) < 2:
        return []
    e0, e1 = end_voxel(p[0], dims, mutant), end_voxel(p[-1], dims, mutant)
    if e0 is None or e1 is None:
        return []
    out = []
    for b, B in enumerate(bundles):
        if mutant == 'shift32' and b >= 32:
            continue
        fwd = B['head'][e0] and B['tail'][e1]
        bwd = B['tail'][e0] and B['head'][e1]
        if fwd or (bwd and mutant != 'one_order'):
            out.append(b)
    return out


def lengths(points, lin):
    """(length, dir[3], absdir[3]) in mm, float64: v_j = lin (c_{j+1} - c_j)."""
    c = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    lin = np.asarray(lin, np.float64).reshape(3, 3)
    e = c[1:] - c[:-1]
    v = np.stack([(lin[k, 0] * e[:, 0] + lin[k, 1] * e[:, 1]) + lin[k, 2] * e[:, 2]
                  for k in range(3)], 1)
    length = float(np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).sum())
    return length, np.abs(v.sum(0)), np.abs(v).sum(0)


def winding_parts(points):
    """(winding in degrees, eigenvalues descending, min |p_j|): dipy's winding
    on the coordinates as they are, the plane from ``numpy.linalg.eigh`` of the
    scatter matrix."""
    c = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    q = c - c.mean(0)
    w, V = np.linalg.eigh(q.T @ q)              # ascending
    proj = q @ V[:, [2, 1]]
    norms = np.sqrt((proj * proj).sum(1))
    turn = 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(len(c) - 1):
            v = np.dot(proj[j], proj[j + 1]) / (norms[j] * norms[j + 1])
            turn += np.arccos(np.clip(v, -1, 1))
    return float(turn * (180.0 / math.pi)), w[::-1], float(norms.min())


def winding(points):
    return winding_parts(points)[0]


def voxels(points, dims):
    """V(s): the in-volume voxels of the walk, as a set."""
    return streamline_voxels(points, dims, walk_segment_planes)


def point_voxels(points, dims):
    out = set()
    for c in np.asarray(points, np.float32).reshape(-1, 3):
        v = end_voxel(c, dims)
        if v is not None:
            out.add(v)
    return out


def _between(lo, x, hi, mutant):
    if mutant == 'strict_bounds':
        return bool(lo < x < hi)
    return bool(lo <= x <= hi)


def criteria(points, dims, B, lin, mutant=None):
    """valid(b) without the end test: every criterion bundle B sets."""
    if B['length'] is not None or B['dir'] is not None or B['absdir'] is not None:
        length, d, a = lengths(points, lin)
        if B['length'] is not None and not _between(B['length'][0], length, B['length'][1],
                                                   mutant):
            return False
        for lim, val in ((B['dir'], d), (B['absdir'], a)):
            if lim is not None:
                for k in range(3):
                    if not _between(lim[k][0], val[k], lim[k][1], mutant):
                        return False
    if B['all'] is not None or B['any'] is not None:
        V = point_voxels(points, dims) if mutant == 'points_only' else voxels(points, dims)
        if B['all'] is not None and not all(B['all'][v] for v in V):
            return False
        if B['any'] is not None and not any(B['any'][v] for v in V):
            return False
    if B['angle'] is not None and not winding(points) < B['angle']:
        return False
    return True


def classify_one(points, dims, bundles, lin, mutant=None):
    """(bundle(s), connected(s) as an int bit set)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    conn = connected_set(p, dims, bundles, mutant)
    word = sum(1 << b for b in conn)
    if len(p) < 2 or not np.isfinite(p).all():
        return -1, word
    if mutant == 'first_connected':
        conn = conn[:1]
    for b in conn:
        if criteria(p, dims, bundles[b], lin, mutant):
            return b, word
    return -1, word


# -------------------------------------------------------------- per tractogram
def score(points, offsets, dims, bundles, lin, mutant=None):
    """{'bundle': int32 [n], 'connected': uint64 [n], 'counts': int64 [B][2],
    'visited': uint64 (X, Y, Z), 'metrics': the validator's dict}."""
    dims = tuple(int(v) for v in dims)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    out_b = np.empty(n, np.int32)
    out_c = np.empty(n, np.uint64)
    M = [set() for _ in bundles]
    for s in range(n):
        row = pts[offsets[s]:offsets[s + 1]]
        b, word = classify_one(row, dims, bundles, lin, mutant)
        out_b[s], out_c[s] = b, word
        if b >= 0 and not (mutant == 'shift32' and b >= 32):
            M[b] |= voxels(row, dims)
    counts = np.zeros((len(bundles), 2), np.int64)
    visited = np.zeros(dims, np.uint64)
    ols = []
    for b, B in enumerate(bundles):
        G = set() if B['gt'] is None else set(zip(*np.nonzero(B['gt'])))
        G = {tuple(int(x) for x in v) for v in G}
        counts[b] = len(M[b] & G), len(M[b] - G)
        for v in M[b]:
            visited[v] |= np.uint64(1) << np.uint64(b)
        if B['gt'] is not None:
            ols.append(len(M[b] & G) / len(G) if G else 0.0)
    vs = int((out_b >= 0).sum())
    vc = vs / n if n else 0.0
    metrics = {'VC': vc, 'IC': 0, 'IS': 0, 'NC': 1 - vc,
               'mean_OL': float(sum(ols) / len(ols)) if ols else 0.0,
               'VB': len({int(b) for b in out_b if b >= 0}), 'IB': 0}
    return {'bundle': out_b, 'connected': out_c, 'counts': counts, 'visited': visited,
            'metrics': metrics}


# ------------------------------------------------- margins the GPU tests assert
REL = 1e-9


def exact_sums(points, lin):
    """(dir / absdir exact, length exact): whether a row's float64 sums come
    out the same in ANY order of summation because every term and every
    partial sum is exact.  Coordinates and lin multiples of 2^-6 below 2^10 and
    at most 4096 points: every v_jk is a multiple of 2^-12 below 2^22, so sums
    of them are exact.  The length is exact as well when every v_j has at most
    one non-zero component (its norm is then |v_jk|, no rounding in the
    square root)."""
    c = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    lin = np.asarray(lin, np.float64).reshape(3, 3)
    if not (np.all(c * 64 == np.round(c * 64)) and np.all(lin * 64 == np.round(lin * 64))):
        return False, False
    if np.abs(c).max() > 1024 or np.abs(lin).max() > 1024 or len(c) > 4096:
        return False, False
    v = (c[1:] - c[:-1]) @ lin.T
    return True, bool(np.all((v != 0).sum(1) <= 1))


def margin_report(points, dims, bundles, lin):
    """What a row's decisions rest on, for every connected bundle: a list of
    (what, value, limit, ok) where ok says the comparison cannot turn with the
    order of a float64 sum: the value is farther than REL (relative) from the
    limit, or the row's sums are exact (``exact_sums``); for a bundle with
    an angle also the eigenvalue gap and the smallest |p_j|."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = []
    if len(p) < 2 or not np.isfinite(p).all():
        return out
    exact_dir, exact_len = exact_sums(p, lin)
    length, d, a = lengths(p, lin)
    c = p.astype(np.float64)
    v = (c[1:] - c[:-1]) @ np.asarray(lin, np.float64).reshape(3, 3).T

    def far(x, lim):
        return abs(x - lim) > REL * max(abs(x), abs(lim)) if np.isfinite(lim) else True

    for b in connected_set(p, dims, bundles):
        B = bundles[b]
        pairs = []          # (what, value, limit, the limit is the lower one, terms)
        if B['length'] is not None:
            pairs += [('length', length, B['length'][i], i == 0, None) for i in range(2)]
        for name, lim3, val in (('dir', B['dir'], d), ('absdir', B['absdir'], a)):
            if lim3 is not None:
                pairs += [(f'{name}{k}', val[k], lim3[k][i], i == 0, v[:, k])
                          for k in range(3) for i in range(2)]
        for what, x, lim, lower, terms in pairs:
            ok = exact_len if what == 'length' else exact_dir
            # a sum of nothing but zeros is zero in every order
            ok = ok or (terms is not None and not terms.any())
            # every quantity is a norm or an absolute value: a lower limit <= 0 always holds
            ok = ok or (lower and lim <= 0)
            out.append((b, what, x, lim, bool(ok or far(x, lim))))
        if B['angle'] is not None:
            w, lam, pmin = winding_parts(p)
            out.append((b, 'winding', w, B['angle'], far(w, B['angle'])))
            out.append((b, 'gap', lam[1] - lam[2], 1e-3 * lam[0],
                        bool(lam[1] - lam[2] >= 1e-3 * lam[0])))
            out.append((b, 'pmin', pmin, 1e-9, bool(pmin >= 1e-9)))
    return out


# ------------------------------------ the classify kernel's values (winding and sums)
# What tests/test_tractometer_values.py measures the kernel against: the
# header's definition at 50 digits, and ``wave_winding`` of
# csrc/ttl_tractometer.hip restated in NumPy float64 with named deviations.
MP_DIGITS = 50

WINDING_MUTANTS = (
    'no_clip',             # acos of the unclipped quotient
    'skip_last_segment',   # j < L - 2
    'radians',             # no 180 / pi
    'non_strict',          # winding <= angle (a decision, not a value: see winding_passes)
    'one_sweep',           # one Jacobi sweep instead of eight
    'drop_largest',        # the plane of the two smallest eigenvalues
    'rotation_sign',       # s negated in the eigenvector update
    'stale_offdiag',       # apr / aqr not updated by a rotation
    'uncentred',           # mean left out
    'first_64_points',     # no stride loop: one point and one segment per lane
)


def _exact(points):
    """The float32 points as Python floats (exact), [L][3]."""
    return np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3).tolist()


def winding_mp(points):
    """The header's winding with mpmath at MP_DIGITS digits, on the float32
    points read exactly, the plane from ``mp.eigsy``.  A dict of mpf:
    ``winding`` (degrees; NaN when some p_j is 0), ``lam`` (eigenvalues,
    descending), ``pmin`` / ``pmax`` (min / max |p_j|) and ``vmin`` / ``vmax``
    (the extreme acos arguments before the clip; None with fewer than 2 points
    or a zero p_j)."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(MP_DIGITS):
        c = [[mp.mpf(x) for x in row] for row in _exact(points)]
        L = len(c)
        mean = [mp.fsum(row[k] for row in c) / L for k in range(3)]
        q = [[row[k] - mean[k] for k in range(3)] for row in c]
        S = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                S[a, b] = mp.fsum(row[a] * row[b] for row in q)
        E, Q = mp.eigsy(S)                               # ascending
        order = sorted(range(3), key=lambda i: E[i], reverse=True)
        u = [[Q[k, order[i]] for k in range(3)] for i in range(2)]
        p = [[mp.fsum(row[k] * u[i][k] for k in range(3)) for i in range(2)] for row in q]
        norms = [mp.sqrt(a * a + b * b) for a, b in p]
        out = {'lam': [E[i] for i in order], 'pmin': min(norms), 'pmax': max(norms),
               'vmin': None, 'vmax': None, 'winding': mp.nan}
        if L >= 2 and min(norms) > 0:
            v = [(p[j][0] * p[j + 1][0] + p[j][1] * p[j + 1][1]) / (norms[j] * norms[j + 1])
                 for j in range(L - 1)]
            out['vmin'], out['vmax'] = min(v), max(v)
            out['winding'] = mp.fsum(mp.acos(max(-1, min(1, x))) for x in v) * 180 / mp.pi
        return out


def sums_mp(points, lin):
    """The header's sums with mpmath at MP_DIGITS digits: a dict of mpf,
    ``length``, ``dir`` [3] and ``absdir`` [3], from the float32 points and the
    float64 ``lin`` read exactly."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(MP_DIGITS):
        c = [[mp.mpf(x) for x in row] for row in _exact(points)]
        m = [[mp.mpf(float(x)) for x in row] for row in np.asarray(lin, np.float64).reshape(3, 3)]
        v = [[mp.fsum(m[k][i] * (c[j + 1][i] - c[j][i]) for i in range(3)) for k in range(3)]
             for j in range(len(c) - 1)]
        return {'length': mp.fsum(mp.sqrt(mp.fsum(x * x for x in row)) for row in v),
                'dir': [abs(mp.fsum(row[k] for row in v)) for k in range(3)],
                'absdir': [mp.fsum(abs(row[k]) for row in v) for k in range(3)]}


_LANES = np.arange(64)


def wave_sum(terms):
    """The kernel's sum of one term per j: lane l adds j = l, l + 64, ... in
    that order onto 0.0, then the xor butterfly 32, 16, .. 1."""
    terms = np.asarray(terms, np.float64)
    rows = -(-len(terms) // 64)
    padded = np.zeros(max(rows, 1) * 64)
    padded[:len(terms)] = terms
    acc = np.zeros(64)
    for r in range(rows):
        acc = acc + padded[64 * r:64 * (r + 1)]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[_LANES ^ off]
    return float(acc[0])


def _jacobi_rotate(a, p, q, r, V, mutant):
    """One rotation in the (p, q) plane of the symmetric 3x3 ``a`` (a dict
    keyed by the sorted index pair), r the third index; V[k][i] = component k
    of eigenvector column i."""
    pq, pr, qr = (min(p, q), max(p, q)), (min(p, r), max(p, r)), (min(q, r), max(q, r))
    apq = a[pq]
    if apq == 0.0:
        return
    theta = (a[(q, q)] - a[(p, p)]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[(p, p)] -= t * apq
    a[(q, q)] += t * apq
    a[pq] = 0.0
    if mutant != 'stale_offdiag':
        x, y = a[pr], a[qr]
        a[pr] = c * x - s * y
        a[qr] = s * x + c * y
    if mutant == 'rotation_sign':
        s = -s
    for k in range(3):
        x, y = V[k][p], V[k][q]
        V[k][p] = c * x - s * y
        V[k][q] = s * x + c * y


def winding_jacobi(points, mutant=None):
    """``wave_winding`` (and the centroid of step 2 of the kernel) restated in
    NumPy float64, operation for operation: (winding in degrees, the slot 0 / 1
    / 2 whose eigenvector is dropped)."""
    c = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    L = len(c)
    mean = np.array([wave_sum(c[:, k]) / float(L) for k in range(3)])
    if mutant == 'uncentred':
        mean = np.zeros(3)
    head = c[:64] if mutant == 'first_64_points' else c
    x, y, z = (head[:, k] - mean[k] for k in range(3))
    a = {(0, 0): wave_sum(x * x), (0, 1): wave_sum(x * y), (0, 2): wave_sum(x * z),
         (1, 1): wave_sum(y * y), (1, 2): wave_sum(y * z), (2, 2): wave_sum(z * z)}
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(1 if mutant == 'one_sweep' else 8):
        _jacobi_rotate(a, 0, 1, 2, V, mutant)
        _jacobi_rotate(a, 0, 2, 1, V, mutant)
        _jacobi_rotate(a, 1, 2, 0, V, mutant)
    s00, s11, s22 = a[(0, 0)], a[(1, 1)], a[(2, 2)]
    if mutant == 'drop_largest':
        drop0 = s00 >= s11 and s00 >= s22
        drop1 = not drop0 and s11 >= s22
    else:
        drop0 = s00 <= s11 and s00 <= s22
        drop1 = not drop0 and s11 <= s22
    i1, i2 = (1 if drop0 else 0), (2 if drop0 or drop1 else 1)
    u1 = [V[k][i1] for k in range(3)]
    u2 = [V[k][i2] for k in range(3)]
    last = L - 2 if mutant == 'skip_last_segment' else L - 1
    if mutant == 'first_64_points':
        last = min(last, 64)
    q = c[:last + 1] - mean
    px = (q[:, 0] * u1[0] + q[:, 1] * u1[1]) + q[:, 2] * u1[2]
    py = (q[:, 0] * u2[0] + q[:, 1] * u2[1]) + q[:, 2] * u2[2]
    ax, ay, bx, by = px[:-1], py[:-1], px[1:], py[1:]
    with np.errstate(invalid='ignore', divide='ignore'):
        v = (ax * bx + ay * by) / (np.sqrt(ax * ax + ay * ay) * np.sqrt(bx * bx + by * by))
        if mutant != 'no_clip':
            v = np.where(v < -1.0, -1.0, np.where(v > 1.0, 1.0, v))      # a NaN stays a NaN
        turn = wave_sum(np.arccos(v))
    if mutant != 'radians':
        turn = turn * (180.0 / 3.14159265358979323846)
    return turn, (0 if drop0 else 1 if drop1 else 2)


def winding_passes(w, angle, mutant=None):
    """The criterion on a winding: strict, so a NaN and w == angle fail."""
    return bool(w <= angle) if mutant == 'non_strict' else bool(w < angle)
