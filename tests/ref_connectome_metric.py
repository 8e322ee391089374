"""The definition of ttl_tract_sample_mean / ttl_connectome_accumulate_metric
(include/ttl_hip.h) as a literal loop over streamlines in
numpy.longdouble, the trilinear sum included: the yardstick of the kernel's
float64 chain.  The decisions (which point is sampled, which row has a mean) are
comparisons of float32 inputs and are the kernel's exactly.

``mutant`` names one deliberate misreading of the definition; the CPU tests show
that the case sets tell each from the definition, so a kernel that made that
mistake could not pass the GPU tests."""
import math

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
MAX_Q = 2.0 ** 40

SAMPLE_MUTANTS = ('no_half_shift', 'truncation', 'uniform_weights', 'ends_not_halved',
                  'nonfinite_corner_zero', 'zero_padding', 'outside_clamped')
ACCUMULATE_MUTANTS = ('nan_rows_counted', 'half_away_from_zero')
MUTANTS = SAMPLE_MUTANTS + ACCUMULATE_MUTANTS


def scale_for(volume):
    """The scale of a metric volume (float32 as uploaded): m = the largest finite
    |value| (1 for none or 0), e the smallest integer with m < 2^e, 2^(39 - e),
    the exponent held to -60 .. 60."""
    v = np.abs(np.asarray(volume, np.float32).astype(np.float64))
    v = v[np.isfinite(v)]
    m = float(v.max()) if v.size and v.max() > 0 else 1.0
    e = math.frexp(m)[1]                # m = f 2^e, 0.5 <= f < 1
    return 2.0 ** min(max(39 - e, -60), 60)


def segment_lengths(row, lin, magnitudes=False):
    """|lin (c_{j+1} - c_j)| per segment in longdouble, 0 where an end is
    non-finite; ``magnitudes``: with |lin| and |c_{j+1} - c_j| (the B_j of the
    header's tolerance)."""
    c = np.asarray(row, np.float32).astype(LD)
    m = np.asarray(lin, np.float64).reshape(9).astype(LD)
    ok = np.isfinite(c).all(axis=1)
    ok = ok[1:] & ok[:-1]
    d = np.where(ok[:, None], c[1:], 0) - np.where(ok[:, None], c[:-1], 0)
    if magnitudes:
        d, m = np.abs(d), np.abs(m)
    v = [(m[3 * r] * d[:, 0] + m[3 * r + 1] * d[:, 1]) + m[3 * r + 2] * d[:, 2]
         for r in range(3)]
    return np.where(ok, np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), LD(0))


def point_weights(row, lin, mutant=None, magnitudes=False):
    """w_j = (|v_{j-1}| + |v_j|) / 2 with |v_{-1}| = |v_{L-1}| = 0 (L >= 2)."""
    seg = segment_lengths(row, lin, magnitudes)
    if mutant == 'uniform_weights':
        return np.ones(len(row), LD)
    before = np.concatenate([[LD(0)], seg])
    after = np.concatenate([seg, [LD(0)]])
    w = (before + after) * LD(0.5)
    if mutant == 'ends_not_halved':
        w[0], w[-1] = seg[0], seg[-1]
    return w


def sample(p, volume, mutant=None):
    """(s, S) at the point ``p``: the trilinear sum in the header's order and the
    same sum of magnitudes; None when the point is not sampled."""
    dims = volume.shape
    p = [float(v) for v in p]
    if not all(math.isfinite(v) for v in p):
        return None
    if not all(0.0 <= p[k] <= dims[k] for k in range(3)):
        if mutant != 'outside_clamped':
            return None
        p = [min(max(p[k], 0.0), float(dims[k])) for k in range(3)]
    lo, hi, f, g = [], [], [], []
    for k in range(3):
        u = LD(p[k]) - (LD(0) if mutant == 'no_half_shift' else LD(0.5))
        # p - 0.5 is exact in float64 for a float32 p
        i = math.trunc(float(u)) if mutant == 'truncation' else math.floor(float(u))
        f.append(u - LD(i))
        g.append(LD(1) - f[k])
        lo.append(i)
        hi.append(i + 1)

    def corner(x, y, z):
        idx = (x, y, z)
        if mutant == 'zero_padding' and not all(0 <= idx[k] < dims[k] for k in range(3)):
            return LD(0)
        v = LD(volume[tuple(min(max(idx[k], 0), dims[k] - 1) for k in range(3))])
        if not np.isfinite(v):
            return LD(0) if mutant == 'nonfinite_corner_zero' else None
        return v
    ys, ys_abs = [], []
    for x in (lo[0], hi[0]):
        zs, zs_abs = [], []
        for y in (lo[1], hi[1]):
            v0, v1 = corner(x, y, lo[2]), corner(x, y, hi[2])
            if v0 is None or v1 is None:
                return None
            zs.append(v0 * g[2] + v1 * f[2])
            zs_abs.append(abs(v0) * abs(g[2]) + abs(v1) * abs(f[2]))
        ys.append(zs[0] * g[1] + zs[1] * f[1])
        ys_abs.append(zs_abs[0] * abs(g[1]) + zs_abs[1] * abs(f[1]))
    return ys[0] * g[0] + ys[1] * f[0], ys_abs[0] * abs(g[0]) + ys_abs[1] * abs(f[0])


def weighted_mean(w, values, sampled):
    """(mean, weight) of the header's result rule; NaN and 0 without a mean."""
    weight = w[sampled].sum() if sampled.any() else LD(0)
    if len(w) < 2 or not weight > 0:
        return LD('nan'), LD(0)
    return (w[sampled] * values[sampled]).sum() / weight, weight


def row_mean(row, volume, lin, mutant=None):
    """(mean, weight, bound of the mean, bound of the weight) of one streamline,
    all longdouble; the bounds are the header's, 0 without a mean."""
    L = len(row)
    if L < 2:
        return LD('nan'), LD(0), LD(0), LD(0)
    values, mags = np.zeros(L, LD), np.zeros(L, LD)
    sampled = np.zeros(L, bool)
    for j in range(L):
        got = sample(row[j], volume, mutant)
        if got is not None:
            sampled[j], values[j], mags[j] = True, got[0], got[1]
    w = point_weights(row, lin, mutant)
    mean, weight = weighted_mean(w, values, sampled)
    if not weight > 0:
        return mean, weight, LD(0), LD(0)
    W = point_weights(row, lin, None, magnitudes=True)
    A, M = W[sampled].sum(), (W[sampled] * mags[sampled]).sum()
    bound_weight = (L + 9) * U * A
    bound_mean = U * ((L + 19) * M + (L + 9) * A * M / weight) / weight
    return mean, weight, bound_mean, bound_weight


def sample_mean(points, offsets, volume, lin, mutant=None):
    """(mean, weight, bound_mean, bound_weight), each (n,) longdouble."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    volume = np.asarray(volume, np.float32)
    n = len(offsets) - 1
    out = np.zeros((4, n), LD)
    for s in range(n):
        out[:, s] = row_mean(points[offsets[s]:offsets[s + 1]], volume, lin, mutant)
    return tuple(out)


def round_half_even(x):
    return int(np.rint(x))              # numpy.rint rounds half to even, as llrint does


def round_half_away(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def accumulate_metric(node, mean, n_nodes, scale, metric_q=None, metric_n=None, mutant=None):
    """metric_q and metric_n ((N + 1, N + 1) int64), added to when given."""
    side = n_nodes + 1
    metric_q = np.zeros((side, side), np.int64) if metric_q is None else metric_q
    metric_n = np.zeros((side, side), np.int64) if metric_n is None else metric_n
    for s in range(len(node)):
        n0, n1 = int(node[s, 0]), int(node[s, 1])
        if n0 < 0 or n1 < 0 or n0 > n_nodes or n1 > n_nodes:
            continue
        a, b = min(n0, n1), max(n0, n1)
        scaled = float(mean[s]) * float(scale)
        if not (math.isfinite(float(mean[s])) and abs(scaled) < MAX_Q):
            if mutant == 'nan_rows_counted':
                metric_n[a, b] += 1
            continue
        metric_q[a, b] += round_half_away(scaled) if mutant == 'half_away_from_zero' \
            else round_half_even(scaled)
        metric_n[a, b] += 1
    return metric_q, metric_n


def edge_means(metric_q, metric_n, scale):
    """``mean_<name>`` and ``<name>_n`` of connectome.metric_matrices_from."""
    def symmetric(m):
        inner = m[1:, 1:]
        return inner + inner.T - np.diag(np.diag(inner))
    q, n = symmetric(np.asarray(metric_q, np.int64)), symmetric(np.asarray(metric_n, np.int64))
    mean = np.full(q.shape, np.nan)
    np.divide(q.astype(np.float64) / scale, n, out=mean, where=n > 0)
    return mean, n
