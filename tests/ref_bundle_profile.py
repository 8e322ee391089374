"""The definition of ttl_bundle_orient / ttl_bundle_profile (include/ttl_hip.h,
DESIGN 3.18) as a literal loop over streamlines.  The stations are the library
resampler's bits (ref_oracle_validator.resample_blocked); the two distances D and
F are numpy.longdouble with the header's bound, the yardstick of the kernel's
float64 chain; the sample value is restated in float64 in the kernel's order
(Python floats: IEEE double, no fused operation), so the integer sums and
``values`` are the kernel's exactly.

``mutant`` names one deliberate misreading of the definition; the CPU tests show
that the witness set tells each from the definition, so a kernel that made that
mistake could not pass the GPU tests."""
import math

import numpy as np

from ref_oracle_validator import resample_blocked

LD = np.longdouble
U = LD(2.0) ** -53
MAX_Q = 2.0 ** 40

ORIENT_MUTANTS = ('flip_on_tie', 'distance_in_voxels', 'sum_not_divided',
                  'reverse_model_not_row', 'half_away_from_zero', 'partial_row_added')
PROFILE_MUTANTS = ('half_away_from_zero', 'unsampled_counts_as_zero', 'square_of_rounded')
MUTANTS = ORIENT_MUTANTS + PROFILE_MUTANTS[1:]


def round_half_even(x):
    return int(np.rint(x))              # numpy.rint rounds half to even, as llrint does


def round_half_away(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _round(x, mutant):
    return round_half_away(x) if mutant == 'half_away_from_zero' else round_half_even(x)


def distances(a, m, lin, magnitudes=False):
    """|lin (a_k - m_k)| per station in longdouble; ``magnitudes``: with |lin| and
    |a - m| (the header's A)."""
    e = np.asarray(a, np.float32).astype(LD) - np.asarray(m, np.float32).astype(LD)
    A = np.asarray(lin, np.float64).reshape(9).astype(LD)
    if magnitudes:
        e, A = np.abs(e), np.abs(A)
    v = [(A[3 * r] * e[:, 0] + A[3 * r + 1] * e[:, 1]) + A[3 * r + 2] * e[:, 2] for r in range(3)]
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def takes_part(row, b, B):
    return 0 <= b < B and len(row) >= 2 and bool(np.isfinite(row).all())


def orient(points, offsets, bundle, B, K, model, lin, scale, mutant=None):
    """dict: flip (n,) int, mdf / mdf_bound (n,) longdouble (mdf_bound: the header's
    (K + 8) u A of the distance that was chosen, D's or F's own), decided (n,) bool
    (|D - F| above the sum of the two bounds), part (n,) bool, sum_q (B, K, 3) and sum_n (B,) int64,
    stations (n, K, 3) float32 (the r_k, zeros for a row that is not resampled)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    model = np.asarray(model, np.float32).reshape(B, K, 3)
    n = len(offsets) - 1
    out = {'flip': np.zeros(n, np.int32), 'mdf': np.full(n, np.nan, LD),
           'mdf_bound': np.zeros(n, LD), 'decided': np.ones(n, bool), 'part': np.zeros(n, bool),
           'sum_q': np.zeros((B, K, 3), object), 'sum_n': np.zeros(B, np.int64),
           'stations': np.zeros((n, K, 3), np.float32)}
    use_lin = np.eye(3) if mutant == 'distance_in_voxels' else lin
    with np.errstate(all='ignore'):
        for s in range(n):
            row, b = points[offsets[s]:offsets[s + 1]], int(bundle[s])
            if not takes_part(row, b, B):
                continue
            r = resample_blocked(row, K)
            out['stations'][s] = r
            in_range = np.abs(r.astype(np.float64) * scale) < MAX_Q
            if not in_range.all():
                if mutant == 'partial_row_added':    # stations before the first bad one
                    stop = int(np.flatnonzero(~in_range.all(axis=1))[0])
                    for k in range(stop):
                        for c in range(3):
                            out['sum_q'][b, k, c] += round_half_even(float(r[k, c]) * scale)
                continue
            out['part'][s] = True
            div = LD(1) if mutant == 'sum_not_divided' else LD(K)
            D = distances(r, model[b], use_lin).sum() / div
            F = distances(r[::-1], model[b], use_lin).sum() / div
            bound_d = (K + 8) * U * distances(r, model[b], use_lin, True).sum() / LD(K)
            bound_f = (K + 8) * U * distances(r[::-1], model[b], use_lin, True).sum() / LD(K)
            flip = bool(F <= D) if mutant == 'flip_on_tie' else bool(F < D)
            out['flip'][s] = int(flip)
            out['mdf'][s] = F if flip else D
            out['mdf_bound'][s] = bound_f if flip else bound_d
            # a NaN distance is decided: every comparison is false
            out['decided'][s] = bool(np.isnan(D) or np.isnan(F) or abs(D - F) > bound_d + bound_f)
            o = r[::-1] if flip and mutant != 'reverse_model_not_row' else r
            for k in range(K):
                for c in range(3):
                    out['sum_q'][b, k, c] += _round(float(o[k, c]) * scale, mutant)
            out['sum_n'][b] += 1
    out['sum_q'] = out['sum_q'].astype(np.int64)
    return out


def sample_f64(p, volume):
    """ttl_tract_sample_mean's sample at ``p`` in float64, in the kernel's order;
    None when the point is not sampled."""
    dims = volume.shape
    p = [float(v) for v in p]
    lo, hi, f = [], [], []
    for k in range(3):
        if not (p[k] >= 0.0 and p[k] <= float(dims[k])):
            return None
        u = p[k] - 0.5
        i = math.floor(u)
        f.append(u - i)
        lo.append(max(int(i), 0))
        hi.append(min(int(i) + 1, dims[k] - 1))
    g = [1.0 - v for v in f]
    cy, finite = [], True
    for x in (lo[0], hi[0]):
        cz = []
        for y in (lo[1], hi[1]):
            v0, v1 = float(volume[x, y, lo[2]]), float(volume[x, y, hi[2]])
            finite = finite and math.isfinite(v0) and math.isfinite(v1)
            cz.append(v0 * g[2] + v1 * f[2])
        cy.append(cz[0] * g[1] + cz[1] * f[1])
    return (cy[0] * g[0] + cy[1] * f[0]) if finite else None


def profile(points, offsets, bundle, flip, B, K, volume, scale, scale_sq, mutant=None):
    """dict: sum_q, sum_qq, count (B, K) int64; values (n, K) float64."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    volume = np.asarray(volume, np.float32)
    n = len(offsets) - 1
    sum_q, sum_qq = np.zeros((B, K), object), np.zeros((B, K), object)
    count = np.zeros((B, K), np.int64)
    values = np.full((n, K), np.nan)
    with np.errstate(all='ignore'):
        for s in range(n):
            row, b = points[offsets[s]:offsets[s + 1]], int(bundle[s])
            if not takes_part(row, b, B):
                continue
            r = resample_blocked(row, K)
            o = r[::-1] if flip[s] else r
            for k in range(K):
                v = sample_f64(o[k], volume)
                if v is None:
                    if mutant != 'unsampled_counts_as_zero':
                        continue
                    v = 0.0
                else:
                    values[s, k] = v
                q, qq = v * scale, (v * v) * scale_sq
                if not (abs(q) < MAX_Q and abs(qq) < MAX_Q):
                    continue
                iq = _round(q, mutant)
                if mutant == 'square_of_rounded':
                    w = iq / scale
                    qq = (w * w) * scale_sq
                sum_q[b, k] += iq
                sum_qq[b, k] += _round(qq, mutant)
                count[b, k] += 1
    return {'sum_q': sum_q.astype(np.int64), 'sum_qq': sum_qq.astype(np.int64), 'count': count,
            'values': values}
