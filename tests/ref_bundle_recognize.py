"""The definition of ttl_bundle_recognize (include/ttl_hip.h) as a
loop over streamlines, written from the header.  The stations are the library
resampler's bits (ref_oracle_validator.resample_blocked); D_m and F_m of every
(row, model) pair are numpy.longdouble with the header's bound b = (K + 8) u A,
the yardstick of the kernel's float64 chain.  ``pair_distances`` is
ref_bundle_profile.distances for one row against all models at once (the loop
over models is NumPy's; a test holds the two to the same bits).

Per row: the winner, ``decided`` (the winner's delta + b is below every other
model's delta - b, and the winner's own |D - F| exceeds its two bounds) and the
intervals [min_m (delta_m - b_m), min_m (delta_m + b_m)] in which a kernel that
is within the bound on every pair must land: over all models for ``mdf``, over
the models of another label than the winner's for ``runner_up``.

``mutant`` names one deliberate misreading of the definition; the CPU tests show
that the witness set tells each from the definition."""
import numpy as np

from ref_oracle_validator import resample_blocked

LD = np.longdouble
U = LD(2.0) ** -53

MUTANTS = ('highest_index_on_tie', 'flip_on_tie', 'distance_in_voxels', 'squared_distances',
           'direct_only', 'flip_of_last_model', 'runner_up_same_label', 'nan_wins',
           'short_row_takes_part')


def pair_distances(a, models, lin, magnitudes=False):
    """|lin (a_k - m_k)| of the stations ``a`` (K, 3) against ``models`` (M, K, 3):
    (M, K) longdouble, ref_bundle_profile.distances per model."""
    e = np.asarray(a, np.float32).astype(LD)[None] - np.asarray(models, np.float32).astype(LD)
    A = np.asarray(lin, np.float64).reshape(9).astype(LD)
    if magnitudes:
        e, A = np.abs(e), np.abs(A)
    v = [(A[3 * r] * e[..., 0] + A[3 * r + 1] * e[..., 1]) + A[3 * r + 2] * e[..., 2]
         for r in range(3)]
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def takes_part(row):
    return len(row) >= 2 and bool(np.isfinite(row).all())


def _lowest(values, keep):
    """(lower end, upper end) of the minimum over ``keep`` of pairs (lo, hi); NaNs
    when nothing is kept."""
    lo, hi = values
    if not keep.any():
        return LD(np.nan), LD(np.nan)
    return lo[keep].min(), hi[keep].min()


def recognize(points, offsets, models, lin, label=None, mutant=None):
    """dict of (n,) arrays: best, flip (int32), mdf / runner_up (longdouble, the
    definition's own value), mdf_lo / mdf_hi / ru_lo / ru_hi (the intervals),
    decided, part (bool); pairs: D, F, bound_d, bound_f (n, M) longdouble."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    models = np.asarray(models, np.float32)
    M, K = models.shape[:2]
    label = np.arange(M) if label is None else np.asarray(label)
    n = len(offsets) - 1
    nan = LD(np.nan)
    out = {'best': np.full(n, -1, np.int32), 'flip': np.zeros(n, np.int32),
           'decided': np.ones(n, bool), 'part': np.zeros(n, bool)}
    for key in ('mdf', 'mdf_lo', 'mdf_hi', 'runner_up', 'ru_lo', 'ru_hi'):
        out[key] = np.full(n, nan, LD)
    for key in ('D', 'F', 'bound_d', 'bound_f'):
        out[key] = np.full((n, M), nan, LD)
    use_lin = np.eye(3) if mutant == 'distance_in_voxels' else lin
    with np.errstate(all='ignore'):
        for s in range(n):
            row = points[offsets[s]:offsets[s + 1]]
            if not takes_part(row):
                if not (mutant == 'short_row_takes_part' and len(row) == 1 and
                        np.isfinite(row).all()):
                    continue
                r = np.repeat(row, K, 0)
            else:
                r = resample_blocked(row, K)
            out['part'][s] = True
            d, f = pair_distances(r, models, use_lin), pair_distances(r[::-1], models, use_lin)
            if mutant == 'squared_distances':
                d, f = d * d, f * f
            D, F = d.sum(1) / LD(K), f.sum(1) / LD(K)
            bd = (K + 8) * U * pair_distances(r, models, use_lin, True).sum(1) / LD(K)
            bf = (K + 8) * U * pair_distances(r[::-1], models, use_lin, True).sum(1) / LD(K)
            for key, v in (('D', D), ('F', F), ('bound_d', bd), ('bound_f', bf)):
                out[key][s] = v
            flips = F <= D if mutant == 'flip_on_tie' else F < D
            if mutant == 'direct_only':
                flips = np.zeros(M, bool)
            delta, bound = np.where(flips, F, D), np.where(flips, bf, bd)
            valid = ~np.isnan(delta)
            if mutant == 'nan_wins' and not valid.all():
                w = int(np.flatnonzero(~valid)[0])
                out['best'][s], out['flip'][s], out['mdf'][s] = w, int(flips[w]), delta[w]
                continue
            if not valid.any():
                continue
            idx = np.flatnonzero(valid)
            lowest = delta[idx].min()
            ties = idx[delta[idx] == lowest]
            w = int(ties[-1] if mutant == 'highest_index_on_tie' else ties[0])
            out['best'][s] = w
            out['flip'][s] = int(flips[M - 1] if mutant == 'flip_of_last_model' else flips[w])
            out['mdf'][s] = delta[w]
            # an infinite distance is exact: it has no interval around it
            finite = np.isfinite(delta)
            ends = (np.where(finite, delta - bound, delta), np.where(finite, delta + bound, delta))
            others = valid.copy()
            others[w] = False
            own = np.isnan(D[w]) or np.isnan(F[w]) or abs(D[w] - F[w]) > bd[w] + bf[w]
            out['decided'][s] = bool(own and (ends[1][w] < ends[0][others]).all())
            out['mdf_lo'][s], out['mdf_hi'][s] = _lowest(ends, valid)
            other_label = valid & (label != label[w])
            if mutant == 'runner_up_same_label':
                other_label = others
            if other_label.any():
                out['runner_up'][s] = delta[other_label].min()
            out['ru_lo'][s], out['ru_hi'][s] = _lowest(ends, other_label)
    return out
