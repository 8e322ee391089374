"""The definition of ttl_bundle_register_cost (include/ttl_hip.h) in
numpy.longdouble, written from the header: every delta_ij(t) with its bound b =
(K + 8) u A + 6 u G, the intervals [min (delta - b), min (delta + b)] of row_min
and col_min, and the cost with its bound.  The untransformed distances are
ref_bundle_recognize.pair_distances (a test holds the transformed ones to the
same bits under the identity).

``mutant`` names one deliberate misreading of the definition; the CPU tests show
that a witness case tells each from the definition.

``evaluate`` is the callable ``bundle_register.register`` takes in place of the
launch: the same cost in float64 by default (the driver is what a test of it
examines, and a fit takes some hundred evaluations), in longdouble on request."""
import numpy as np

from ref_bundle_recognize import pair_distances

LD = np.longdouble
U = LD(2.0) ** -53

MUTANTS = ('one_sided', 'no_flip', 'unsquared', 'no_quarter', 'distance_in_voxels',
           'transforms_fixed_set', 'transposed_matrix', 'translation_first',
           'nan_line_counts_as_zero', 'mean_over_all_lines', 'first_transform_for_all_t',
           'col_min_over_own_block_only')
#: fixed lines of a workgroup of the kernel (the mutant that forgets the other workgroups)
BLOCK_ROWS = 8


def apply(x, lines, magnitudes=False, translation_first=False):
    """m' of the header for the (3, 4) ``x`` on ``lines`` (.., 3) float32, longdouble;
    with ``magnitudes`` M_c of the header."""
    x = np.asarray(x, np.float64).reshape(3, 4).astype(LD)
    m = np.asarray(lines, np.float32).astype(LD)
    if magnitudes:
        x, m = np.abs(x), np.abs(m)
    with np.errstate(all='ignore'):
        if translation_first:
            m = m + x[:, 3]
            return np.stack([(x[c, 0] * m[..., 0] + x[c, 1] * m[..., 1]) + x[c, 2] * m[..., 2]
                             for c in range(3)], -1)
        return np.stack([((x[c, 0] * m[..., 0] + x[c, 1] * m[..., 1]) + x[c, 2] * m[..., 2]) +
                         x[c, 3] for c in range(3)], -1)


def _dist(a, m, lin, magnitudes=False):
    """|lin (a_k - m_k)| of stations ``a`` (K, 3) against ``m`` (B, K, 3), both
    longdouble: pair_distances without the cast of the models to float32."""
    e = a[None] - m
    A = np.asarray(lin, np.float64).reshape(9).astype(LD)
    if magnitudes:
        e, A = np.abs(e), np.abs(A)
    v = [(A[3 * r] * e[..., 0] + A[3 * r + 1] * e[..., 1]) + A[3 * r + 2] * e[..., 2]
         for r in range(3)]
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def table(fixed, moving, x, lin, mutant=None):
    """delta (A, B) and the ends lo, hi of the interval the kernel's value lies
    in, NaN where a line takes no part; part_f (A,), part_m (B,)."""
    fixed = np.asarray(fixed, np.float32)
    moving = np.asarray(moving, np.float32)
    K = fixed.shape[1]
    use_lin = np.eye(3) if mutant == 'distance_in_voxels' else lin
    x = np.asarray(x, np.float64).reshape(3, 4)
    if mutant == 'transposed_matrix':
        x = np.concatenate([x[:, :3].T, x[:, 3:]], 1)
    a_all, m_all = fixed.astype(LD), moving.astype(LD)
    if mutant == 'transforms_fixed_set':
        a_all = apply(x, fixed)
        big = np.zeros_like(m_all)
    else:
        m_all = apply(x, moving, translation_first=mutant == 'translation_first')
        big = apply(x, moving, magnitudes=True)
    with np.errstate(all='ignore'):
        part_f = np.isfinite(a_all).all((1, 2)) & np.isfinite(fixed).all((1, 2))
        part_m = np.isfinite(m_all).all((1, 2)) & np.isfinite(moving).all((1, 2))
        if mutant == 'nan_line_counts_as_zero':
            a_all = np.where(np.isfinite(a_all), a_all, 0)
            m_all = np.where(np.isfinite(m_all), m_all, 0)
            part_f[:], part_m[:] = True, True
        A_n, B_n = len(fixed), len(moving)
        delta, lo, hi = (np.full((A_n, B_n), np.nan, LD) for _ in range(3))
        zero = np.zeros((1, 3), LD)
        G = _dist(zero, big, use_lin, True).sum(1) / LD(K)           # (B,)
        for i in np.flatnonzero(part_f):
            a = a_all[i]
            D = _dist(a, m_all, use_lin).sum(1) / LD(K)
            F = _dist(a[::-1], m_all, use_lin).sum(1) / LD(K)
            bd = (K + 8) * U * _dist(a, m_all, use_lin, True).sum(1) / LD(K) + 6 * U * G
            bf = (K + 8) * U * _dist(a[::-1], m_all, use_lin, True).sum(1) / LD(K) + 6 * U * G
            if mutant == 'no_flip':
                F, bf = D, bd
            # the kernel's min(D', F') with D' within bd of D and F' within bf of F
            delta[i] = np.minimum(D, F)
            lo[i], hi[i] = np.minimum(D - bd, F - bf), np.minimum(D + bd, F + bf)
        for v in (delta, lo, hi):
            v[:, ~part_m] = np.nan
    return delta, lo, hi, part_f, part_m


def _mean(v):
    v = v[~np.isnan(v.astype(np.float64))]
    return (v.sum() / LD(len(v))) if len(v) else LD(np.nan)


def _minima(delta, lo, hi, axis):
    """(value, lo, hi) of the minimum along ``axis``; NaN where there is none."""
    with np.errstate(all='ignore'):
        nan = np.isnan(delta.astype(np.float64))
        none = nan.all(axis)
        out = [np.where(none, LD(np.nan), np.where(nan, LD(np.inf), v).min(axis))
               for v in (delta, lo, hi)]
    return out


def cost(fixed, moving, xf, lin, mutant=None):
    """dict over the T transforms ``xf`` (T, 3, 4): row_min, row_lo, row_hi (T, A),
    col_min, col_lo, col_hi (T, B), cost, cost_bound (T,), longdouble; NaN where
    the header says NaN."""
    xf = np.asarray(xf, np.float64).reshape(-1, 3, 4)
    T, A_n, B_n = len(xf), len(fixed), len(moving)
    out = {k: np.full((T, A_n), np.nan, LD) for k in ('row_min', 'row_lo', 'row_hi')}
    out.update({k: np.full((T, B_n), np.nan, LD) for k in ('col_min', 'col_lo', 'col_hi')})
    out['cost'], out['cost_bound'] = np.full(T, np.nan, LD), np.full(T, np.nan, LD)
    for t in range(T):
        x = xf[0] if mutant == 'first_transform_for_all_t' else xf[t]
        delta, lo, hi, part_f, part_m = table(fixed, moving, x, lin, mutant)
        out['row_min'][t], out['row_lo'][t], out['row_hi'][t] = _minima(delta, lo, hi, 1)
        if mutant == 'col_min_over_own_block_only':
            delta, lo, hi = delta[:BLOCK_ROWS], lo[:BLOCK_ROWS], hi[:BLOCK_ROWS]
        out['col_min'][t], out['col_lo'][t], out['col_hi'][t] = _minima(delta, lo, hi, 0)
        rows, cols = out['row_min'][t], out['col_min'][t]
        if mutant == 'mean_over_all_lines':
            with np.errstate(all='ignore'):
                r = np.nansum(rows.astype(np.float64)).astype(LD) / LD(A_n)
                c = np.nansum(cols.astype(np.float64)).astype(LD) / LD(B_n)
        else:
            r, c = _mean(rows), _mean(cols)
        s = r if mutant == 'one_sided' else r + c
        value = s if mutant == 'unsquared' else s * s
        out['cost'][t] = value if mutant == 'no_quarter' else value / LD(4)
        with np.errstate(all='ignore'):
            e_r = _mean(out['row_hi'][t] - out['row_lo'][t]) + (-(-A_n // 64) + 6) * U * r
            e_c = _mean(out['col_hi'][t] - out['col_lo'][t]) + (-(-B_n // 64) + 6) * U * c
            e_s = e_r + e_c + U * s
            out['cost_bound'][t] = (2 * s * e_s + e_s * e_s) / 4 + 2 * U * out['cost'][t]
    return out


def evaluate(fixed, moving, lin, dtype=np.float64):
    """``evaluate(mats (T, 3, 4)) -> costs (T,)`` for bundle_register.register:
    the definition's cost over the lines that take part, all T at once in
    ``dtype``."""
    fixed = np.asarray(fixed, np.float32).astype(dtype)
    moving = np.asarray(moving, np.float32).astype(dtype)
    lin = np.asarray(lin, np.float64).astype(dtype)
    fixed = fixed[np.isfinite(fixed).all((1, 2))]
    la = fixed @ lin.T                                   # (A, K, 3)

    def run(mats):
        mats = np.asarray(mats, np.float64).reshape(-1, 3, 4).astype(dtype)
        out = np.full(len(mats), np.nan)
        for t, x in enumerate(mats):
            with np.errstate(all='ignore'):
                m = moving @ x[:, :3].T + x[:, 3]
                m = m[np.isfinite(m).all((1, 2))]
                if not len(m) or not len(la):
                    continue
                lm = m @ lin.T
                D = np.sqrt(((la[:, None] - lm[None]) ** 2).sum(-1)).mean(-1)
                F = np.sqrt(((la[:, None, ::-1] - lm[None]) ** 2).sum(-1)).mean(-1)
                delta = np.minimum(D, F)
                s = delta.min(1).mean() + delta.min(0).mean()
                out[t] = float(s * s / 4)
        return out
    return run


__all__ = ['MUTANTS', 'apply', 'table', 'cost', 'evaluate', 'pair_distances', 'LD', 'U']
