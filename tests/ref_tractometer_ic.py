"""NumPy statement of the Tractometer's invalid connections and full scores
(include/ttl_hip.h, ttl_tractometer_invalid; test infrastructure
only).  The pair of a streamline is found by a literal double loop over the
invalid pair list P; the scores come from Python sets.  ``mutant`` plants one
named deviation; the tests show that each changes what the GPU tests compare.

ROIs are a list of bool (X, Y, Z) masks, already dilated; ``valid`` is a bool
(R, R) matrix (symmetric; the diagonal does not matter).
"""
import numpy as np

import ref_tractometer as ref

MUTANTS = (
    'one_order',       # only e0 in the lower ROI and e1 in the higher one
    'last_pair',       # the last connecting pair of P instead of the first
    'valid_kept',      # valid pairs stay in P
    'assigned_kept',   # rows with a bundle are candidates too
    'trunc_ends',      # int cast for floor
    'shift32',         # a 32-bit shift of the 1: ROIs with r % 64 >= 32 lost
    'word0_only',      # only the first word of a voxel: ROIs >= 64 lost
)


def pair_list(valid, mutant=None):
    """P: the invalid (i, j), i < j, in lexicographic order."""
    R = len(valid)
    return [(i, j) for i in range(R) for j in range(i + 1, R)
            if mutant == 'valid_kept' or not (valid[i][j] or valid[j][i])]


def end_set(c, dims, rois, mutant=None):
    """{r : D_r[floor(c)]}; empty for an end that is non-finite or outside."""
    v = ref.end_voxel(c, dims, 'trunc_ends' if mutant == 'trunc_ends' else None)
    if v is None:
        return frozenset()
    out = set()
    for r, mask in enumerate(rois):
        if mutant == 'shift32' and r % 64 >= 32:
            continue
        if mutant == 'word0_only' and r >= 64:
            continue
        if mask[v]:
            out.add(r)
    return frozenset(out)


def first_pair(A, B, P, R, mutant=None):
    """i * R + j of the first (i, j) of P with connects(i, j), else -1."""
    found = -1
    for i, j in P:
        connects = i in A and j in B
        if mutant != 'one_order':
            connects = connects or (j in A and i in B)
        if connects:
            found = i * R + j
            if mutant != 'last_pair':
                break
    return found


def pairs(points, offsets, bundle, dims, rois, valid, mutant=None):
    """pair int32 [n] of a packed tractogram whose rows carry ``bundle``."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    R = len(rois)
    P = pair_list(valid, mutant)
    memo = {}
    out = np.full(len(offsets) - 1, -1, np.int32)
    for s in range(len(out)):
        row = pts[offsets[s]:offsets[s + 1]]
        if len(row) < 2 or (bundle[s] >= 0 and mutant != 'assigned_kept'):
            continue
        key = (end_set(row[0], dims, rois, mutant), end_set(row[-1], dims, rois, mutant))
        if key not in memo:
            memo[key] = first_pair(key[0], key[1], P, R, mutant)
        out[s] = memo[key]
    return out


# ------------------------------------------------------------------- scores
def _ratio(num, den):
    return num / den if den else 0.0


def _mean(values):
    return float(sum(values) / len(values)) if values else 0.0


def full_result(points, offsets, dims, bundles, names, lin, rois=None, valid=None,
                roi_names=None):
    """The full result of DESIGN 3.12 from sets: ``bundles`` as in
    ref_tractometer (heads and tails dilated), ``rois`` / ``valid`` the
    distinct ROIs (None: the invalid connections are not computed).  Returns
    the dict of ``TractometerValidator.score`` (``index`` left out)."""
    sc = ref.score(points, offsets, dims, bundles, lin)
    bundle, connected = sc['bundle'], sc['connected']
    n = len(bundle)
    vs = int((bundle >= 0).sum())
    pair = np.full(n, -1, np.int32)
    invalid_bundles = {}
    if rois is not None:
        pair = pairs(points, offsets, bundle, dims, rois, valid)
        R = len(rois)
        for p in sorted({int(p) for p in pair if p >= 0}):
            invalid_bundles[f'{roi_names[p // R]}__{roi_names[p % R]}'] = int((pair == p).sum())
    n_ic = int((pair >= 0).sum())
    out_b, per_gt = {}, {'OL': [], 'OR_gt': [], 'OR_vs': [], 'f1': []}
    for b, (B, name) in enumerate(zip(bundles, names)):
        wpc = sum(1 for s in range(n) if bundle[s] < 0 and (int(connected[s]) >> b) & 1)
        entry = {'VS': int((bundle == b).sum()), 'WPC': wpc}
        if B['gt'] is None:
            entry.update(dict.fromkeys(('TP', 'FP', 'FN', 'OL', 'OR_gt', 'OR_vs', 'f1')))
        else:
            M = (sc['visited'] >> np.uint64(b)) & np.uint64(1) != 0
            G = B['gt'] != 0
            tp, fp, fn = int((M & G).sum()), int((M & ~G).sum()), int((G & ~M).sum())
            entry.update(TP=tp, FP=fp, FN=fn, OL=_ratio(tp, int(G.sum())),
                         OR_gt=_ratio(fp, int(G.sum())), OR_vs=_ratio(fp, int(M.sum())),
                         f1=_ratio(2 * tp, int(M.sum()) + int(G.sum())))
            for key in per_gt:
                per_gt[key].append(entry[key])
        out_b[name] = entry
    computed = rois is not None
    ic = n_ic / n if computed else 0
    nc = (n - vs - n_ic) / n if computed else 1 - vs / n
    return {'n': n, 'VS': vs, 'VC': vs / n, 'IC': ic, 'IS': ic + nc if computed else 0, 'NC': nc,
            'VB': len({int(b) for b in bundle if b >= 0}),
            'IB': len(invalid_bundles) if computed else 0,
            'mean_OL': _mean(per_gt['OL']), 'mean_OR_gt': _mean(per_gt['OR_gt']),
            'mean_OR_vs': _mean(per_gt['OR_vs']), 'mean_f1': _mean(per_gt['f1']),
            'bundles': out_b, 'invalid_bundles': invalid_bundles,
            'bundle': bundle, 'pair': pair}
