"""The ROI sets and streamlines that tests/test_tractometer_ic.py launches,
built once (test infrastructure only).  Volume (12, 9, 7), as
tests/tractometer_cases.py.  A set of R ROIs has its deciding ROIs at the
indices of DECIDING that are below R (0-2, 62-66, 125-127: a pair can straddle
the boundary between a voxel's two words); the k-th of them owns the column of
voxels x = k, y 0-2, z 1-2, and shares the voxels x = k, y 4-5, z 1-2 with the
(k + 1)-th.  Every other index is a filler: a few random voxels of the slab
z = 0, where the random walks end, so that their end sets hold many ROIs.

Valid pairs: (0, 1) when R >= 3 and (63, 64) when R >= 65 among the deciding
ROIs, a random third of the pairs that involve a filler.
"""
import functools

import numpy as np

import ref_tractometer_ic as ric
from ref_oracle_validator import random_walks
from tractometer_cases import _line, pack

DIMS = (12, 9, 7)
SETS = (2, 3, 64, 65, 128)
DECIDING = (0, 1, 2, 62, 63, 64, 65, 66, 125, 126, 127)


def deciding(R):
    return [r for r in DECIDING if r < R]


@functools.lru_cache(maxsize=None)
def roi_set(R):
    """(rois: list of R bool masks, valid: bool (R, R))."""
    rng = np.random.default_rng(500 + R)
    S = deciding(R)
    rois = [None] * R
    for k, r in enumerate(S):
        m = np.zeros(DIMS, bool)
        m[k, 0:3, 1:3] = True
        m[k, 4:6, 1:3] = True
        if k > 0:
            m[k - 1, 4:6, 1:3] = True
        rois[r] = m
    for r in range(R):
        if rois[r] is None:
            m = np.zeros(DIMS, bool)
            m[rng.integers(0, 12, 6), rng.integers(0, 9, 6), 0] = True
            rois[r] = m
    valid = rng.random((R, R)) < 0.3
    valid = valid | valid.T
    for i in S:
        for j in S:
            valid[i, j] = False
    if R >= 3:
        valid[0, 1] = valid[1, 0] = True
    if R >= 65:
        valid[63, 64] = valid[64, 63] = True
    valid |= np.eye(R, dtype=bool)
    return rois, valid


def own(k, y=1.5, z=1.5):
    """A point in the k-th deciding ROI and in no other."""
    return (k + 0.5, y, z)


def shared(k):
    """A point in the k-th and the (k + 1)-th deciding ROI."""
    return (k + 0.5, 4.5, 1.5)


def designed_rows(R):
    """[(name, points, bundle carried, expected pair as (i, j), None for no
    pair)]: the expectations are worked out by hand from the layout above."""
    S = deciding(R)
    rows = []

    def add(name, pts, want, bundle=-1):
        rows.append((name, _line(*pts), bundle, want))

    def inv(p, q):      # the deciding ROIs at positions p, q as an invalid pair
        i, j = sorted((S[p], S[q]))
        return (i, j)

    nan, inf = float('nan'), float('inf')
    if R == 2:          # one pair, and it is invalid
        far, pair = 1, inv(0, 1)
        add('same_two_rois', [shared(0), shared(0)], pair)
    else:
        far, pair = 2, inv(0, 2)
        add('valid_only_wpc', [own(0), own(1)], None)
        add('valid_only_reversed', [own(1), own(0)], None)
        add('valid_then_invalid', [own(0), shared(1)], pair)
        add('invalid_then_valid_ends_swapped', [shared(1), own(0)], pair)
        # A = {0, 1}, B = {1, 2}: (0, 1) is valid, (0, 2) comes before (1, 2)
        add('overlap_priority', [shared(0), shared(1)], pair)
        add('overlap_priority_reversed', [shared(1), shared(0)], pair)
        add('same_two_rois', [shared(0), shared(0)], None)         # (0, 1) is valid
    add('forward', [own(0), own(far)], pair)
    add('backward', [own(far), own(0)], pair)
    add('three_points', [own(0), (6.5, 7.5, 5.5), own(far)], pair)
    add('same_roi', [own(0), own(0, 2.5, 2.5)], None)
    add('same_roi_overlap_voxel', [own(0), (0.5, 5.5, 2.5)], None if R > 2 else pair)
    add('end_on_face', [(0.0, 0.0, 1.0), (float(far), 2.999, 2.999)], pair)
    add('end_minus_third', [(-0.3, 1.5, 1.5), own(far)], None)      # floor(-0.3) = -1
    add('end_minus_third_last', [own(far), (0.5, -0.3, 1.5)], None)
    add('end_outside', [own(0), (12.5, 1.5, 1.5)], None)
    add('end_nan', [own(0), (far + 0.5, nan, 1.5)], None)
    add('end_inf', [(inf, 1.5, 1.5), own(far)], None)
    add('nan_inside_is_not_read', [own(0), (nan, inf, nan), own(far)], pair)
    add('no_points', [], None)
    add('one_point', [own(0)], None)
    add('carries_bundle', [own(0), own(far)], None, bundle=0)
    add('carries_bundle_high', [own(far), own(0)], None, bundle=63)
    add('end_in_no_roi', [own(0), (6.5, 7.5, 5.5)], None)
    if R >= 64:         # bits 62, 63: a 32-bit shift loses them
        add('top_of_word0', [own(3), own(4)], inv(3, 4))
        add('low_and_top_of_word0', [own(4), own(1)], inv(1, 4))
    if R >= 65:         # i in word 0, j in word 1
        add('straddle', [own(3), own(5)], inv(3, 5))                  # (62, 64)
        add('straddle_reversed', [own(5), own(3)], inv(3, 5))
        add('straddle_valid', [own(4), own(5)], None)                 # (63, 64) is valid
        add('low_to_word1', [own(5), own(2)], inv(2, 5))              # (2, 64)
        # A = {62, 63}, B = {63, 64}: (62, 63) before (62, 64); (63, 64) is valid
        add('straddle_priority', [shared(3), shared(4)], inv(3, 4))
    if R >= 128:
        add('both_in_word1', [own(6), own(7)], inv(6, 7))             # (65, 66)
        add('last_bits', [own(10), own(9)], inv(9, 10))               # (126, 127)
        add('first_to_last', [own(10), own(0)], inv(0, 10))           # (0, 127)
        # A = {63}, B = {64, 65}: (63, 64) is valid, (63, 65) is not
        add('valid_then_invalid_straddle', [own(4), shared(5)], inv(4, 6))
        add('word1_priority', [shared(8), shared(9)], inv(8, 9))      # (125, 126) first
    # every ordered pair of deciding ROIs
    for p in range(len(S)):
        for q in range(len(S)):
            i, j = sorted((S[p], S[q]))
            valid = (i, j) in ((0, 1), (63, 64)) and R >= 3
            add(f'own_{S[p]}_to_{S[q]}', [own(p), own(q)],
                None if p == q or valid else (i, j))
    return rows


@functools.lru_cache(maxsize=None)
def case(R):
    """The designed rows and 120 random walks whose ends lie in the fillers'
    slab, packed: dict(points, offsets, bundle, names, want (pair number, -1,
    or None where only the definition says), rois, valid, pair = the
    definition's)."""
    rng = np.random.default_rng(40 + R)
    rows = designed_rows(R)
    walks = random_walks(rng, 120, 2, 30, 12, step=(0.3, 1.9), start=(0, 9))
    walks = [np.clip(w, np.float32(0.05), np.float32(8.9)) for w in walks]
    for w in walks:
        w[0, 2] = w[-1, 2] = 0.5
    for w in walks[:30]:                      # from a filler voxel into a deciding ROI
        w[-1] = own(int(rng.integers(0, len(deciding(R)))))
    lines = [r[1] for r in rows] + walks
    names = [r[0] for r in rows] + [f'walk_{i}' for i in range(len(walks))]
    bundle = np.array([r[2] for r in rows] + [3 if i % 5 == 4 else -1
                                              for i in range(len(walks))], np.int32)
    want = [-1 if r[3] is None else r[3][0] * R + r[3][1] for r in rows] + [None] * len(walks)
    points, offsets = pack(lines)
    rois, valid = roi_set(R)
    return {'points': points, 'offsets': offsets, 'bundle': bundle, 'names': names,
            'want': want, 'rois': rois, 'valid': valid,
            'pair': ric.pairs(points, offsets, bundle, DIMS, rois, valid)}


GRID_BLOCKS = 2048                   # the launch's cap on workgroups (ttl_hip.h)
GRID_PASS = GRID_BLOCKS * 256        # rows of one pass of the capped grid
PERIOD = 37                          # prime: no two rows a pass apart are the same row


@functools.lru_cache(maxsize=None)
def periodic_case(n_rows, R=128):
    """``n_rows`` rows that repeat PERIOD rows of the R-ROI set (two or three
    points each, with and without a pair, some carrying a bundle), and their
    pairs: the period's, repeated."""
    c = case(R)
    lens = np.diff(c['offsets'])
    short = [r for r in range(len(lens)) if 2 <= lens[r] <= 3]
    with_pair = [r for r in short if c['pair'][r] >= 0][:24]
    without = [r for r in short if c['pair'][r] < 0][:PERIOD - len(with_pair)]
    chosen = (with_pair + without)[:PERIOD]
    assert len(chosen) == PERIOD and len(with_pair) >= 12
    chosen = [chosen[(5 * k) % PERIOD] for k in range(PERIOD)]        # mixed
    lines = [c['points'][c['offsets'][r]:c['offsets'][r + 1]] for r in chosen]
    points, offsets = pack(lines)
    reps = -(-n_rows // PERIOD)
    all_points = np.tile(points, (reps, 1))
    lens = np.tile(np.diff(offsets), reps)[:n_rows]
    all_offsets = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=all_offsets[1:])
    return {'points': np.ascontiguousarray(all_points[:all_offsets[-1]]), 'offsets': all_offsets,
            'bundle': np.tile(c['bundle'][chosen], reps)[:n_rows].copy(),
            'pair': np.tile(c['pair'][chosen], reps)[:n_rows].copy(),
            'rois': c['rois'], 'valid': c['valid'], 'period_rows': chosen}
