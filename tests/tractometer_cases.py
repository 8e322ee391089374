"""The scoring sets and streamlines that tests/test_tractometer.py launches,
built once (test infrastructure only).  Volume (12, 9, 7): unequal dims, so a
swapped index shows.  A set of B bundles has its roles at these bits:

    B = 3:   0 limits (L),  1 all / any masks (AY),  2 angle (W)
    B = 33: 32 L, 31 AY, 30 W,  2 and 5 the priority pair (P2, P5)
    B = 64: 63 L, 62 AY, 61 W,  2 and 5 the priority pair

Every other bit is a filler bundle: a few random ROI voxels in the slab z = 0,
which the designed rows never end in.  The roles live in slabs of their own
(AY z 1-2, P z 3, L z 4, W z 5-6) with the head at low x and the tail at high x.

Also the scaffolding that test_tractometer.py, test_tractometer_ic.py and
tractometer_ic_cases.py share: ``_box``, ``_line``, ``pack``, the end-to-end
space ``AFFINE`` with its env (``env``) and .trk files (``save_trk``), and the
trainer runs' dataset and arguments (``_write_dataset``, ``_train_args``).
"""
import functools
from types import SimpleNamespace

import numpy as np

import ref_tractometer as ref
from ref_oracle_validator import random_walks

DIMS = (12, 9, 7)
AFFINE = np.array([[1.8793852415718169, -0.5130302149885031, 0.0, -11.0],
                   [0.6840402866513374, 1.4095389311788626, 0.0, 4.5],
                   [0.0, 0.0, 1.25, -3.0],
                   [0.0, 0.0, 0.0, 1.0]])      # 20 degrees about z, zooms (2, 1.5, 1.25)
# not symmetric, so a transposed lin shows; entries multiples of 2^-2
LIN = np.array([[2.0, 0.5, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 1.25]])
ROLES = {3: {'L': 0, 'AY': 1, 'W': 2},
         33: {'L': 32, 'AY': 31, 'W': 30, 'P2': 2, 'P5': 5},
         64: {'L': 63, 'AY': 62, 'W': 61, 'P2': 2, 'P5': 5}}
INF = float('inf')
ANGLE = 215.0        # between the shallow arcs' winding and the deep ones' (asserted)


def _box(x, y, z):
    m = np.zeros(DIMS, bool)
    m[x[0]:x[1], y[0]:y[1], z[0]:z[1]] = True
    return m


@functools.lru_cache(maxsize=None)
def scoring_set(B):
    """The list of bundle dicts (ref_tractometer.bundle) of a B-bundle set."""
    rng = np.random.default_rng(100 + B)
    roles = ROLES[B]
    bundles = [None] * B
    all_y = (0, 9)
    bundles[roles['L']] = ref.bundle(
        _box((0, 2), all_y, (4, 5)), _box((10, 12), all_y, (4, 5)),
        gt=_box((0, 12), (2, 5), (4, 5)), length=[16.5, 26.0],
        dir=[[16.5, 23.0], [0, 3.0], [0, INF]], absdir=[[0, INF], [0, INF], [0, 2.5]])
    inside = _box((0, 12), all_y, (1, 3))
    inside[5, 4, 1] = False                      # the hole
    touch = np.zeros(DIMS, bool)
    touch[5, 4, 2] = touch[8, 5, 1] = True
    bundles[roles['AY']] = ref.bundle(
        _box((0, 2), all_y, (1, 3)), _box((10, 12), all_y, (1, 3)), all=inside, any=touch)
    bundles[roles['W']] = ref.bundle(
        _box((0, 3), all_y, (5, 7)), _box((9, 12), all_y, (5, 7)),
        gt=_box((3, 9), (2, 7), (5, 7)), angle=ANGLE)
    if 'P2' in roles:
        head, tail = _box((0, 2), all_y, (3, 4)), _box((10, 12), all_y, (3, 4))
        tube = _box((0, 12), (3, 6), (3, 4))
        bundles[roles['P2']] = ref.bundle(head, tail, gt=tube, length=[0, 24.0])
        bundles[roles['P5']] = ref.bundle(head, tail, gt=tube)
    for b in range(B):
        if bundles[b] is not None:
            continue
        rois = []
        for _ in range(2):
            m = np.zeros(DIMS, bool)
            m[rng.integers(0, 12, 6), rng.integers(0, 9, 6), 0] = True
            rois.append(m)
        gt = None
        if rng.random() < 0.5:
            gt = rng.random(DIMS) < 0.1
        bundles[b] = ref.bundle(rois[0], rois[1], gt=gt)
    return bundles


def tables(bundles):
    """The arguments of ``ScoringData`` / ``limits_table`` from bundle dicts:
    (heads, tails, alls, anys, gts, lengths, angles, dirs, absdirs)."""
    cols = [[B[k] for B in bundles] for k in
            ('head', 'tail', 'all', 'any', 'gt', 'length', 'angle', 'dir', 'absdir')]
    return tuple(cols)


def _line(*pts):
    return np.array(pts, np.float32).reshape(-1, 3)


def pack(lines):
    offsets = np.zeros(len(lines) + 1, np.int64)
    np.cumsum([len(s) for s in lines], out=offsets[1:])
    points = np.concatenate([np.asarray(s, np.float32).reshape(-1, 3) for s in lines])
    return points.astype(np.float32), offsets


def env(affine=AFFINE):
    """What a validator reads of an env whose tracking and reference space is
    ``affine`` over DIMS."""
    from tracktolearn_amd.datasets.utils import MRIDataVolume
    return SimpleNamespace(tracking_mask=MRIDataVolume(np.ones(DIMS, np.uint8), affine),
                           affine_vox2rasmm=affine, reference={'affine': affine, 'shape': DIMS})


def save_trk(streamlines, path, data_per_streamline=None):
    """Tracker-voxel streamlines of AFFINE's space (centre origin) as a .trk."""
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    world = Tractogram(streamlines, data_per_streamline).apply_affine(AFFINE)
    sio.save_trk(world, path, sio.create_tractogram_header(AFFINE, DIMS, (2.0, 1.5, 1.25)))


def _write_dataset(path, D=20):
    # the synthetic dataset of tests/test_oracle_validator.py
    from tracktolearn_amd.datasets.SubjectDataset import write_npz_dataset
    from tracktolearn_amd.utils.synthetic import synthetic_volumes
    subs = {}
    for i, sid in enumerate(('sub-a', 'sub-b')):
        sh, mask, pk = synthetic_volumes(D, 45, seed=50 + i)
        aff = np.eye(4, dtype=np.float32)
        subs[sid] = {'input_volume': (sh, aff), 'peaks_volume': (pk, aff),
                     'tracking_volume': (mask, aff), 'seeding_volume': (mask, aff)}
    write_npz_dataset(path, {'training': subs})


def _train_args(tmp_path, extra):
    return [str(tmp_path / 'exp'), 'toy', 'run1', str(tmp_path / 'ds.npz'), '--max_ep', '2',
            '--log_interval', '1', '--n_actor', '512', '--hidden_dims', '32-32',
            '--batch_size', '64', '--replay_size', '20000', '--npv', '1', '--min_length', '2',
            '--max_length', '20', '--oracle_bonus', '0', '--rng_seed', '4'] + extra


def arc(n, sagitta, seed, z=5.9):
    """n points on a circular arc in the plane z from (1.5, 1.5) to (10.5, 1.5)
    bulging to y = 1.5 + sagitta, with a little noise off the plane."""
    half = 4.5
    r = (half * half + sagitta * sagitta) / (2 * sagitta)
    a = np.arcsin(half / r) if sagitta <= half else np.pi - np.arcsin(half / r)
    t = np.linspace(-a, a, n)
    cy = 1.5 + sagitta - r
    rng = np.random.default_rng(seed)
    return np.stack([6.0 + r * np.sin(t), cy + r * np.cos(t),
                     z + rng.normal(0, 0.03, n).clip(-0.09, 0.09)], 1).astype(np.float32)


def designed_rows(B):
    """[(name, points, expected bundle or None)]: expected is the hand-computed
    answer as a role name, '-' for no bundle, None where only the reference
    says."""
    rows = []

    def add(name, pts, want=None):
        rows.append((name, np.asarray(pts, np.float32).reshape(-1, 3), want))

    y, z = 3.5, 4.5
    # ---- ends, on the limits bundle (lengths inside its limits)
    add('head_to_tail', _line((0.5, y, z), (11.5, y, z)), 'L')
    add('tail_to_head', _line((11.5, y, z), (0.5, y, z)), 'L')
    add('head_to_head', _line((0.5, y, z), (5.0, y, z), (1.5, y, z)), '-')
    add('end_on_face_in', _line((1.75, y, z), (10.0, y, z)), 'L')       # length = lo = dir lo
    add('end_on_face_out', _line((2.0, y, z), (11.5, y, z)), '-')        # voxel 2: no head
    add('end_minus_third', _line((0.5, -0.3, z), (11.5, -0.3, z)), '-')  # floor(-0.3) = -1
    add('end_outside', _line((0.5, y, z), (12.5, y, z)), '-')
    add('no_points', np.zeros((0, 3), np.float32), '-')
    add('one_point', _line((0.5, y, z)), '-')
    add('nan_mid_row', _line((0.5, y, z), (np.nan, y, z), (11.5, y, z)), '-')
    add('inf_mid_row', _line((0.5, y, z), (6.5, np.inf, z), (11.5, y, z)), '-')
    # ---- limits at their inclusive bounds (sums exact: see ref.exact_sums)
    add('length_at_hi', _line((0.5, y, z), (11.5, y, z), (10.5, y, z), (11.5, y, z)), 'L')  # 26
    add('length_above_hi', _line((0.5, y, z), (11.5, y, z), (10.25, y, z), (11.5, y, z)), '-')
    add('length_below_lo', _line((1.875, y, z), (10.0, y, z)), '-')                   # 16.25
    add('dir_y_at_hi', _line((0.5, y, z), (0.5, y + 2, z), (11.5, y + 2, z)), 'L')    # 3.0, x 23
    add('dir_y_above_hi', _line((0.5, y, z), (0.5, y + 2.25, z), (11.5, y + 2.25, z)), '-')
    add('dir_x_above_hi', _line((0.25, y, z), (0.25, y + 2, z), (11.5, y + 2, z)), '-')  # 23.5
    add('absdir_z_at_hi', _line((0.5, y, z), (0.5, y, z + 1), (11.5, y, z + 1), (11.5, y, z)),
        'L')                                                                          # 2.5
    add('absdir_z_above_hi', _line((0.5, y, z), (0.5, y, z + 1.25), (11.5, y, z + 1.25),
                                   (11.5, y, z + 0.25)), '-')
    # ---- row lengths across the lane boundaries, several segments per lane
    for n in (64, 65, 66, 200):
        x = np.linspace(0.5, 11.5, n)
        add(f'straight_{n}', np.stack([x, np.full(n, y), np.full(n, z)], 1), 'L')
        add(f'straight_{n}_nan_last_lane',
            np.stack([x, np.full(n, y), np.where(np.arange(n) == n - 2, np.nan, z)], 1), '-')
    # ---- all_mask / any_mask: left / reached only through a voxel that holds no point
    diag = [(0.5, 3.5), (4.5, 3.5), (6.5, 5.5), (8.5, 5.5), (11.5, 5.5)]
    add('any_by_walk_only', [(px, py, 2.5) for px, py in diag], 'AY')     # (5, 4, 2) walked
    add('hole_by_walk_only', [(px, py, 1.5) for px, py in diag], '-')     # (5, 4, 1) walked
    add('touches_nothing', _line((0.5, 7.5, 2.5), (11.5, 7.5, 2.5)), '-')
    add('plain_inside', [(px, 5.5, 1.5) for px in np.arange(0.5, 12, 1.0)], 'AY')
    add('leaves_slab', _line((0.5, 5.5, 1.5), (8.5, 5.5, 1.5), (8.5, 5.5, 3.5), (11.5, 5.5, 1.5)),
        '-')
    # ---- winding on planar arcs
    for n in (64, 65, 66, 200):
        add(f'shallow_arc_{n}', arc(n, 1.0, n), 'W')
    for n in (65, 200):
        add(f'deep_arc_{n}', arc(n, 4.5, n), '-')
    add('shallow_arc_reversed', arc(130, 1.5, 1)[::-1], 'W')
    # ---- priority
    if 'P2' in ROLES[B]:
        add('valid_for_2_and_5', _line((0.5, 4.5, 3.5), (11.5, 4.5, 3.5)), 'P2')
        add('valid_for_5_only', _line((0.5, 4.5, 3.5), (0.5, 6.5, 3.5), (11.5, 6.5, 3.5),
                                      (11.5, 4.5, 3.5)), 'P5')
    return rows


@functools.lru_cache(maxsize=None)
def case(B):
    """The designed rows and 300 random walks, packed: dict(points, offsets,
    names, want (bundle index, -1, or None), score = ref.score(...))."""
    rng = np.random.default_rng(B)
    rows = designed_rows(B)
    walks = random_walks(rng, 300, 2, 90, 12, step=(0.3, 1.9), start=(-1, 12))
    walks = [np.minimum(w, np.float32(11.9)) for w in walks]
    # ends dropped into the filler slab so that some walks connect fillers
    for w in walks[:200]:
        w[0, 2] = w[-1, 2] = 0.5
    names = [r[0] for r in rows] + [f'walk_{i}' for i in range(len(walks))]
    lines = [r[1] for r in rows] + walks
    roles = ROLES[B]
    want = [None if r[2] is None else (-1 if r[2] == '-' else roles[r[2]]) for r in rows]
    want += [None] * len(walks)
    points, offsets = pack(lines)
    bundles = scoring_set(B)
    return {'points': points, 'offsets': offsets, 'names': names, 'want': want,
            'bundles': bundles, 'score': ref.score(points, offsets, DIMS, bundles, LIN)}


GRID_ROWS = 40000
GRID_PASS = 4 * 8192          # rows of one pass of the capped grid


@functools.lru_cache(maxsize=None)
def grid_case():
    """40 000 rows for the B = 3 set: above the 32 768 rows of one pass, so the
    waves of rows 0 .. 7231 take a second row.  Most rows are two or three
    points; every 97th row of the first pass is a long one whose partner in the
    second pass is short, and the other way round every 89th."""
    B = 3
    rng = np.random.default_rng(7)
    designed = {r[0]: r[1] for r in designed_rows(B)}
    long_rows = [designed[k] for k in ('shallow_arc_200', 'straight_65', 'deep_arc_65',
                                       'plain_inside', 'straight_200', 'any_by_walk_only')]
    lines = []
    for r in range(GRID_ROWS):
        first = r if r < GRID_PASS else r - GRID_PASS
        is_long = (first % 97 == 0) if r < GRID_PASS else (first % 89 == 1)
        if is_long:
            lines.append(long_rows[(first // 7) % len(long_rows)])
            continue
        n = 2 + (r & 1)
        # below the angle bundle's slab: two or three points span no plane to wind in
        p = rng.uniform(0, 1, (n, 3)) * (12, 9, 5)
        if r % 3 == 0:            # a third of the short rows run from head to tail of L
            p[0] = (rng.uniform(0, 2), rng.uniform(0, 9), 4.5)
            p[-1] = (rng.uniform(10, 12), rng.uniform(0, 9), 4.5)
        lines.append(p.astype(np.float32))
    points, offsets = pack(lines)
    bundles = scoring_set(B)
    return {'points': points, 'offsets': offsets, 'bundles': bundles,
            'score': ref.score(points, offsets, DIMS, bundles, LIN)}
