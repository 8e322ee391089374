"""Deterministic case generators for tests/test_bundle_register.py: nothing is
committed as data.  A kernel case is a dict of NumPy arrays: fixed (A, K, 3) and
moving (B, K, 3) float32 stations, xf (T, 3, 4) float64, lin (3, 3), and special
({name: index} of what was built on purpose).  ``recovery`` is the planted-
transform case of the driver."""
import functools

import numpy as np

import ref_bundle_register as ref
from bundle_profile_cases import DIMS, LINS, walk
from ref_oracle_validator import resample_blocked

F32 = np.float32
KS = (2, 3, 20, 64, 65, 256)
AS = (1, 7, 8, 9, 70)
BS = (1, 63, 64, 65, 300)
TS = (1, 2, 25, 64)
#: moving lines of a tile of the kernel and fixed lines of a workgroup
#: (ttl_bundle_register.hip TILE_LINES, ROWS)
TILE_LINES = 64
WORKGROUP_ROWS = ref.BLOCK_ROWS


def _lines(rng, n, K):
    return np.stack([resample_blocked(walk(rng, 40, DIMS, 0.5), K) for _ in range(n)])


def transforms(rng, T):
    """T voxel-space transforms near the identity, the first the identity itself;
    from T = 25 on: one with a NaN entry, the all-zero one and one with an Inf."""
    xf = np.zeros((T, 3, 4))
    xf[:, :, :3] = np.eye(3) + rng.normal(0.0, 0.05, (T, 3, 3))
    xf[:, :, 3] = rng.normal(0.0, 0.7, (T, 3))
    xf[0] = np.eye(4)[:3]
    special = {}
    if T >= 25:
        xf[3, 1, 2] = np.nan
        xf[4] = 0.0
        xf[5, 0, 3] = np.inf
        special = {'xf_nan': 3, 'xf_zero': 4, 'xf_inf': 5}
    return xf, special


@functools.lru_cache(maxsize=None)
def case(K, A, B, T, lin_name='oblique', seed=0):
    """``A`` fixed and ``B`` moving random lines under ``T`` transforms.  With A
    >= 7: fixed line 2 has a NaN and line 5 an Inf station, line 6 is line 4 again;
    with B >= 63: moving line 3 has a NaN and line 10 an Inf station, line 7 is
    line 6 again."""
    rng = np.random.default_rng(1000003 * K + 1009 * A + 17 * B + T + seed)
    fixed, moving = _lines(rng, A, K), _lines(rng, B, K)
    xf, special = transforms(rng, T)
    if A >= 7:
        fixed[2, K // 2, 1] = np.nan
        fixed[5, 0, 0] = np.inf
        fixed[6] = fixed[4]
        special.update(fixed_nan=2, fixed_inf=5, fixed_twice=(4, 6))
    if B >= 63:
        moving[3, K - 1, 2] = np.nan
        moving[10, 1, 0] = -np.inf
        moving[7] = moving[6]
        special.update(moving_nan=3, moving_inf=10, moving_twice=(6, 7))
    return {'fixed': np.ascontiguousarray(fixed, F32), 'moving': np.ascontiguousarray(moving, F32),
            'xf': xf, 'lin': LINS[lin_name], 'K': K, 'A': A, 'B': B, 'T': T, 'special': special}


GPU_CASES = [(2, 70, 300, 2, 'axis'), (3, 1, 1, 1, 'anisotropic'), (20, 9, 65, 25, 'oblique'),
             (64, 8, 64, 2, 'axis'), (65, 7, 63, 64, 'anisotropic'), (256, 70, 65, 1, 'oblique'),
             (256, 9, 300, 2, 'axis'), (20, 70, 300, 2, 'oblique')]
SPECIAL_CASES = ('all_nan_fixed', 'all_nan_moving')


@functools.lru_cache(maxsize=None)
def special_case(name):
    """A set that is all NaN: no entry of either minimum, no cost."""
    c = dict(case(20, 9, 65, 25, 'oblique'))
    key = 'fixed' if name == 'all_nan_fixed' else 'moving'
    lines = c[key].copy()
    lines[:, 1, 2] = np.nan
    c[key] = lines
    return c


def get(key):
    return special_case(key) if isinstance(key, str) else case(*key)


@functools.lru_cache(maxsize=None)
def reference(key):
    c = get(key)
    return ref.cost(c['fixed'], c['moving'], c['xf'], c['lin'])


def hand():
    """A 2 mm grid, K = 3.  Fixed line 0 along x at y = 1, fixed line 1 the same
    line 3 voxels up, stored backwards.  Moving line 0 is fixed line 0 shifted by
    -1 voxel in x, moving line 1 lies 1 voxel above fixed line 1.  Transform 0 is
    the identity, transform 1 the shift by +1 voxel in x."""
    fixed = np.array([[(2, 1, 1), (3, 1, 1), (4, 1, 1)],
                      [(4, 4, 1), (3, 4, 1), (2, 4, 1)]], F32)
    moving = np.array([[(1, 1, 1), (2, 1, 1), (3, 1, 1)],
                       [(2, 5, 1), (3, 5, 1), (4, 5, 1)]], F32)
    xf = np.stack([np.eye(4)[:3], np.eye(4)[:3]])
    xf[1, 0, 3] = 1.0
    return {'fixed': fixed, 'moving': moving, 'xf': xf, 'lin': np.diag([2.0, 2.0, 2.0]),
            'K': 3, 'A': 2, 'B': 2, 'T': 2, 'special': {}}


def witness():
    """The witness case of the named mutants.  lin = diag(0.5, 1, 4), K = 3.  9
    fixed lines (more than a workgroup's 8), 3 moving lines, 2 transforms: a
    rotation about z with a scale and a translation, and the identity.  Fixed line
    1 has a NaN station, moving line 2 an Inf station; fixed line 8, alone behind
    the first workgroup's lines, is the nearest of moving line 1; moving line 0 is
    nearer its partner when read backwards."""
    rng = np.random.default_rng(5)
    K = 3
    base = np.array([(2, 1, 1), (3, 1.5, 1), (4, 1, 1.5)], np.float64)
    fixed = np.stack([base + rng.normal(0, 0.4, (K, 3)) + (0, i % 3, i // 3) for i in range(9)])
    fixed[0] = fixed[0][::-1]
    fixed[1, 1, 0] = np.nan
    moving = np.stack([base + (0.3, 0.2, -0.1), base + (0.5, 2.2, 2.1), base + (1.0, 1.0, 0.0)])
    fixed[8] = moving[1] + (0.1, -0.1, 0.05)
    moving[2, 0, 2] = np.inf
    c, s = np.cos(0.3), np.sin(0.3)
    x = np.array([[1.1 * c, -1.1 * s, 0.0, 0.8], [1.1 * s, 1.1 * c, 0.0, -0.9],
                  [0.0, 0.0, 1.1, 0.4]])
    xf = np.stack([x, np.eye(4)[:3]])
    return {'fixed': np.ascontiguousarray(fixed, F32), 'moving': np.ascontiguousarray(moving, F32),
            'xf': xf, 'lin': np.diag([0.5, 1.0, 4.0]), 'K': K, 'A': 9, 'B': 3, 'T': 2,
            'special': {}}


# -- the driver's case: a planted transform ---------------------------------
AFFINE = np.array([[2.0, 0.0, 0.0, -60.0], [0.0, 2.0, 0.0, -50.0], [0.0, 0.0, 2.0, -40.0],
                   [0.0, 0.0, 0.0, 1.0]])
GRID = (60, 50, 40)
SIGMA = 0.5                                     # mm
PLANTED = {'rigid': np.array([6.0, -4.0, 3.0, 8.0, -5.0, 10.0]),
           'affine': np.array([6.0, -4.0, 3.0, 8.0, -5.0, 10.0, 1.08, 0.95, 1.03, 0.05, -0.04,
                               0.03])}
PER_BUNDLE, N_DISTRACTORS, K_RECOVERY = 10, 6, 12


def _bundles(rng, per_bundle, K):
    """Three curved bundles of ``per_bundle`` lines each, about 80 mm long: (3
    per_bundle, K, 3) mm and the bundle of every line.  Bundle 1 is bundle 0's
    shape 7 mm beside it, along the planted translation's (y, z) direction, so
    that the unregistered subject's bundle 0 lies nearer the atlas's bundle 1;
    bundle 2 has a shape and a place of its own."""
    s = np.linspace(0.0, 1.0, K)[:, None]
    lines, label = [], []
    for b, (y0, z0, bend, rise) in enumerate(((0.0, 0.0, 12.0, 5.0), (-5.6, 4.2, 12.0, 5.0),
                                              (14.0, -6.0, 16.0, -8.0))):
        core = np.concatenate([80.0 * s - 40.0, y0 + 0.5 * bend * np.sin(np.pi * s),
                               z0 + rise * np.cos(np.pi * s) + bend * np.sin(np.pi * s)], 1)
        for _ in range(per_bundle):
            spread = rng.normal(0.0, 0.8, 3) * (0.3, 1.0, 1.0)
            lines.append(core + spread + rng.normal(0.0, 0.6, 3) * (2.0 * s - 1.0))
            label.append(b)
    return np.stack(lines), np.asarray(label, np.int32)


def to_vox(mm):
    """RAS mm -> corner-origin voxel coordinates of the recovery grid."""
    inv = np.linalg.inv(AFFINE)
    return np.asarray(mm, np.float64) @ inv[:3, :3].T + inv[:3, 3] + 0.5


@functools.lru_cache(maxsize=None)
def recovery(kind):
    """The atlas (moving: the three bundles, one model per line) and the subject
    (fixed: the atlas under the planted ``kind`` transform about the atlas's mean
    station, Gaussian jitter of SIGMA mm on every station, every second line
    reversed, and N_DISTRACTORS straight lines across the bundles).  mm arrays and
    their float32 voxel forms; ``planted`` is the (4, 4) mm matrix."""
    from tracktolearn_amd.bundle_register import compose
    rng = np.random.default_rng(11)
    atlas_mm, label = _bundles(rng, PER_BUNDLE, K_RECOVERY)
    centre = atlas_mm.reshape(-1, 3).mean(0)
    planted = compose(PLANTED[kind], kind, centre)
    subject = atlas_mm @ planted[:3, :3].T + planted[:3, 3]
    subject = subject + rng.normal(0.0, SIGMA, subject.shape)
    subject[1::2] = subject[1::2, ::-1]
    s = np.linspace(0.0, 1.0, K_RECOVERY)[:, None]
    noise = []
    for _ in range(N_DISTRACTORS):
        a, e = rng.uniform((-35, -30, -25), (35, 30, 25), (2, 3))
        noise.append(a + s * (e - a))
    fixed_mm = np.concatenate([subject, np.stack(noise)])
    truth = np.concatenate([label, np.full(N_DISTRACTORS, -1, np.int32)])
    return {'atlas_mm': atlas_mm, 'label': label, 'fixed_mm': fixed_mm, 'truth': truth,
            'planted': planted, 'centre': centre, 'affine': AFFINE, 'dims': GRID,
            'moving_vox': to_vox(atlas_mm).astype(F32), 'fixed_vox': to_vox(fixed_mm).astype(F32)}


def displacement(c, matrix):
    """The largest distance in mm between an atlas station under ``matrix`` and
    under the planted transform."""
    p = c['atlas_mm'].reshape(-1, 3)
    a = p @ np.asarray(matrix)[:3, :3].T + np.asarray(matrix)[:3, 3]
    b = p @ c['planted'][:3, :3].T + c['planted'][:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1)).max())


def labels_by_reference(c, matrix):
    """The label of the nearest atlas line (moved by the mm ``matrix``) of every
    subject line, by the reference's table; the distractors included."""
    from tracktolearn_amd.bundle_register import to_voxel
    x = to_voxel(matrix, c['affine'])
    delta = ref.table(c['fixed_vox'], c['moving_vox'], x, c['affine'][:3, :3])[0]
    return c['label'][np.argmin(delta.astype(np.float64), 1)]
