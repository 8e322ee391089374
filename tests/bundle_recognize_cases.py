"""Deterministic case generators for tests/test_bundle_recognize.py: nothing is
committed as data.  A case is a dict of NumPy arrays: points (P, 3) float32,
offsets (n + 1,) int64, models (M, K, 3) float32, label (M,) int32 or None, lin
(3, 3), and M, K, special ({name: row} of the rows built on purpose)."""
import functools

import numpy as np

import ref_bundle_recognize as ref
from bundle_profile_cases import DIMS, LINS, pack, tie_rows, walk

F32 = np.float32
KS = (2, 3, 64, 65, 256)
MS = (1, 2, 63, 64, 65, 4096)
NS = (1, 70, 300)
LENGTHS = (2, 3, 64, 65, 200)
#: models of a tile of the kernel (ttl_bundle_recognize.hip TILE_MODELS, at every K) and
#: rows of a workgroup
TILE_MODELS = 64
WORKGROUP_ROWS = 8
#: label values of the 'grouped' mode: negative, large, and each repeated
LABEL_VALUES = np.array([-7, 5, 2 ** 31 - 1, 0], np.int32)
#: the rows and models built on purpose live this far from the volume, each kind along its
#: own axis: no random row is near them (a walk of 200 points drifts by some 20 voxels) and
#: they are near no random model
FAR = 200.0


def _stations(line, K):
    return ref.resample_blocked(np.asarray(line, F32), K)


@functools.lru_cache(maxsize=None)
def case(K, M, n, lin_name='oblique', labels='grouped', seed=0):
    """``n`` rows of the lengths LENGTHS in turn against ``M`` random model lines.
    labels: 'null' (no label array: every model its own), 'grouped' (LABEL_VALUES
    in turn) or 'one' (every model the same label).  With n >= 16 the first rows
    are special: a NaN point, an Inf point, a single point (no part); and with M
    >= 8 as well: models 5 and 6 get a NaN and an Inf station, and the ties are
    built from bit-identical duplicated models far from everything else --
    'tie_same': models 1 and 3 the same line under one label, a row along it (the
    winner is 1); 'tie_cross': models 2 and 4 the same line under two labels (the
    winner is 2 and runner_up is mdf); 'tie_flip' (axis-aligned lin, K - 1 a power
    of two): bundle_profile_cases.tie_rows, a row whose distances to a model that
    is one point read the same both ways (flip 0), model 7."""
    rng = np.random.default_rng(100000 * K + 10 * M + n + seed)
    models = np.stack([_stations(walk(rng, 40, DIMS, 0.5), K) for _ in range(M)])
    if labels == 'null':
        label = None
    elif labels == 'one':
        label = np.full(M, 3, np.int32)
    else:
        label = LABEL_VALUES[np.arange(M) % len(LABEL_VALUES)].copy()
    rows, special = [], {}
    if n >= 16:
        for name, value in (('nan', np.nan), ('inf', np.inf)):
            r = walk(rng, 70, DIMS)
            r[-1 if name == 'nan' else 3, 2] = value
            special[name] = len(rows)
            rows.append(r)
        special['single'] = len(rows)
        rows.append(walk(rng, 1, DIMS))
        if M >= 8:
            models[5, K // 2, 1] = np.nan
            models[6, 0, 0] = np.inf
            if labels != 'null':        # without labels every model is a label of its own
                line = walk(rng, 30, DIMS, 0.5) + F32([0, FAR, 0])
                models[1] = models[3] = _stations(line, K)
                label[3] = label[1]
                special['tie_same'] = len(rows)
                rows.append(models[1].copy())
            if labels != 'one':
                line = walk(rng, 30, DIMS, 0.5) + F32([FAR, 0, 0])
                models[2] = models[4] = _stations(line, K)
                special['tie_cross'] = len(rows)
                rows.append(models[2][::-1].copy())     # stored backwards: flip is 1
            tie = tie_rows(K) if lin_name == 'axis' else None
            if tie is not None:
                models[7] = tie[1] + F32([0, -1.75, FAR])      # 0.25 voxels beside the row
                special['tie_flip'] = len(rows)
                rows.append(tie[0] + F32([0, 0, FAR]))
    while len(rows) < n:
        rows.append(walk(rng, LENGTHS[len(rows) % len(LENGTHS)], DIMS))
    points, offsets = pack(rows)
    return {'points': points, 'offsets': offsets, 'models': np.ascontiguousarray(models, F32),
            'label': label, 'lin': LINS[lin_name], 'M': M, 'K': K, 'special': special}


GPU_CASES = [(2, 4096, 70, 'axis', 'grouped'), (3, 1, 1, 'anisotropic', 'null'),
             (3, 2, 70, 'axis', 'grouped'), (64, 63, 70, 'oblique', 'grouped'),
             (65, 64, 300, 'axis', 'grouped'), (65, 65, 70, 'oblique', 'null'),
             (256, 65, 70, 'anisotropic', 'one'), (256, 2, 1, 'oblique', 'grouped')]


@functools.lru_cache(maxsize=None)
def all_nan_case():
    """Every model has a NaN station: no row has a winner."""
    c = dict(case(3, 2, 70, 'axis', 'grouped'))
    models = c['models'].copy()
    models[:, 1, 2] = np.nan
    return dict(c, models=models, special={k: v for k, v in c['special'].items()
                                           if not k.startswith('tie')})


@functools.lru_cache(maxsize=None)
def reference(key):
    c = all_nan_case() if key == 'all_nan' else case(*key)
    return ref.recognize(c['points'], c['offsets'], c['models'], c['lin'], c['label'])


def ties(c):
    return sorted(v for k, v in c['special'].items() if k.startswith('tie'))


def hand():
    """Three models on a 2 mm grid, K = 3, rows whose stations are their points:
    row 0 lies on model 0 backwards and 1 voxel (2 mm) from model 1; row 1 lies 1
    voxel above model 2 and 1.5 voxels from model 1.  Models 0 and 1 are one
    bundle."""
    rows = [np.array([(4, 1, 1), (3, 1, 1), (2, 1, 1)], F32),
            np.array([(2, 3.5, 1), (3, 3.5, 1), (4, 3.5, 1)], F32)]
    models = np.array([[(2, 1, 1), (3, 1, 1), (4, 1, 1)],
                       [(2, 2, 1), (3, 2, 1), (4, 2, 1)],
                       [(2, 4.5, 1), (3, 4.5, 1), (4, 4.5, 1)]], F32)
    points, offsets = pack(rows)
    return {'points': points, 'offsets': offsets, 'models': models,
            'label': np.array([0, 0, 1], np.int32), 'lin': np.diag([2.0, 2.0, 2.0]), 'M': 3,
            'K': 3, 'special': {}}


def witness():
    """The witness set of the named mutants.  lin = diag(0.1, 1, 10).
    row 0: between the bit-identical models 0 and 1 (the tie on the index);
    row 1: tie_rows against model 2 (the tie on the flip);
    row 2: nearer model 3 in mm, nearer model 4 in voxels and with squared distances
           (model 3 has one far station);
    row 3: lies backwards on model 5 and, read forwards, is nearer model 4;
    row 4: a single point on a station of model 3 (takes no part);
    model 6, the last, has a NaN station; the labels pair models 3 and 4."""
    K = 3
    tie_row, tie_model = tie_rows(3)
    models = np.zeros((7, K, 3), F32)
    models[0] = models[1] = [(1, 1, 40), (2, 1, 40), (3, 1, 40)]
    models[2] = tie_model + F32([0, 0, 80])
    # row 2 = (10, 10, 10) .. (12, 10, 10): model 3 is 3 voxels off in x (0.3 mm) but for a
    # station 30 voxels off in x (3 mm); model 4 is 0.15 voxels off in z (1.5 mm)
    # (its first station a little off in z: on the row's own line D and F would be equal)
    models[3] = [(13, 10, 10.05), (14, 10, 10), (42, 10, 10)]
    models[4] = [(10, 10, 10.15), (11, 10, 10.15), (12, 10, 10.15)]
    models[5] = [(12, 10, 10.3), (11, 10, 10.2), (10, 10, 9.6)]
    models[6] = [(0, 0, 0), (np.nan, 0, 0), (1, 0, 0)]
    rows = [np.array([(1, 1.5, 40), (2, 1.5, 40), (3, 1.5, 40)], F32),
            tie_row + F32([0, 0, 80]),
            np.array([(10, 10, 10), (11, 10, 10), (12, 10, 10)], F32),
            np.array([(10, 10, 9.6), (11, 10, 10.2), (12, 10, 10.3)], F32),
            np.array([(13, 10, 10)], F32)]
    points, offsets = pack(rows)
    return {'points': points, 'offsets': offsets, 'models': models,
            'label': np.array([0, 0, 1, 2, 2, 3, 4], np.int32),
            'lin': np.diag([0.1, 1.0, 10.0]), 'M': 7, 'K': K, 'special': {}}
