"""Inputs and expected values of tests/test_env_step_vectors.py.

Two sets of isolated vectors for the arithmetic core of the environment step
(``advance_row`` in tracktolearn_amd/csrc/ttl_hip.hip):

  A. action vectors: the reference's 512 recorded rows of ``normalize_vectors``
     / ``_format_actions`` (tests/golden/isolated_functions.npz) plus generated
     rows whose float32 squares are denormal, underflow to zero or overflow;
  B. a peaks volume whose centre voxels hold peaks that underflow, overflow or
     are not finite, with seeds inside those voxels and outside the volume.

Every expected value comes from the recorded file or from oracle/env_oracle.py
(imported, not edited); nothing here looks at the library under test.  The
tracking mask is all ones: its spline value is 1 everywhere inside the volume,
so no mask decision sits near the threshold.
"""
import functools

import numpy as np

from helpers import load_trace, synthetic_subject
from oracle import env_oracle as orc

D = 12
K = 4
THR = 0.1
STEP32 = np.float32(0.75)
STEP64 = np.float64(0.75)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)      # smallest normal float32
N_RECORDED = 512

#: arithmetic modes of the step -> (oracle class is the noisy one, step size as
#: the reference would hold it)
ORACLE_MODES = {
    'f32': (False, STEP32),         # TTL_MODE_F32: plain env, float32 affine
    'f32norm': (False, STEP64),     # TTL_MODE_F32NORM: plain env, float64 affine
    'f64': (True, STEP64),          # TTL_MODE_F64DIR: noisy env, sigma 0
}

ORIGIN = (0.0, 0.0, 0.0)
CENTRE = (6.0, 6.0, 6.0)


# --------------------------------------------------------------------------- #
# A. action vectors
def tiny_rows(rng, n=256):
    """Components around 1e-23 .. 1e-19: float32 squares are denormal or zero."""
    g = rng.standard_normal((n, 3))
    return (g * 10.0 ** rng.uniform(-23.0, -19.2, (n, 1))).astype(np.float32)


def huge_rows(rng, n=256):
    """Components around 1e18.5 .. 1e19.5: the float32 sum of squares overflows
    for some rows and stays finite for others."""
    g = rng.standard_normal((n, 3))
    return (g * 10.0 ** rng.uniform(18.5, 19.5, (n, 1))).astype(np.float32)


def mixed_rows():
    """Tiny and huge components in one vector, signed zeros, one component
    exactly +-FLT_MAX, the smallest denormal, and sums next to the underflow
    and overflow borders."""
    F = FLT_MAX
    rows = [
        # tiny and huge together
        [1e-21, 2e19, -1e-20], [-3e19, 1e-23, 2e19], [1e-20, 1e10, 1.0], [1e-38, 1e38, 0.0],
        [1e-20, 1e20, 1.0], [-1e-22, -1e-22, 1e19], [5e-23, 1.0, -1e19],
        # signed zeros
        [-0.0, 0.0, 1.0], [0.0, -0.0, -0.0], [-0.0, -0.0, -0.0], [-0.0, 1e-22, 0.0],
        [-0.0, 1e-30, 0.0], [-0.0, -1e19, 1e19], [-0.0, -0.0, -1e-21], [3.0, -0.0, -4.0],
        # one component exactly +-FLT_MAX
        [F, 0.0, 0.0], [-F, 0.0, 0.0], [0.0, F, 1.0], [1e-30, -F, -0.0], [0.0, 0.0, -F],
        [F, 1e-22, -1e-22], [-1e19, 1e-45, F], [1.0, -F, 1e19],
        # the smallest denormal as a component
        [1e-45, 0.0, 0.0], [1e-45, 1e-45, 1e-45], [1e-45, 1.0, 0.0], [1e-45, 1e-3, 0.0],
        [-1e-40, 1.0, 1.0], [1e-45, -1e-22, 1e-45],
        # squares next to the smallest normal and the smallest denormal
        [1.0842e-19, 0.0, 0.0], [1.0843e-19, 0.0, 0.0], [7.7e-20, 7.6e-20, 0.0],
        [2.7e-23, 0.0, 0.0], [2.6e-23, 0.0, 0.0], [3.8e-23, -2.6e-23, 2.6e-23],
        [0.0, 5.3e-23, -5.3e-23], [2.0e-23, 2.0e-23, 2.0e-23],
        # sums next to FLT_MAX
        [1.3e19, 1.3e19, 0.0], [1.31e19, -1.31e19, 1e10], [18446744073709551616.0, 0.0, 0.0],
        [1.8446743e19, 1.0, 0.0], [1.0650232e19, 1.0650232e19, 1.0650232e19],
        [1.06503e19, 1.06503e19, -1.06503e19],
    ]
    return np.array(rows, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def action_vectors():
    """(n, 3) float32: the recorded rows first, then tiny, huge and mixed rows."""
    z = load_trace('isolated_functions')
    rng = np.random.RandomState(5)
    a = np.concatenate([z['norm_in'], tiny_rows(rng), huge_rows(rng), mixed_rows()])
    assert a.dtype == np.float32 and a.shape[0] <= 1100
    a.flags.writeable = False
    return a


def scaled(a, mode):
    """The oracle's scaled directions of action rows ``a`` in an arithmetic
    mode: float32 for 'f32', float64 otherwise."""
    noisy, step = ORACLE_MODES[mode]
    with np.errstate(all='ignore'):
        if noisy:
            return orc.scale_actions(a + np.zeros(a.shape), step)
        return orc.scale_actions(a, step)


def direction_classes(a):
    """Boolean row masks of the regimes the vectors are meant to reach."""
    with np.errstate(all='ignore'):
        s32 = np.einsum('ij,ij->i', a, a)
    d32 = scaled(a, 'f32')
    d64 = scaled(a, 'f64')
    with np.errstate(all='ignore'):
        h64 = (-d64).astype(np.float32)

    def denormal(x):
        return ((np.abs(x) > 0) & (np.abs(x) < FLT_MIN)).any(axis=1)
    return {
        'denormal sum of squares': (s32 > 0) & (s32 < FLT_MIN),
        'zero sum, nonzero component': (s32 == 0) & (a != 0).any(axis=1),
        'overflowing sum': np.isinf(s32) & np.isfinite(a).all(axis=1),
        'NaN result (float32)': np.isnan(d32).any(axis=1),
        'NaN result (float64)': np.isnan(d64).any(axis=1),
        '+inf result': (d32 == np.inf).any(axis=1),
        '-inf result': (d32 == -np.inf).any(axis=1),
        'denormal float32 output (float32 mode)': denormal(d32),
        'denormal float32 output (float64 modes)': denormal(h64),
    }


def ones_subject(peaks=None):
    """(sh, all-ones mask, peaks) on the D^3 grid."""
    sh, _, pk = synthetic_subject(D)
    return sh, np.ones((D, D, D), np.uint8), pk if peaks is None else peaks


def oracle_env(mode, seeds, *, max_nb_steps, peaks=None, reward=False, theta=30.0):
    noisy, step = ORACLE_MODES[mode]
    sh, mask, pk = ones_subject(peaks)
    kw = dict(n_dirs=K, theta=theta, step_size=step, max_nb_steps=max_nb_steps,
              mask_threshold=THR, peaks=pk, compute_reward=reward, alignment_weighting=1.0)
    if noisy:
        return orc.OracleNoisyTrackingEnv(sh, mask, seeds, noise=0.0, **kw)
    return orc.OracleTrackingEnv(sh, mask, seeds, **kw)


def one_step(mode, seed, max_nb_steps, fed=None):
    """The oracle's first step from ``reset`` with every streamline seeded at
    ``seed``, row i taking action vector i (``fed``: other action rows, e.g.
    float64 actions that already carry their noise)."""
    a = action_vectors() if fed is None else fed
    n = a.shape[0]
    ref = oracle_env(mode, np.tile(np.asarray(seed, np.float64), (n, 1)),
                     max_nb_steps=max_nb_steps)
    with np.errstate(all='ignore'):
        ref.reset(0, n)
        _, _, done, _ = ref.step(a.copy())
        ref.harvest()
    return dict(head=ref.streamlines[:, 1].copy(), done=done.astype(bool),
                flip=ref.last_flip.copy(), flags=ref.flags.copy(),
                lengths=ref.lengths.copy(), continue_idx=ref.continue_idx.copy(),
                streamlines=ref.streamlines.copy())


@functools.lru_cache(maxsize=None)
def one_step_expected(mode, seed, max_nb_steps):
    return one_step(mode, seed, max_nb_steps)


def head_of(seed, d, flip):
    """The new point of streamlines at ``seed`` (one coordinate value on every
    axis) whose scaled directions are ``d`` -- float32: all float32; float64:
    ``float32(float64(seed) + d)`` -- with the rows ``flip`` reversed."""
    with np.errstate(all='ignore'):
        signed = np.where(np.asarray(flip)[:, None], -d, d)
        if d.dtype == np.float32:
            return np.float32(seed) + signed
        return (np.float64(np.float32(seed)) + signed).astype(np.float32)


def same_bits(got, want):
    """float32 arrays equal bit for bit, except that any NaN equals any NaN
    (the payload of a NaN is not pinned)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


# --------------------------------------------------------------------------- #
# B. peaks reward
#: voxels of the centre block whose peaks are overwritten
BLOCK = [(x, y, z) for x in (5, 6, 7) for y in (5, 6, 7) for z in (5, 6, 7)]
REWARD_STEPS = 4
#: the step (0-based) whose action overflows in float32 for every fifth row
OVERFLOW_STEP = 2
REWARD_THETA = 60.0
REWARD_MAX_NB_STEPS = 26


def _peak_kinds():
    """Five peaks (15 floats) per kind of adversarial voxel."""
    inf, nan, F = np.inf, np.nan, FLT_MAX
    o = [0.3, -0.5, 0.8]            # an ordinary peak
    kinds = {
        # squares underflow to 0: components become inf, then FLT_MAX
        'underflow': [[1e-30, 1e-30, 0.0], [-1e-30, 0.0, 0.0], o, [0.0, 1e-30, -1e-30],
                      [1e-30, -1e-25, 1e-30]],
        # squares are denormal: a finite unit vector only with gradual underflow
        'denormal': [[1e-20, -2e-21, 3e-21], [4e-22, 4e-22, -4e-22], [0.0, 6e-23, 5e-23],
                     [-7e-21, 1e-22, 0.0], [3e-23, 3e-23, 3e-23]],
        # the norm overflows to inf: a zero vector
        'overflow': [[1e20, 1.0, 1.0], [3e38, 0.0, 0.0], [1e20, 1e20, -1e20], [-F, 1e-30, F],
                     [1.0, -3e38, 1e-20]],
        # inf, -inf, NaN, the smallest denormal, -0.0
        'nonfinite': [[inf, 1.0, 0.0], [-inf, -inf, 2.0], [nan, 0.5, 0.5], [1e-45, 0.0, -0.0],
                      [-0.0, -0.0, 1e-45]],
        'zero': [[0.0, 0.0, 0.0]] * 5,
        # all five tiny: every dot product is a sum of FLT_MAX multiples
        'all tiny': [[1e-30, 1e-30, 1e-30], [-1e-30, 1e-30, 1e-30], [1e-30, -1e-30, 1e-30],
                     [1e-30, 1e-30, -1e-30], [-1e-31, -1e-31, -1e-31]],
        'mixed': [[1e-30, 0.0, 0.0], [2e-20, 2e-20, 0.0], [1e20, 1.0, 1.0], [nan, inf, -inf], o],
        'signed zeros': [[-0.0, -0.0, -0.0], [-0.0, 1.0, 0.0], [0.0, -0.0, -2.0], o,
                         [-0.0, 1e-30, -0.0]],
        'one denormal': [[1e-45, 1e-45, 1e-45], [1e-45, 1.0, 0.0], [0.0, 0.0, 1e-45],
                         [-1e-40, 1e-40, 0.0], [1e-38, 0.0, 0.0]],
    }
    with np.errstate(all='ignore'):
        return {k: np.array(v, np.float32).reshape(15) for k, v in kinds.items()}


@functools.lru_cache(maxsize=None)
def reward_case():
    """(peaks volume, seeds, action batches): ``synthetic_subject``'s peaks with
    the centre block overwritten kind by kind; 12 seeds at random offsets in
    every block voxel, 120 in ordinary voxels next to the block, and seeds
    outside the volume on each side of each axis, so that the clip of
    ``int32(p[-2])`` runs at the first step.

    Every coordinate stays below 2^31 in magnitude: beyond it the C conversion
    of a float to int32 saturates where NumPy's ``astype(int32)`` gives
    INT32_MIN, so the reference and the kernel would read different voxels.
    (For the same reason no position here is +-inf: an overflowing float32
    action has a zero direction, the point does not move.)
    """
    _, _, pk = synthetic_subject(D)
    pk = pk.copy()
    kinds = _peak_kinds()
    names = sorted(kinds)
    for n, v in enumerate(BLOCK):
        pk[v] = kinds[names[n % len(names)]]
    rng = np.random.RandomState(17)
    inside = np.repeat(np.array(BLOCK, np.float64), 12, axis=0)
    inside = inside + rng.uniform(0.05, 0.95, inside.shape)
    near = rng.uniform(4.0, 9.0, (120, 3))
    outside = np.array([[-3.0, 6.2, 6.4], [40.0, 5.5, 6.5], [6.3, -2.5, 6.1], [5.2, 15.0, 6.0],
                        [6.6, 6.7, -7.0], [5.9, 6.8, 13.2], [-1e9, 6.5, 6.5], [6.5, 1e9, 5.5],
                        [6.5, 6.5, -1e9], [1e9, -1e9, 1e9], [-0.4, 12.3, 6.0]])
    assert np.abs(np.float32(outside)).max() < 2.0 ** 31
    seeds = np.concatenate([inside, near, outside])
    n = len(seeds)
    # actions: a fixed direction per row, wobbled a little per step, so that rows
    # survive the curvature test; at OVERFLOW_STEP every fifth row's action
    # has components of 1e19 .. 3e19 (the float32 sum of squares overflows, the
    # float64 one does not)
    base = rng.standard_normal((n, 3))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    actions = []
    for s in range(REWARD_STEPS):
        a = (base + 0.12 * rng.standard_normal((n, 3))) * rng.uniform(0.2, 3.0, (n, 1))
        if s == OVERFLOW_STEP:
            a[::5] = np.sign(a[::5]) * rng.uniform(1e19, 3e19, a[::5].shape)
        actions.append(np.ascontiguousarray(a, np.float32))
    pk.flags.writeable = False
    return pk, seeds, actions


@functools.lru_cache(maxsize=None)
def reward_expected(mode):
    """The oracle's episode on ``reward_case()``: per step the rows that were
    active, their new heads, rewards and dones."""
    pk, seeds, actions = reward_case()
    n = len(seeds)
    ref = oracle_env(mode, seeds, max_nb_steps=REWARD_MAX_NB_STEPS, peaks=pk, reward=True,
                     theta=REWARD_THETA)
    steps = []
    with np.errstate(all='ignore'):
        ref.reset(0, n)
        for a in actions:
            idx = ref.continue_idx.copy()
            _, rew, done, _ = ref.step(a[idx].copy())
            steps.append(dict(idx=idx, head=ref.streamlines[idx, ref.length - 1].copy(),
                              prev=ref.streamlines[idx, ref.length - 2].copy(),
                              reward=np.asarray(rew).copy(), done=done.astype(bool)))
            ref.harvest()
    return steps, dict(flags=ref.flags.copy(), lengths=ref.lengths.copy(),
                       streamlines=ref.streamlines.copy(), continue_idx=ref.continue_idx.copy())
