"""Inputs of the fODF policy tests (tests/test_odf_policy_reference.py): every
case is what one launch of ``ttl_odf_actions`` reads -- ``sh`` [n][C], ``p``
[n][3], ``B`` [C][V], ``dirs`` [V][3], cos_theta, rel, mode, seed, id base,
continue_idx, step (scalar, or per row for the reference alone), optionally a
state pitch -- plus, for the hand-built ones, the literal expected vertices."""
import functools

import numpy as np

import ref_odf_policy as ref
from tracktolearn_amd.reconst import peaks as pk

F32 = np.float32
DET, PROB = ref.DET, ref.PROB


def cos_deg(deg):
    return float(F32(np.cos(np.deg2rad(deg))))


def n_coef(order):
    return (order + 1) * (order + 2) // 2


@functools.lru_cache(maxsize=None)
def tables(order, n_vertices=None):
    """(B [C][V], dirs [V][3]) of hemisphere(3) -- hemisphere(4) for more than
    its 321 vertices --, cut to the first n_vertices."""
    verts, _ = pk.hemisphere(4 if (n_vertices or 0) > 321 else 3)
    verts = verts[:n_vertices]
    return (np.ascontiguousarray(pk.sh_to_sf_matrix(verts, order), F32),
            np.ascontiguousarray(verts, F32))


def fodf_like(n, C, seed):
    """The peaks tests' fields: 0.2 * randn, DC 1 + U(0, 1)."""
    rng = np.random.RandomState(seed)
    sh = (rng.standard_normal((n, C)) * 0.2).astype(F32)
    sh[:, 0] = 1.0 + rng.uniform(0, 1, n)
    return sh


def unit_p(n, seed, zero_every=0):
    rng = np.random.RandomState(seed)
    p = rng.standard_normal((n, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(F32)
    if zero_every:
        p[::zero_every] = 0
    return p


def case(sh, p, B, dirs, cos_theta, rel=0.1, mode=DET, seed=0, ids_base=0, idx=None, step=3,
         pitch=None, expect=None):
    n = len(sh)
    return dict(sh=np.ascontiguousarray(sh, F32), p=np.ascontiguousarray(p, F32), B=B, dirs=dirs,
                cos_theta=float(F32(cos_theta)), rel=float(F32(rel)), mode=mode, seed=seed,
                ids_base=ids_base,
                idx=np.arange(n, dtype=np.int32) if idx is None else np.asarray(idx, np.int32),
                step=step, pitch=pitch, expect=expect)


def reference_args(c, **more):
    """Keyword arguments of ref_odf_policy.actions_* for a case."""
    kw = dict(sh=c['sh'], p=c['p'], B=c['B'], dirs=c['dirs'], cos_theta=c['cos_theta'],
              rel=c['rel'], mode=c['mode'], seed=c['seed'],
              ids=c['ids_base'] + c['idx'].astype(np.int64), step=c['step'])
    kw.update(more)
    return kw


# ------------------------------------------------------------ random fields
RANDOM_N = 4000


@functools.lru_cache(maxsize=None)
def random_case(order, theta, mode):
    """4 000 fODF-like rows with random unit p on hemisphere(3)."""
    B, dirs = tables(order)
    C = n_coef(order)
    return case(fodf_like(RANDOM_N, C, 100 + order), unit_p(RANDOM_N, 200 + int(theta)), B, dirs,
                cos_deg(theta), 0.1, mode, seed=0x1234567887654321, ids_base=5000, step=7)


RANDOM_KEYS = [(order, theta, mode) for order in (6, 8) for theta in (20.0, 30.0, 45.0, 60.0)
               for mode in (DET, PROB)]


# ---------------------------------------------------- hand-built, exact cases
# five vertices, B = identity (sf = sh), cos_theta = 0.6: float32(0.6) * 1 is
# float32(0.6), so d2 = (0.6, 0.8, 0) sits exactly on the cone edge of p = +-x
HAND_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [0, 0, 1], [0, 0.6, 0.8]], F32)
HAND_B = np.eye(5, dtype=F32)
X, MX, Z0 = (1, 0, 0), (-1, 0, 0), (0, 0, 0)


def _hand(sf, p, cos_theta=0.6, rel=0.25, mode=DET, expect=None, **kw):
    return case(np.array([sf], F32), np.array([p], F32), HAND_B, HAND_DIRS, cos_theta, rel, mode,
                expect=expect, **kw)


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> case with ``expect`` = (vertex, action)."""
    d = HAND_DIRS
    nan = float('nan')
    cases = {
        # d2 is exactly on the cone edge and has the larger value
        'cone_edge_is_in': _hand([2, 8, 4, 8, 0], X, expect=(2, d[2])),
        # admissible only through -d: the action is -d0
        'through_minus_d': _hand([4, 0, 0, 0, 0], MX, expect=(0, -d[0])),
        # p . d0 = 0 at cos_theta = 0: in the cone, sign +
        'perpendicular_plus': _hand([4, 0, 0, 0, 0], (0, 0, 1), cos_theta=0.0, expect=(0, d[0])),
        'tie_lowest_index': _hand([1, 4, 1, 4, 1], Z0, expect=(1, d[1])),
        # gmax = 8 outside the cone, d0 = 2 = 0.25 * 8 sits on the threshold
        'at_threshold_is_in': _hand([2, 0, 1, 8, 0], X, expect=(0, d[0])),
        # d0 = 1 is 100 % of the cone's maximum but below 0.125 * 16
        'hemisphere_relative': _hand([1, 0, 0.5, 16, 0], X, rel=0.125, expect=(-1, X)),
        'cone_not_positive': _hand([-1, 4, 0, 4, 2], X, expect=(-1, X)),
        'no_p_whole_hemisphere': _hand([1, 2, 1, 8, 2], Z0, expect=(3, d[3])),
        'no_p_nothing_positive': _hand([-1, 0, -2, 0, -1], Z0, expect=(-1, d[0])),
        # NaN * 0 is NaN: every sf is NaN and no comparison holds
        'nan_coefficient': _hand([nan, 4, 4, 4, 4], X, expect=(-1, X)),
    }
    return cases


# prob mode with an injected u (the reference alone): weights 1, 2, -, 1, - of
# the admissible vertices 0, 1, 3 (0.25 * 2 = 0.5 cuts nothing positive), cdf
# edges 1, 3, 4 of a total of 4
PROB_SF = [1, 2, 0, 1, 0]
PROB_U = [(0.0, 0), (0.25 - 2.0 ** -24, 0), (0.25, 1), (0.25 + 2.0 ** -24, 1),
          (0.75 - 2.0 ** -24, 1), (0.75, 3), (1.0 - 2.0 ** -24, 3)]


def prob_hand_case():
    return _hand(PROB_SF, Z0, mode=PROB)


# --------------------------------------------------- shapes the GPU part adds
#: streamline ids whose u under (seed 77, step 2) is a multiple of 1/64 (37, 62,
#: 60, 34, 35, 53 sixty-fourths; found by search, asserted by the CPU tests)
EDGE_IDS = (469160, 509384, 1052207, 1534820, 1834744, 2051604)


@functools.lru_cache(maxsize=None)
def uniform_weights_case():
    """64 vertices of weight 1 and no p: every multiple of 1/64 is a cdf edge.
    Rows 0..5 carry the ids of EDGE_IDS, whose u sits exactly on an edge -- the
    inputs on which ``>`` and ``>=`` in the cdf search differ; the other rows
    have ordinary ids."""
    verts = tables(0, 64)[1]
    n = 100
    idx = np.arange(n, dtype=np.int64)
    idx[:len(EDGE_IDS)] = np.asarray(EDGE_IDS) - 1000
    return case(np.ones((n, 1), F32), np.zeros((n, 3), F32), np.ones((1, 64), F32), verts,
                0.5, 0.1, PROB, seed=77, ids_base=1000, idx=idx, step=2)


@functools.lru_cache(maxsize=None)
def cone_prob_case():
    """fODF-like rows, prob mode, a narrow cone: most of the positive weight
    lies outside the cone."""
    B, dirs = tables(6)
    return case(fodf_like(500, 28, 9), unit_p(500, 10), B, dirs, cos_deg(20.0), 0.1, PROB, seed=5,
                ids_base=100, step=4)


def shape_case(C, V, n, mode, seed=0):
    """C coefficients (random B where C is no full even order), V vertices, a
    pitch wider than the row, step-0 rows (p = 0) mixed in, continue_idx a
    non-identity permutation over a non-zero id base."""
    rng = np.random.RandomState(1000 * C + 10 * V + n + seed)
    verts = tables(0, V)[1]
    if C in (1, 6, 15, 28, 45):
        B = tables({1: 0, 6: 2, 15: 4, 28: 6, 45: 8}[C], V)[0]
    else:
        B = (rng.standard_normal((C, V)) * 0.3).astype(F32)
        B[0] = 0.28
    idx = rng.permutation(n + 7)[:n].astype(np.int32)
    return case(fodf_like(n, C, C + V + n), unit_p(n, V + n, zero_every=5), B, verts,
                cos_deg(45.0), 0.1, mode, seed=0xABCDEF0123456789, ids_base=(1 << 33) + 11,
                idx=idx, step=5, pitch=7 * C + 3 + 5)


SHAPES = [(C, V, n) for C in (6, 28, 45) for V in (1, 2, 63, 64, 65, 321) for n in (65,)] + \
    [(28, 65, n) for n in (0, 1, 63, 64, 1000)] + \
    [(C, 65, 130) for C in (1, 15, 7, 33, 64)] + \
    [(64, 321, 130), (45, 700, 65)]         # B and dirs in two and in three LDS chunks


def state_rows(c, dir_offset=None):
    """The case as state rows [n][pitch] (garbage between the columns the
    kernel reads) and the dir_offset."""
    n, C = c['sh'].shape
    dir_offset = 7 * C if dir_offset is None else dir_offset
    pitch = c['pitch'] or dir_offset + 3
    rng = np.random.RandomState(n + C)
    state = rng.standard_normal((n, pitch)).astype(F32)
    state[:, :C] = c['sh']
    state[:, dir_offset:dir_offset + 3] = c['p']
    return state, dir_offset
