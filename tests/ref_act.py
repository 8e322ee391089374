"""NumPy restatement of the ACT / CMC stopping criterion (include/ttl_hip.h,
ttl_act_flags).  The GPU tests hold the library to this file bit
for bit; the CPU tests hold this file to hand-made cases and show that every
named mutant below is told apart by the committed cases.

Definition.  For row r < n: g = ids[r] (r without ids); p = point n_points - 1
of history row g (float32); x_c = float64(p_c) + coord_shift.  The point is
inside iff x_c >= -0.5 and x_c < dim_c - 0.5 for every c (NaN compares false).
Outside: include = exclude = 0, no flag.  Inside: i_c = floor(x_c), f_c = x_c -
i_c, lo_c = clamp(i_c, 0, dim_c - 1), hi_c = clamp(i_c + 1, 0, dim_c - 1); in
float64, every multiply and add rounded once: along z c_ab = v[a][b][lo_z] *
(1 - f_z) + v[a][b][hi_z] * f_z, along y c_a = c_a,lo * (1 - f_y) + c_a,hi *
f_y, along x val = c_lo * (1 - f_x) + c_hi * f_x.
Suppression: with init_len a row with n_points <= init_len[g] gets flag 0.
THRESHOLD: TARGET iff include > 0.5, else EXCLUDE iff exclude > 0.5, else 0.
CMC: s = include + exclude; not s > 0: 0.  num = max(1 - s, 0); den = num + s;
rho = num / den; P = pow(rho, exponent) (rho itself for exponent == 1).
Philox4x32-10, key = halves of seed, counter = (id low, id high, n_points,
ACT_STREAM), id = ids_base + g; u1 = (word0 >> 8) * 2^-24, u2 = (word1 >> 8) *
2^-24.  Stops iff u1 >= P; a stopped row is TARGET iff u2 < include / s, else
EXCLUDE."""
import numpy as np

import ref_noise

TARGET, EXCLUDE = 8, 128
THRESHOLD, CMC = 0, 1
ACT_STREAM = 0x41435420
F64 = np.float64

MUTANTS = (
    'xyz_swapped',         # maps indexed [z][y][x]
    'ge_threshold',        # >= 0.5 in place of > 0.5
    'exclude_first',       # the exclude map has priority
    'shift_sign',          # x - coord_shift
    'zero_pad',            # corners outside the grid contribute 0 instead of clamping
    'outside_inclusive',   # x <= dim - 0.5 is still inside
    'judge_seed',          # suppression with n_points < init_len
    'same_word',           # u2 from word 0
    'stop_gt',             # stops iff u1 > P
    'step_off_by_one',     # counter word 2 = n_points - 1
)


def uniforms(seed, ids, n_points):
    """(u1, u2) float64 of streamline ids (int64 >= 0) at ``n_points``."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    u = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    key = np.array([seed & ref_noise.MASK32, seed >> 32], dtype=np.uint64)
    ctr = np.stack([u & np.uint64(ref_noise.MASK32), u >> np.uint64(32),
                    np.full_like(u, int(n_points) & ref_noise.MASK32),
                    np.full_like(u, ACT_STREAM)], axis=-1)
    w = ref_noise.philox(ctr, key)
    return ((w[:, 0] >> np.uint32(8)).astype(F64) * 2.0 ** -24,
            (w[:, 1] >> np.uint32(8)).astype(F64) * 2.0 ** -24)


def _lerp(a, b, f):
    return a * (F64(1.0) - f) + b * f


def _sample(vol, x, inside, mutate):
    """Trilinear value (float64, the stated order) of ``vol`` at x (n, 3)."""
    vol = np.asarray(vol, dtype=np.float32)
    dim = vol.shape
    n = len(x)
    val = np.zeros(n, F64)
    rows = np.nonzero(inside)[0]
    if not len(rows):
        return val
    xi = x[rows]
    fl = np.floor(xi)
    f = xi - fl
    i = fl.astype(np.int64)
    lo, hi, wlo, whi = [], [], [], []
    for c in range(3):
        a, b = i[:, c], i[:, c] + 1
        lo.append(np.clip(a, 0, dim[c] - 1))
        hi.append(np.clip(b, 0, dim[c] - 1))
        # zero_pad: a corner whose index was clamped counts as 0
        wlo.append(((a >= 0) & (a <= dim[c] - 1)) if mutate == 'zero_pad' else np.ones(len(a), bool))
        whi.append(((b >= 0) & (b <= dim[c] - 1)) if mutate == 'zero_pad' else np.ones(len(b), bool))

    def v(ix, iy, iz, ok):
        if mutate == 'xyz_swapped':
            # the wrong raster: flat offset computed as if the volume were [Z][Y][X]
            flat = (iz * dim[1] + iy) * dim[0] + ix
            got = vol.reshape(-1)[flat]
        else:
            got = vol[ix, iy, iz]
        return np.where(ok, got.astype(F64), F64(0.0))

    c = {}
    for a, (ix, okx) in enumerate(((lo[0], wlo[0]), (hi[0], whi[0]))):
        for b, (iy, oky) in enumerate(((lo[1], wlo[1]), (hi[1], whi[1]))):
            c[a, b] = _lerp(v(ix, iy, lo[2], okx & oky & wlo[2]),
                            v(ix, iy, hi[2], okx & oky & whi[2]), f[:, 2])
    c0 = _lerp(c[0, 0], c[0, 1], f[:, 1])
    c1 = _lerp(c[1, 0], c[1, 1], f[:, 1])
    val[rows] = _lerp(c0, c1, f[:, 0])
    return val


def _values(include, exclude, history, n_points, ids, n, coord_shift, mutate):
    history = np.asarray(history, dtype=np.float32)
    g = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)[:n]
    p = history[g, n_points - 1].astype(F64)
    shift = F64(coord_shift)
    x = p - shift if mutate == 'shift_sign' else p + shift
    dim = np.asarray(np.shape(include), dtype=F64)
    with np.errstate(invalid='ignore'):
        upper = (x <= dim - 0.5) if mutate == 'outside_inclusive' else (x < dim - 0.5)
        inside = ((x >= -0.5) & upper).all(axis=1)
    inc = _sample(include, x, inside, mutate)
    exc = _sample(exclude, x, inside, mutate)
    return g, inside, inc, exc


def act_values_ordered(include, exclude, history, n_points, ids=None, n=None, coord_shift=0.0,
                       mutate=None):
    """(n, 2) float64: include and exclude at the newest point of every row."""
    n = (len(history) if ids is None else len(ids)) if n is None else n
    _, _, inc, exc = _values(include, exclude, history, n_points, ids, n, coord_shift, mutate)
    return np.stack([inc, exc], axis=1)


def cmc_terms(inc, exc, exponent):
    """(s, rho, P) of the CMC rule; P = 1 where not s > 0 (never read there)."""
    s = inc + exc
    num = np.maximum(F64(1.0) - s, F64(0.0))
    den = num + s
    with np.errstate(invalid='ignore', divide='ignore'):
        rho = np.where(s > 0, num / np.where(den > 0, den, 1.0), 1.0)
        P = rho if F64(exponent) == 1.0 else np.power(rho, F64(exponent))
    return s, rho, P


def act_flags_ordered(include, exclude, history, n_points, mode, ids=None, init_len=None, n=None,
                      coord_shift=0.0, exponent=1.0, seed=0, ids_base=0, mutate=None,
                      return_terms=False):
    """uint8 flags (n,) of ``ttl_act_flags``; ``mutate`` names one of MUTANTS.
    ``return_terms``: also a dict with the values, u1, P, rho and the judged mask
    (what the undecided-row check needs)."""
    n = (len(history) if ids is None else len(ids)) if n is None else n
    g, inside, inc, exc = _values(include, exclude, history, n_points, ids, n, coord_shift, mutate)
    judged = inside.copy()
    if init_len is not None:
        il = np.asarray(init_len, dtype=np.int64)[g]
        judged &= (n_points >= il) if mutate == 'judge_seed' else (n_points > il)
    flags = np.zeros(n, np.uint8)
    terms = dict(values=np.stack([inc, exc], axis=1), judged=judged)
    if mode == THRESHOLD:
        t = (inc >= 0.5) if mutate == 'ge_threshold' else (inc > 0.5)
        e = (exc >= 0.5) if mutate == 'ge_threshold' else (exc > 0.5)
        if mutate == 'exclude_first':
            out = np.where(e, EXCLUDE, np.where(t, TARGET, 0))
        else:
            out = np.where(t, TARGET, np.where(e, EXCLUDE, 0))
    elif mode == CMC:
        s, rho, P = cmc_terms(inc, exc, exponent)
        step = n_points - 1 if mutate == 'step_off_by_one' else n_points
        u1, u2 = uniforms(seed, int(ids_base) + g, step)
        if mutate == 'same_word':
            u2 = u1
        stop = (s > 0) & ((u1 > P) if mutate == 'stop_gt' else (u1 >= P))
        with np.errstate(invalid='ignore', divide='ignore'):
            share = inc / np.where(s > 0, s, 1.0)
        out = np.where(stop, np.where(u2 < share, TARGET, EXCLUDE), 0)
        terms.update(u1=u1, u2=u2, P=P, rho=rho, s=s)
    else:
        raise ValueError(f'unknown mode {mode}')
    flags[judged] = out[judged].astype(np.uint8)
    return (flags, terms) if return_terms else flags


def undecided(terms, exponent):
    """Rows whose CMC comparison u1 >= P could fall either way between two
    float64 ``pow`` implementations: judged, 0 < rho < 1, the power actually
    computed (exponent != 1) and |u1 - P| <= 2^-40."""
    if F64(exponent) == 1.0:
        return np.zeros(len(terms['judged']), bool)
    rho = terms['rho']
    return terms['judged'] & (terms['s'] > 0) & (rho > 0) & (rho < 1) & \
        (np.abs(terms['u1'] - terms['P']) <= 2.0 ** -40)
