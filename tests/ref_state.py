"""References of the state gather (HIP kernels ``k_state``, ``k_state_dd`` and
the fused step tails of csrc/ttl_state.hip; test infrastructure only, NumPy
only): ``state_rows_f64``, the plain float64 definition with its error scale;
``emulate_k_state`` / ``emulate_k_state_dd``, float32 NumPy in each kernel's
own operation order; ``MUTATIONS``, deliberately wrong references.

The bound
---------
A state row is ``|kernel - value| <= BOUND_ULPS * 2**-24 * S`` per element,
``S = sum |w_i v_i|`` over the 8 corners.  Re-derived from the code: every
float32 rounding on the path of one term ``w_i v_i`` perturbs the result by at
most ``2**-24`` of a partial sum whose magnitude is at most ``S`` (first
order), so the number of roundings on the longest path bounds the error in
units of ``2**-24 S``.  Coordinates, floors and fractions are formed in
float32 by the reference exactly as by the kernels and carry no error.

  ``k_state``     ``e = 1 - d`` (1), ``(e_x e_y)`` and ``(.) e_z`` (2),
                  ``v w`` (1), seven adds of the 8-term chain (7): 11.
  ``k_state_dd``  ``e = 1 - d`` (1), the weight ``a b`` (1), the first product
                  ``v (a b)`` (1), three FMAs of the blend (3), then the 1-D
                  lerp: ``1 - d'`` (1), one product (1), one FMA (1): 9.

``k_state_dd`` states every fused operation in its source (``blend<>`` and
``lerp<>`` of ttl_state.hip), and ``emulate_k_state_dd`` takes the same order
with ``fma32``, a float32 FMA of one rounding: the kernel's finite rows equal
the emulation bit for bit.  ``k_state`` is compiled with fp contract fast and
its fused operations are the compiler's; ``emulate_k_state`` rounds every
product and sum, which contraction can only improve on.  16 leaves headroom
for a miscount, not for tuning.  The inputs must keep every product clear of
underflow: |v| >= 2**-20 and every weight 0 or >= 2**-72 (``check_inputs``).
"""
import itertools

import numpy as np

f32, f64 = np.float32, np.float64

BOUND_ULPS = 16.0
EPS = 2.0 ** -24

MUTATIONS = (
    'clip_weights',        # corners outside the volume get weight 0 (weights
                           # clipped, not indices: zero padding, no edge replication)
    'swap_yz_strides',     # the y and z strides of the volume swapped
    'plus_no_cross',       # a plus point that crossed into the next cell still uses slices f, f+1
    'minus_no_cross',      # a minus point that crossed down still uses slices f, f+1
    'offset_sign',         # point 5 (-y) sits at +y
    'shift_centre_only',   # the coordinate shift reaches the centre point only
    'tail_columns_zero',   # columns C-4 .. C-2 of all 7 points are 0 in rows with row % 5 == 2
    'dirs_off_by_one',     # direction j is segment j + 1
    'dirs_not_padded',     # the entry after the last segment is p_0 - 0, not 0
)


def stencil_points(heads, radius, shift, mutate=None):
    """(N, 7, 3) float32: head + [0, +x, +y, +z, -x, -y, -z] * float32(radius),
    added in float32; then + float32(shift), in float32, when it is non-zero."""
    heads = np.asarray(heads, dtype=f32)
    r = f32(radius)
    off = np.zeros((7, 3), dtype=f32)
    for a in range(3):
        off[1 + a, a] = r
        off[4 + a, a] = -r
    if mutate == 'offset_sign':
        off[5, 1] = r
    with np.errstate(invalid='ignore'):
        pts = (heads[:, None, :] + off[None]).astype(f32)
        s = f32(shift)
        if s != 0:
            if mutate == 'shift_centre_only':
                pts[:, 0] = pts[:, 0] + s
            else:
                pts = (pts + s).astype(f32)
    return pts


def _floor_frac(pts):
    with np.errstate(invalid='ignore'):
        fl = np.floor(pts).astype(f32)
        d = (pts - fl).astype(f32)
    return fl, d


def check_inputs(vol, heads, radius, shift):
    """The conditions under which no product of the gather can underflow."""
    assert np.abs(vol).min() >= 2.0 ** -20 and np.isfinite(vol).all()
    pts = stencil_points(heads, radius, shift)
    pts = pts[np.isfinite(pts).all(axis=(1, 2))]
    _, d = _floor_frac(pts)
    d = d.astype(f64)
    for bits in itertools.product((0, 1), repeat=3):
        w = np.prod([d[..., a] if b else 1.0 - d[..., a] for a, b in enumerate(bits)], axis=0)
        assert ((w == 0) | (w >= 2.0 ** -72)).all()


def direction_block(history, length, n_dirs, mutate=None):
    """(N, 3 n_dirs) float32: np.diff of the first ``length`` stored float32
    positions, most recent first, zero padded."""
    hist = np.asarray(history, dtype=f32)[:, :length]
    N = hist.shape[0]
    if mutate == 'dirs_not_padded':
        hist = np.concatenate((np.zeros((N, 1, 3), f32), hist), axis=1)
    seg = np.diff(hist, axis=1)[:, ::-1]
    if mutate == 'dirs_off_by_one':
        seg = seg[:, 1:]
    out = np.zeros((N, n_dirs, 3), dtype=f32)
    n = min(seg.shape[1], n_dirs)
    out[:, :n] = seg[:, :n]
    return out.reshape(N, 3 * n_dirs)


def state_rows_f64(vol, heads, radius, shift, history, length, n_dirs, mutate=None):
    """The state rows of streamlines whose newest points are ``heads`` (N, 3)
    float32 and whose first ``length`` points are ``history`` (N, >= length, 3).

    Returns ``(value, S)``: value (N, 7 C + 3 n_dirs) float64 -- the signal
    block is the plain 8-term trilinear sum in float64 (weights prod(d or
    1 - d), corner indices clipped to the volume, weights not), NaN for the
    whole block of a row with a non-finite coordinate; the direction block
    holds exact float32 values -- and S (N, 7 C) float64, sum |w_i v_i|."""
    assert mutate is None or mutate in MUTATIONS, mutate
    vol64 = np.asarray(vol, dtype=f64)
    X, Y, Z, C = vol64.shape
    dims = np.array([X, Y, Z])
    flat = vol64.reshape(-1, C)
    pts = stencil_points(heads, radius, shift, mutate)
    N = pts.shape[0]
    finite = np.isfinite(pts).all(axis=(1, 2))
    fl, d = _floor_frac(pts)
    for name, first in (('plus_no_cross', 1), ('minus_no_cross', 4)):
        if mutate == name:
            for a in range(3):      # the centre's cell, the point's own fraction
                fl[:, first + a, a] = fl[:, 0, a]
    base = np.nan_to_num(fl.astype(f64), nan=0.0, posinf=1e12, neginf=-1e12).astype(np.int64)
    d = np.where(np.isfinite(d), d, 0).astype(f64)
    value = np.zeros((N, 7, C), dtype=f64)
    S = np.zeros((N, 7, C), dtype=f64)
    for bits in itertools.product((0, 1), repeat=3):
        idx = base + np.array(bits)
        w = np.ones(idx.shape[:2], dtype=f64)
        for a, b in enumerate(bits):
            w = w * (d[..., a] if b else 1.0 - d[..., a])
        if mutate == 'clip_weights':
            w = np.where(((idx >= 0) & (idx < dims)).all(axis=-1), w, 0.0)
        ci = np.clip(idx, 0, dims - 1)
        if mutate == 'swap_yz_strides':
            lin = ci[..., 0] * (Y * Z) + ci[..., 1] + ci[..., 2] * Y
        else:
            lin = (ci[..., 0] * Y + ci[..., 1]) * Z + ci[..., 2]
        t = w[..., None] * flat[lin]
        value = value + t
        S = S + np.abs(t)
    if mutate == 'tail_columns_zero':
        value[np.arange(N) % 5 == 2, :, max(C - 4, 0):C - 1] = 0.0
    value[~finite] = np.nan
    S[~finite] = np.nan
    dirs = direction_block(history, length, n_dirs, mutate)
    return (np.concatenate((value.reshape(N, 7 * C), dirs.astype(f64)), axis=1),
            S.reshape(N, 7 * C))


def excess(got, value, S):
    """Per element: |got - value| in units of the bound (<= 1 passes); rows the
    reference makes NaN count 0 where ``got`` is NaN too and inf where not."""
    got = np.asarray(got, dtype=f64)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.abs(got - value) / (BOUND_ULPS * EPS * S)
    e = np.where(np.isnan(value), np.where(np.isnan(got), 0.0, np.inf), e)
    return np.where(np.isnan(e), np.inf, e)     # got NaN where the reference is finite


# --------------------------------------------------------------------------- #
# float32 emulations of the kernels' operation order
def fma32(a, b, c):
    """float32 ``a * b + c`` with one rounding.  The float64 product of two
    float32 values is exact; the float64 sum is rounded to odd (TwoSum gives its
    error: where there is one and the sum's last bit is even, the neighbour on
    the error's side is taken), and a value rounded to odd at 53 bits rounds to
    24 bits as the exact one does.  A plain float64 sum can double-round."""
    p = np.asarray(a, dtype=f32).astype(f64) * np.asarray(b, dtype=f32).astype(f64)
    c = np.asarray(c, dtype=f32).astype(f64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        towards = np.where(err > 0, np.inf, -np.inf)
        s = np.where((err != 0) & even & np.isfinite(s), np.nextafter(s, towards), s)
        return s.astype(f32)


def _clamp_int(fl, lo, hi):
    """(int) fminf(fmaxf(fl, lo), hi): NaN comes out as lo."""
    with np.errstate(invalid='ignore'):
        c = np.where(np.isnan(fl), f32(lo), np.minimum(np.maximum(fl, f32(lo)), f32(hi)))
    return c.astype(np.int64)


def emulate_k_state(vol, heads, radius, shift):
    """The 56-fetch kernel: (N, 7 C) float32."""
    vol = np.asarray(vol, dtype=f32)
    dims = vol.shape[:3]
    C = vol.shape[3]
    pts = stencil_points(heads, radius, shift)
    fl, d = _floor_frac(pts)
    e = (f32(1) - d).astype(f32)
    lo, hi = [], []
    for a in range(3):
        i0 = _clamp_int(fl[..., a], -1, dims[a])
        lo.append(np.clip(i0, 0, dims[a] - 1))
        hi.append(np.clip(i0 + 1, 0, dims[a] - 1))
    acc = None
    with np.errstate(invalid='ignore'):
        for bx, by, bz in itertools.product((0, 1), repeat=3):     # 000, 001, 010, ...
            w = (((d if bx else e)[..., 0] * (d if by else e)[..., 1]).astype(f32) *
                 (d if bz else e)[..., 2]).astype(f32)
            v = vol[(hi if bx else lo)[0], (hi if by else lo)[1], (hi if bz else lo)[2]]
            t = (v * w[..., None]).astype(f32)
            acc = t if acc is None else (acc + t).astype(f32)
    return acc.reshape(-1, 7 * C)


def emulate_k_state_dd(vol, heads, radius, shift):
    """The register-deduplicated kernel (0 < radius < 1): (N, 7 C) float32."""
    vol = np.asarray(vol, dtype=f32)
    dims = vol.shape[:3]
    C = vol.shape[3]
    pts = stencil_points(heads, radius, shift)
    N = pts.shape[0]
    fl, d = _floor_frac(pts)
    fc, dc = fl[:, 0], d[:, 0]                          # the centre point
    ec = (f32(1) - dc).astype(f32)
    sl = []                                             # slices f-1 .. f+2, clipped
    for a in range(3):
        i = _clamp_int(fc[:, a], -4, dims[a] + 4)
        sl.append([np.clip(i + k, 0, dims[a] - 1) for k in (-1, 0, 1, 2)])

    def rec(i, j, k):
        return vol[sl[0][i], sl[1][j], sl[2][k]]

    def blend(outer, v00, v01, v10, v11, a0, a1, b0, b1):
        # a centre slice (f, f+1) starts from v00 w00, an outer one (f-1, f+2) from v01 w01
        terms = [(v, (a * b).astype(f32)[:, None]) for v, a, b in
                 ((v00, a0, b0), (v01, a0, b1), (v10, a1, b0), (v11, a1, b1))]
        if outer:
            terms[0], terms[1] = terms[1], terms[0]
        r = (terms[0][0] * terms[0][1]).astype(f32)
        for v, w in terms[1:]:
            r = fma32(v, w, r)
        return r

    def lerp(minus, lo, hi, dd):
        e, dd = (f32(1) - dd).astype(f32)[:, None], dd[:, None]
        if minus:
            return fma32(hi, dd, (lo * e).astype(f32))
        return fma32(lo, e, (hi * dd).astype(f32))

    out = np.zeros((N, 7, C), dtype=f32)
    with np.errstate(invalid='ignore'):
        for a in range(3):
            b, c = [x for x in range(3) if x != a]

            def at(s, jb, jc):
                ijk = [0, 0, 0]
                ijk[a], ijk[b], ijk[c] = s, jb, jc
                return rec(*ijk)
            B = [blend(s in (0, 3), at(s, 1, 1), at(s, 1, 2), at(s, 2, 1), at(s, 2, 2),
                       ec[:, b], dc[:, b], ec[:, c], dc[:, c]) for s in range(4)]
            if a == 0:
                out[:, 0] = lerp(False, B[1], B[2], dc[:, 0])
            up = (fl[:, 1 + a, a] > fc[:, a])[:, None]
            dn = (fl[:, 4 + a, a] < fc[:, a])[:, None]
            out[:, 1 + a] = lerp(False, np.where(up, B[2], B[1]), np.where(up, B[3], B[2]),
                                 d[:, 1 + a, a])
            out[:, 4 + a] = lerp(True, np.where(dn, B[0], B[1]), np.where(dn, B[1], B[2]),
                                 d[:, 4 + a, a])
    return out.reshape(N, 7 * C)
