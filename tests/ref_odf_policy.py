"""References of the fODF policy kernel (``k_odf`` in csrc/ttl_odf_policy.hip;
definition at ``ttl_odf_actions`` in include/ttl_hip.h; test infrastructure
only).  ``actions_ordered`` is NumPy float32 in the kernel's own operation
order, which both entry points must equal bit for bit; ``actions_float64`` is
the plain definition in float64 with a per-row flag saying where it is
decisive.  Both take what the kernel reads of a state row -- sh [n][C] and the
previous direction p [n][3] -- and return (actions [n][3], vertex [n] int32,
-1 = fallback)."""
import numpy as np

import ref_noise

DET, PROB = 0, 1
STREAM = 0x4F444650          # TTL_ODF_STREAM
U32 = 2.0 ** -24             # unit roundoff of float32

MUTATIONS = (
    'one_sided_cone',            # p.d >= ... instead of |p.d| >= ...
    'strict_cone',               # > instead of >= in the cone test
    'last_tie',                  # deterministic ties to the highest index
    'no_sign_flip',              # the action is +d whatever p.d
    'cone_relative_threshold',   # threshold relative to the cone's maximum
    'no_fallback',               # nothing admissible: the hemisphere's maximum
    'cdf_ignores_cone',          # probabilistic weights outside the cone
    'pick_at_or_below',          # >= instead of > in the cdf search
)


def uniforms(seed, ids, step):
    """u [n] float32 in [0, 1) of streamlines ``ids`` at ``step``: word 0 of
    Philox4x32-10 keyed by the seed, counter (id low, id high, step, STREAM),
    top 24 bits."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    ctr = np.stack([ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32),
                    np.full_like(ids, int(step) & 0xFFFFFFFF), np.full_like(ids, STREAM)], axis=-1)
    w0 = ref_noise.philox(ctr, key)[:, 0]
    return ((w0 >> np.uint32(8)).astype(np.float32) * np.float32(U32)).astype(np.float32)


def _u_for(n, mode, u, seed, ids, step):
    if mode != PROB:
        return np.zeros(n, np.float32)
    if u is not None:
        return np.broadcast_to(np.asarray(u, np.float32), (n,)).copy()
    steps = np.broadcast_to(np.asarray(step, np.int64), (n,))
    out = np.empty(n, np.float32)
    for s in np.unique(steps):          # rows of one launch may be at different steps
        sel = steps == s
        out[sel] = uniforms(seed, np.asarray(ids)[sel], int(s))
    return out


def _select(T, sf, p, dirs, cos_theta, rel, mode, u, mutate):
    """The rules on sf [n][V] in dtype T (every operation rounds to T).
    Returns (actions, vertex, parts) -- parts: what ``actions_float64`` derives
    its margins from."""
    n, V = sf.shape
    p, dirs = p.astype(T), dirs.astype(T)
    cos_theta, rel = T(cos_theta), T(rel)
    with np.errstate(invalid='ignore', over='ignore'):
        has_p = (p != 0).any(axis=1)
        dot = (p[:, 0:1] * dirs[None, :, 0] + p[:, 1:2] * dirs[None, :, 1]) + \
            p[:, 2:3] * dirs[None, :, 2]
        norm = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        cone_min = cos_theta * norm
        lhs = dot if mutate == 'one_sided_cone' else np.abs(dot)
        in_cone = (lhs > cone_min[:, None]) if mutate == 'strict_cone' else \
            (lhs >= cone_min[:, None])
        cone_ok = in_cone | ~has_p[:, None]
        pos = sf > 0
        cand = cone_ok & pos
        gmax = np.where(np.isnan(sf), -np.inf, sf).max(axis=1).astype(T)
        if mutate == 'cone_relative_threshold':
            gmax = np.where(cand, sf, -np.inf).max(axis=1).astype(T)
        thr = rel * gmax
        above = sf >= thr[:, None]
        adm = cand & above
        any_adm = adm.any(axis=1)
        if mode == DET:
            key = np.where(adm, sf, -np.inf)
            chosen = key.argmax(axis=1)
            if mutate == 'last_tie':
                chosen = V - 1 - key[:, ::-1].argmax(axis=1)
            cdf = t = None
        else:
            weighted = (pos & above) if mutate == 'cdf_ignores_cone' else adm
            any_adm = weighted.any(axis=1)
            w = np.where(weighted, sf, 0).astype(T)
            cdf = np.empty((n, V), T)
            run = np.zeros(n, T)
            for v in range(V):              # serial, vertex order
                run = run + w[:, v]
                cdf[:, v] = run
            t = u.astype(T) * cdf[:, -1]
            hit = (cdf >= t[:, None]) if mutate == 'pick_at_or_below' else (cdf > t[:, None])
            chosen = hit.argmax(axis=1)
            any_adm &= hit.any(axis=1)
        vertex = np.where(any_adm, chosen, -1).astype(np.int32)
        if mutate == 'no_fallback':
            top = np.where(np.isnan(sf), -np.inf, sf).argmax(axis=1)
            vertex = np.where(vertex < 0, top, vertex).astype(np.int32)
        rows = np.arange(n)
        safe = np.maximum(vertex, 0)
        d = dirs[safe]
        flip = dot[rows, safe] < 0
        if mutate == 'no_sign_flip':
            flip = np.zeros(n, bool)
        act = np.where(flip[:, None], -d, d)
        fallback = np.where(has_p[:, None], p, dirs[0][None, :])
        act = np.where((vertex >= 0)[:, None], act, fallback).astype(T)
    parts = dict(has_p=has_p, dot=dot, cone_min=cone_min, gmax=gmax, thr=thr, in_cone=in_cone,
                 pos=pos, above=above, adm=adm, cdf=cdf, t=t)
    return act, vertex, parts


def sf_ordered(sh, B):
    """sf [n][V] float32 as the kernel sums it: c ascending from 0.0f, one
    rounding per multiply and per add."""
    sh = np.ascontiguousarray(sh, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    acc = np.zeros((sh.shape[0], B.shape[1]), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(sh.shape[1]):
            acc = acc + sh[:, c:c + 1] * B[c][None, :]
    return acc


def actions_ordered(sh, p, B, dirs, cos_theta, rel, mode, seed=0, ids=None, step=0, u=None,
                    mutate=None):
    """``k_odf`` in NumPy float32, operation for operation in the kernel's own
    order.  ``ids`` [n]: id base + continue_idx; ``step`` scalar or [n];
    ``u`` (test-only) replaces the generator's uniforms; ``mutate`` (test-only)
    plants one of ``MUTATIONS``."""
    assert mutate is None or mutate in MUTATIONS, mutate
    f32 = np.float32
    n = len(sh)
    uu = _u_for(n, mode, u, seed, ids, step)
    act, vertex, _ = _select(f32, sf_ordered(sh, B), np.asarray(p, f32), np.asarray(dirs, f32),
                             f32(cos_theta), f32(rel), mode, uu, mutate)
    return act, vertex


def actions_float64(sh, p, B, dirs, cos_theta, rel, mode, seed=0, ids=None, step=0, u=None,
                    mutate=None):
    """The definition in float64 on the same float32 inputs.  Returns (actions,
    vertex, decided): a row is decided when every comparison that can reach its
    output has a float64 margin above what serial float32 arithmetic can move it
    by (each bound generous by a small factor):
      sf           tau[v] = 2 C 2^-24 sum_c |sh_c| |B[c][v]|
      gmax         max_v tau[v];  rel * gmax: + 2^-23 |rel gmax|
      p.d          6 * 2^-24 sum_i |p_i| |d_i|;  cos ||p||: 8 * 2^-24 cos ||p||
      cdf          sum of tau over the weighted vertices + V 2^-24 total;
                   u * total: the same + 2^-23 total
    A vertex is settled when one of its three admissibility tests fails
    decidedly or all hold decidedly; a row needs every vertex settled, the
    winner clear of every other admissible vertex by the sum of their tau (det)
    or u * total clear of both neighbouring cdf edges (prob), and the sign of
    p.d of the chosen vertex decided."""
    assert mutate is None or mutate in MUTATIONS, mutate
    f64 = np.float64
    sh64, B64 = np.asarray(sh, np.float32).astype(f64), np.asarray(B, np.float32).astype(f64)
    p64, d64 = np.asarray(p, np.float32).astype(f64), np.asarray(dirs, np.float32).astype(f64)
    cos64, rel64 = f64(np.float32(cos_theta)), f64(np.float32(rel))
    n, C = sh64.shape
    V = B64.shape[1]
    uu = _u_for(n, mode, u, seed, ids, step)
    with np.errstate(invalid='ignore', over='ignore'):
        sf = sh64 @ B64
        act, vertex, q = _select(f64, sf, p64, d64, cos64, rel64, mode, uu, mutate)
        tau = 2.0 * C * U32 * (np.abs(sh64) @ np.abs(B64))
        tau_dot = 6.0 * U32 * (np.abs(p64) @ np.abs(d64).T)
        tau_cone = tau_dot + 8.0 * U32 * np.abs(q['cone_min'])[:, None]
        tau_thr = tau + (abs(rel64) * tau.max(axis=1) + 2.0 * U32 * np.abs(q['thr']))[:, None]
        cone_sure = (np.abs(np.abs(q['dot']) - q['cone_min'][:, None]) > tau_cone) | \
            ~q['has_p'][:, None]
        cone_val = q['in_cone'] | ~q['has_p'][:, None]
        pos_sure = np.abs(sf) > tau
        thr_sure = np.abs(sf - q['thr'][:, None]) > tau_thr
        fails = (cone_sure & ~cone_val) | (pos_sure & ~q['pos']) | (thr_sure & ~q['above'])
        holds = cone_sure & cone_val & pos_sure & q['pos'] & thr_sure & q['above']
        decided = (fails | holds).all(axis=1) & np.isfinite(sf).all(axis=1)
        rows = np.arange(n)
        safe = np.maximum(vertex, 0)
        if mode == DET:
            gap = sf[rows, safe][:, None] - sf                     # to every other admissible one
            need = tau[rows, safe][:, None] + tau
            other = q['adm'].copy()
            other[rows, safe] = False
            decided &= (vertex < 0) | ~(other & ~(gap > need)).any(axis=1)
        else:
            total = q['cdf'][:, -1]
            bound = 2.0 * ((np.where(q['adm'], tau, 0.0)).sum(axis=1) + V * U32 * total) + \
                2.0 * U32 * total
            hi = q['cdf'][rows, safe]
            lo = np.where(safe > 0, q['cdf'][rows, np.maximum(safe - 1, 0)], -np.inf)
            decided &= (vertex < 0) | ((hi - q['t'] > bound) & (q['t'] - lo > bound))
        sign_sure = np.abs(q['dot'][rows, safe]) > tau_dot[rows, safe]
        decided &= (vertex < 0) | ~q['has_p'] | sign_sure
    return act, vertex, decided
