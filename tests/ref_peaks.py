"""References of the fODF peak extraction (HIP kernel ``k_peaks``; test
infrastructure only): ``peaks_from_sh``, a plain PyTorch fp32 restatement with
the semantics of tracktolearn_amd.reconst.peaks.peaks_from_sh (GEMM, another
summation order); ``peaks_ordered``, NumPy float32 in the kernel's own order,
which the kernel must equal bit for bit; ``peaks_float64``, the plain
definition with a per-voxel flag saying where it is decisive."""
import numpy as np
import torch

from tracktolearn_amd.reconst.peaks import hemisphere, sh_to_sf_matrix


@torch.no_grad()
def peaks_from_sh(sh, npeaks=5, relative_threshold=0.1, absolute_threshold=0.0,
                  min_separation_angle=25.0, subdivisions=3, chunk=1 << 18,
                  max_candidates=16):
    """fODF peaks of an SH volume.

    sh: (X, Y, Z, C) float32 tensor (any device).  Returns (X, Y, Z, 3*npeaks)
    float32 on the same device: up to ``npeaks`` unit directions sorted by
    decreasing SF value, each scaled by value / first value; zeros where a
    voxel has no signal (sum of coefficients == 0, env.py:418) or no peak.
    """
    dev = sh.device
    X, Y, Z, C = sh.shape
    order = int(round((-3 + np.sqrt(1 + 8 * C)) / 2))
    verts, nbr = hemisphere(subdivisions)
    B = torch.from_numpy(sh_to_sf_matrix(verts, order).astype(np.float32)).to(dev)
    V = torch.from_numpy(verts.astype(np.float32)).to(dev)
    nbr = torch.from_numpy(nbr).to(dev)
    cos_sep = float(np.cos(np.deg2rad(min_separation_angle)))
    flat = sh.reshape(-1, C)
    out = torch.zeros((flat.shape[0], npeaks, 3), dtype=torch.float32, device=dev)
    K = max_candidates
    for lo in range(0, flat.shape[0], chunk):
        part = flat[lo:lo + chunk]
        sf = part @ B                                            # GEMM (MFMA)
        sf = torch.where(sf < absolute_threshold, torch.zeros_like(sf), sf)
        # local maxima on the hemisphere graph: strictly above no neighbour
        # and above at least one (dipy local_maxima), positive
        nb_vals = sf[:, nbr]                                     # (n, V, D)
        is_max = (sf[:, :, None] >= nb_vals).all(dim=2) & \
            (sf[:, :, None] > nb_vals).any(dim=2) & (sf > 0)
        cand = torch.where(is_max, sf, torch.full_like(sf, -1.0))
        vals, idx = cand.topk(K, dim=1)                          # descending
        valid = vals > 0
        # relative threshold on (value - min(odf, floor 0))
        odf_min = sf.min(dim=1, keepdim=True).values.clamp(min=0.0)
        norm = vals - odf_min
        valid &= norm >= relative_threshold * norm[:, :1]
        dirs = V[idx]                                            # (n, K, 3)
        # greedy minimum-separation pruning, antipodally symmetric
        kept = torch.zeros_like(valid)
        for i in range(K):
            ok = valid[:, i].clone()
            if i:
                cosang = (dirs[:, :i] * dirs[:, i:i + 1]).sum(dim=2).abs()
                ok &= ~((cosang > cos_sep) & kept[:, :i]).any(dim=1)
            kept[:, i] = ok
        # first npeaks kept candidates, in order
        rank = kept.cumsum(dim=1) - 1
        take = kept & (rank < npeaks)
        rows = torch.nonzero(take)
        res = torch.zeros((part.shape[0], npeaks, 3), dtype=torch.float32, device=dev)
        first = torch.where(valid[:, :1], vals[:, :1], torch.ones_like(vals[:, :1]))
        scale = vals / first
        res[rows[:, 0], rank[rows[:, 0], rows[:, 1]]] = \
            dirs[rows[:, 0], rows[:, 1]] * scale[rows[:, 0], rows[:, 1], None]
        has_signal = part.sum(dim=1) != 0
        out[lo:lo + chunk] = res * has_signal[:, None, None]
    return out.reshape(X, Y, Z, 3 * npeaks)


# --------------------------------------------------------------------------
# The two references of ``k_peaks`` itself.  Both take the arguments of the C
# ABI (``ttl_peaks_from_sh``): sh [n][C] f32, B [C][V] f32, verts [V][3] f32,
# nbr [V][deg], npeaks, rel, abs, cos_sep, max_candidates -- any graph, not
# only the icosphere -- and return the chosen vertex indices [n][npeaks]
# (-1 where empty) next to the [n][3 * npeaks] output.
# --------------------------------------------------------------------------
MUTATIONS = (
    'max_ge_to_gt',          # >= -> > in the maximum test
    'no_gt_any',             # "above at least one neighbour" dropped
    'no_positive',           # x > 0 dropped (maximum test and the argmax's end test)
    'ties_highest',          # argmax ties to the highest index
    'min_unclamped',         # odf_min not clamped at 0
    'min_not_subtracted',    # odf_min not subtracted
    'rel_ge_to_gt',          # relative >= -> >
    'abs_lt_to_le',          # absolute < -> <=
    'sep_no_fabs',           # no fabs in the separation test
    'sep_gt_to_ge',          # separation > -> >=
    'sep_first_only',        # separation against the first kept peak only
    'scale_first_norm',      # scale by first_norm instead of first_val
    'drop_last_lane_group',  # vertices v >= 64 * (V // 64) ignored
    'drop_coef_64',          # coefficients c >= 64 ignored
    'cap_minus_one',         # max_candidates - 1
    'signal_abs_sum',        # no-signal test on sum |s| instead of sum s
)


def peaks_ordered(sh, B, verts, nbr, npeaks, rel, abs_thr, cos_sep, max_candidates,
                  mutate=None):
    """``k_peaks`` in NumPy float32, operation for operation in the kernel's
    own order (the library is built with -ffp-contract=off -fno-fast-math and
    IEEE division, so the kernel must give these bits): serial accumulation
    over the coefficients, one rounding per multiply and per add; min and
    argmax do not depend on the order.  Vectorised over voxels and vertices
    only.  ``mutate`` (test-only) plants one of ``MUTATIONS``."""
    assert mutate is None or mutate in MUTATIONS, mutate
    f32 = np.float32
    sh = np.ascontiguousarray(sh, f32)
    B = np.ascontiguousarray(B, f32)
    verts = np.ascontiguousarray(verts, f32)
    nbr = np.asarray(nbr, np.int64)
    n, C = sh.shape
    V = B.shape[1]
    rel, abs_thr, cos_sep = f32(rel), f32(abs_thr), f32(cos_sep)
    n_coef = min(C, 64) if mutate == 'drop_coef_64' else C
    total = np.zeros(n, f32)
    acc = np.zeros((n, V), f32)
    for c in range(n_coef):
        s = np.abs(sh[:, c]) if mutate == 'signal_abs_sum' else sh[:, c]
        total = total + s
        acc = acc + sh[:, c:c + 1] * B[c][None, :]
    signal = total != f32(0)
    if mutate == 'abs_lt_to_le':
        acc[acc <= abs_thr] = f32(0)
    else:
        acc[acc < abs_thr] = f32(0)
    lo = acc.min(axis=1)
    odf_min = lo if mutate == 'min_unclamped' else np.maximum(lo, f32(0))
    ge_all = np.ones((n, V), bool)
    gt_any = np.zeros((n, V), bool)
    for d in range(nbr.shape[1]):
        y = acc[:, nbr[:, d]]
        ge_all &= (acc > y) if mutate == 'max_ge_to_gt' else (acc >= y)
        gt_any |= acc > y
    is_cand = ge_all.copy()
    if mutate != 'no_gt_any':
        is_cand &= gt_any
    if mutate != 'no_positive':
        is_cand &= acc > f32(0)
    if mutate == 'drop_last_lane_group':
        is_cand[:, 64 * (V // 64):] = False
    is_cand &= signal[:, None]
    # candidates keep their value, the rest sit below every value
    low = f32(-3.0e38)
    cand = np.where(is_cand, acc, low)
    rows = np.arange(n)
    idx = np.full((n, npeaks), -1, np.int64)
    kdir = np.zeros((n, npeaks, 3), f32)
    kval = np.zeros((n, npeaks), f32)
    n_keep = np.zeros(n, np.int64)
    first_val = np.ones(n, f32)
    first_norm = np.zeros(n, f32)
    running = signal.copy()
    n_iter = max_candidates - 1 if mutate == 'cap_minus_one' else max_candidates
    for it in range(n_iter):
        running &= n_keep < npeaks
        if not running.any():
            break
        if mutate == 'ties_highest':
            bi = V - 1 - np.argmax(cand[:, ::-1], axis=1)
        else:
            bi = np.argmax(cand, axis=1)               # ties -> lowest index
        bv = cand[rows, bi]
        running &= (bv > low) if mutate == 'no_positive' else (bv > f32(0))
        cand[rows[running], bi[running]] = low         # retire it
        sub = f32(0) if mutate == 'min_not_subtracted' else odf_min
        norm = bv - sub
        if it == 0:
            first_val = np.where(running, bv, first_val)
            first_norm = np.where(running, norm, first_norm)
        with np.errstate(invalid='ignore', over='ignore'):
            cut = rel * first_norm
            running &= (norm > cut) if mutate == 'rel_ge_to_gt' else (norm >= cut)
        d = verts[bi]                                   # (n, 3)
        dot = (kdir[:, :, 0] * d[:, None, 0] + kdir[:, :, 1] * d[:, None, 1]) \
            + kdir[:, :, 2] * d[:, None, 2]
        ca = dot if mutate == 'sep_no_fabs' else np.abs(dot)
        close = (ca >= cos_sep) if mutate == 'sep_gt_to_ge' else (ca > cos_sep)
        slots = np.arange(npeaks)[None, :] < \
            (np.minimum(n_keep, 1) if mutate == 'sep_first_only' else n_keep)[:, None]
        ok = running & ~(close & slots).any(axis=1)
        r = rows[ok]
        idx[r, n_keep[r]] = bi[r]
        kdir[r, n_keep[r]] = d[r]
        kval[r, n_keep[r]] = bv[r]
        n_keep[r] += 1
    kept = np.arange(npeaks)[None, :] < n_keep[:, None]
    den = first_norm if mutate == 'scale_first_norm' else first_val
    with np.errstate(invalid='ignore', divide='ignore'):
        sc = np.where(kept, kval / den[:, None], f32(0)).astype(f32)
    out = np.where(kept[:, :, None], kdir * sc[:, :, None], f32(0)).astype(f32)
    return idx, out.reshape(n, 3 * npeaks)


_U = 2.0 ** -24


def peaks_float64(sh, B, verts, nbr, npeaks, rel, abs_thr, cos_sep, max_candidates,
                  exact=False):
    """The plain definition in float64, after the reference's call
    (env.py:405-432): ``get_maximas(odf, sphere, B, 0.1, 0)`` zeroes the SF
    below the absolute threshold and is dipy's documented ``peak_directions``
    -- local maxima (>= every neighbour, > at least one, positive), values
    minus max(min odf, 0), ``search_descending`` at the relative threshold,
    greedy ``remove_similar_vertices``, the first ``npeaks``; zeros where
    sum(coefs) == 0.  ``max_candidates`` bounds the candidates examined; None
    = unlimited (dipy).  Equal values go lowest index first.

    Returns (idx [n][npeaks], out [n][3 * npeaks] float64, decided [n] bool).
    A voxel is decided when every decision that can reach its output has a
    float64 margin above the float32 error bound of the quantities compared.
    Serial float32 accumulation of C products is off by at most
    gamma_C * sum |s_c| |B_cv| with gamma_C ~ C * 2^-24; the bound used is
    twice that, tau[v] = 2 C 2^-24 sum_c |s_c| |B[c][v]|, and the other half
    pays for the two or three roundings of the subtraction and the product
    in the relative cut.  ``exact=True`` is for the dyadic hand-built cases:
    every bound is 0 and ties are ties, and a voxel is decided only where
    nothing rounds in float32 -- the serial sums, the subtraction of the
    minimum, the product of the relative cut, value / first and the dot
    products of the vertices examined are all compared with float64."""
    sh = np.asarray(sh, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    verts = np.asarray(verts, np.float32).astype(np.float64)
    nbr = np.asarray(nbr, np.int64)
    rel = float(np.float32(rel))
    abs_thr = float(np.float32(abs_thr))
    cos_sep = float(np.float32(cos_sep))
    n, C = sh.shape
    V = B.shape[1]
    idx = np.full((n, npeaks), -1, np.int64)
    out = np.zeros((n, npeaks, 3), np.float64)
    decided = np.ones(n, bool)
    sep_eps = 0.0 if exact else 1e-6
    sf_all = sh @ B
    tau_all = np.zeros((n, V)) if exact else 2.0 * C * _U * (np.abs(sh) @ np.abs(B))

    def apart(margin, bound):
        return True if exact else margin > bound

    def same_in_f32(op, a, b):
        """float32 ``op(a, b)`` of two float32 values loses nothing."""
        with np.errstate(all='ignore'):
            return float(op(np.float32(a), np.float32(b))) == op(float(a), float(b))

    if exact:                     # the serial float32 sums against float64
        tot32 = np.zeros(n, np.float32)
        sf32 = np.zeros((n, V), np.float32)
        for c in range(C):
            tot32 = tot32 + sh[:, c].astype(np.float32)
            sf32 = sf32 + sh[:, c:c + 1].astype(np.float32) * B[c][None, :].astype(np.float32)
        decided &= (tot32.astype(np.float64) == sh.sum(axis=1))
        decided &= (sf32.astype(np.float64) == sf_all).all(axis=1)

    for i in range(n):
        s = sh[i]
        tot = float(s.sum())
        if not exact and np.any(s != 0) and not abs(tot) > 2.0 * C * _U * np.abs(s).sum():
            decided[i] = False
        if tot == 0.0:
            continue
        sf, tau = sf_all[i].copy(), tau_all[i].copy()
        ok = True
        # absolute threshold.  abs == 0 is a clamp (1-Lipschitz): the bound
        # carries over and needs no margin; a value robustly below the
        # threshold is exactly 0 on both sides
        zero = sf < abs_thr
        if not exact and abs_thr != 0.0 and np.any(np.abs(sf - abs_thr) <= tau):
            ok = False
        robust_zero = zero if exact else zero & (np.abs(sf - abs_thr) > tau)
        sf[zero] = 0.0
        tau[robust_zero] = 0.0
        # odf_min and its bound
        m = max(float(sf.min()), 0.0)
        if m == 0.0 and (robust_zero.any() or exact):
            tau_m = 0.0
        else:
            near_min = (sf - tau) <= float((sf + tau).min())
            tau_m = float(tau[near_min].max())
        # local maxima in float64
        nb = sf[nbr]                                            # (V, deg)
        x = sf[:, None]
        is_max = (x >= nb).all(1) & (x > nb).any(1) & (sf > 0.0)
        if not is_max.any():
            # robust only if no vertex can become one: checked below with first = 0
            first = 0.0
            tau_first = 0.0
        else:
            first = float(sf[is_max].max())
            tau_first = float(tau[is_max & (sf == first)].max())
        ulps = 0.0 if exact else 4.0 * _U * abs(first)
        cut = m + rel * (first - m)
        slack = tau + tau_m + rel * (tau_first + tau_m) + ulps     # per vertex
        under = (sf + slack < cut) if is_max.any() else np.zeros(V, bool)
        # maximum status of every vertex not robustly under the cut
        self_nb = nbr == np.arange(V)[:, None]
        gap = np.abs(x - nb)
        both_zero = robust_zero[:, None] & robust_zero[nbr]
        pair_ok = self_nb | both_zero | (gap > tau[:, None] + tau[nbr])
        pos_ok = robust_zero | (np.abs(sf) > tau)
        # one robustly greater neighbour settles "no maximum" on its own
        beaten = ((nb - x) > tau[:, None] + tau[nbr]).any(1) | robust_zero
        if not exact and np.any(~under & ~beaten & ~(pair_ok.all(1) & pos_ok)):
            ok = False
        # walk the candidates in descending order (ties: lowest index)
        cands = np.flatnonzero(is_max & ~under)
        cands = cands[np.lexsort((cands, -sf[cands]))]
        kept = []
        limit = len(cands) if max_candidates is None else min(len(cands), max_candidates)
        for k in range(limit):
            if len(kept) >= npeaks:
                break
            v = cands[k]
            if k + 1 < len(cands):
                w = cands[k + 1]
                if not apart(sf[v] - sf[w], tau[v] + tau[w]):
                    ok = False
            norm, norm0 = sf[v] - m, first - m
            if exact and not (same_in_f32(np.subtract, sf[v], m)
                              and same_in_f32(np.multiply, rel, norm0)
                              and same_in_f32(np.divide, sf[v], first)):
                ok = False
            if k > 0:
                if not apart(abs(norm - rel * norm0), slack[v]):
                    ok = False
                if not norm >= rel * norm0:
                    break
            close = False
            for q in kept:
                ca = abs(float(verts[q] @ verts[v]))
                if exact:
                    a, b = verts[q].astype(np.float32), verts[v].astype(np.float32)
                    if float((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) != float(
                            verts[q] @ verts[v]):
                        ok = False
                if not apart(abs(ca - cos_sep), sep_eps):
                    ok = False
                close |= ca > cos_sep
            if not close:
                kept.append(v)
        for j, v in enumerate(kept):
            idx[i, j] = v
            out[i, j] = verts[v] * (sf[v] / first)
        decided[i] &= ok
    return idx, out.reshape(n, 3 * npeaks), decided


def output_bound(sh, B, idx):
    """Per-component bound of |peaks_ordered - peaks_float64| on a decided
    voxel: (tau_v + tau_first * val / first) / first + 2^-23, [n][npeaks]
    (vertex coordinates are at most 1 in magnitude)."""
    sh = np.asarray(sh, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    C = sh.shape[1]
    sf = sh @ B
    tau = 2.0 * C * _U * (np.abs(sh) @ np.abs(B))
    safe = np.maximum(idx, 0)
    rows = np.arange(len(sh))[:, None]
    val, tv = sf[rows, safe], tau[rows, safe]
    first, tf = val[:, :1], tv[:, :1]
    with np.errstate(invalid='ignore', divide='ignore'):
        b = (tv + tf * np.abs(val / first)) / np.abs(first) + 2.0 ** -23
    return np.where(idx >= 0, b, 0.0)


def fibonacci_hemisphere(n_vertices, degree):
    """A synthetic graph for the kernel's vertex-count edges: a Fibonacci
    lattice on the upper half-sphere and, per vertex, its ``degree`` nearest
    other vertices up to sign (largest |cos|, ties to the lowest index), rows
    padded with the vertex itself where there are fewer.  (verts (V, 3)
    float64, nbr (V, degree) int64)."""
    k = np.arange(n_vertices, dtype=np.float64)
    z = 1.0 - (k + 0.5) / n_vertices
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    verts = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    c = np.abs(verts @ verts.T)
    np.fill_diagonal(c, -1.0)
    order = np.argsort(-c, axis=1, kind='stable')
    nbr = np.tile(np.arange(n_vertices)[:, None], (1, degree))
    take = min(degree, n_vertices - 1)
    nbr[:, :take] = order[:, :take]
    return verts, nbr
