"""The learner kernels (tracktolearn_amd/csrc/ttl_learner.hip) in NumPy float32,
operation for operation in the kernels' own order (test infrastructure only).

The library is built with -ffp-contract=off -fno-fast-math and correctly
rounded division and square root, and the kernels sum in fixed orders, so
everything below except the four libm calls (expf, logf, log1pf, tanhf) is a
fixed sequence of correctly rounded float32 operations: the kernels must give
these bits.  The libm calls are taken through ``libm`` (NumPy's by default):
outputs behind one are NOT expected to match to the bit and are held to the
measured tolerance of tests/ref_learner_ops.py instead.  Per function the
docstring says which outputs are which.

Line numbers cite ttl_learner.hip.  Every function takes ``mutate``: one of
``MUTATIONS`` planted into the restatement (test only), to show that the
suite's inputs and assertions would notice that bug in a kernel.
"""
import math

import numpy as np

f32 = np.float32
HEAD_PLAIN, HEAD_SAC, HEAD_TANH = 0, 1, 2
NW = 4                    # waves per workgroup (:19)
FWD_ROWS = 4              # rows per workgroup of the forward / head backward (:82)
LOSS_BLOCK = 256          # rows per workgroup of the loss kernels (:18)
HALF_LOG_2PI = f32(0.91893853320467274178)     # :20
LOG_2 = f32(0.69314718055994530942)            # :21
LS_MIN, LS_MAX = f32(-20.0), f32(2.0)          # :22

MUTATIONS = (
    # forward / the split dot product (also the head backward's)
    'fwd_drop_last_chunk',        # a wave's last column chunk dropped
    'fwd_skip_wave3',             # wave 3's quarter of the columns skipped
    'fwd_no_bias',                # bias omitted
    'fwd_ls_raw_clamped',         # log_std_raw stored clamped
    'fwd_clamp_one_side',         # clamp(raw, -20, 2) -> min(raw, 2)
    'fwd_ent_le',                 # entropy window m <= entropy_rows
    'fwd_ent_dup_last',           # clamped duplicate of the last row in a partial block's partial
    'fwd_tanh_corr_sign',         # logp = gauss + correction
    'fwd_softplus_no_threshold',  # log1p(exp(x)) for every x
    'fwd_bd_critic0',             # block diagonal: critic 0's activations for every output
    'fwd_bd_planes_as_side',      # block stride taken as n_in (side by side) for planes
    # losses
    'loss_no_not_done',           # not_done dropped from the backup / target
    'loss_min_is_q1',             # min(tq1, tq2) -> tq1
    'loss_logp_row_i',            # logp[i] in the backup instead of logp[n + i]
    'loss_tie_full',              # a tie gives each critic the whole -1/n
    'loss_no_factor2',            # dq = (q - backup) / n
    'loss_inv_2n',                # 1 / (2 n)
    'loss_drop_last_block',       # the last, partial block's rows left out of loss_part
    'loss_tick_unticked',         # optimizers outside tick_mask ticked too
    'loss_consts_from_pows_before',   # lr / (1 - beta^(step-1)), sqrt(1 - beta2^(step-1))
    'td3_nq1_row_2i',             # n_q = 1: row 2 i read instead of row i
    # thin backward / ReLU backward
    'bwd_relu_ge',                # a >= 0 instead of a > 0
    'bwd_sum_outside_window',     # rows outside [r0, r1) summed
    'bwd_dz_window_only',         # dz not stored for rows outside the window
    'bwd_skip_block_tail',        # rows i >= 4 (rpb // 4) of a block skipped
    'bwd_dw_post_relu',           # weight gradient d * g (post-ReLU gradient) instead of d * a
    'bwd_bias_wave0_only',        # d_out column sums from wave 0 only
    'bwd_zero_slab_unwritten',    # a block without a window row leaves its slab row unwritten
    # finalize
    'fin_drop_remainder',         # wide path: rows after the 32-row unrolled body dropped
    'fin_scale_after_accumulate',     # (sum + out) * scale
    'fin_ignore_accumulate',      # out never added
    # head backward
    'hb_strict_indicator',        # -20 < raw < 2
    'hb_alpha_2n',                # alpha / (2 n)
    'hb_no_one_minus_pi2',        # (1 - pi^2) missing
    'hb_tanh_stride_2na',         # TANH head written at stride 2 n_act
    # Adam / Polyak
    'adam_eps_inside_bc2',        # (sqrt(v) + eps) / bc2
    'adam_polyak_before_step',    # target averaged with the parameter before the step
    'adam_skip_tail',             # the n % 4 tail elements skipped
    'adam_omb1_f32',              # 1 - beta1 formed in float32   (rounding level)
    # input rows
    'build_pi_rows_from_next',    # rows [n, 2n) filled from next_state
    'build_wa_untransposed',      # wa[i][j] read from w1[i][n_state + j]
)


def _chk(mutate):
    assert mutate is None or mutate in MUTATIONS, mutate


class NumpyLibm:
    """float32 -> float32; the kernels' libm is the device's, so outputs behind
    these are compared under a tolerance, not to the bit."""
    exp = staticmethod(lambda x: np.exp(np.asarray(x, f32)).astype(f32))
    log = staticmethod(lambda x: np.log(np.asarray(x, f32)).astype(f32))
    log1p = staticmethod(lambda x: np.log1p(np.asarray(x, f32)).astype(f32))
    tanh = staticmethod(lambda x: np.tanh(np.asarray(x, f32)).astype(f32))


def wave_sum(x):
    """wave_sum (:31-45) over the last axis (64 lanes).  row_shr 1, 2, 4, 8 leave
    in lane 15 of each row of 16 the balanced pairwise tree of its lanes
    (a4[15] = ((v15+v14)+(v13+v12) + ...) + (... + (v1+v0))); row_bcast:15 on
    rows 1 and 3 gives T1+T0 in lane 31 and T3+T2 in lane 63, row_bcast:31 on
    rows 2 and 3 adds lane 31 to lane 63: (T3+T2)+(T1+T0).  Float addition
    commutes, so this is the balanced pairwise tree over the lanes in lane
    order."""
    x = np.asarray(x, f32)
    assert x.shape[-1] == 64
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _four(p):
    return ((p[0] + p[1]) + p[2]) + p[3]


def vec_width(n, strides=(), offsets=()):
    """The dispatch rule of the C entry points (:881, :932, :965, :1011): float4
    loads when the width and every row / block / plane stride is a multiple of
    four floats and every base pointer is 16-byte aligned (``offsets``: each
    base pointer's distance in floats from a 16-byte aligned allocation), else
    scalar loads.  For the forward and the head backward the width decides the
    summation order."""
    ok = n % 4 == 0 and all(s % 4 == 0 for s in strides) and all(o % 4 == 0 for o in offsets)
    return 4 if ok else 1


def split_dot(A, w, V, mutate=None):
    """sum_j A[m][j] w[j] as k_thin_forward (:95-153) and
    k_sac_actor_head_backward (:584-632) form it, before the bias: wave wv owns
    the columns [wv pw, min((wv+1) pw, n)), pw = ceil(n / (4 * 64 V)) * 64 V
    (:98-99); lane l accumulates acc += a[c + l V + v] * w[c + l V + v] over its
    chunks c and v < V in order (:112-125, :601-620); then wave_sum (:146), then
    ((p0 + p1) + p2) + p3 (:152, :632).  (A lane past c_hi skips the add; adding
    the +0 product of the zero padding below gives the same bits, an
    accumulator that starts at +0 never being -0.)"""
    _chk(mutate)
    A, w = np.asarray(A, f32), np.asarray(w, f32)
    M, n = A.shape
    chunk = 64 * V
    pw = -(-n // (NW * chunk)) * chunk
    n_chunks = pw // chunk
    prod = np.zeros((M, NW * pw), f32)
    prod[:, :n] = A * w[None, :]
    prod = prod.reshape(M, NW, n_chunks, 64, V)
    parts = []
    for wv in range(NW):
        c_lo, c_hi = wv * pw, min((wv + 1) * pw, n)
        mine = max(0, -(-(c_hi - c_lo) // chunk))
        if mutate == 'fwd_drop_last_chunk' and mine:
            mine -= 1
        if mutate == 'fwd_skip_wave3' and wv == 3:
            mine = 0
        acc = np.zeros((M, 64), f32)
        for ci in range(mine):
            for v in range(V):
                acc = acc + prod[:, wv, ci, :, v]
        parts.append(wave_sum(acc))
    return _four(parts)


def _softplus(x, libm, mutate):
    """softplus_t (:65-68)"""
    with np.errstate(over='ignore'):
        soft = libm.log1p(libm.exp(x))
    if mutate == 'fwd_softplus_no_threshold':
        return soft
    return np.where(x > f32(20.0), x, soft).astype(f32)


def thin_forward(a, lda, a_bs, w, b, n_rows, n_in, n_out, block_diagonal, head, V, eps=None,
                 entropy_rows=0, libm=NumpyLibm, mutate=None):
    """k_thin_forward (:90-197).  ``a``: the flat buffer from the base pointer,
    addressed as the kernel does (:109, :135).  Returns a dict:
      y            [M][n_out]  pre-activations                 bit-exact
      out          PLAIN [M][n_out]: bit-exact; TANH [M][n_out] and SAC [M][n_act]
                   (pi): behind tanhf / expf, tolerance
      log_std_raw  [M][n_act]                                  bit-exact
      logp [M], entropy_part [ceil(M / 4)]                     tolerance"""
    _chk(mutate)
    a = np.asarray(a, f32).reshape(-1)
    w = np.asarray(w, f32).reshape(n_out, n_in)
    b = np.asarray(b, f32).reshape(n_out)
    if mutate == 'fwd_bd_critic0':
        a_bs = 0
    if mutate == 'fwd_bd_planes_as_side':
        a_bs = n_in
    rows = np.arange(n_rows, dtype=np.int64)[:, None] * lda + np.arange(n_in, dtype=np.int64)
    y = np.zeros((n_rows, n_out), f32)
    for o in range(n_out):
        A = a[rows + (o * a_bs if block_diagonal else 0)]
        s = split_dot(A, w[o], V, mutate)
        y[:, o] = s if mutate == 'fwd_no_bias' else s + b[o]            # :152
    res = {'y': y}
    if head == HEAD_PLAIN:
        res['out'] = y.copy()
        return res
    if head == HEAD_TANH:
        res['out'] = libm.tanh(y)                                      # :160
        return res
    na = n_out // 2
    eps = np.asarray(eps, f32).reshape(n_rows, na)
    pi = np.zeros((n_rows, na), f32)
    raw_out = np.zeros((n_rows, na), f32)
    lg = corr = None
    for i in range(na):                                                # :172-185
        mu, raw = y[:, i], y[:, na + i]
        ls = np.minimum(raw, LS_MAX) if mutate == 'fwd_clamp_one_side' else \
            np.minimum(np.maximum(raw, LS_MIN), LS_MAX)
        with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
            sd = libm.exp(ls)
            u = mu + eps[:, i] * sd
            var = sd * sd
            d = u - mu
            g = -(d * d) / (f32(2.0) * var) - libm.log(sd) - HALF_LOG_2PI
            cr = f32(2.0) * (LOG_2 - u - _softplus(f32(-2.0) * u, libm, mutate))
            lg = g if i == 0 else lg + g
            corr = cr if i == 0 else corr + cr
        pi[:, i] = libm.tanh(u)
        raw_out[:, i] = ls if mutate == 'fwd_ls_raw_clamped' else raw
    with np.errstate(invalid='ignore'):
        lp = (lg + corr if mutate == 'fwd_tanh_corr_sign' else lg - corr).astype(f32)   # :186
    n_blocks = -(-n_rows // FWD_ROWS)
    m = np.arange(n_blocks * FWD_ROWS)
    src = np.minimum(m, n_rows - 1)
    inside = (m <= entropy_rows) if mutate == 'fwd_ent_le' else (m < entropy_rows)
    if mutate == 'fwd_ent_dup_last':
        inside = src < entropy_rows
    else:
        inside = inside & (m < n_rows)                                 # :189
    e = np.where(inside, lp[src], f32(0.0)).astype(f32).reshape(n_blocks, FWD_ROWS)
    with np.errstate(invalid='ignore'):
        ent = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]                # :194
    res.update(out=pi, log_std_raw=raw_out, logp=lp, entropy_part=ent)
    return res


def _block_wave_sums(s):
    """[n][k] per-row terms -> [blocks][k]: rows past n are +0 lanes; wave_sum per
    wave, then ((r0 + r1) + r2) + r3 (:231-245, :287-301)."""
    n, k = s.shape
    nb = -(-n // LOSS_BLOCK)
    pad = np.zeros((nb * LOSS_BLOCK, k), f32)
    pad[:n] = s
    t = wave_sum(pad.reshape(nb, NW, 64, k).transpose(0, 1, 3, 2))      # [nb][NW][k]
    return (t[:, 0] + t[:, 1]) + t[:, 2] + t[:, 3]


def adam_counters(steps, consts, beta_pows, n_opt, tick_mask, lr, beta1, beta2, mutate=None):
    """:246-257 / :302-312: float64 running products, the two scalars rounded to
    float32 once.  ``beta_pows`` float64, ``steps`` / ``consts`` float32; returns
    updated copies."""
    steps, consts = np.array(steps, f32), np.array(consts, f32)
    pows = np.array(beta_pows, np.float64)
    for k in range(n_opt):
        if not (tick_mask >> k) & 1 and mutate != 'loss_tick_unticked':
            continue
        steps[k] = steps[k] + f32(1.0)
        old1, old2 = float(pows[2 * k]), float(pows[2 * k + 1])
        p1, p2 = old1 * beta1, old2 * beta2
        pows[2 * k], pows[2 * k + 1] = p1, p2
        if mutate == 'loss_consts_from_pows_before':
            p1, p2 = old1, old2
        with np.errstate(divide='ignore'):
            consts[2 * k] = f32(np.float64(lr) / np.float64(1.0 - p1))
        consts[2 * k + 1] = f32(math.sqrt(1.0 - p2))
    return steps, consts, pows


def sac_losses(q_on, q_tg, logp, reward, not_done, n, alpha, gamma, mutate=None):
    """k_sac_losses (:211-245), per-row algebra as written.  ``alpha``: the
    float32 value the kernel uses (alpha_const, or expf(log_alpha): exact for
    log_alpha = 0).  Returns dq [2n][2] and loss_part [blocks][8]: bit-exact
    given alpha."""
    _chk(mutate)
    q_on = np.asarray(q_on, f32).reshape(2 * n, 2)
    q_tg = np.asarray(q_tg, f32).reshape(n, 2)
    logp, reward, nd = (np.asarray(t, f32).reshape(-1) for t in (logp, reward, not_done))
    alpha, gamma = f32(alpha), f32(gamma)
    inv_n = f32(1.0) / f32(2 * n if mutate == 'loss_inv_2n' else n)    # :214
    tq = q_tg[:, 0] if mutate == 'loss_min_is_q1' else np.minimum(q_tg[:, 0], q_tg[:, 1])
    lp_next = logp[:n] if mutate == 'loss_logp_row_i' else logp[n:2 * n]
    gate = np.full(n, gamma, f32) if mutate == 'loss_no_not_done' else gamma * nd
    backup = reward + gate * (tq - alpha * lp_next)                    # :218-219
    q1, q2 = q_on[:n, 0], q_on[:n, 1]
    e1, e2 = q1 - backup, q2 - backup
    two = f32(1.0) if mutate == 'loss_no_factor2' else f32(2.0)
    dq = np.zeros((2 * n, 2), f32)
    dq[:n, 0] = two * e1 * inv_n                                       # :222-223
    dq[:n, 1] = two * e2 * inv_n
    p1, p2 = q_on[n:, 0], q_on[n:, 1]
    tie = -inv_n if mutate == 'loss_tie_full' else f32(-0.5) * inv_n
    zero = f32(0.0)
    dq[n:, 0] = np.where(p1 < p2, -inv_n, np.where(p1 == p2, tie, zero))   # :226-227
    dq[n:, 1] = np.where(p2 < p1, -inv_n, np.where(p1 == p2, tie, zero))
    s = np.zeros((n, 8), f32)
    s[:, 0] = alpha * logp[:n] - np.minimum(p1, p2)                    # :228-229
    s[:, 1], s[:, 2], s[:, 3], s[:, 4], s[:, 5] = e1 * e1, e2 * e2, q1, q2, backup
    if mutate == 'loss_drop_last_block' and n % LOSS_BLOCK:
        s[(n // LOSS_BLOCK) * LOSS_BLOCK:] = 0
    return {'dq': dq, 'loss_part': _block_wave_sums(s)}


def td3_losses(q_on, q_tg, reward, not_done, n, n_q, gamma, mutate=None):
    """k_td3_losses (:269-301).  dq [n][n_q], loss_part [blocks][8]: bit-exact."""
    _chk(mutate)
    q_on = np.asarray(q_on, f32).reshape(-1)
    q_tg = np.asarray(q_tg, f32).reshape(-1)
    reward, nd = np.asarray(reward, f32).reshape(-1), np.asarray(not_done, f32).reshape(-1)
    gamma = f32(gamma)
    i = np.arange(n)
    row = i
    if mutate == 'td3_nq1_row_2i' and n_q == 1:
        row = np.minimum(2 * i, n - 1)
    inv_n = f32(1.0) / f32(2 * n if mutate == 'loss_inv_2n' else n)    # :271
    tq = q_tg[n_q * row]                                               # :274-275
    if n_q == 2 and mutate != 'loss_min_is_q1':
        tq = np.minimum(tq, q_tg[2 * i + 1])
    gate = np.full(n, gamma, f32) if mutate == 'loss_no_not_done' else nd * gamma
    target = reward + gate * tq                                        # :277
    two = f32(1.0) if mutate == 'loss_no_factor2' else f32(2.0)
    dq = np.zeros((n, n_q), f32)
    s = np.zeros((n, 8), f32)
    q1 = q_on[n_q * row]
    e1 = q1 - target
    dq[:, 0] = two * e1 * inv_n                                        # :279
    s[:, 1], s[:, 3], s[:, 5] = e1 * e1, q1, target
    if n_q == 2:
        q2 = q_on[2 * i + 1]
        e2 = q2 - target
        dq[:, 1] = two * e2 * inv_n
        s[:, 2], s[:, 4] = e2 * e2, q2
    if mutate == 'loss_drop_last_block' and n % LOSS_BLOCK:
        s[(n // LOSS_BLOCK) * LOSS_BLOCK:] = 0
    return {'dq': dq, 'loss_part': _block_wave_sums(s)}


def _block_sums(x, in_window, n_rows, rpb, mutate=None, wave0_only=False):
    """Column sums of x [M][C] per block of rpb rows: wave wv adds the rows mb +
    wv, mb + wv + 4, ... inside the window sequentially (:397-438, :485-498),
    then ((l0 + l1) + l2) + l3 (:360, :458).  (A wave without a row adds its +0
    accumulator, as the kernel does; an accumulator that starts at +0 is never
    -0, so the zeros the kernel writes for a block outside the window are +0.)"""
    n_blocks = -(-n_rows // rpb)
    out = np.zeros((n_blocks,) + x.shape[1:], f32)
    lim = (rpb // NW) * NW if mutate == 'bwd_skip_block_tail' else rpb
    for y in range(n_blocks):
        lanes = []
        for wv in range(NW):
            acc = np.zeros(x.shape[1:], f32)
            for i in range(wv, lim, NW):
                m = y * rpb + i
                if m >= n_rows:
                    break
                if in_window[m] or mutate == 'bwd_sum_outside_window':
                    acc = acc + x[m]
            lanes.append(acc)
        out[y] = lanes[0] if wave0_only else _four(lanes)
    return out


def _window(n_rows, r0, r1):
    m = np.arange(n_rows)
    return (m >= r0) & (m < r1)


def _blocks_with_rows(n_rows, rpb, win):
    n_blocks = -(-n_rows // rpb)
    return np.array([win[y * rpb:(y + 1) * rpb].any() for y in range(n_blocks)])


def thin_backward(d_out, ld_dout, a, lda, a_bs, w, n_rows, n_in, n_out, block_diagonal, r0, r1,
                  rpb, dz, ld_dz, dz_bs, part, ld_part, mutate=None):
    """k_thin_backward (:364-461).  d_out, a, dz, part: flat buffers from their
    base pointers, dz and part as they are before the call; the returned copies
    hold what the kernel leaves, untouched entries included.  Every column is
    independent, so float4 against scalar loads does not change a bit here.
    All outputs bit-exact."""
    _chk(mutate)
    d_buf = np.asarray(d_out, f32).reshape(-1)
    a = np.asarray(a, f32).reshape(-1)
    w = np.asarray(w, f32).reshape(n_out, n_in)
    dz = np.array(dz, f32).reshape(-1)
    part = np.array(part, f32).reshape(-1)
    n_cols = n_out * n_in if block_diagonal else n_in
    d = d_buf[np.arange(n_rows)[:, None] * ld_dout + np.arange(n_out)]           # :402
    col = np.arange(n_cols)
    ob = col // n_in if block_diagonal else np.zeros(n_cols, np.int64)           # :374
    a_off = ob * a_bs + (col - ob * n_in) if block_diagonal else col             # :377-378
    dz_off = ob * dz_bs + (col - ob * n_in) if block_diagonal else col
    m_idx = np.arange(n_rows, dtype=np.int64)[:, None]
    av = a[m_idx * lda + a_off]
    if block_diagonal:
        dsel = d[:, ob]                                                          # :405-410
        g = dsel * w.reshape(-1)[col][None, :]
    else:
        g = d[:, 0:1] * w[0][None, :]                                            # :414-417
        for o in range(1, n_out):
            g = g + d[:, o:o + 1] * w[o][None, :]
    keep = av >= 0 if mutate == 'bwd_relu_ge' else av > 0                        # :421
    g = np.where(keep, g, f32(0.0)).astype(f32)
    win = _window(n_rows, r0, r1)
    stored = win if mutate == 'bwd_dz_window_only' else np.ones(n_rows, bool)
    idx = (m_idx * ld_dz + dz_off)[stored]
    dz[idx] = g[stored]                                                          # :422
    n_w = n_out * n_in
    if block_diagonal:
        dw = (d[:, ob] * g) if mutate == 'bwd_dw_post_relu' else dsel * av       # :428
    else:
        src = g if mutate == 'bwd_dw_post_relu' else av
        dw = np.concatenate([d[:, o:o + 1] * src for o in range(n_out)], axis=1)  # :433
    sums = np.concatenate([
        _block_sums(g, win, n_rows, rpb, mutate),
        _block_sums(dw, win, n_rows, rpb, mutate),
        _block_sums(d, win, n_rows, rpb, mutate, wave0_only=mutate == 'bwd_bias_wave0_only'),
    ], axis=1)                                                                   # :439-459
    written = np.ones(len(sums), bool)
    if mutate == 'bwd_zero_slab_unwritten':
        written = _blocks_with_rows(n_rows, rpb, win)
    for y in np.nonzero(written)[0]:
        part[y * ld_part:y * ld_part + n_cols + n_w + n_out] = sums[y]
    return {'dz': dz, 'part': part}


def relu_backward_bias(dz, ld_dz, dz_ps, a, lda, a_ps, n_planes, n_rows, n_cols, r0, r1, rpb,
                       part, ld_part, mutate=None):
    """k_relu_backward_bias (:470-503); buffers as in thin_backward.  Bit-exact."""
    _chk(mutate)
    dz = np.array(dz, f32).reshape(-1)
    a = np.asarray(a, f32).reshape(-1)
    part = np.array(part, f32).reshape(-1)
    win = _window(n_rows, r0, r1)
    m_idx = np.arange(n_rows, dtype=np.int64)[:, None]
    col = np.arange(n_cols)
    written = np.ones(-(-n_rows // rpb), bool)
    if mutate == 'bwd_zero_slab_unwritten':
        written = _blocks_with_rows(n_rows, rpb, win)
    for z in range(n_planes):
        av = a[z * a_ps + m_idx * lda + col]
        idx = z * dz_ps + m_idx * ld_dz + col
        keep = av >= 0 if mutate == 'bwd_relu_ge' else av > 0                    # :492
        g = np.where(keep, dz[idx], f32(0.0)).astype(f32)
        stored = win if mutate == 'bwd_dz_window_only' else np.ones(n_rows, bool)
        dz[idx[stored]] = g[stored]                                              # :497
        sums = _block_sums(g, win, n_rows, rpb, mutate)
        for y in np.nonzero(written)[0]:
            part[y * ld_part + z * n_cols:y * ld_part + (z + 1) * n_cols] = sums[y]   # :500
    return {'dz': dz, 'part': part}


def colsum_finalize(part, ld, n_part, n, out, scale, accumulate, mutate=None):
    """One segment of k_colsum_finalize (:514-563).  ``part``: flat from the
    segment's pointer; ``out`` [n] before the call.  Bit-exact."""
    _chk(mutate)
    part = np.asarray(part, f32).reshape(-1)
    x = part[np.arange(n_part)[:, None] * ld + np.arange(n)]
    out, scale = np.array(out, f32).reshape(-1)[:n], f32(scale)
    if n > 8:                                                                    # :520-544
        lanes = []
        for wv in range(NW):
            acc = np.zeros(n, f32)
            r = wv
            while r + 7 * NW < n_part:            # eight rows, added in row order (:527-533)
                for k in range(8):
                    acc = acc + x[r + k * NW]
                r += 8 * NW
            if mutate != 'fin_drop_remainder':
                while r < n_part:                                                # :534
                    acc = acc + x[r]
                    r += NW
            lanes.append(acc)
        t = _four(lanes)
    else:                                                                        # :549-562
        groups = []
        for g in range(32):
            acc = np.zeros(n, f32)
            for r in range(g, n_part, 32):
                acc = acc + x[r]
            groups.append(acc)
        t = groups[0]
        for k in range(1, 32):
            t = t + groups[k]
    if mutate == 'fin_scale_after_accumulate' and accumulate:
        return (t + out) * scale
    t = t * scale
    if accumulate and mutate != 'fin_ignore_accumulate':
        t = t + out
    return t


def actor_head_backward(dh, ld_dh, h, ld_h, wa, n_rows, n_cols, n_act, head, V, pi, ld_pi,
                        eps, log_std_raw, alpha, d_head, libm=NumpyLibm, mutate=None):
    """k_sac_actor_head_backward (:580-648).  dh, h, pi, d_head: flat buffers from
    their base pointers (d_head as before the call).  Returns
      dpi     [M][n_act]   the split dot product                    bit-exact
      d_head  flat; TANH head and the mu half of the SAC head: bit-exact given
              alpha; the log-std half is behind expf: tolerance."""
    _chk(mutate)
    dh, h, pi = (np.asarray(t, f32).reshape(-1) for t in (dh, h, pi))
    wa = np.asarray(wa, f32).reshape(n_act, n_cols)
    d_head = np.array(d_head, f32).reshape(-1)
    m_idx = np.arange(n_rows, dtype=np.int64)[:, None]
    col = np.arange(n_cols)
    g = np.where(h[m_idx * ld_h + col] > 0, dh[m_idx * ld_dh + col], f32(0.0)).astype(f32)  # :609
    dpi = np.stack([split_dot(g, wa[i], V, mutate) for i in range(n_act)], axis=1)
    t = pi[m_idx * ld_pi + np.arange(n_act)]
    one_m = np.ones_like(t) if mutate == 'hb_no_one_minus_pi2' else f32(1.0) - t * t
    rows = np.arange(n_rows)[:, None]
    if head == HEAD_TANH:                                                        # :633-637
        stride = 2 * n_act if mutate == 'hb_tanh_stride_2na' else n_act
        keep = rows * stride + np.arange(n_act) < len(d_head)
        d_head[(rows * stride + np.arange(n_act))[keep]] = (dpi * one_m)[keep]
        return {'dpi': dpi, 'd_head': d_head}
    eps = np.asarray(eps, f32).reshape(n_rows, n_act)
    raw = np.asarray(log_std_raw, f32).reshape(n_rows, n_act)
    alpha = f32(alpha)
    an = alpha / f32(2 * n_rows if mutate == 'hb_alpha_2n' else n_rows)         # :640
    du = an * (f32(2.0) * t) + dpi * one_m                                       # :642
    inside = (raw > LS_MIN) & (raw < LS_MAX) if mutate == 'hb_strict_indicator' else \
        (raw >= LS_MIN) & (raw <= LS_MAX)                                        # :644
    sd = libm.exp(np.minimum(np.maximum(raw, LS_MIN), LS_MAX))
    ls_half = np.where(inside, du * (eps * sd) - an, f32(0.0)).astype(f32)       # :647
    d_head[rows * 2 * n_act + np.arange(n_act)] = du
    d_head[rows * 2 * n_act + n_act + np.arange(n_act)] = ls_half
    return {'dpi': dpi, 'd_head': d_head}


def _adam_scalars(beta1, beta2, eps, tau, mutate=None):
    """:1035-1036: 1 - beta1, 1 - beta2, 1 - tau in float64, rounded once."""
    om_b1 = f32(1.0) - f32(beta1) if mutate == 'adam_omb1_f32' else f32(1.0 - beta1)
    om_tau = f32(1.0 - tau)       # (in float32 the same bits at tau = 0.005: no mutant to plant)
    return om_b1, f32(beta2), f32(1.0 - beta2), f32(eps), f32(tau), om_tau


def adam_polyak(p, g, m, v, target, consts, beta1, beta2, eps, tau, mutate=None):
    """adam_one (:662-669) over an arena; the float4 body and the scalar tail
    (:674-690) are the same arithmetic per element.  Returns p, m, v, target
    (None without one).  Bit-exact."""
    _chk(mutate)
    p, g, m, v = (np.array(t, f32).reshape(-1) for t in (p, g, m, v))
    om_b1, b2, om_b2, eps_f, tau_f, om_tau = _adam_scalars(beta1, beta2, eps, tau, mutate)
    step_size, bc2s = f32(consts[0]), f32(consts[1])
    m1 = m + (g - m) * om_b1                                                     # :664
    v1 = v * b2 + (om_b2 * g) * g                                                # :665
    with np.errstate(divide='ignore', invalid='ignore'):
        if mutate == 'adam_eps_inside_bc2':
            denom = (np.sqrt(v1) + eps_f) / bc2s
        else:
            denom = np.sqrt(v1) / bc2s + eps_f                                   # :666
        p1 = p + (-step_size) * (m1 / denom)                                     # :667
    t1 = None
    if target is not None:
        t0 = np.array(target, f32).reshape(-1)
        src = p if mutate == 'adam_polyak_before_step' else p1
        t1 = t0 * om_tau + src * tau_f                                           # :668
    if mutate == 'adam_skip_tail':
        body = (len(p) // 4) * 4
        p1[body:], m1[body:], v1[body:] = p[body:], m[body:], v[body:]
        if t1 is not None:
            t1[body:] = t0[body:]
    return {'p': p1, 'm': m1, 'v': v1, 'target': t1}


def polyak(target, p, tau, mutate=None):
    """k_polyak (:315-328): target (1 - tau) + p tau.  Bit-exact."""
    _chk(mutate)
    t0, p = np.array(target, f32).reshape(-1), np.asarray(p, f32).reshape(-1)
    _, _, _, _, tau_f, om_tau = _adam_scalars(0.9, 0.999, 1e-8, tau, mutate)
    t1 = t0 * om_tau + p * tau_f
    if mutate == 'adam_skip_tail':
        body = (len(p) // 4) * 4
        t1[body:] = t0[body:]
    return {'target': t1}


def alpha_step(log_alpha, m, v, mean_logp, target_entropy, consts, beta1, beta2, eps,
               libm=NumpyLibm, mutate=None):
    """k_sac_alpha_step (:700-710), scalars.  log_alpha, m, v: bit-exact; grad is
    behind expf(log_alpha): tolerance (exact for log_alpha = 0)."""
    _chk(mutate)
    ml, te = f32(mean_logp), f32(target_entropy)
    g = -(ml + te)                                                               # :703
    alpha_before = libm.exp(f32(log_alpha)).reshape(())[()]
    r = adam_polyak([log_alpha], [g], [m], [v], None, consts, beta1, beta2, eps, 0.0, mutate)
    return {'log_alpha': r['p'], 'm': r['m'], 'v': r['v'],
            'grad': np.array([g + alpha_before * ml], f32)}                      # :709


def build_learner_inputs(state, ld_s, action, ld_a, next_state, ld_s2, n, n_state, n_act, xs, ld,
                         w1=None, ld_w1=0, n_w1_rows=0, wa=None, mutate=None):
    """k_build_learner_inputs (:723-745): copies only.  Flat buffers; xs and wa
    as before the call."""
    _chk(mutate)
    s, ac, s2 = (np.asarray(t, f32).reshape(-1) for t in (state, action, next_state))
    xs = np.array(xs, f32).reshape(-1)
    m = np.arange(n, dtype=np.int64)[:, None]
    c = np.arange(n_state)
    xs[m * ld + c] = s[m * ld_s + c]                                             # :740
    xs[(n + m) * ld + c] = (s2[m * ld_s2 + c] if mutate == 'build_pi_rows_from_next'
                            else s[m * ld_s + c])                                # :741
    xs[(2 * n + m) * ld + c] = s2[m * ld_s2 + c]                                 # :742
    xs[m * ld + n_state + np.arange(n_act)] = ac[m * ld_a + np.arange(n_act)]    # :744
    res = {'xs': xs}
    if w1 is not None:
        w1 = np.asarray(w1, f32).reshape(-1)
        wa = np.array(wa, f32).reshape(-1)
        j = np.arange(n_w1_rows, dtype=np.int64)
        for i in range(n_act):                                                   # :728-730
            src = w1[j * ld_w1 + n_state + i]
            if mutate == 'build_wa_untransposed':
                src = w1[(i * ld_w1 + n_state + j) % len(w1)]
            wa[i * n_w1_rows + j] = src
        res['wa'] = wa
    return res
