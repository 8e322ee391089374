"""Every learner kernel (csrc/ttl_learner.hip) against its restatement in the
kernel's own order (tests/ref_learner_ordered.py: equal bit for bit, padding
and slab fill included) and against the float64 definition with a per-element
bound (tests/ref_learner_ops.py), at the shapes where each structure of a
kernel is exercised.

CPU part: on every GPU input the restatement is inside the float64 bound on
every element; every planted mutation of the restatement is caught by a named
GPU input -- it changes bits there, leaves the float64 bound (rounding-level
mutants excepted) and fails the very assertion the GPU tests apply to the
kernels.  GPU part (-m gpu): the kernels on those inputs, each launched twice
(same bits), and the refusals of the entry points.

Outputs behind a libm call (expf, logf, log1pf, tanhf) cannot be restated to
the bit.  They are held on every element to 4 x the spread of the definition's
float32 twins + one ulp (ref_learner_ops.twin_tolerance), the definition taken
at the float32 sums the kernel itself forms (which are pinned to the bit: the
pre-activations ``y`` through the PLAIN head of the same instantiation, ``dpi``
through the TANH head at pi = 0), so that the tolerance measures the libm step alone.
Which output is which: ``_reference`` below, third tuple entry."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import ref_learner_ops as D
import ref_learner_ordered as R

DEV = 'cuda:0'
f32 = np.float32
SENT = f32(1234.5)                       # pre-fill of every output
PLAIN, SAC, TANH = R.HEAD_PLAIN, R.HEAD_SAC, R.HEAD_TANH
B1, B2, AEPS, LR = 0.9, 0.999, 1e-8, 3e-4

# mutants that differ from the kernel by a few float32 roundings only: not
# required to leave the float64 bound, the bit equality is what catches them
ROUNDING_LEVEL = ('adam_omb1_f32',)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _randn(g, *shape):
    return g.standard_normal(shape).astype(f32)


def _sparse(g, *shape):
    """Activations with exact zeros, negatives and positives."""
    x = _randn(g, *shape)
    x[g.random(shape) < 0.3] = 0
    return x


# --------------------------------------------------------------------------
# the GPU inputs: name -> (kind, parameters)
# --------------------------------------------------------------------------
CASES = {}


def _case(kind, tag, **p):
    name = f'{kind}-{tag}'
    assert name not in CASES, name
    CASES[name] = (kind, p)


def _fwd(tag, M, n_in, n_out, head=PLAIN, bd=None, **p):
    _case('fwd', tag, M=M, n_in=n_in, n_out=n_out, head=head, bd=bd, **p)


# float4 widths x rows x every dense instantiation
for _k, (_n_in, _M, _n_out, _head) in enumerate([
        (4, 1, 1, PLAIN), (256, 4, 2, SAC), (260, 5, 3, TANH), (1024, 7, 4, SAC),
        (1028, 261, 6, SAC), (2052, 5, 8, SAC), (256, 7, 8, PLAIN), (1024, 4, 4, PLAIN)]):
    _fwd(f'v4-{_n_in}x{_M}-o{_n_out}h{_head}', _M, _n_in, _n_out, _head,
         ent_rows=_M // 2 + 1 if _head == SAC else 0)
# scalar widths
for _n_in, _M, _n_out, _head in [(1, 4, 1, PLAIN), (63, 5, 2, SAC), (65, 7, 3, PLAIN),
                                 (257, 1, 6, SAC), (2050, 5, 4, TANH), (2050, 261, 2, PLAIN)]:
    _fwd(f'v1-{_n_in}x{_M}-o{_n_out}h{_head}', _M, _n_in, _n_out, _head,
         ent_rows=_M if _head == SAC else 0)
# the scalar path forced at a float4 width: row stride, base pointer, weights
_fwd('v1-forced-lda', 5, 256, 6, SAC, lda=257, ent_rows=3)
_fwd('v1-forced-base', 5, 256, 2, PLAIN, lda=260, a_off=1)
_fwd('v1-forced-w', 5, 256, 3, PLAIN, w_off=1)
_fwd('v4-wide-lda', 7, 256, 6, PLAIN, lda=264)
# block diagonal, 1 and 2 networks, side by side and in planes, both widths
for _n_out in (1, 2):
    for _lay in ('side', 'planes'):
        _fwd(f'bd{_n_out}-{_lay}-v4', 7, 260, _n_out, PLAIN, bd=_lay, pad=4)
        _fwd(f'bd{_n_out}-{_lay}-v1', 5, 65, _n_out, PLAIN, bd=_lay, pad=3)
_fwd('bd2-planes-tanh', 9, 512, 2, TANH, bd='planes')
# the SAC head: n_act 1..4, entropy window, NULL partials, clamp edges, a wide output row
for _na in (1, 2, 3, 4):
    _fwd(f'sac-edges-a{_na}', 11, 68, 2 * _na, SAC, edges=True, ent_rows=(0, 11, 6, 9)[_na - 1],
         ld_out=_na + 5, out_off=2)
_fwd('sac-ent-null', 7, 64, 6, SAC, ent_rows=7, ent_null=True)
_fwd('sac-ent-partial-block', 7, 130, 4, SAC, ent_rows=7)
_fwd('sac-ent-inside-block', 261, 36, 6, SAC, ent_rows=6)


def _bwd(tag, M, n_in, n_out, rpb, win, bd=None, **p):
    _case('bwd', tag, M=M, n_in=n_in, n_out=n_out, rpb=rpb, win=win, bd=bd, **p)


# columns x rows_per_block (a partial last block everywhere) x windows x n_out
for _n_in, _M, _rpb, _win, _n_out in [
        (252, 5, 1, 'whole', 1), (256, 10, 3, 'empty', 3), (260, 11, 4, 'third', 6),
        (63, 23, 5, 'edge', 8), (64, 70, 32, 'inside', 2), (65, 150, 64, 'third', 4),
        (520, 23, 5, 'third', 6), (130, 11, 4, 'whole', 1), (64, 9, 4, 'empty', 1)]:
    _bwd(f'{_n_in}x{_M}-rpb{_rpb}-{_win}-o{_n_out}', _M, _n_in, _n_out, _rpb, _win)
_bwd('forced-scalar-ld', 11, 256, 6, 4, 'third', lda=257)
_bwd('forced-scalar-base', 11, 256, 3, 3, 'third', lda=260, a_off=1)
_bwd('strided', 23, 68, 6, 5, 'third', lda=72, ld_dz=76, ld_dout=9, ld_part_pad=5)
_bwd('bd2-side-v4', 23, 68, 2, 5, 'third', bd='side', pad=4)
_bwd('bd2-side-v1', 11, 65, 2, 4, 'edge', bd='side', pad=3)
_bwd('bd2-planes-v4', 23, 260, 2, 5, 'third', bd='planes')
_bwd('bd2-planes-v1', 10, 63, 2, 3, 'whole', bd='planes')
_bwd('bd1-side', 10, 64, 1, 3, 'third', bd='side')
_bwd('bd1-planes-empty', 9, 65, 1, 4, 'empty', bd='planes')

for _tag, _p in {
        'p1-256x11': dict(planes=1, M=11, n_cols=256, rpb=4, win='third'),
        'p2-260x23': dict(planes=2, M=23, n_cols=260, rpb=5, win='third'),
        'p2-65x10-scalar': dict(planes=2, M=10, n_cols=65, rpb=3, win='edge'),
        'p1-63x5-rpb1': dict(planes=1, M=5, n_cols=63, rpb=1, win='whole'),
        'p1-empty-window': dict(planes=1, M=9, n_cols=64, rpb=4, win='empty'),
        'p2-wide-sliced-slab': dict(planes=2, M=70, n_cols=252, rpb=32, win='inside',
                                    part_off=8, ld_part_pad=20, ld=256),
        'p1-520x150-rpb64': dict(planes=1, M=150, n_cols=520, rpb=64, win='third'),
        'p1-forced-scalar': dict(planes=1, M=11, n_cols=64, rpb=4, win='third', ld=65)}.items():
    _case('relu', _tag, **_p)

# finalize: (n_part, n, ld - n, column offset, scale, accumulate)
for _k, _seg in enumerate([(1, 1, 0, 0, 1.0, 0), (3, 8, 2, 1, 0.25, 1), (4, 9, 0, 0, 1.0, 1),
                           (5, 63, 7, 3, 0.5, 0), (31, 64, 0, 0, 1.0 / 31, 0),
                           (32, 65, 1, 0, 1.0, 1), (33, 130, 0, 2, 1.0 / 77, 0),
                           (128, 9, 3, 0, 1.0, 0), (129, 8, 0, 0, 1.0 / 129, 1),
                           (300, 64, 5, 5, 1.0, 1), (300, 1, 0, 0, 1.0 / 300, 0),
                           (33, 3, 4, 2, 1.0, 0)]):
    _case('fin', f'{_seg[0]}x{_seg[1]}-acc{_seg[5]}', segs=[_seg])
_case('fin', 'twelve-mixed', segs=[(5, 63, 7, 3, 0.5, 0), (33, 8, 0, 0, 1.0, 1),
                                   (4, 130, 2, 0, 0.125, 1), (1, 1, 0, 0, 2.0, 0),
                                   (129, 9, 1, 1, 1.0, 0), (32, 2, 0, 0, 1.0 / 32, 1),
                                   (31, 65, 0, 0, 1.0, 0), (3, 7, 3, 2, 1.0, 1),
                                   (128, 64, 0, 0, 1.0 / 128, 0), (40, 5, 0, 0, 1.0, 0),
                                   (7, 200, 8, 0, 1.0, 1), (64, 6, 2, 0, 0.5, 0)])

for _n, _la, _null, _n_opt, _mask, _calls in [
        (1, None, False, 0, 0, 1), (2, 0.0, False, 3, 0b101, 1), (255, None, True, 8, 0b10010010, 1),
        (256, 0.0, False, 3, 0b010, 3), (257, None, False, 8, 0b11111111, 3),
        (513, 0.0, False, 3, 0b111, 1)]:
    _case('sac', f'n{_n}', n=_n, log_alpha=_la, loss_null=_null, n_opt=_n_opt, mask=_mask,
          calls=_calls)
for _n, _nq, _null, _n_opt, _mask, _calls in [
        (1, 2, False, 3, 0b001, 1), (2, 1, False, 0, 0, 1), (255, 2, False, 8, 0b01000001, 3),
        (256, 1, True, 3, 0b110, 1), (257, 1, False, 3, 0b111, 3), (513, 2, False, 8, 0b1, 1),
        (513, 1, False, 0, 0, 1)]:
    _case('td3', f'n{_n}-q{_nq}', n=_n, n_q=_nq, loss_null=_null, n_opt=_n_opt, mask=_mask,
          calls=_calls)


def _hb(tag, M, n_cols, n_act, head, **p):
    _case('hb', tag, M=M, n_cols=n_cols, n_act=n_act, head=head, **p)


for _n_cols, _M, _na, _head, _la in [
        (4, 1, 1, SAC, None), (256, 4, 2, SAC, 0.0), (260, 5, 3, TANH, None),
        (1024, 7, 4, SAC, None), (1028, 261, 3, SAC, 0.0), (2052, 5, 1, TANH, None),
        (1, 4, 2, TANH, None), (63, 5, 3, SAC, 0.0), (65, 7, 4, TANH, None),
        (257, 1, 2, SAC, None), (2050, 5, 3, SAC, None)]:
    _hb(f'{_n_cols}x{_M}-a{_na}h{_head}-la{_la}', _M, _n_cols, _na, _head, log_alpha=_la)
_hb('forced-scalar-ld', 5, 256, 3, SAC, ld_dh=257)
_hb('forced-scalar-base', 7, 256, 2, TANH, ld_h=260, h_off=1)
_hb('wide-pi', 9, 68, 3, SAC, ld_pi=9, pi_off=4, ld_dh=72)
_hb('wide-pi-tanh', 9, 68, 3, TANH, ld_pi=9, pi_off=4)

ADAM_N = (1, 3, 4, 5, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1028, 3 * 1024 + 7)
for _k, _n in enumerate(ADAM_N):
    _case('adam', f'n{_n}', n=_n, target=_k % 3 != 1, tau=0.0 if _k % 4 == 2 else 0.005)
    _case('polyak', f'n{_n}', n=_n, tau=0.0 if _k % 4 == 1 else 0.005)
for _k, _st in enumerate([(0.0, 0.3, 2.0, -2.2, -3.0), (-1.6, 0.0, 0.0, 0.7, -3.0),
                          (0.4, -0.01, 1e-4, -3.0, -1.0)]):
    _case('alpha', f'state{_k}', state=_st)
for _n, _S, _A, _w1 in [(5, 1, 1, 1), (9, 63, 2, 255), (4, 64, 3, 256), (7, 65, 4, 257),
                        (13, 327, 3, None)]:
    _case('build', f'{_n}x{_S}a{_A}-w{_w1}', n=_n, S=_S, A=_A, n_w1=_w1)
_case('build', 'strided', n=6, S=65, A=3, n_w1=70, ld_s=70, ld_a=5, ld_s2=67, ld=75, ld_w1=71)


def _window(win, M, rpb):
    return {'whole': (0, M), 'empty': (0, 0), 'third': (M // 3, M - 2),
            'edge': (rpb, rpb + 1), 'inside': (rpb + 1, 2 * rpb - 1)}[win]


# --------------------------------------------------------------------------
# inputs of a case (NumPy; the same buffers go to the restatement, the float64
# definition and the kernel)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    kind, p = CASES[name]
    g = _rng(name)
    I = dict(p)
    if kind == 'fwd':
        M, n_in, n_out, bd = p['M'], p['n_in'], p['n_out'], p['bd']
        pad = p.get('pad', 0)
        if bd == 'side':
            lda, a_bs, size = n_out * n_in + pad, n_in, M * (n_out * n_in + pad)
        elif bd == 'planes':
            lda, a_bs, size = n_in + pad, M * (n_in + pad), n_out * M * (n_in + pad)
        else:
            lda = p.get('lda', n_in)
            a_bs, size = 0, M * lda
        a_off, w_off = p.get('a_off', 0), p.get('w_off', 0)
        a = _randn(g, a_off + size)
        w = _randn(g, w_off + n_out * n_in) / f32(math.sqrt(n_in))
        b = _randn(g, n_out)
        na = n_out // 2
        if p['head'] == SAC:
            wv = w[w_off:].reshape(n_out, n_in)
            wv[na:] *= 4                                       # some log_std beyond the clamp
            b[na:] += np.array([-1.0, 3.0, -25.0, 0.0], f32)[:na]
            if p.get('edges'):
                # rows 0..5: one non-zero input, so that log_std_raw is exactly
                # -25, -20, 0.5, 2, 3 and mu + eps std < -44 (softplus(-2u) past
                # its threshold and past the overflow of expf) in row 5
                wv[na:, 0], wv[:na, 0] = 1.0, 2.5
                b[na:], b[:na] = 0.0, 0.25
                av = a[a_off:].reshape(M, lda)
                av[:6] = 0
                av[:6, 0] = [-25.0, -20.0, 0.5, 2.0, 3.0, -20.0]
                wv[:na, 0] = 2.5
        I.update(a=a, w=w, b=b, lda=lda, a_bs=a_bs, a_off=a_off, w_off=w_off,
                 eps=_randn(g, M, max(na, 1)), ld_out=p.get('ld_out', n_out),
                 out_off=p.get('out_off', 0), ent_rows=p.get('ent_rows', 0),
                 V=R.vec_width(n_in, (lda,) + ((a_bs,) if bd else ()), (a_off, w_off)))
    elif kind == 'bwd':
        M, n_in, n_out, bd = p['M'], p['n_in'], p['n_out'], p['bd']
        pad = p.get('pad', 0)
        if bd == 'side':
            lda = ld_dz = n_out * n_in + pad
            a_bs = dz_bs = n_in
            size = M * lda
        elif bd == 'planes':
            lda = ld_dz = n_in
            a_bs = dz_bs = M * n_in
            size = n_out * M * n_in
        else:
            lda, ld_dz = p.get('lda', n_in), p.get('ld_dz', n_in)
            a_bs = dz_bs = 0
            size = M * max(lda, ld_dz)
        n_cols = n_out * n_in if bd else n_in
        ld_part = n_cols + n_out * n_in + n_out + p.get('ld_part_pad', 0)
        ld_dout = p.get('ld_dout', n_out)
        a_off = p.get('a_off', 0)
        r0, r1 = _window(p['win'], M, p['rpb'])
        I.update(a=_sparse(g, a_off + size), d_out=_randn(g, M * ld_dout), w=_randn(g, n_out * n_in),
                 lda=lda, ld_dz=ld_dz, a_bs=a_bs, dz_bs=dz_bs, ld_part=ld_part, ld_dout=ld_dout,
                 a_off=a_off, r0=r0, r1=r1, dz=np.full(size, SENT),
                 part=np.full(-(-M // p['rpb']) * ld_part, SENT))
    elif kind == 'relu':
        M, n_cols, planes = p['M'], p['n_cols'], p['planes']
        ld = p.get('ld', n_cols)
        ps = M * ld
        ld_part = planes * n_cols + p.get('ld_part_pad', 0)
        r0, r1 = _window(p['win'], M, p['rpb'])
        I.update(a=_sparse(g, planes * ps), dz=_randn(g, planes * ps), ld=ld, ps=ps, r0=r0, r1=r1,
                 ld_part=ld_part, part_off=p.get('part_off', 0),
                 part=np.full(p.get('part_off', 0) + -(-M // p['rpb']) * ld_part, SENT))
        if ld > n_cols:                       # the gap between rows is not the kernel's to touch
            I['dz'].reshape(planes * M, ld)[:, n_cols:] = SENT
    elif kind == 'fin':
        I['part'] = [_randn(g, n_part * (n + dld + off)) for n_part, n, dld, off, _, _ in p['segs']]
        I['out'] = [_randn(g, n + 3) for _, n, *_ in p['segs']]
    elif kind in ('sac', 'td3'):
        n, n_q = p['n'], p.get('n_q', 2)
        rows = 2 * n if kind == 'sac' else n
        q_on, q_tg = _randn(g, rows, n_q), _randn(g, n, n_q)
        if n_q == 2:
            q_on[rows - 1, 1] = q_on[rows - 1, 0]              # ties of the two critics
            q_tg[0, 1] = q_tg[0, 0]
            if n > 2:
                q_on[n // 2, 1] = q_on[n // 2, 0]
        nd = (g.random(n) > 0.2).astype(f32)                   # exactly 0 and 1
        nd[0], nd[-1] = 1.0, 0.0 if n > 1 else 1.0
        n_opt = p['n_opt']
        steps = np.array([4.0, 9.0, 0.0, 1.0, 0.0, 2.0, 0.0, 30.0], f32)[:n_opt]
        pows = np.array([[B1 ** int(s), B2 ** int(s)] for s in steps], np.float64).reshape(-1)
        I.update(q_on=q_on, q_tg=q_tg, logp=_randn(g, 2 * n) * f32(3), reward=g.random(n).astype(f32),
                 not_done=nd, steps=steps, pows=pows, consts=np.full(2 * n_opt, SENT), gamma=0.99,
                 alpha_const=0.2, n_q=n_q)
    elif kind == 'hb':
        M, n_cols, na = p['M'], p['n_cols'], p['n_act']
        ld_dh, ld_h = p.get('ld_dh', n_cols), p.get('ld_h', n_cols)
        ld_pi, pi_off, h_off = p.get('ld_pi', na), p.get('pi_off', 0), p.get('h_off', 0)
        raw = _randn(g, M, na) * f32(8)
        raw.reshape(-1)[0] = -20.0                             # exactly at both clamp ends
        raw.reshape(-1)[-1] = 2.0 if raw.size > 1 else -20.0
        I.update(dh=_randn(g, M * ld_dh), h=_sparse(g, h_off + M * ld_h),
                 wa=_randn(g, na * n_cols) / f32(math.sqrt(n_cols)), ld_dh=ld_dh, ld_h=ld_h,
                 ld_pi=ld_pi, pi_off=pi_off, h_off=h_off,
                 pi=np.tanh(_randn(g, pi_off + M * ld_pi)).astype(f32), eps=_randn(g, M, na),
                 raw=raw, alpha_const=0.2, log_alpha=p.get('log_alpha'),
                 d_head=np.full(M * 2 * na + 4, SENT),
                 V=R.vec_width(n_cols, (ld_dh, ld_h), (h_off,)))
    elif kind in ('adam', 'polyak'):
        n = p['n']
        v = g.random(n).astype(f32)
        gr = _randn(g, n)
        v[::5], gr[::5] = 0, 0                                 # eps alone decides the step
        I.update(p=_randn(g, n), g=gr, m=_randn(g, n) * f32(0.1) + f32(0.01), v=v, t=_randn(g, n),
                 consts=np.array([LR / (1 - B1 ** 3), math.sqrt(1 - B2 ** 3)], f32))
    elif kind == 'alpha':
        I.update(consts=np.array([LR / (1 - B1 ** 2), math.sqrt(1 - B2 ** 2)], f32))
    elif kind == 'build':
        n, S, A, n_w1 = p['n'], p['S'], p['A'], p['n_w1']
        ld_s, ld_a, ld_s2 = p.get('ld_s', S), p.get('ld_a', A), p.get('ld_s2', S)
        ld, ld_w1 = p.get('ld', S + A + 2), p.get('ld_w1', S + A)
        I.update(state=_randn(g, n * ld_s), action=_randn(g, n * ld_a), next=_randn(g, n * ld_s2),
                 ld_s=ld_s, ld_a=ld_a, ld_s2=ld_s2, ld=ld, ld_w1=ld_w1,
                 xs=np.full(3 * n * ld, SENT), w1=None if n_w1 is None else _randn(g, n_w1 * ld_w1),
                 wa=None if n_w1 is None else np.full(A * n_w1 + 2, SENT))
    return I


def _alpha(I):
    """The float32 temperature the kernel works with: alpha_const, or
    expf(log_alpha) -- the cases give log_alpha = 0, where it is exactly 1."""
    if I.get('log_alpha') is None:
        return f32(I['alpha_const'])
    assert I['log_alpha'] == 0.0
    return f32(1.0)


# --------------------------------------------------------------------------
# the restatement on a case's inputs: name -> array as the kernel leaves it
# --------------------------------------------------------------------------
def _ordered(name, mutate=None):
    kind, _ = CASES[name]
    I = _inputs(name)
    if kind == 'fwd':
        r = R.thin_forward(I['a'][I['a_off']:], I['lda'], I['a_bs'], I['w'][I['w_off']:], I['b'],
                           I['M'], I['n_in'], I['n_out'], bool(I['bd']), I['head'], I['V'],
                           eps=I['eps'], entropy_rows=I['ent_rows'], mutate=mutate)
        n_w = I['n_out'] // 2 if I['head'] == SAC else I['n_out']
        out = np.full(I['out_off'] + I['M'] * I['ld_out'], SENT)
        out[I['out_off'] + np.arange(I['M'])[:, None] * I['ld_out'] + np.arange(n_w)] = r['out']
        res = {'y': r['y'], 'out': out}
        if I['head'] == SAC:
            res.update(logp=r['logp'], log_std_raw=r['log_std_raw'])
            res['entropy_part'] = np.full_like(r['entropy_part'], SENT) if I.get('ent_null') \
                else r['entropy_part']
        return res
    if kind == 'bwd':
        return R.thin_backward(I['d_out'], I['ld_dout'], I['a'][I['a_off']:], I['lda'], I['a_bs'],
                               I['w'], I['M'], I['n_in'], I['n_out'], bool(I['bd']), I['r0'],
                               I['r1'], I['rpb'], I['dz'], I['ld_dz'], I['dz_bs'], I['part'],
                               I['ld_part'], mutate=mutate)
    if kind == 'relu':
        r = R.relu_backward_bias(I['dz'], I['ld'], I['ps'], I['a'], I['ld'], I['ps'], I['planes'],
                                 I['M'], I['n_cols'], I['r0'], I['r1'], I['rpb'],
                                 I['part'][I['part_off']:], I['ld_part'], mutate=mutate)
        r['part'] = np.concatenate([I['part'][:I['part_off']], r['part']])
        return r
    if kind == 'fin':
        res = {}
        for k, (n_part, n, dld, off, scale, acc) in enumerate(I['segs']):
            out = I['out'][k].copy()
            out[:n] = R.colsum_finalize(I['part'][k][off:], n + dld + off, n_part, n, out, scale,
                                        acc, mutate=mutate)
            res[f'out{k}'] = out
        return res
    if kind in ('sac', 'td3'):
        if kind == 'sac':
            r = R.sac_losses(I['q_on'], I['q_tg'], I['logp'], I['reward'], I['not_done'], I['n'],
                             _alpha(I), I['gamma'], mutate=mutate)
        else:
            r = R.td3_losses(I['q_on'], I['q_tg'], I['reward'], I['not_done'], I['n'], I['n_q'],
                             I['gamma'], mutate=mutate)
        if I['loss_null']:
            r['loss_part'] = np.full_like(r['loss_part'], SENT)
        steps, consts, pows = I['steps'], I['consts'], I['pows']
        for _ in range(I['calls']):
            steps, consts, pows = R.adam_counters(steps, consts, pows, I['n_opt'], I['mask'], LR,
                                                  B1, B2, mutate=mutate)
        r.update(steps=steps, consts=consts, beta_pows=pows)
        return r
    if kind == 'hb':
        return R.actor_head_backward(I['dh'], I['ld_dh'], I['h'][I['h_off']:], I['ld_h'], I['wa'],
                                     I['M'], I['n_cols'], I['n_act'], I['head'], I['V'],
                                     I['pi'][I['pi_off']:], I['ld_pi'], I['eps'], I['raw'],
                                     _alpha(I), I['d_head'], mutate=mutate)
    if kind == 'adam':
        r = R.adam_polyak(I['p'], I['g'], I['m'], I['v'], I['t'] if I['target'] else None,
                          I['consts'], B1, B2, AEPS, I['tau'], mutate=mutate)
        if not I['target']:
            del r['target']
        return r
    if kind == 'polyak':
        return R.polyak(I['t'], I['p'], I['tau'], mutate=mutate)
    if kind == 'alpha':
        la, m, v, ml, te = I['state']
        return R.alpha_step(la, m, v, ml, te, I['consts'], B1, B2, AEPS, mutate=mutate)
    if kind == 'build':
        return R.build_learner_inputs(I['state'], I['ld_s'], I['action'], I['ld_a'], I['next'],
                                      I['ld_s2'], I['n'], I['S'], I['A'], I['xs'], I['ld'], I['w1'],
                                      I['ld_w1'], I['n_w1'] or 0, I['wa'], mutate=mutate)
    raise AssertionError(kind)


@functools.lru_cache(maxsize=None)
def _base(name):
    return _ordered(name)


# --------------------------------------------------------------------------
# the float64 definition on a case: name -> (value, bound, libm mask).  mask
# None: the output is restated to the bit and ``bound`` is the derived bound of
# any float32 evaluation; else the elements under it are behind a libm call and
# ``bound`` is the measured tolerance there (the others bit-exact).
# --------------------------------------------------------------------------
def _exact(x):
    x = np.asarray(x, np.float64)
    return x, np.zeros_like(x), None


@functools.lru_cache(maxsize=None)
def _reference(name):
    kind, _ = CASES[name]
    I = _inputs(name)
    base = _base(name)
    if kind == 'fwd':
        M, n_out, head = I['M'], I['n_out'], I['head']
        y, yb = D.thin_forward_f64(I['a'][I['a_off']:], I['lda'], I['a_bs'], I['w'][I['w_off']:],
                                   I['b'], M, I['n_in'], n_out, bool(I['bd']))
        ref = {'y': (y, yb, None)}
        n_w = n_out // 2 if head == SAC else n_out
        idx = I['out_off'] + np.arange(M)[:, None] * I['ld_out'] + np.arange(n_w)
        ov, ob = np.full(len(base['out']), float(SENT)), np.zeros(len(base['out']))
        mask = np.zeros(len(base['out']), bool)
        if head == PLAIN:
            ov[idx], ob[idx] = y, yb
            ref['out'] = (ov, ob, None)
            return ref
        y32 = torch.from_numpy(base['y'])
        if head == TANH:
            (tv, tt), = D.twin_tolerance(lambda xs: torch.tanh(xs[0]), [y32])
            ov[idx], ob[idx], mask[idx] = tv, tt, True
            ref['out'] = (ov, ob, mask)
            return ref
        na = n_out // 2
        (pv, pt), (lv, lt), (ev, et) = D.twin_tolerance(
            lambda xs: D.sac_head(xs[0], xs[1], I['ent_rows']), [y32, torch.from_numpy(I['eps'])])
        ov[idx], ob[idx], mask[idx] = pv, pt, True
        ref.update(out=(ov, ob, mask), logp=(lv, lt, np.ones(M, bool)),
                   log_std_raw=(y[:, na:], yb[:, na:], None),
                   entropy_part=_exact(base['entropy_part']) if I.get('ent_null')
                   else (ev, et, np.ones(len(ev), bool)))
        return ref
    if kind == 'bwd':
        r = D.thin_backward_f64(I['d_out'], I['ld_dout'], I['a'][I['a_off']:], I['lda'], I['a_bs'],
                                I['w'], I['M'], I['n_in'], I['n_out'], bool(I['bd']), I['r0'],
                                I['r1'], I['rpb'], I['dz'], I['ld_dz'], I['dz_bs'], I['part'],
                                I['ld_part'])
        return {k: v + (None,) for k, v in r.items()}
    if kind == 'relu':
        r = D.relu_backward_bias_f64(I['dz'], I['ld'], I['ps'], I['a'], I['ld'], I['ps'],
                                     I['planes'], I['M'], I['n_cols'], I['r0'], I['r1'], I['rpb'],
                                     I['part'][I['part_off']:], I['ld_part'])
        pre = np.asarray(I['part'][:I['part_off']], np.float64)
        r['part'] = (np.concatenate([pre, r['part'][0]]),
                     np.concatenate([np.zeros_like(pre), r['part'][1]]))
        return {k: v + (None,) for k, v in r.items()}
    if kind == 'fin':
        ref = {}
        for k, (n_part, n, dld, off, scale, acc) in enumerate(I['segs']):
            v, b = D.colsum_finalize_f64(I['part'][k][off:], n + dld + off, n_part, n, I['out'][k],
                                         scale, acc)
            ov, ob = np.asarray(I['out'][k], np.float64).copy(), np.zeros(n + 3)
            ov[:n], ob[:n] = v, b
            ref[f'out{k}'] = (ov, ob, None)
        return ref
    if kind in ('sac', 'td3'):
        if kind == 'sac':
            r = D.sac_losses_f64(I['q_on'], I['q_tg'], I['logp'], I['reward'], I['not_done'], I['n'],
                                 _alpha(I), I['gamma'])
        else:
            r = D.td3_losses_f64(I['q_on'], I['q_tg'], I['reward'], I['not_done'], I['n'], I['n_q'],
                                 I['gamma'])
        if I['loss_null']:
            r['loss_part'] = _exact(base['loss_part'])[:2]
        ref = {k: v + (None,) for k, v in r.items()}
        # counters: float64 Python with pow(), `calls` ticks at once
        steps, pows = np.array(I['steps'], np.float64), np.array(I['pows'], np.float64)
        consts = np.array(I['consts'], np.float64)
        for k in range(I['n_opt']):
            if (I['mask'] >> k) & 1:
                steps[k] += I['calls']
                pows[2 * k], pows[2 * k + 1] = B1 ** steps[k], B2 ** steps[k]
                consts[2 * k] = LR / (1 - pows[2 * k])
                consts[2 * k + 1] = math.sqrt(1 - pows[2 * k + 1])
        ticked = np.repeat([(I['mask'] >> k) & 1 for k in range(I['n_opt'])], 2).astype(bool)
        # a running product of t factors against pow(): 2^-53 per factor and for
        # pow() itself, passed on by 1 / (1 - x) with its condition number
        t = np.repeat(steps, 2) + 2
        pb = ticked * t * 2.0 ** -52 * pows
        cond = np.where(ticked, pows / np.maximum(1 - pows, 1e-300), 0.0)
        ref.update(steps=_exact(steps), beta_pows=(pows, pb, None),
                   consts=(consts, ticked * (D.ulp32(consts) + np.abs(consts) * cond * t * 2.0 ** -52),
                           None))
        return ref
    if kind == 'hb':
        M, na, head = I['M'], I['n_act'], I['head']
        r = D.head_backward_f64(I['dh'], I['ld_dh'], I['h'][I['h_off']:], I['ld_h'], I['wa'], M,
                                I['n_cols'], na, head, I['pi'][I['pi_off']:], I['ld_pi'], _alpha(I),
                                I['d_head'])
        ref = {'dpi': r['dpi'] + (None,)}
        dv, db = r['d_head']
        if head == TANH:
            ref['d_head'] = (dv, db, None)
            return ref
        t = I['pi'][I['pi_off']:][np.arange(M)[:, None] * I['ld_pi'] + np.arange(na)]
        raw, alpha = torch.from_numpy(I['raw']), float(_alpha(I))
        (hv, ht), = D.twin_tolerance(
            lambda xs: D.head_log_std_half(xs[0], xs[1], xs[2], raw, alpha, M),
            [base['dpi'], t, I['eps']])
        idx = np.arange(M)[:, None] * 2 * na + na + np.arange(na)
        mask = np.zeros(len(dv), bool)
        dv[idx], db[idx], mask[idx] = hv, ht, True
        ref['d_head'] = (dv, db, mask)
        return ref
    if kind == 'adam':
        r = D.adam_polyak_f64(I['p'], I['g'], I['m'], I['v'], I['t'] if I['target'] else None,
                              I['consts'], B1, B2, AEPS, I['tau'])
        return {k: v + (None,) for k, v in r.items()}
    if kind == 'polyak':
        return {k: v + (None,) for k, v in D.polyak_f64(I['t'], I['p'], I['tau']).items()}
    if kind == 'alpha':
        la, m, v, ml, te = I['state']
        g = -(D.E(np.array([float(f32(ml))])) + float(f32(te)))     # one rounding of its own
        r = D.adam_polyak_f64([la], g, [m], [v], None, I['consts'], B1, B2, AEPS, 0.0)
        ref = {'log_alpha': r['p'] + (None,), 'm': r['m'] + (None,), 'v': r['v'] + (None,)}
        (gv, gt), = D.twin_tolerance(lambda xs: -(xs[1] + te) + torch.exp(xs[0]) * xs[1],
                                     [np.array([la], f32), np.array([ml], f32)])
        ref['grad'] = (gv, gt, np.ones(1, bool))
        return ref
    if kind == 'build':
        return {k: _exact(v) for k, v in base.items()}
    raise AssertionError(kind)


# --------------------------------------------------------------------------
# the assertion the GPU tests apply to a kernel's outputs
# --------------------------------------------------------------------------
def _bits(x):
    x = np.ascontiguousarray(x)
    return x.reshape(-1).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def assert_kernel_outputs(name, got):
    """``got``: name -> array, what a kernel left.  Every output the restatement
    gives to the bit must have its bits; every element behind a libm call must
    be within its tolerance of the float64 definition.  Returns the largest
    |got - float64| / tolerance per libm output."""
    want, ref = _base(name), _reference(name)
    shares = {}
    for key, g in got.items():
        w = want[key]
        g = np.asarray(g).reshape(np.shape(w))
        assert g.dtype == np.asarray(w).dtype, (name, key, g.dtype)
        v, tol, mask = ref[key]
        exact = np.ones(g.size, bool) if mask is None else ~mask.reshape(-1)
        same = _bits(g) == _bits(w)
        bad = np.nonzero(exact & ~same)[0]
        assert bad.size == 0, (name, key, 'bits differ at', bad[:5], g.reshape(-1)[bad[:5]],
                               np.asarray(w).reshape(-1)[bad[:5]])
        if mask is not None and mask.any():
            m = mask.reshape(-1)
            err = np.abs(g.reshape(-1).astype(np.float64) - v.reshape(-1))[m]
            t = tol.reshape(-1)[m]
            with np.errstate(invalid='ignore'):
                ok = err <= t
            assert ok.all(), (name, key, 'beyond the libm tolerance', float(np.nanmax(err / t)),
                              int((~ok).sum()))
            finite = np.isfinite(t) & (t > 0)
            shares[key] = float((err[finite] / t[finite]).max()) if finite.any() else 0.0
    return shares


def _leaves_bound(name, out):
    """Some element of some output of ``out`` is outside the float64 bound."""
    for key, (v, tol, _) in _reference(name).items():
        if key not in out:
            continue
        with np.errstate(invalid='ignore'):
            err = np.abs(np.asarray(out[key], np.float64).reshape(-1) - v.reshape(-1))
            if not (err <= tol.reshape(-1)).all():
                return True
    return False


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
# mutation -> the GPU input that catches it
CAUGHT_BY = {
    'fwd_drop_last_chunk': 'fwd-v4-1028x261-o6h1',
    'fwd_skip_wave3': 'fwd-v4-1024x7-o4h1',
    'fwd_no_bias': 'fwd-v4-4x1-o1h0',
    'fwd_ls_raw_clamped': 'fwd-sac-edges-a2',
    'fwd_clamp_one_side': 'fwd-sac-edges-a1',
    'fwd_ent_le': 'fwd-sac-edges-a3',
    'fwd_ent_dup_last': 'fwd-sac-ent-partial-block',
    'fwd_tanh_corr_sign': 'fwd-v4-256x4-o2h1',
    'fwd_softplus_no_threshold': 'fwd-sac-edges-a4',
    'fwd_bd_critic0': 'fwd-bd2-side-v4',
    'fwd_bd_planes_as_side': 'fwd-bd2-planes-v1',
    'loss_no_not_done': 'sac-n257',
    'loss_min_is_q1': 'td3-n255-q2',
    'loss_logp_row_i': 'sac-n2',
    'loss_tie_full': 'sac-n513',
    'loss_no_factor2': 'td3-n257-q1',
    'loss_inv_2n': 'sac-n1',
    'loss_drop_last_block': 'td3-n513-q2',
    'loss_tick_unticked': 'sac-n255',
    'loss_consts_from_pows_before': 'sac-n256',
    'td3_nq1_row_2i': 'td3-n513-q1',
    'bwd_relu_ge': 'bwd-260x11-rpb4-third-o6',
    'bwd_sum_outside_window': 'bwd-64x70-rpb32-inside-o2',
    'bwd_dz_window_only': 'bwd-256x10-rpb3-empty-o3',
    'bwd_skip_block_tail': 'bwd-520x23-rpb5-third-o6',
    'bwd_dw_post_relu': 'bwd-bd2-side-v4',
    'bwd_bias_wave0_only': 'bwd-65x150-rpb64-third-o4',
    'bwd_zero_slab_unwritten': 'relu-p1-empty-window',
    'fin_drop_remainder': 'fin-33x130-acc0',
    'fin_scale_after_accumulate': 'fin-3x8-acc1',
    'fin_ignore_accumulate': 'fin-twelve-mixed',
    'hb_strict_indicator': 'hb-63x5-a3h1-la0.0',
    'hb_alpha_2n': 'hb-1024x7-a4h1-laNone',
    'hb_no_one_minus_pi2': 'hb-260x5-a3h2-laNone',
    'hb_tanh_stride_2na': 'hb-wide-pi-tanh',
    'adam_eps_inside_bc2': 'adam-n1021',
    'adam_polyak_before_step': 'adam-n1025',
    'adam_skip_tail': 'polyak-n1027',
    'adam_omb1_f32': 'adam-n1028',
    'build_pi_rows_from_next': 'build-9x63a2-w255',
    'build_wa_untransposed': 'build-strided',
}


def test_every_mutation_names_the_gpu_input_that_catches_it():
    assert set(CAUGHT_BY) == set(R.MUTATIONS)
    assert set(CAUGHT_BY.values()) <= set(CASES)
    assert set(ROUNDING_LEVEL) <= set(R.MUTATIONS)


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_is_inside_the_float64_bound_on_every_element(name):
    out, ref = _base(name), _reference(name)
    assert set(out) == set(ref)
    for key, (v, tol, _) in ref.items():
        x = np.asarray(out[key], np.float64).reshape(-1)
        assert x.shape == v.reshape(-1).shape, (name, key)
        assert np.isfinite(v).all() and np.isfinite(tol).all(), (name, key, 'no element unchecked')
        with np.errstate(invalid='ignore'):
            ok = np.abs(x - v.reshape(-1)) <= tol.reshape(-1)
        assert ok.all(), (name, key, np.nonzero(~ok)[0][:5])
    # ... and passes the GPU tests' assertion in a kernel's place
    assert_kernel_outputs(name, out)


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_mutation_is_caught_by_its_gpu_input(mutation):
    name = CAUGHT_BY[mutation]
    base, mut = _base(name), _ordered(name, mutate=mutation)
    assert any((_bits(mut[k]) != _bits(base[k])).any() for k in base), 'same bits'
    if mutation not in ROUNDING_LEVEL:
        assert _leaves_bound(name, mut), 'the mutant is inside the float64 bound'
    with pytest.raises(AssertionError):
        assert_kernel_outputs(name, mut)


def test_wave_sum_is_the_dpp_sequence():
    """wave_sum restated from the six DPP steps themselves (row_shr 1, 2, 4, 8
    with zero fill, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2
    and 3, lane 63) equals the balanced pairwise tree the restatement uses."""
    v = _randn(_rng('wave'), 50, 64) * f32(1e3)
    x = v.copy()
    lane = np.arange(64)
    for s in (1, 2, 4, 8):
        src = np.where(lane % 16 >= s, lane - s, 0)
        x = x + np.where(lane % 16 >= s, x[:, src], f32(0))
    for last, rows in ((15, (1, 3)), (31, (2, 3))):
        src = (lane // 16) * 16 - 1 if last == 15 else np.full(64, 31)
        take = np.isin(lane // 16, rows)
        x = x + np.where(take, x[:, np.where(take, src, 0)], f32(0))
    assert np.array_equal(_bits(x[:, 63]), _bits(R.wave_sum(v)))


def test_float64_functions_are_the_torchops_definition():
    """The float64 values the bounds go with are TorchOps' (the plain definition
    the schedule tests use), on one case of each kernel with a sum."""
    ops = D.TorchOps()
    t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))      # noqa: E731
    I = _inputs('bwd-260x11-rpb4-third-o6')
    M, H = I['M'], I['n_in']
    dz, part = torch.zeros(M, H, dtype=torch.float64), torch.zeros(3, 7 * H + 6, dtype=torch.float64)
    ops.thin_backward(t64(I['d_out']).view(M, 6), t64(I['a']).view(M, H), t64(I['w']), 6, False,
                      I['r0'], I['r1'], dz, part, rows_per_block=4)
    ref = _reference('bwd-260x11-rpb4-third-o6')
    assert np.allclose(ref['dz'][0].reshape(M, H), dz.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(ref['part'][0].reshape(3, -1), part.numpy(), rtol=1e-13, atol=1e-13)
    I = _inputs('fin-3x8-acc1')
    n_part, n, dld, off, scale, acc = I['segs'][0]
    out = t64(I['out'][0]).clone()
    ops.colsum_finalize([(t64(I['part'][0]).view(n_part, -1), off, n, out, float(f32(scale)), acc)])
    assert np.allclose(_reference('fin-3x8-acc1')['out0'][0], out.numpy(), rtol=1e-13, atol=1e-13)
    I = _inputs('td3-n257-q1')
    dq, lp = torch.zeros(257, 1, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.float64)
    ops.td3_losses(t64(I['q_on']), t64(I['q_tg']), t64(I['reward']), t64(I['not_done']),
                   float(f32(0.99)), dq, lp, torch.zeros(0), None, None, 0, LR)
    ref = _reference('td3-n257-q1')
    assert np.allclose(ref['dq'][0], dq.numpy(), rtol=1e-13, atol=1e-15)
    assert np.allclose(ref['loss_part'][0], lp.numpy(), rtol=1e-12, atol=1e-13)
    I = _inputs('adam-n1025')
    p, m, v, t = (t64(I[k]).clone() for k in 'pmvt')
    ops.adam_polyak(p, t64(I['g']), m, v, t, t64(I['consts']), I['tau'])
    ref = _reference('adam-n1025')
    for key, x in (('p', p), ('m', m), ('v', v), ('target', t)):
        assert np.allclose(ref[key][0], x.numpy(), rtol=1e-12, atol=1e-14), key


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
class _Gpu:
    """The C ABI through ctypes on device copies of a case's buffers."""

    def __init__(self):
        from tracktolearn_amd import _lib
        self.mod, self.lib = _lib, _lib.load()
        self.keep = []

    def dev(self, x, off=0):
        """Device copy of a NumPy buffer; returns (tensor, pointer at `off` items)."""
        if x is None:
            return None, None
        t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.keep.append(t)
        return t, C.c_void_p(t.data_ptr() + off * t.element_size())

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(self, code, what):
        self.mod.check(code, what)
        torch.cuda.synchronize()


def _run_hip(name):
    kind, _ = CASES[name]
    I = _inputs(name)
    G = _Gpu()
    lib, s = G.lib, G.stream()
    if kind == 'fwd':
        M, n_out, head = I['M'], I['n_out'], I['head']
        _, a = G.dev(I['a'], I['a_off'])
        _, w = G.dev(I['w'], I['w_off'])
        _, b = G.dev(I['b'])
        na = n_out // 2
        _, eps = G.dev(I['eps'])
        base = _base(name)
        out_t, out = G.dev(np.full_like(base['out'], SENT), I['out_off'])
        y_t, y = G.dev(np.full((M, n_out), SENT))
        sac = head == SAC
        logp_t, logp = G.dev(np.full(M, SENT) if sac else None)
        raw_t, raw = G.dev(np.full((M, na), SENT) if sac else None)
        ent_t, ent = G.dev(np.full(-(-M // 4), SENT) if sac else None)
        G.ok(lib.ttl_thin_forward(a, I['lda'], I['a_bs'], w, b, M, I['n_in'], n_out, int(bool(I['bd'])),
                                  head, eps if sac else None, I['ent_rows'], out, I['ld_out'], logp, raw,
                                  None if I.get('ent_null') else ent, s), name)
        # the pre-activations: the PLAIN head of the same instantiation
        G.ok(lib.ttl_thin_forward(a, I['lda'], I['a_bs'], w, b, M, I['n_in'], n_out, int(bool(I['bd'])),
                                  PLAIN, None, 0, y, n_out, None, None, None, s), name)
        res = {'out': out_t, 'y': y_t}
        if sac:
            res.update(logp=logp_t, log_std_raw=raw_t, entropy_part=ent_t)
    elif kind == 'bwd':
        _, d = G.dev(I['d_out'])
        _, a = G.dev(I['a'], I['a_off'])
        _, w = G.dev(I['w'])
        dz_t, dz = G.dev(I['dz'])
        part_t, part = G.dev(I['part'])
        G.ok(lib.ttl_thin_backward(d, I['ld_dout'], a, I['lda'], I['a_bs'], w, I['M'], I['n_in'],
                                   I['n_out'], int(bool(I['bd'])), I['r0'], I['r1'], I['rpb'], dz,
                                   I['ld_dz'], I['dz_bs'], part, I['ld_part'], s), name)
        res = {'dz': dz_t, 'part': part_t}
    elif kind == 'relu':
        dz_t, dz = G.dev(I['dz'])
        _, a = G.dev(I['a'])
        part_t, part = G.dev(I['part'], I['part_off'])
        G.ok(lib.ttl_relu_backward_bias(dz, I['ld'], I['ps'], a, I['ld'], I['ps'], I['planes'], I['M'],
                                        I['n_cols'], I['r0'], I['r1'], I['rpb'], part, I['ld_part'],
                                        s), name)
        res = {'dz': dz_t, 'part': part_t}
    elif kind == 'fin':
        arr = (G.mod.ColsumSeg * len(I['segs']))()
        res = {}
        for k, (n_part, n, dld, off, scale, acc) in enumerate(I['segs']):
            _, part = G.dev(I['part'][k], off)
            out_t, out = G.dev(I['out'][k])
            arr[k].part, arr[k].ld, arr[k].n_part, arr[k].n = part.value, n + dld + off, n_part, n
            arr[k].out, arr[k].scale, arr[k].accumulate = out.value, scale, acc
            res[f'out{k}'] = out_t
        G.ok(lib.ttl_colsum_finalize(arr, len(I['segs']), s), name)
    elif kind in ('sac', 'td3'):
        n = I['n']
        ptrs = {k: G.dev(I[k])[1] for k in ('q_on', 'q_tg', 'logp', 'reward', 'not_done')}
        base = _base(name)
        dq_t, dq = G.dev(np.full_like(base['dq'], SENT))
        lp_t, lp = G.dev(np.full_like(base['loss_part'], SENT))
        n_opt = I['n_opt']
        st_t, st = G.dev(I['steps'] if n_opt else None)
        co_t, co = G.dev(I['consts'] if n_opt else None)
        po_t, po = G.dev(I['pows'] if n_opt else None)
        _, la = G.dev(None if I.get('log_alpha') is None else np.array([I['log_alpha']], f32))
        for _ in range(I['calls']):
            if kind == 'sac':
                code = lib.ttl_sac_losses(ptrs['q_on'], ptrs['q_tg'], ptrs['logp'], ptrs['reward'],
                                          ptrs['not_done'], n, la, I['alpha_const'], I['gamma'], dq,
                                          None if I['loss_null'] else lp, st, co, po, n_opt,
                                          I['mask'], LR, B1, B2, s)
            else:
                code = lib.ttl_td3_losses(ptrs['q_on'], ptrs['q_tg'], ptrs['reward'],
                                          ptrs['not_done'], n, I['n_q'], I['gamma'], dq,
                                          None if I['loss_null'] else lp, st, co, po, n_opt,
                                          I['mask'], LR, B1, B2, s)
            G.ok(code, name)
        res = {'dq': dq_t, 'loss_part': lp_t}
        if n_opt:
            res.update(steps=st_t, consts=co_t, beta_pows=po_t)
    elif kind == 'hb':
        _, dh = G.dev(I['dh'])
        _, h = G.dev(I['h'], I['h_off'])
        _, wa = G.dev(I['wa'])
        _, pi = G.dev(I['pi'], I['pi_off'])
        _, eps = G.dev(I['eps'])
        _, raw = G.dev(I['raw'])
        _, la = G.dev(None if I['log_alpha'] is None else np.array([I['log_alpha']], f32))
        dh_t, d_head = G.dev(I['d_head'])
        sac = I['head'] == SAC
        G.ok(lib.ttl_sac_actor_head_backward(dh, I['ld_dh'], h, I['ld_h'], wa, I['M'], I['n_cols'],
                                             I['n_act'], I['head'], pi, I['ld_pi'],
                                             eps if sac else None, raw if sac else None, la,
                                             I['alpha_const'], d_head, s), name)
        res = {'d_head': dh_t}
        # dpi itself: the TANH head of the same instantiation with pi = 0, where
        # dpi (1 - 0 * 0) = dpi exactly
        _, zero_pi = G.dev(np.zeros(I['M'] * I['n_act'], f32))
        dpi_t, dpi = G.dev(np.full((I['M'], I['n_act']), SENT))
        G.ok(lib.ttl_sac_actor_head_backward(dh, I['ld_dh'], h, I['ld_h'], wa, I['M'], I['n_cols'],
                                             I['n_act'], TANH, zero_pi, I['n_act'], None, None, None,
                                             0.0, dpi, s), name)
        res['dpi'] = dpi_t
    elif kind == 'adam':
        ts = {k: G.dev(I[k]) for k in 'pgmvt'}
        _, co = G.dev(I['consts'])
        G.ok(lib.ttl_adam_polyak(ts['p'][1], ts['g'][1], ts['m'][1], ts['v'][1],
                                 ts['t'][1] if I['target'] else None, I['n'], co, B1, B2, AEPS,
                                 I['tau'], s), name)
        res = {'p': ts['p'][0], 'm': ts['m'][0], 'v': ts['v'][0]}
        if I['target']:
            res['target'] = ts['t'][0]
    elif kind == 'polyak':
        t_t, t = G.dev(I['t'])
        _, p = G.dev(I['p'])
        G.ok(lib.ttl_polyak_average(t, p, I['n'], I['tau'], s), name)
        res = {'target': t_t}
    elif kind == 'alpha':
        la, m, v, ml, te = I['state']
        ts = [G.dev(np.array([x], f32)) for x in (la, SENT, m, v, ml)]
        _, co = G.dev(I['consts'])
        G.ok(lib.ttl_sac_alpha_step(ts[0][1], ts[1][1], ts[2][1], ts[3][1], ts[4][1], te, co, B1, B2,
                                    AEPS, s), name)
        res = {'log_alpha': ts[0][0], 'grad': ts[1][0], 'm': ts[2][0], 'v': ts[3][0]}
    elif kind == 'build':
        _, st = G.dev(I['state'])
        _, ac = G.dev(I['action'])
        _, nx = G.dev(I['next'])
        xs_t, xs = G.dev(I['xs'])
        _, w1 = G.dev(I['w1'])
        wa_t, wa = G.dev(I['wa'])
        G.ok(lib.ttl_build_learner_inputs(st, I['ld_s'], ac, I['ld_a'], nx, I['ld_s2'], I['n'], I['S'],
                                          I['A'], xs, I['ld'], w1, I['ld_w1'], I['n_w1'] or 0, wa, s),
             name)
        res = {'xs': xs_t}
        if wa_t is not None:
            res['wa'] = wa_t
    else:
        raise AssertionError(kind)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_equals_its_restatement(name):
    got = _run_hip(name)
    shares = assert_kernel_outputs(name, got)
    again = _run_hip(name)                          # determinism: the same bits
    for key in got:
        assert np.array_equal(_bits(got[key]), _bits(again[key])), (name, key)
    for key, share in shares.items():
        print(f'libm share {CASES[name][0]} {key} {name}: {share:.3f}')


@pytest.mark.gpu
def test_three_adam_steps_from_scratch_equal_torch_optim_adam():
    """Counters from ttl_td3_losses + ttl_adam_polyak against torch.optim.Adam on
    the device (<= 1 ulp) and against the restatement (bit for bit)."""
    from tracktolearn_amd.algorithms.shared.fused import HipOps
    hip = HipOps(DEV)
    g = _rng('three steps')
    n = 1027
    p0 = _randn(g, n)
    w = torch.nn.Parameter(torch.from_numpy(p0).to(DEV))
    opt = torch.optim.Adam([w], lr=LR)
    z = dict(device=DEV)
    p, m, v = torch.from_numpy(p0).to(DEV), torch.zeros(n, **z), torch.zeros(n, **z)
    steps, consts = torch.zeros(1, **z), torch.zeros(2, **z)
    pows = torch.ones(2, dtype=torch.float64, device=DEV)
    one = torch.zeros(1, 1, **z)
    rp, rm, rv = p0, np.zeros(n, f32), np.zeros(n, f32)
    rs, rc, rpw = np.zeros(1, f32), np.zeros(2, f32), np.ones(2)
    for _ in range(3):
        gi = _randn(g, n)
        w.grad = torch.from_numpy(gi).to(DEV)
        opt.step()
        hip.td3_losses(one, one, one[0], one[0], 0.99, torch.zeros(1, 1, **z), None, steps, consts,
                       pows, 0b1, LR)
        hip.adam_polyak(p, w.grad, m, v, None, consts, 0.0)
        rs, rc, rpw = R.adam_counters(rs, rc, rpw, 1, 1, LR, B1, B2)
        r = R.adam_polyak(rp, gi, rm, rv, None, rc, B1, B2, AEPS, 0.0)
        rp, rm, rv = r['p'], r['m'], r['v']
    assert float(steps) == 3.0
    assert np.array_equal(_bits(consts.cpu().numpy()), _bits(rc))
    for x, y in ((p, rp), (m, rm), (v, rv)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y))
    err = (p - w.data).abs().double().cpu().numpy()
    assert (err <= D.ulp32(w.data.cpu().numpy())).all(), float(err.max())


def _refusals(buf, odd, seg):
    """(entry point, arguments, expected code): every argument list is rejected
    by the entry point's own checks, before anything is launched.  ``buf``: a
    valid, 16-byte aligned device pointer; ``odd``: the same + 4 bytes."""
    INV, UNS = -1, -4
    fwd = dict(a=buf, lda=8, a_bs=0, w=buf, b=buf, n_rows=4, n_in=8, n_out=2, bd=0, head=PLAIN,
               eps=buf, ent=0, out=buf, ld_out=2, logp=buf, raw=buf, part=buf)
    bwd = dict(d=buf, ld_d=2, a=buf, lda=8, a_bs=0, w=buf, n_rows=4, n_in=8, n_out=2, bd=0, r0=0, r1=4,
               rpb=4, dz=odd, ld_dz=8, dz_bs=0, part=buf, ld_part=26)
    relu = dict(dz=odd, ld_dz=8, dz_ps=0, a=buf, lda=8, a_ps=0, planes=1, n_rows=4, n_cols=8, r0=0,
                r1=4, rpb=4, part=buf, ld_part=8)
    loss = dict(q=buf, qt=buf, lp=buf, r=buf, nd=buf, n=4, la=None, ac=0.2, gamma=0.99, dq=buf,
                part=None, steps=buf, consts=buf, pows=buf, n_opt=1, mask=0, lr=LR, b1=B1, b2=B2)
    td3 = dict(q=buf, qt=buf, r=buf, nd=buf, n=4, n_q=2, gamma=0.99, dq=buf, part=None, steps=buf,
               consts=buf, pows=buf, n_opt=1, mask=0, lr=LR, b1=B1, b2=B2)
    hb = dict(dh=buf, ld_dh=8, h=buf, ld_h=8, wa=buf, n_rows=4, n_cols=8, n_act=2, head=SAC, pi=buf,
              ld_pi=2, eps=buf, raw=buf, la=None, ac=0.2, d_head=buf)
    adam = dict(p=buf, g=buf, m=buf, v=buf, t=buf, n=8, consts=buf, b1=B1, b2=B2, eps=AEPS, tau=0.005)
    alpha = dict(la=buf, g=buf, m=buf, v=buf, ml=buf, te=-3.0, consts=buf, b1=B1, b2=B2, eps=AEPS)
    build = dict(s=buf, ld_s=8, a=buf, ld_a=2, s2=buf, ld_s2=8, n=4, n_state=8, n_act=2, xs=buf,
                 ld=10, w1=None, ld_w1=0, n_w1=0, wa=None)
    pol = dict(t=buf, p=buf, n=8, tau=0.005)

    def variants(fn, base, code_changes):
        for code, change in code_changes:
            yield fn, list({**base, **change}.values()), code, change
    yield from variants('ttl_thin_forward', fwd, [
        (INV, dict(a=None)), (INV, dict(w=None)), (INV, dict(b=None)), (INV, dict(out=None)),
        (INV, dict(n_rows=0)), (INV, dict(n_in=0)), (INV, dict(lda=7)), (INV, dict(bd=1, a_bs=7)),
        (INV, dict(bd=1, a_bs=8, lda=12)), (INV, dict(ld_out=1)), (INV, dict(head=3)),
        (UNS, dict(n_out=5, ld_out=8)), (UNS, dict(n_out=7, ld_out=8)), (UNS, dict(n_out=3, bd=1, a_bs=8, lda=24, ld_out=3)),
        (INV, dict(head=SAC, bd=1, a_bs=8, lda=16)), (INV, dict(head=SAC, n_out=3, ld_out=3)),
        (INV, dict(head=SAC, ent=5)), (INV, dict(head=SAC, ent=-1)), (INV, dict(head=SAC, eps=None)),
        (INV, dict(head=SAC, logp=None)), (INV, dict(head=SAC, raw=None)),
        (INV, dict(head=SAC, ld_out=0))])
    yield from variants('ttl_thin_backward', bwd, [
        (INV, dict(d=None)), (INV, dict(a=None)), (INV, dict(w=None)), (INV, dict(dz=None)),
        (INV, dict(part=None)), (INV, dict(n_rows=0)), (INV, dict(n_in=0)), (INV, dict(rpb=0)),
        (INV, dict(dz=buf)), (INV, dict(lda=7)), (INV, dict(ld_dz=7)), (INV, dict(ld_d=1)),
        (INV, dict(ld_part=25)), (INV, dict(bd=1, a_bs=7, dz_bs=8, ld_part=34)),
        (INV, dict(bd=1, a_bs=8, dz_bs=7, ld_part=34)), (UNS, dict(n_out=5, ld_d=5, ld_part=53)),
        (UNS, dict(n_out=7, ld_d=7, ld_part=71))])
    yield from variants('ttl_relu_backward_bias', relu, [
        (INV, dict(dz=None)), (INV, dict(a=None)), (INV, dict(part=None)), (INV, dict(n_rows=0)),
        (INV, dict(n_cols=0)), (INV, dict(rpb=0)), (INV, dict(planes=0)), (INV, dict(planes=65)),
        (INV, dict(ld_dz=7)), (INV, dict(lda=7)), (INV, dict(ld_part=7)),
        (INV, dict(planes=2, ld_part=15))])
    yield from variants('ttl_sac_losses', loss, [
        (INV, dict(q=None)), (INV, dict(qt=None)), (INV, dict(lp=None)), (INV, dict(r=None)),
        (INV, dict(nd=None)), (INV, dict(dq=None)), (INV, dict(n=0)), (INV, dict(n_opt=9)),
        (INV, dict(n_opt=-1)), (INV, dict(steps=None)), (INV, dict(consts=None)),
        (INV, dict(pows=None))])
    yield from variants('ttl_td3_losses', td3, [
        (INV, dict(q=None)), (INV, dict(qt=None)), (INV, dict(r=None)), (INV, dict(nd=None)),
        (INV, dict(dq=None)), (INV, dict(n=0)), (INV, dict(n_q=3)), (INV, dict(n_q=0)),
        (INV, dict(n_opt=9)), (INV, dict(n_opt=-1)), (INV, dict(steps=None)), (INV, dict(consts=None)),
        (INV, dict(pows=None))])
    yield from variants('ttl_sac_actor_head_backward', hb, [
        (INV, dict(head=PLAIN)), (INV, dict(dh=None)), (INV, dict(h=None)), (INV, dict(wa=None)),
        (INV, dict(pi=None)), (INV, dict(d_head=None)), (INV, dict(n_rows=0)), (INV, dict(n_cols=0)),
        (INV, dict(eps=None)), (INV, dict(raw=None)), (INV, dict(ld_dh=7)), (INV, dict(ld_h=7)),
        (INV, dict(ld_pi=1)), (UNS, dict(n_act=5, ld_pi=5)), (UNS, dict(n_act=0))])
    yield from variants('ttl_adam_polyak', adam, [
        (INV, dict(p=None)), (INV, dict(g=None)), (INV, dict(m=None)), (INV, dict(v=None)),
        (INV, dict(consts=None)), (INV, dict(n=0)), (INV, dict(p=odd)), (INV, dict(g=odd)),
        (INV, dict(m=odd)), (INV, dict(v=odd)), (INV, dict(t=odd))])
    yield from variants('ttl_polyak_average', pol, [
        (INV, dict(t=None)), (INV, dict(p=None)), (INV, dict(n=0)), (INV, dict(t=odd)),
        (INV, dict(p=odd))])
    yield from variants('ttl_sac_alpha_step', alpha, [
        (INV, dict(la=None)), (INV, dict(g=None)), (INV, dict(m=None)), (INV, dict(v=None)),
        (INV, dict(ml=None)), (INV, dict(consts=None))])
    yield from variants('ttl_build_learner_inputs', build, [
        (INV, dict(s=None)), (INV, dict(a=None)), (INV, dict(s2=None)), (INV, dict(xs=None)),
        (INV, dict(n=0)), (INV, dict(n_state=0)), (INV, dict(n_act=0)), (INV, dict(ld_s=7)),
        (INV, dict(ld_s2=7)), (INV, dict(ld_a=1)), (INV, dict(ld=9)), (INV, dict(n_act=65, ld_a=65, ld=80)),
        (INV, dict(w1=buf, wa=None, ld_w1=10, n_w1=4)), (INV, dict(w1=buf, wa=buf, ld_w1=10, n_w1=0)),
        (INV, dict(w1=buf, wa=buf, ld_w1=9, n_w1=4))])
    for code, n_segs, change in [(INV, 13, {}), (INV, 0, {}), (INV, 1, dict(part=None)),
                                 (INV, 1, dict(out=None)), (INV, 1, dict(n=0)),
                                 (INV, 1, dict(n_part=0)), (INV, 1, dict(ld=3))]:
        arr = (seg * 13)()
        for k in range(13):
            vals = {**dict(part=buf, ld=4, n_part=2, n=4, out=buf, scale=1.0, accumulate=0), **change}
            for key, val in vals.items():
                setattr(arr[k], key, val)
        yield 'ttl_colsum_finalize', [arr, n_segs], code, dict(n_segs=n_segs, **change)
    yield 'ttl_colsum_finalize', [None, 1], INV, 'no segments'


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments_and_write_nothing():
    """Each refusal returns its TTL_ERR_* with a message naming the entry point
    and launches nothing: the one buffer every pointer aims at keeps its
    pre-fill."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    buf_t = torch.full((4096,), float(SENT), device=DEV)
    torch.cuda.synchronize()
    buf = buf_t.data_ptr()
    assert buf % 16 == 0
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = set()
    for fn, args, code, change in _refusals(buf, buf + 4, _lib.ColsumSeg):
        got = getattr(lib, fn)(*args, stream)
        assert got == code, (fn, change, got)
        msg = lib.ttl_last_error().decode()
        assert msg.startswith(fn), (fn, change, msg)
        seen.add(fn)
    assert len(seen) == 11
    torch.cuda.synchronize()
    assert bool((buf_t == float(SENT)).all())
