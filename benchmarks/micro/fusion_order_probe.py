"""Which fused-multiply-add order are the merged-tail gather kernels compiled to?

csrc/ttl_state.hip leaves the contraction of its blends to the compiler, and
`x * a + y * b` may be fused either way.  The separate-tail kernels
(TTL_STATE_KERNEL=3) state the order explicitly (`blend<PINNED>` /
`lerp<PINNED>`) so that they give the bits of the merged-tail kernels
(TTL_STATE_KERNEL=4).  When tests/test_state_gather_reference.py::
test_all_k_state_dd_runs_are_bit_identical fails after a compiler update, run
this on the GPU: it gathers the width sweep's rows with knob 4 and, per stencil
point, tries both orders of every blend's first add and of the lerp in NumPy
(fma = one rounding of the exact float64 product and sum) and prints the
combination that reproduces the kernel's bits, with the share of elements it
matches (1.0 expected; the runner-up stays below 0.995) per float of a column.

    python benchmarks/micro/fusion_order_probe.py [C ...]      (default 8 28 45 64)

Legend of a key (b0, b1, b2, b3, lerp): b0 / b3 the outer slices f-1 / f+2,
b1 / b2 the centre slices; 'A' = fma(first operand pair, second product), i.e.
blend fma(v00, w00, v01 w01) and lerp fma(lo, 1 - d, hi d); 'B' the other way;
'-' = not used by that point.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import ref_state as rs                              # noqa: E402
import test_state_gather_reference as t             # noqa: E402

f32 = np.float32


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def mul(a, b):
    return (a * b).astype(f32)


def blend(vs, ws, order):
    (v00, v01, v10, v11), (w00, w01, w10, w11) = vs, ws
    w00, w01, w10, w11 = (w[:, None] * np.ones_like(v00) for w in (w00, w01, w10, w11))
    r = fma(v00, w00, mul(v01, w01)) if order == 'A' else fma(v01, w01, mul(v00, w00))
    return fma(v11, w11, fma(v10, w10, r))


def lerp(lo, hi, d, order):
    e = (f32(1) - d).astype(f32)[:, None] * np.ones_like(lo)
    d = d[:, None] * np.ones_like(lo)
    return fma(lo, e, mul(hi, d)) if order == 'A' else fma(hi, d, mul(lo, e))


def search(C, got):
    vol, heads, r = t.volume(C), t.sweep_seeds(C), t.SWEEP_R
    dims = vol.shape[:3]
    fl, d = rs._floor_frac(rs.stencil_points(heads, r, 0.0))
    fc, dc = fl[:, 0], d[:, 0]
    ec = (f32(1) - dc).astype(f32)
    sl = [[np.clip(rs._clamp_int(fc[:, a], -4, dims[a] + 4) + k, 0, dims[a] - 1)
           for k in (-1, 0, 1, 2)] for a in range(3)]
    got = got[:, :7 * C].reshape(-1, 7, C).view(np.int32)
    for a in range(3):
        b, c = [x for x in range(3) if x != a]

        def at(s, jb, jc):
            ijk = [0, 0, 0]
            ijk[a], ijk[b], ijk[c] = s, jb, jc
            return vol[sl[0][ijk[0]], sl[1][ijk[1]], sl[2][ijk[2]]]
        ws = [mul(p, q) for p in (ec[:, b], dc[:, b]) for q in (ec[:, c], dc[:, c])]
        B = {o: [blend((at(s, 1, 1), at(s, 1, 2), at(s, 2, 1), at(s, 2, 2)), ws, o)
                 for s in range(4)] for o in 'AB'}
        up = (fl[:, 1 + a, a] > fc[:, a])[:, None]
        dn = (fl[:, 4 + a, a] < fc[:, a])[:, None]
        for name, pt in (('centre', 0), ('plus', 1 + a), ('minus', 4 + a)):
            if name == 'centre' and a:
                continue
            found = {}
            for o0, o1, o2, o3, ol in itertools.product('AB', repeat=5):
                b0, b1, b2, b3 = B[o0][0], B[o1][1], B[o2][2], B[o3][3]
                if name == 'centre':
                    out, key = lerp(b1, b2, dc[:, 0], ol), ('-', o1, o2, '-', ol)
                elif name == 'plus':
                    out = lerp(np.where(up, b2, b1), np.where(up, b3, b2), d[:, pt, a], ol)
                    key = ('-', o1, o2, o3, ol)
                else:
                    out = lerp(np.where(dn, b0, b1), np.where(dn, b1, b2), d[:, pt, a], ol)
                    key = (o0, o1, o2, '-', ol)
                m = out.view(np.int32) == got[:, pt]
                found[key] = (round(float(m.mean()), 4),
                              [round(float(m[:, k::4].mean()), 4) for k in range(4)])
            ranked = sorted(found.items(), key=lambda kv: -kv[1][0])
            print(f'C={C} axis {"xyz"[a]} {name:6s} best {ranked[0][0]} share {ranked[0][1][0]} '
                  f'per float {ranked[0][1][1]}  runner-up {ranked[1][1][0]}')


if __name__ == '__main__':
    from tracktolearn_amd import _lib
    for C in [int(v) for v in sys.argv[1:]] or [8, 28, 45, 64]:
        rig = t._Rig(t.volume(C), _lib.SH_BRICK4, t.N_SWEEP, t.SWEEP_K)
        words = rig.gather(t.sweep_seeds(C), t.SWEEP_R, 0.0, knobs=dict(TTL_STATE_KERNEL=4))
        search(C, t._contained(words, t.N_SWEEP, 7 * C + 3 * t.SWEEP_K))
