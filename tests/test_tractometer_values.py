"""The values inside ``k_tractometer_classify`` (csrc/ttl_tractometer.hip): the
winding and the seven float64 sums, against the header's definition at 50
digits (``ref.winding_mp``, ``ref.sums_mp``), read through a ruler of bundles
(tests/tractometer_value_cases.py).

On the CPU: the measured curves meet the input conditions (asserted on every
one), the kernel's eigen-solve restated in float64 (``ref.winding_jacobi``) and
the ``eigh`` reference of the other tests agree with 50 digits within 1e-12,
all three eigenvector slots are dropped somewhere, and every named deviation of
``ref.WINDING_MUTANTS`` has a witness among the launched rows.  On the GPU: the
winding of every curve between the marks -1e-9 and +1e-9, every sum inside the
any-order bound (n + 8) 2^-52 sum |terms|, the hand-built rows at the marks
worked out by hand, ``connected`` the full set.

Measured on an MI355X (printed by the tests, nothing tighter asserted): the
worst winding within 1e-13 of 50 digits, the worst sum below the mark at 0.12
of its bound; the restatement within 6.8e-14 of 50 digits."""
import math

import numpy as np
import pytest
import torch

import ref_tractometer as ref
import tractometer_cases as tc
import tractometer_value_cases as vc

DEV = 'cuda:0'
FULL = np.uint64(2 ** 64 - 1)
REL = 1e-9                       # the margin test_tractometer.py's exact comparisons rest on
POINT_COUNTS = {3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 200, 1000}


def _wound():
    return [(name, pts) for name, pts, wound in vc.curves() if wound]


def _hand_rows():
    return {'nan': vc.nan_row(), 'square': vc.square_row(), 'rays': vc.rays_row()}


# ----------------------------------------------------------------- CPU tests
def test_curves_cover_the_families_and_point_counts():
    curves = vc.curves()
    assert 40 <= len(curves) <= 48
    assert {len(p) for _, p, _ in curves} >= POINT_COUNTS
    for name, pts, _ in curves:
        assert pts.dtype == np.float32 and np.isfinite(pts).all(), name
        assert vc.ends_ok(pts), name
    windings = [float(r['winding']) for r in vc.winding_refs().values()]
    assert min(windings) < 200 and max(windings) > 900
    # rows whose dir_k cancels to almost nothing while absdir_k is large, under both lins
    for lin in vc.LINS:
        sums = vc.sum_refs(lin)
        for name, _, wound in curves:
            if not wound:
                assert all(0 < d < 1e-5 * a for d, a in zip(sums[name]['dir'],
                                                            sums[name]['absdir'])), name
    # the second linear part is not dyadic: its products round
    assert not np.all(vc.LINS['AFFINE'] * 2 ** 20 == np.round(vc.LINS['AFFINE'] * 2 ** 20))


def test_rulers_are_nested_and_exact():
    r = vc.WINDING_R
    assert list(r) == sorted(r) and r[vc.W_ZERO] == 0.0 and len(r) == 63
    for x in (1e-15, 1e-12, 1e-9, 1e-6, 1e-3, 0.3):
        assert vc.winding_mark(-x) < vc.W_ZERO < vc.winding_mark(x)
    angles = vc.winding_angles(260.5)
    assert len(angles) == 64 and angles[-1] == math.inf and angles[vc.W_ZERO] == 260.5
    assert vc.winding_limits(angles)[:, 14].tolist() == angles
    assert vc.winding_reach(vc.W_ZERO) == vc.winding_reach(vc.W_ZERO + 1) == 1e-15
    assert vc.winding_reach(vc.winding_mark(1e-9)) == 1e-9
    assert vc.winding_reach(vc.winding_mark(-1e-9) + 1) == 1e-9
    # windows: exactly the float64 within the width, nested, the bound among them
    import mpmath
    sums = vc.sum_refs('AFFINE')['walk_65']
    for q in vc.QUANTITIES:
        value, scale = vc.sum_reference(sums, q)
        windows, widths, at = vc.sum_windows(value, scale, 64)
        assert len(windows) == 64 and windows[-1] is None and widths[at] == 72 * 2.0 ** -52
        assert widths[0] == 0.0 and widths == sorted(widths)
        with mpmath.mp.workdps(ref.MP_DIGITS):
            for (lo, hi), w in zip(windows[:-1], widths):
                t = mpmath.mpf(w) * scale
                assert value - t <= lo and hi <= value + t
                assert np.nextafter(lo, -np.inf) < value - t
                assert np.nextafter(hi, np.inf) > value + t
        for a, b in zip(windows[:-2], windows[1:-1]):
            assert b[0] <= a[0] and a[1] <= b[1]
        table = vc.sum_limits(q, windows)
        col = {'length': 0, 'dir': 2, 'absdir': 8}[q.rstrip('012')] + \
            (2 * int(q[-1]) if q != 'length' else 0)
        assert table[:-1, col:col + 2].tolist() == windows[:-1]
        assert np.isinf(np.delete(table, [col, col + 1, 15], 1)).all()


def test_measured_curves_meet_the_input_conditions():
    """Asserted at 50 digits on every wound curve, none left out:
    (lambda2 - lambda3) / lambda1 >= 1e-2, min |p_j| >= 1e-2 max |p_j|, every
    acos argument within [-1 + 1e-6, 1 - 1e-9]."""
    refs = vc.winding_refs()
    assert len(refs) == len(_wound()) >= 40
    for name, r in refs.items():
        lam = r['lam']
        assert (lam[1] - lam[2]) / lam[0] >= 1e-2, name
        assert r['pmin'] >= 1e-2 * r['pmax'], name
        assert r['vmin'] >= -1 + 1e-6 and r['vmax'] <= 1 - 1e-9, name


def test_restatement_and_eigh_agree_with_50_digits():
    """``winding_jacobi`` (the kernel's operations) and ``winding`` (eigh, the
    other tests' reference) within 1e-12 relative of ``winding_mp``."""
    refs = vc.winding_refs()
    worst = {'jacobi': (0.0, None), 'eigh': (0.0, None)}
    for name, pts in _wound():
        want = float(refs[name]['winding'])
        for key, got in (('jacobi', ref.winding_jacobi(pts)[0]), ('eigh', ref.winding(pts))):
            worst[key] = max(worst[key], (abs(got / want - 1), name))
    print('worst relative deviation from 50 digits:', worst)
    assert worst['jacobi'][0] <= 1e-12 and worst['eigh'][0] <= 1e-12, worst


def test_all_three_slots_are_dropped():
    slots = {name: ref.winding_jacobi(pts)[1] for name, pts in _wound()}
    assert set(slots.values()) == {0, 1, 2}
    # the copies of the oblique arc under the axis permutations: one slot each
    assert {slots[f'oblique_{k}'] for k in ('xyz', 'yzx', 'zxy')} == {0, 1, 2}
    w = [float(vc.winding_refs()[f'oblique_{k}']['winding']) for k in ('xyz', 'yzx', 'zxy')]
    assert max(w) - min(w) < 1e-3            # the same arc up to float32 rounding


def test_float64_sums_sit_inside_the_bound():
    """The bound the GPU test asserts holds for the NumPy float64 definition
    (another order of summation) on every curve and both linear parts."""
    worst = (0.0, None)
    for lin_name, lin in vc.LINS.items():
        sums = vc.sum_refs(lin_name)
        for name, pts, _ in vc.curves():
            length, d, a = ref.lengths(pts, lin)
            got = dict(zip(vc.QUANTITIES, [length] + list(d) + list(a)))
            for q in vc.QUANTITIES:
                value, scale = vc.sum_reference(sums[name], q)
                bound = vc.sum_bound(len(pts) - 1) * scale
                dev = abs(got[q] - value)
                worst = max(worst, (float(dev / bound), (lin_name, name, q)))
                assert dev <= bound, (lin_name, name, q, float(dev), float(bound))
    print('worst float64 deviation as a multiple of the bound:', worst)


def test_hand_rows_by_hand():
    rows = _hand_rows()
    # the middle point is the centroid: 0 / 0
    assert math.isnan(ref.winding_jacobi(rows['nan'])[0]) and math.isnan(ref.winding(rows['nan']))
    r = ref.winding_mp(rows['nan'])
    assert r['pmin'] == 0 and r['winding'] != r['winding']
    for angle in (0.0, 180.0, 1e300):
        assert not ref.winding_passes(math.nan, angle)
        assert not ref.winding_passes(math.nan, angle, 'non_strict')
    # four turns of exactly 90 degrees, no rotation, slot 2
    w, slot = ref.winding_jacobi(rows['square'])
    assert w == vc.SQUARE_WINDING == 4 * math.acos(0.0) * (180.0 / math.pi) and slot == 2
    assert ref.winding_mp(rows['square'])['winding'] == 360
    assert vc.winding_angles(vc.SQUARE_WINDING)[vc.W_ZERO] == 360.0
    # seven turns between the eight rays, none within a ray
    r = ref.winding_mp(rows['rays'])
    assert abs(r['vmax'] - 1) < 1e-40 and abs(r['winding'] - 465.6548217036) < 1e-9
    assert abs(ref.winding_jacobi(rows['rays'])[0] / float(r['winding']) - 1) < 1e-6


def test_every_winding_mutant_has_a_witness():
    """Each named deviation moves ``winding_jacobi`` outside 1e-9 (relative) of
    ``winding_mp`` on a launched curve, or changes a hand row's answer: a NaN
    for a number, or, for the comparison itself, the square's pass at the mark
    it equals."""
    refs = vc.winding_refs()
    hand = _hand_rows()
    for mutant in ref.WINDING_MUTANTS:
        seen = []
        for name, pts in _wound():
            got = ref.winding_jacobi(pts, mutant)[0]
            if not abs(got / float(refs[name]['winding']) - 1) <= REL:
                seen.append(name)
        for name, pts in hand.items():
            got, want = ref.winding_jacobi(pts, mutant)[0], ref.winding_jacobi(pts)[0]
            if math.isnan(got) != math.isnan(want):
                seen.append(name)
            elif name == 'square' and ref.winding_passes(got, 360.0, mutant) != \
                    ref.winding_passes(want, 360.0):
                seen.append(name)
        print(mutant, len(seen), seen[:3])
        assert seen, mutant
    # the clip and the comparison show nowhere else
    assert ref.winding_jacobi(hand['rays'], 'no_clip')[0] != ref.winding_jacobi(hand['rays'])[0]
    assert ref.winding_passes(360.0, 360.0, 'non_strict') and not ref.winding_passes(360.0, 360.0)


# ----------------------------------------------------------------- GPU tests
def _ruler():
    """The 64 bundles of the ruler on the device, limits to be set per launch."""
    from tracktolearn_amd.experiment.tractometer_validator import ScoringData, limits_table
    head, tail = vc.masks()
    none = [None] * vc.B
    return ScoringData(vc.DIMS, [head] * vc.B, [tail] * vc.B, none, none, none,
                       limits_table(none, none, none, none), DEV)


def _upload(pts):
    """The row and the row reversed (tail to head: the same values)."""
    points, offsets = tc.pack([pts, pts[::-1]])
    return torch.from_numpy(points).to(DEV), torch.from_numpy(offsets).to(DEV)


def _read(data, rows, limits, lin=tc.LIN):
    """(bundle, connected) of one launch of ``rows`` under ``limits``."""
    from tracktolearn_amd.experiment.tractometer_validator import classify
    data.limits = torch.from_numpy(np.ascontiguousarray(limits, np.float64)).to(DEV)
    bundle, connected = classify(rows[0], rows[1], data, lin)
    return bundle.cpu().numpy(), connected.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
def test_winding_between_the_marks():
    """Every curve, in both orders of its ends: ref (1 - 1e-9) <= w < ref (1 +
    1e-9), the margin the exact comparisons of test_tractometer.py rest on.
    The decade each curve reaches is printed, nothing tighter is asserted."""
    data = _ruler()
    refs = vc.winding_refs()
    lo, hi = vc.winding_mark(-REL), vc.winding_mark(REL)
    bad, worst = [], (0.0, None)
    for name, pts in _wound():
        angles = vc.winding_angles(refs[name]['winding'])
        bundle, connected = _read(data, _upload(pts), vc.winding_limits(angles))
        reach = max(vc.winding_reach(int(b)) for b in bundle)
        print(f'{name:18s} n = {len(pts):4d}  bundles {bundle.tolist()}  within {reach:.0e}')
        worst = max(worst, (reach, name))
        assert (connected == FULL).all() and ((bundle >= 0) & (bundle <= vc.B - 1)).all(), name
        if not all(lo < b <= hi for b in bundle):
            bad.append((name, bundle.tolist(), reach))
    print('worst winding deviation (relative, upper mark):', worst)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('lin_name', sorted(vc.LINS))
def test_sums_inside_the_bound(lin_name):
    """Each of the seven quantities of every curve, in both orders of its
    ends, within t = (n + 8) 2^-52 sum |terms| of its value at 50 digits: n - 1
    roundings of an n-term sum in any order and at most eight on the way to a
    term, each relative to a quantity no larger than the term's magnitude."""
    data = _ruler()
    lin = vc.LINS[lin_name]
    sums = vc.sum_refs(lin_name)
    bad, worst = [], (0.0, None)
    for name, pts, _ in vc.curves():
        rows = _upload(pts)
        for q in vc.QUANTITIES:
            value, scale = vc.sum_reference(sums[name], q)
            windows, widths, at = vc.sum_windows(value, scale, len(pts) - 1)
            bundle, connected = _read(data, rows, vc.sum_limits(q, windows), lin)
            assert (connected == FULL).all() and ((bundle >= 0) & (bundle <= vc.B - 1)).all()
            b = int(bundle.max())
            ratio = widths[b] / widths[at] if b < vc.B - 1 else math.inf
            worst = max(worst, (ratio, (name, q)))
            if b > at:
                bad.append((name, q, bundle.tolist(), at, ratio))
        print(f'{name:18s} n = {len(pts):4d}  done')
    print(f'{lin_name}: worst sum deviation as a multiple of the bound (upper mark):', worst)
    assert not bad, bad


@pytest.mark.gpu
def test_hand_rows_at_their_marks():
    data = _ruler()
    rows = _hand_rows()
    # a NaN fails every finite angle, 1e300 included, and passes the bundle that sets none
    angles = vc.winding_angles(180.0)[:-2] + [1e300, math.inf]
    assert angles == sorted(angles) and len(angles) == vc.B
    bundle, connected = _read(data, _upload(rows['nan']), vc.winding_limits(angles))
    assert bundle.tolist() == [vc.B - 1] * 2 and (connected == FULL).all()
    # 360.0 exactly: not below the mark 0, below the next one
    bundle, connected = _read(data, _upload(rows['square']),
                              vc.winding_limits(vc.winding_angles(vc.SQUARE_WINDING)))
    print('square', bundle.tolist())
    assert bundle.tolist() == [vc.W_ZERO + 1] * 2 and (connected == FULL).all()
    # the clip: 465.65 degrees within 1e-6, not a NaN
    want = ref.winding_mp(rows['rays'])['winding']
    bundle, connected = _read(data, _upload(rows['rays']),
                              vc.winding_limits(vc.winding_angles(want)))
    print('rays', bundle.tolist())
    assert all(vc.winding_mark(-1e-6) < b <= vc.winding_mark(1e-6) for b in bundle)
    assert (connected == FULL).all()
