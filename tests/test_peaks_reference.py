"""``k_peaks`` pinned twice.

``ref_peaks.peaks_ordered`` restates the kernel in NumPy float32, operation
for operation in the kernel's order; the library is built without contraction
or fast-math, so the kernel must equal it bit for bit on every voxel (GPU
tests).  ``ref_peaks.peaks_float64`` is the plain definition in float64 with a
per-voxel ``decided`` flag; where it is decisive the restatement must pick its
vertices (CPU tests).  Hand-built dyadic cases, in which nothing rounds, pin
both to literal index lists, and a set of planted mutations shows that the
inputs the GPU test feeds would catch a kernel carrying any of them."""
import functools

import numpy as np
import pytest

import ref_peaks
from ref_peaks import peaks_float64, peaks_ordered
from tracktolearn_amd.reconst import peaks as pk

F32 = np.float32
COS25 = float(F32(np.cos(np.deg2rad(25.0))))


def _cos(deg):
    return float(F32(np.cos(np.deg2rad(deg))))


# ------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def _ico(subdivisions, order):
    verts, nbr = pk.hemisphere(subdivisions)
    B = np.ascontiguousarray(pk.sh_to_sf_matrix(verts, order), F32)
    return B, np.ascontiguousarray(verts, F32), np.ascontiguousarray(nbr, np.int32)


@functools.lru_cache(maxsize=None)
def _fib(n_vertices, degree, order=8):
    verts, nbr = ref_peaks.fibonacci_hemisphere(n_vertices, degree)
    B = np.ascontiguousarray(pk.sh_to_sf_matrix(verts, order), F32)
    return B, np.ascontiguousarray(verts, F32), np.ascontiguousarray(nbr, np.int32)


def _random_sh(n, C, seed):
    """Random smooth fODF-like coefficients, as in tests/test_peaks.py."""
    rng = np.random.RandomState(seed)
    sh = (rng.standard_normal((n, C)) * 0.2).astype(F32)
    sh[:, 0] = 1.0 + rng.uniform(0, 1, n)
    return sh


def _case(sh, tables, npeaks=5, rel=0.1, abs_thr=0.0, cos_sep=COS25, max_candidates=16):
    B, verts, nbr = tables
    return dict(sh=sh, B=B, verts=verts, nbr=nbr, npeaks=npeaks, rel=rel, abs_thr=abs_thr,
                cos_sep=cos_sep, max_candidates=max_candidates)


def _n_coef(order):
    return (order + 1) * (order + 2) // 2


# ------------------------------------------------- hand-built, exact cases
@functools.lru_cache(maxsize=None)
def _dyadic_graph(subdivisions):
    """Icosphere hemisphere with the vertex table rounded to eighths (every
    product and sum of the separation test is then exact) and B = identity."""
    verts, nbr = pk.hemisphere(subdivisions)
    q = (np.round(verts * 8.0) / 8.0).astype(F32)
    return np.eye(len(q), dtype=F32), q, np.ascontiguousarray(nbr, np.int32)


def _field(V, background, values):
    sf = np.full((1, V), background, F32)
    for v, x in values.items():
        sf[0, v] = x
    return sf


def _hand_cases():
    """name -> (case, expected index list).  hemisphere(1) has 21 vertices;
    0..5 are mutually non-adjacent, 10 / 14 / 20 are mutually orthogonal and
    non-adjacent, 3 and 14 are adjacent (cos 56/64), 0 and 19 are not adjacent
    with cos -34/64, 4 and 14 are not adjacent with cos exactly 32/64, 4 and
    10 are orthogonal.  Values are small integers or dyadic, the first value
    a power of two, so value / first and the scaled coordinates are exact."""
    g1 = _dyadic_graph(1)
    hand = functools.partial(_case, tables=g1, rel=0.25, cos_sep=0.5)
    cases = {}
    # two adjacent equal maxima: both are >= all and > some neighbour
    cases['plateau_adjacent'] = (hand(_field(21, 1, {3: 4, 14: 4}), cos_sep=1.0), [3, 14])
    # two distant equal maxima: lowest index first
    cases['distant_equal'] = (hand(_field(21, 1, {10: 4, 14: 4})), [10, 14])
    # odf_min 8, norms 8 / 2 / 1.5, cut 0.25 * 8 = 2: vertex 14 sits on it
    cases['at_relative_cut'] = (hand(_field(21, 8, {10: 16, 14: 10, 20: 9.5})), [10, 14])
    # background 1 < abs is zeroed, vertex 14 sits on abs and stays
    cases['at_absolute'] = (hand(_field(21, 1, {10: 4, 14: 2}), abs_thr=2.0), [10, 14])
    cases['all_equal'] = (hand(_field(21, 2, {})), [])
    neg = -(1.0 + np.arange(21) % 3).astype(F32)[None, :]
    neg[0, 14] = 4
    cases['negative_but_one'] = (hand(neg.copy()), [14])
    # negative values kept (abs -8) and let through the cut (rel -4): only
    # the positive maximum is a peak; the -1 maxima among -2 / -3 are not
    cases['negative_maxima_kept'] = (hand(neg.copy(), abs_thr=-8.0, rel=-4.0, cos_sep=1.0), [14])
    # min -8 clamps to 0: norm 2 < 0.5 * 8 (unclamped: 10 >= 8)
    cases['min_clamped'] = (hand(_field(21, -8, {10: 8, 14: 2}), abs_thr=-8.0, rel=0.5), [10])
    # +1 -1: a field with a maximum, but sum(coefs) == 0 means no signal
    cases['plus_minus'] = (hand(_field(21, 0, {0: 1, 1: -1})), [])
    one = (np.eye(1, dtype=F32), np.array([[0, 0, 1]], F32), np.zeros((1, 1), np.int32))
    cases['single_vertex'] = (_case(np.full((1, 1), 2, F32), one, rel=0.25, cos_sep=0.5), [])
    # cos(0, 19) = -34/64: only |cos| > 1/2 rejects 19
    cases['antipodal_side'] = (hand(_field(21, 1, {0: 4, 19: 2})), [0])
    # 4 is within cos 1/4 of the second peak (32/64), orthogonal to the first
    cases['third_near_second'] = (hand(_field(21, 1, {10: 8, 14: 4, 4: 2}), rel=0.125,
                                       cos_sep=0.25), [10, 14])
    # the same at cos_sep = 32/64 exactly: not closer than the limit, kept
    cases['separation_equal'] = (hand(_field(21, 1, {10: 8, 14: 4, 4: 2}), rel=0.125), [10, 14, 4])
    six = _field(21, 1, {0: 16, 1: 14, 2: 12, 3: 10, 4: 8, 5: 6})
    cases['many_survivors'] = (hand(six, rel=0.125, cos_sep=1.0), [0, 1, 2, 3, 4])
    cases['many_survivors_3'] = (hand(six, rel=0.125, cos_sep=1.0, npeaks=3), [0, 1, 2])
    # hemisphere(2), 81 vertices: a maximal set of mutually non-adjacent
    # vertices (80, 78, 75, 72, 70, 68, ...), values 32, 31, ... in the order
    # 80, 78, 75, 72, 68, 70, ..., 60 degrees, max_candidates = npeaks = 5:
    # the five candidates examined are 80, 78, 75, 72, 68, of which 78 and 72
    # fall to the separation test against 80 (cos -54/64, 56/64); without
    # the cap the search goes on to 25
    g2 = _dyadic_graph(2)
    cases['cap_bites'] = (_case(_cap_field(), g2, rel=0.0, cos_sep=0.5, max_candidates=5),
                          CAP_EXPECTED)
    return cases


def _cap_field():
    _, _, nbr = _dyadic_graph(2)
    chosen = []
    for v in range(80, -1, -1):
        if not any(v in nbr[w] for w in chosen):
            chosen.append(v)
    assert chosen[:6] == [80, 78, 75, 72, 70, 68]
    chosen[4], chosen[5] = chosen[5], chosen[4]
    return _field(81, 1, {v: 32 - k for k, v in enumerate(chosen)})


CAP_EXPECTED = [80, 75, 68]
CAP_EXPECTED_UNLIMITED = [80, 75, 68, 25]


@functools.lru_cache(maxsize=None)
def hand_cases():
    return _hand_cases()


def _literal_output(case, expected):
    """The output the literal index list stands for (exact in float32)."""
    sf = case['sh'][0] @ case['B']                     # identity: exact
    out = np.zeros((case['npeaks'], 3), F32)
    for j, v in enumerate(expected):
        out[j] = case['verts'][v] * F32(sf[v] / sf[expected[0]])
    return out.reshape(1, -1)


def _padded(expected, npeaks):
    return np.array([list(expected) + [-1] * (npeaks - len(expected))], np.int64)


# ------------------------------------------- CPU: restatement vs float64
ORDERS = (2, 4, 6, 8, 10, 12)


def _random_inputs():
    """name -> case: about 500 voxels each.  Separation angles stay off 45
    degrees: the icosphere has vertex pairs at exactly that angle, which the
    float64 definition cannot decide (the bit-exact GPU test feeds 45)."""
    inputs = {}
    for order in ORDERS:
        inputs[f'ico3_order{order}'] = _case(_random_sh(500, _n_coef(order), order),
                                             _ico(3, order))
    inputs['ico1_order8'] = _case(_random_sh(500, 45, 21), _ico(1, 8))
    inputs['ico2_order8'] = _case(_random_sh(500, 45, 81), _ico(2, 8))
    inputs['ico3_abs'] = _case(_random_sh(500, 45, 31), _ico(3, 8), abs_thr=0.15)
    inputs['ico3_rel'] = _case(_random_sh(500, 45, 32), _ico(3, 8), rel=0.5)
    inputs['ico3_sep15'] = _case(_random_sh(500, 45, 33), _ico(3, 8), cos_sep=_cos(15.0))
    return inputs


RANDOM_INPUTS = tuple(f'ico3_order{o}' for o in ORDERS) + (
    'ico1_order8', 'ico2_order8', 'ico3_abs', 'ico3_rel', 'ico3_sep15')
UNDECIDED_CAP = 0.05


@pytest.mark.parametrize('name', RANDOM_INPUTS)
def test_ordered_restatement_picks_the_float64_peaks(name):
    """On decided voxels the float32 restatement picks the vertices of the
    float64 definition in the same order, its output within
    (tau_v + tau_first * val / first) / first + 2^-23 per component; at most
    5 % of the voxels may be undecided (measured: DESIGN section 9)."""
    case = _random_inputs()[name]
    idx32, out32 = peaks_ordered(**case)
    idx64, out64, decided = peaks_float64(**case)
    share = 1.0 - decided.mean()
    print(f'{name}: {100 * share:.2f} % of {len(decided)} voxels undecided')
    assert share <= UNDECIDED_CAP, f'{name}: {100 * share:.2f} % undecided'
    assert (idx64[decided, 0] >= 0).mean() > 0.9           # the input has peaks
    wrong = np.flatnonzero(decided & (idx32 != idx64).any(axis=1))
    assert len(wrong) == 0, (name, wrong[:5], idx32[wrong[:5]], idx64[wrong[:5]])
    bound = np.repeat(ref_peaks.output_bound(case['sh'], case['B'], idx64), 3, axis=1)
    err = np.abs(out32.astype(np.float64) - out64)
    assert np.all(err[decided] <= bound[decided]), (name, (err - bound)[decided].max())


HAND_NAMES = ('plateau_adjacent', 'distant_equal', 'at_relative_cut', 'at_absolute', 'all_equal',
              'negative_but_one', 'negative_maxima_kept', 'min_clamped', 'plus_minus',
              'single_vertex', 'antipodal_side', 'third_near_second', 'separation_equal',
              'many_survivors', 'many_survivors_3', 'cap_bites')


def test_hand_names_are_complete():
    assert set(HAND_NAMES) == set(hand_cases())


@pytest.mark.parametrize('name', HAND_NAMES)
def test_hand_built_cases_equal_their_literals(name):
    """Exact arithmetic: both references give the index list written out in
    ``_hand_cases`` and the output it stands for, every voxel decided."""
    case, expected = hand_cases()[name]
    want_idx = _padded(expected, case['npeaks'])
    want_out = _literal_output(case, expected)
    idx32, out32 = peaks_ordered(**case)
    idx64, out64, decided = peaks_float64(**case, exact=True)
    assert decided.all()
    assert np.array_equal(idx32, want_idx), (idx32, want_idx)
    assert np.array_equal(idx64, want_idx), (idx64, want_idx)
    assert np.array_equal(out32, want_out)
    assert np.array_equal(out64, want_out.astype(np.float64))


def test_exact_mode_refuses_inputs_that_round():
    """``exact=True`` decides a voxel only where float32 loses nothing: a
    second value of 2 against a first of 3 (2 / 3 rounds) and a non-dyadic
    vertex table (the dot product rounds) are both undecided."""
    g1 = _dyadic_graph(1)
    thirds = _case(_field(21, 1, {10: 3, 14: 2}), g1, rel=0.25, cos_sep=0.5)
    assert not peaks_float64(**thirds, exact=True)[2].any()
    B, _, nbr = g1
    field = _field(21, 1, {0: 4, 19: 2})
    rough = _case(field, (B, _ico(1, 8)[1], nbr), rel=0.25, cos_sep=0.5)
    assert not peaks_float64(**rough, exact=True)[2].any()
    assert peaks_float64(**_case(field, g1, rel=0.25, cos_sep=0.5), exact=True)[2].all()


def test_the_candidate_cap_changes_the_selection():
    """max_candidates is part of the contract, not of dipy: on 'cap_bites'
    the capped and the unlimited (dipy) selection differ.  Random fields at
    25 degrees do not cover it: a cap of 16 changes no voxel of them, at any
    order of ``ORDERS``."""
    case, expected = hand_cases()['cap_bites']
    unlimited = dict(case, max_candidates=None)
    idx_cap, _, _ = peaks_float64(**case, exact=True)
    idx_all, _, _ = peaks_float64(**unlimited, exact=True)
    assert idx_cap[0].tolist() == CAP_EXPECTED + [-1, -1]
    assert idx_all[0].tolist() == CAP_EXPECTED_UNLIMITED + [-1]
    assert np.array_equal(peaks_ordered(**dict(case, max_candidates=81))[0], idx_all)
    for order in ORDERS:
        random = _random_inputs()[f'ico3_order{order}']
        assert np.array_equal(peaks_float64(**random)[0],
                              peaks_float64(**dict(random, max_candidates=None))[0]), order


# ------------------------------------------------- the inputs discriminate
#: mutation -> the input of the GPU test (a hand-built case) that catches it
CAUGHT_BY = {
    'max_ge_to_gt': 'plateau_adjacent',
    'no_gt_any': 'all_equal',
    # x > 0 is observable only where negative values survive the absolute
    # threshold and the relative cut (abs < 0, rel < 0): for abs >= 0 every
    # value is >= 0, for rel >= 0 a negative candidate fails the cut
    'no_positive': 'negative_maxima_kept',
    'ties_highest': 'distant_equal',
    'min_unclamped': 'min_clamped',
    'min_not_subtracted': 'at_relative_cut',
    'rel_ge_to_gt': 'at_relative_cut',
    'abs_lt_to_le': 'at_absolute',
    'sep_no_fabs': 'antipodal_side',
    'sep_gt_to_ge': 'separation_equal',
    'sep_first_only': 'third_near_second',
    'scale_first_norm': 'at_relative_cut',
    'drop_last_lane_group': 'cap_bites',
    'drop_coef_64': 'cap_bites',
    'cap_minus_one': 'cap_bites',
    'signal_abs_sum': 'plus_minus',
}


def test_every_mutation_is_listed():
    assert set(CAUGHT_BY) == set(ref_peaks.MUTATIONS)


@pytest.mark.parametrize('mutation', ref_peaks.MUTATIONS)
def test_mutations_are_caught_by_a_gpu_input(mutation):
    """A kernel carrying ``mutation`` would give the mutated restatement's
    output on the named input, which differs from the unmutated one (so the
    bit-equality GPU test fails) and from the literals / the float64
    definition on a decided voxel (so it is the mutation that is wrong)."""
    case, expected = hand_cases()[CAUGHT_BY[mutation]]
    assert CAUGHT_BY[mutation] in GPU_CASES
    idx, out = peaks_ordered(**case)
    midx, mout = peaks_ordered(**case, mutate=mutation)
    assert not np.array_equal(out.view(np.uint32), mout.view(np.uint32)), mutation
    idx64, out64, decided = peaks_float64(**case, exact=True)
    assert decided.all() and np.array_equal(idx64, _padded(expected, case['npeaks']))
    assert not np.array_equal(mout.astype(np.float64), out64), mutation
    assert not np.array_equal(mout, _literal_output(case, expected)), mutation


#: the random GPU inputs built for the two block faults catch them as well
ALSO_CAUGHT_BY = {
    'drop_coef_64': ('ico3_order12', 'ico2_order16'),
    'drop_last_lane_group': ('fib65', 'fib767', 'ico1_order8'),
}


@pytest.mark.parametrize('mutation, name', [(m, n) for m, names in ALSO_CAUGHT_BY.items()
                                            for n in names])
def test_block_mutations_are_caught_by_the_random_gpu_inputs(mutation, name):
    """The mutated restatement differs from the unmutated one on the input,
    and on a voxel the float64 definition decides it picks other vertices
    than that definition."""
    case = GPU_CASES[name]()
    idx, out = peaks_ordered(**case)
    midx, mout = peaks_ordered(**case, mutate=mutation)
    assert not np.array_equal(out.view(np.uint32), mout.view(np.uint32))
    idx64, _, decided = peaks_float64(**case)
    assert (decided & (midx != idx64).any(axis=1)).any()
    assert not (decided & (idx != idx64).any(axis=1)).any()


# ---------------------------------------------------------------- GPU tests
#: npeaks, max_candidates, abs, rel, separation in degrees: npeaks {1, 3, 8} x
#: max_candidates {npeaks, 64}, abs 0.15, rel {0, 0.5, 1}, 0 / 45 / 60 / 90 degrees
PARAMS = ((1, 1, 0.0, 0.0, 0.0), (1, 64, 0.15, 0.5, 45.0), (3, 3, 0.0, 0.0, 45.0),
          (3, 64, 0.15, 0.0, 60.0), (8, 8, 0.0, 0.0, 0.0), (8, 64, 0.0, 0.0, 45.0),
          (8, 8, 0.15, 0.5, 45.0), (8, 64, 0.15, 0.0, 60.0), (3, 3, 0.0, 1.0, 25.0),
          (3, 64, 0.0, 0.5, 90.0), (8, 64, 0.0, 0.0, 90.0), (1, 64, 0.15, 1.0, 0.0))


def _param_case(k):
    """The parameter sweep on hemisphere(3), order 8."""
    npeaks, cap, abs_thr, rel, sep = PARAMS[k]
    return _case(_random_sh(200, 45, 100 + k), _ico(3, 8), npeaks=npeaks, max_candidates=cap,
                 abs_thr=abs_thr, rel=rel, cos_sep=_cos(sep))


def _voxel_count_case(n):
    """n voxels on hemisphere(3), order 8.  The grid caps at 1024 workgroups
    of four waves: from 4097 voxels on a wave takes a second voxel and reuses
    its LDS row, so no-signal voxels sit at i with signal at i + 4096 (i % 3
    == 0) and the other way round (i % 3 == 1).  Below that one voxel has no
    signal; a single voxel has signal."""
    sh = _random_sh(n, 45, 1000 + n)
    i = np.arange(n)
    if n >= 4096:
        sh[(i < 4096) & (i % 3 == 0)] = 0
        sh[(i >= 4096) & (i % 3 == 1)] = 0
    elif n > 1:
        sh[n // 2] = 0                 # one voxel without signal, n = 1 keeps its signal
    return _case(sh, _ico(3, 8))


#: V -> degree, npeaks, max_candidates, abs, rel, separation in degrees
FIB = {1: (1, 3, 3, 0.0, 0.1, 25.0), 63: (6, 8, 64, 0.0, 0.0, 45.0),
       64: (12, 3, 3, 0.15, 0.0, 60.0), 65: (1, 3, 64, 0.0, 0.1, 0.0),
       128: (6, 8, 8, 0.0, 0.0, 25.0), 640: (12, 5, 64, 0.15, 0.1, 45.0),
       767: (1, 8, 64, 0.0, 0.0, 60.0), 768: (6, 8, 64, 0.0, 0.0, 25.0)}


def _fib_case(V):
    """Fibonacci half-sphere, C = 45 (at V = 768 the LDS is 147 of the 160
    KB), k-nearest-neighbour tables of degree 1 / 6 / 12 (the row padded with
    the vertex itself at V = 1)."""
    degree, npeaks, cap, abs_thr, rel, sep = FIB[V]
    return _case(_random_sh(96, 45, 2000 + V), _fib(V, degree), npeaks=npeaks,
                 max_candidates=cap, abs_thr=abs_thr, rel=rel, cos_sep=_cos(sep))


def _gpu_cases():
    cases = {}
    for order in (2, 8, 12):                       # C = 6, 45, 91
        cases[f'ico3_order{order}'] = lambda o=order: _case(
            _random_sh(500, _n_coef(o), o), _ico(3, o))
    cases['ico2_order16'] = lambda: _case(_random_sh(300, 153, 16), _ico(2, 16))   # C = 153
    cases['ico1_order8'] = lambda: _case(_random_sh(300, 45, 21), _ico(1, 8))
    for V in FIB:
        cases[f'fib{V}'] = lambda V=V: _fib_case(V)
    for n in (1, 3, 5, 4096, 8195):
        cases[f'voxels{n}'] = lambda n=n: _voxel_count_case(n)
    for k in range(len(PARAMS)):
        cases[f'params{k}'] = lambda k=k: _param_case(k)
    for name in HAND_NAMES:
        cases[name] = lambda name=name: hand_cases()[name][0]
    return cases


GPU_CASES = _gpu_cases()


def _launch(case, n_voxels=None, **override):
    """``ttl_peaks_from_sh`` through the C ABI on a NaN-filled output:
    (return code, output [n][3 * npeaks])."""
    import ctypes as C

    import torch

    from tracktolearn_amd import _lib
    lib = _lib.load()
    a = dict(case, **override)
    dev = torch.device('cuda')
    sh = torch.from_numpy(np.ascontiguousarray(a['sh'], F32)).to(dev)
    B = torch.from_numpy(np.ascontiguousarray(a['B'], F32)).to(dev)
    verts = torch.from_numpy(np.ascontiguousarray(a['verts'], F32)).to(dev)
    nbr = torch.from_numpy(np.ascontiguousarray(a['nbr'], np.int32)).to(dev)
    n = sh.shape[0] if n_voxels is None else n_voxels
    out = torch.full((sh.shape[0], 3 * max(a['npeaks'], 1)), float('nan'), dtype=torch.float32,
                     device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.ttl_peaks_from_sh(
        sh.data_ptr(), n, a.get('n_coef', B.shape[0]), B.data_ptr(), verts.data_ptr(),
        nbr.data_ptr(), a.get('n_vertices', B.shape[1]), a.get('degree', nbr.shape[1]),
        a['npeaks'], float(a['rel']), float(a['abs_thr']), float(a['cos_sep']),
        int(a['max_candidates']), out.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GPU_CASES))
def test_hip_peaks_equal_the_ordered_restatement(name):
    """Bit equality on every voxel of every input, no share left out."""
    case = GPU_CASES[name]()
    rc, got = _launch(case)
    assert rc == 0
    idx, want = peaks_ordered(**case)
    assert got.shape == want.shape
    differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(differ) == 0, (name, len(differ), differ[:5], got[differ[:2]], want[differ[:2]])
    assert np.array_equal(got, want)
    if name in HAND_NAMES:
        assert np.array_equal(got, _literal_output(case, hand_cases()[name][1]))
    if name.startswith(('ico', 'voxels', 'params', 'fib')) and name != 'fib1':
        assert (idx[:, 0] >= 0).mean() > 0.5               # the input has peaks


WRAPPER_KW = dict(npeaks=3, relative_threshold=0.6, absolute_threshold=0.1,
                  min_separation_angle=50.0, subdivisions=2, max_candidates=7)


def _wrapper_case():
    """The wrapper test's field and the restatement's arguments for WRAPPER_KW."""
    sh = _random_sh(7 * 5 * 3, 45, 77)
    return sh, _case(sh, _ico(2, 8), npeaks=3, rel=0.6, abs_thr=0.1, cos_sep=_cos(50.0),
                     max_candidates=7)


def test_wrapper_input_has_full_and_short_peak_lists():
    """The wrapper test's input fills the third slot in some voxels and leaves
    it empty in others, so both the packing and the -1 fill are exercised."""
    idx, _ = peaks_ordered(**_wrapper_case()[1])
    assert (idx[:, 1] >= 0).any() and (idx[:, 2] >= 0).any() and (idx[:, 2] < 0).any()


@pytest.mark.gpu
def test_hip_peaks_wrapper_with_other_arguments():
    """``peaks.peaks_from_sh`` with every keyword argument off its default
    builds the tables and the cosine the restatement is given."""
    import torch
    sh, case = _wrapper_case()
    got = pk.peaks_from_sh(torch.from_numpy(sh.reshape(7, 5, 3, 45)).cuda(),
                           **WRAPPER_KW).cpu().numpy()
    idx, want = peaks_ordered(**case)
    assert got.shape == (7, 5, 3, 9)
    assert np.array_equal(got.reshape(-1, 9).view(np.uint32), want.view(np.uint32))
    assert (idx[:, 1] >= 0).any() and (idx[:, 2] < 0).any()


REFUSED = {
    'V=769': dict(n_vertices=769),
    'npeaks=9': dict(npeaks=9, max_candidates=16),
    'max_candidates<npeaks': dict(npeaks=5, max_candidates=4),
    'C*V over the LDS': dict(n_coef=153, n_vertices=321),
    'degree=0': dict(degree=0),
    'n_voxels=0': dict(),
}


@pytest.mark.gpu
@pytest.mark.parametrize('what', list(REFUSED))
def test_hip_peaks_refusals(what):
    """Refused with ERR_INVALID before any launch: the output stays as it was.
    (The buffers are large enough for the refused sizes.)"""
    from tracktolearn_amd import _lib
    V = 769 if what == 'V=769' else 321
    C = 153 if what == 'C*V over the LDS' else 45
    tables = (np.zeros((C, V), F32), np.zeros((V, 3), F32), np.zeros((V, 6), np.int32))
    case = _case(np.ones((4, C), F32), tables, npeaks=9 if what == 'npeaks=9' else 5)
    rc, out = _launch(case, n_voxels=0 if what == 'n_voxels=0' else None, **REFUSED[what])
    assert rc == _lib.ERR_INVALID, (what, rc)
    assert np.isnan(out).all()
