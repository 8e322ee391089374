"""Streamline registration (include/ttl_hip.h, ttl_bundle_register_cost; DESIGN
3.20): on the CPU a hand-computed case, a witness for every named mutant, the
transforms of ``compose`` by hand, the header, the refusals, the Python layer's
argument checks, the command's options, and the driver on the reference's
``evaluate`` recovering a planted transform; on the GPU the kernel against the
reference (row_min and col_min inside the reference's intervals on every entry,
NaN patterns exactly, the cost within its bound), the same bits whatever the
order of the lines or the split of the transforms, the agreement with
ttl_bundle_recognize under the identity, and register -> recognise end to end.

Figures of the recovery case (3 bundles of 10 lines, 6 distractors, K = 12, jitter
0.5 mm) with the driver's defaults on the reference's float64 ``evaluate``:
rigid 0.15 mm, cost 9.961 found against 9.976 at the plant, 37 evaluations;
affine 0.22 mm, 10.507 against 10.558, 100 evaluations; 30 % / 33 % of the labels
wrong before the fit, none at the plant.  On the GPU through ``register_atlas``
(stations from the library's resampler): rigid 0.15 mm, 9.274 against 9.290, 45
evaluations; affine 0.42 mm, 9.865 against 9.970, 121 evaluations."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bundle_register_cases as cases
import ref_bundle_register as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
I64 = np.int64
LD = ref.LD
CAP_MM = 2 * cases.SIGMA                        # condition (b): 2 sigma = 1 mm


def f64(v):
    return np.asarray(v, np.float64)


def _ref(c, mutant=None):
    return ref.cost(c['fixed'], c['moving'], c['xf'], c['lin'], mutant)


# ------------------------------------------------------------------ CPU part
def test_two_lines_by_hand():
    """2 mm voxels, K = 3.  Identity: every fixed line has a moving line 1 voxel
    = 2 mm away (fixed line 1 read backwards), so both means are 2 and the cost is
    (2 + 2)^2 / 4 = 4.  Shift by +1 voxel in x: moving line 0 falls on fixed line
    0, moving line 1 is (1, 1) voxels = 2 sqrt 2 mm from fixed line 1 read
    backwards: both means sqrt 2, the cost (2 sqrt 2)^2 / 4 = 2."""
    got = _ref(cases.hand())
    r2 = float(2 * np.sqrt(LD(2)))
    assert f64(got['row_min']).tolist() == [[2.0, 2.0], [0.0, r2]]
    assert f64(got['col_min']).tolist() == [[2.0, 2.0], [0.0, r2]]
    assert float(got['cost'][0]) == 4.0 and abs(float(got['cost'][1]) - 2.0) < 1e-15
    delta = ref.table(cases.hand()['fixed'], cases.hand()['moving'], np.eye(4)[:3],
                      np.diag([2.0, 2.0, 2.0]))[0]
    assert f64(delta).tolist() == [[2.0, 8.0], [float(2 * np.sqrt(LD(10))), 2.0]]
    for k, lo, hi in (('row_min', 'row_lo', 'row_hi'), ('col_min', 'col_lo', 'col_hi')):
        assert (got[lo] <= got[k]).all() and (got[k] <= got[hi]).all()
    assert (got['cost_bound'] < 1e-13).all()


def test_identity_distances_are_the_recognise_references():
    c = cases.case(20, 9, 65, 25, 'oblique')
    delta = ref.table(c['fixed'], c['moving'], np.eye(4)[:3], c['lin'])[0]
    for i in (0, 3, 8):
        a = c['fixed'][i]
        D = ref.pair_distances(a, c['moving'], c['lin']).sum(1) / LD(c['K'])
        F = ref.pair_distances(a[::-1], c['moving'], c['lin']).sum(1) / LD(c['K'])
        want = np.minimum(D, F)
        want[[c['special']['moving_nan'], c['special']['moving_inf']]] = np.nan
        assert np.array_equal(delta[i], want, equal_nan=True)
    assert np.isnan(f64(delta[c['special']['fixed_nan']])).all()


WITNESS = {'one_sided': 'cost', 'no_flip': 'row_min', 'unsquared': 'cost', 'no_quarter': 'cost',
           'distance_in_voxels': 'row_min', 'transforms_fixed_set': 'col_min',
           'transposed_matrix': 'row_min', 'translation_first': 'col_min',
           'nan_line_counts_as_zero': 'row_min', 'mean_over_all_lines': 'cost',
           'first_transform_for_all_t': 'row_min', 'col_min_over_own_block_only': 'col_min'}


def _outside(good, bad, key):
    """Entries of ``bad[key]`` a check against ``good`` rejects: another NaN
    pattern, a minimum outside its interval, a cost beyond its bound."""
    with np.errstate(all='ignore'):
        if key == 'cost':
            return np.flatnonzero(~(np.abs(bad['cost'] - good['cost']) <= good['cost_bound']))
        lo, hi = good[key[:3] + '_lo'], good[key[:3] + '_hi']
        nan_g, nan_b = np.isnan(f64(good[key])), np.isnan(f64(bad[key]))
        return np.argwhere((nan_g != nan_b) | (~nan_g & ~nan_b & ((bad[key] < lo) |
                                                                   (bad[key] > hi))))


def test_every_mutant_is_named_once():
    assert set(WITNESS) == set(ref.MUTANTS) and len(ref.MUTANTS) == 12


def test_the_witness_case_by_the_definition():
    w = cases.witness()
    good = _ref(w)
    assert np.isnan(f64(good['row_min'][:, 1])).all() and np.isnan(f64(good['col_min'][:, 2])).all()
    assert not np.isnan(f64(np.delete(good['row_min'], 1, 1))).any()
    assert not np.isnan(f64(good['cost'])).any()
    for key in ('row_min', 'col_min', 'cost'):
        assert len(_outside(good, good, key)) == 0
    # fixed line 8, behind the first workgroup's 8, is the nearest of moving line 1
    delta = ref.table(w['fixed'], w['moving'], w['xf'][1], w['lin'])[0]
    assert np.nanargmin(f64(delta[:, 1])) == 8


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_mutants_have_a_witness(mutant):
    w = cases.witness()
    assert len(_outside(_ref(w), _ref(w, mutant), WITNESS[mutant])) > 0


def test_compose_by_hand():
    from tracktolearn_amd.bundle_register import compose
    zero = np.zeros(3)
    got = compose([1, 2, 3], 'translation', zero)
    assert np.array_equal(got, [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    got = compose([0, 0, 0, 0, 0, 90], 'rigid', zero)
    assert np.allclose(got[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    got = compose([0, 0, 0, 90, 0, 90], 'rigid', zero)          # Rz Rx: x first
    assert np.allclose(got[:3, :3], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-15)
    got = compose([0, 0, 0, 0, 90, 0], 'rigid', zero)
    assert np.allclose(got[:3, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)
    got = compose([0, 0, 0, 0, 0, 90, 2], 'similarity', zero)
    assert np.allclose(got[:3, :3], [[0, -2, 0], [2, 0, 0], [0, 0, 2]], atol=1e-15)
    got = compose([0, 0, 0, 0, 0, 0, 2, 3, 4, 0.5, 0.25, -1], 'affine', zero)
    assert np.array_equal(got[:3, :3], [[2, 1.5, 1], [0, 3, -4], [0, 0, 4]])    # H diag(s)
    assert np.array_equal(got[:, 3], [0, 0, 0, 1]) and got.dtype == np.float64
    for bad, word in ((([1, 2], 'translation', zero), r'\(3,\)'),
                      (([0] * 7, 'rigid', zero), r'\(6,\)'),
                      (([0] * 6, 'similarity', zero), r'\(7,\)'),
                      (([0] * 6, 'affine', zero), r'\(12,\)'),
                      (([0] * 6, 'shear', zero), 'kind')):
        with pytest.raises(ValueError, match=word):
            compose(*bad)


def test_compose_about_a_centre_and_to_voxel_round_trip():
    """x' = A (x - c) + c + t: a quarter turn about z through c = (1, 2, 3) and t
    = (10, 0, 0) sends c to c + t; the translation column is c + t - A c = (13, 1,
    0)."""
    from tracktolearn_amd.bundle_register import compose, from_voxel, to_mm, to_voxel
    got = compose([10, 0, 0, 0, 0, 90], 'rigid', [1, 2, 3])
    assert np.allclose(got[:3, 3], [13, 1, 0], atol=1e-14)
    assert np.allclose(got @ [1, 2, 3, 1], [11, 2, 3, 1], atol=1e-14)
    affine = np.array([[1.5, 0.25, -0.5, -20], [-0.375, 1.25, 0.5, 7], [0.25, -0.75, 2.0, 3],
                       [0, 0, 0, 1.0]])
    m = compose([3, -2, 1, 10, 20, -30, 1.1, 0.9, 1.2, 0.1, -0.2, 0.05], 'affine', [4, 5, 6])
    v = to_voxel(m, affine)
    assert v.shape == (3, 4) and v.dtype == np.float64
    assert np.allclose(from_voxel(v, affine), m, rtol=0, atol=1e-12)
    # the voxel form moves voxel coordinates as the matrix moves their mm
    vox = np.array([[0.5, 0.5, 0.5], [3.25, 1.0, 7.5]])
    mm = to_mm(vox, affine)
    assert np.allclose(mm[0], affine[:3, 3])            # the first voxel's centre
    assert np.allclose(to_mm(vox @ v[:, :3].T + v[:, 3], affine),
                       mm @ m[:3, :3].T + m[:3, 3], rtol=0, atol=1e-12)
    assert np.array_equal(to_voxel(np.eye(4), np.diag([2.0, 2.0, 2.0, 1.0])), np.eye(4)[:3])


def test_header_announces_the_feature_and_keeps_the_abi():
    from tracktolearn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'^#define TTL_HAS_BUNDLE_REGISTER 1$', header, re.M)
    assert re.search(r'^#define TTL_REGISTER_MAX_TRANSFORMS 64$', header, re.M)
    assert re.search(r'^#define TTL_REGISTER_MAX_LINES 1048576$', header, re.M)
    assert re.search(r'^#define TTL_ABI_VERSION 13$', header, re.M)
    assert header.index('TTL_HAS_BUNDLE_RECOGNIZE 1') < header.index('TTL_HAS_BUNDLE_REGISTER 1')
    assert (_lib.HAS_BUNDLE_REGISTER, _lib.REGISTER_MAX_TRANSFORMS, _lib.REGISTER_MAX_LINES,
            _lib.ABI_VERSION) == (1, 64, 1048576, 13)
    lib = _lib.load()
    name = 'ttl_bundle_register_cost'
    assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert re.search(r'^TTL_API int ' + name + r'\(', header, re.M)
    from tracktolearn_amd.csrc import build
    assert any(s.endswith('ttl_bundle_register.hip') for s in build.SOURCES)


def _args():
    p = C.c_void_p(4096)                # never dereferenced: every call here is refused
    return dict(fixed=p, n_fixed=110, moving=p, n_moving=90, nb_points=20, xf=p, n_xf=25,
                lin=(C.c_double * 9)(*np.eye(3).reshape(-1)), row_min=p, col_min=p, cost=p,
                stream=None)


INVALID = [(k, None) for k in ('fixed', 'moving', 'xf', 'lin', 'row_min', 'col_min', 'cost')] + \
    [('n_fixed', 0), ('n_fixed', 1048577), ('n_moving', 0), ('n_moving', 1048577), ('n_xf', 0),
     ('n_xf', 65), ('nb_points', 1), ('nb_points', 257), ('n_fixed', -1)]


def test_refusals_come_before_any_hip_call():
    """On a machine without a GPU a HIP call would answer TTL_ERR_HIP."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    for key, value in INVALID:
        rc = lib.ttl_bundle_register_cost(*dict(_args(), **{key: value}).values())
        assert rc == _lib.ERR_INVALID, (key, value)
        assert b'ttl_bundle_register_cost' in lib.ttl_last_error()


def test_python_layer_refuses_with_the_shape_wanted():
    import torch
    from tracktolearn_amd.bundle_register import bundle_register_cost, register
    fixed = torch.zeros((4, 5, 3), dtype=torch.float32)
    moving = torch.zeros((6, 5, 3), dtype=torch.float32)
    xf = torch.zeros((2, 3, 4), dtype=torch.float64)
    lin = np.eye(3)
    for bad, word in (((fixed.double(), moving, xf, lin), r'\(A, K, 3\) float32'),
                      ((fixed[:, :, :2].contiguous(), moving, xf, lin), r'\(A, K, 3\)'),
                      ((fixed, moving.double(), xf, lin), r'\(B, 5, 3\) float32'),
                      ((fixed, moving[:, :4].contiguous(), xf, lin), r'\(B, 5, 3\)'),
                      ((fixed[:0], moving, xf, lin), '1 .. 1048576 lines'),
                      ((fixed[:, :1].contiguous(), moving[:, :1].contiguous(), xf, lin),
                       '2 .. 256 stations'),
                      ((fixed, moving, xf.float(), lin), r'\(T, 3, 4\) float64'),
                      ((fixed, moving, xf.reshape(2, 4, 3), lin), r'\(T, 3, 4\)'),
                      ((fixed, moving, torch.zeros((65, 3, 4), dtype=torch.float64), lin),
                       '1 .. 64 transforms'),
                      ((fixed, moving, xf[:0], lin), '1 .. 64 transforms'),
                      ((fixed, moving, xf, np.eye(4)), r'\(3, 3\)')):
        with pytest.raises(ValueError, match=word):
            bundle_register_cost(*bad)
    affine = np.diag([2.0, 2.0, 2.0, 1.0])
    nothing = lambda mats: np.zeros(len(mats))
    for args, kw, word in (((fixed.numpy(), moving.numpy()[:, :4], affine), {}, r'\(B, K, 3\)'),
                           ((fixed.numpy(), moving.numpy(), affine), {'kind': 'shear'}, 'kind'),
                           ((fixed.numpy(), moving.numpy(), affine), {'x0': [0, 0, 0]},
                            r'\(12,\)'),
                           ((fixed.numpy(), moving.numpy() * np.nan, affine), {},
                            'no finite station')):
        with pytest.raises(ValueError, match=word):
            register(*args, evaluate=nothing, **kw)


def test_atlas_transformed_keeps_labels_and_names():
    from tracktolearn_amd.bundle_recognize import BundleAtlas
    from tracktolearn_amd.bundle_register import compose, to_mm
    c = cases.recovery('rigid')
    atlas = BundleAtlas(c['dims'], c['affine'], c['moving_vox'], list('abc'), label=c['label'],
                        device='cpu')
    moved = atlas.transformed(c['planted'])
    assert moved.names == atlas.names and np.array_equal(moved.label, atlas.label)
    assert moved.dims == atlas.dims and np.array_equal(moved.affine, atlas.affine)
    assert moved.models_vox.dtype == F32 and moved.models_vox.shape == atlas.models_vox.shape
    want = c['atlas_mm'] @ c['planted'][:3, :3].T + c['planted'][:3, 3]
    assert np.abs(to_mm(moved.models_vox, c['affine']) - want).max() < 1e-4
    assert np.array_equal(atlas.transformed(np.eye(4)).models_vox, atlas.models_vox)
    assert np.array_equal(atlas.models_vox, c['moving_vox'])    # the atlas itself is not moved
    assert compose(cases.PLANTED['rigid'], 'rigid', c['centre']).tolist() == c['planted'].tolist()


def test_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_recognize_bundles as cmd
    with pytest.raises(SystemExit) as e:
        cmd.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--register {rigid,similarity,affine}', '--register_max_fixed N',
                '--register_no_progressive', '_registration.json'):
        assert opt in text
    for name in ('t.trk', 'ref.nii.gz', 'a_centroids.npy', 'held_registration.json'):
        (tmp_path / name).write_bytes(b'')
    p = lambda name: str(tmp_path / name)
    base = [p('t.trk'), p('ref.nii.gz'), p('a_centroids.npy')]
    args = cmd.parse_args(base + [p('out')])            # --register absent: as before
    assert args.register is None and not args.register_no_progressive
    assert args.profile == {} and args.max_mdf is None and args.max_ratio is None
    assert not args.save_bundles and args.atlas_labels is None and args.nb_points == 20
    assert cmd.parse_args(base + [p('held')])           # _registration.json is not written
    args = cmd.parse_args(base + [p('out'), '--register', 'affine'])
    assert (args.register, args.register_max_fixed, args.register_no_progressive) == \
        ('affine', 4096, False)
    args = cmd.parse_args(base + [p('out'), '--register', 'rigid', '--register_max_fixed', '500',
                                  '--register_no_progressive'])
    assert (args.register, args.register_max_fixed, args.register_no_progressive) == \
        ('rigid', 500, True)
    assert cmd.parse_args(base + [p('held'), '--register', 'rigid', '-f'])
    for argv, word in ((base + [p('out'), '--register', 'translation'], 'invalid choice'),
                       (base + [p('out'), '--register_max_fixed', '9'], 'only with --register'),
                       (base + [p('out'), '--register_no_progressive'], 'only with --register'),
                       (base + [p('out'), '--register', 'rigid', '--register_max_fixed', '0'],
                        '1 or more'),
                       (base + [p('held'), '--register', 'rigid'], 'use -f')):
        with pytest.raises(SystemExit) as e:
            cmd.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_the_cases_cover_the_issue_ranges():
    keys = cases.GPU_CASES
    assert sorted({k[0] for k in keys}) == list(cases.KS) == [2, 3, 20, 64, 65, 256]
    assert sorted({k[1] for k in keys}) == list(cases.AS) == [1, 7, 8, 9, 70]
    assert sorted({k[2] for k in keys}) == list(cases.BS) == [1, 63, 64, 65, 300]
    assert sorted({k[3] for k in keys}) == list(cases.TS) == [1, 2, 25, 64]
    assert cases.TILE_LINES + 1 in cases.BS and cases.WORKGROUP_ROWS + 1 in cases.AS
    assert {k[4] for k in keys} == set(cases.LINS)
    c = cases.case(20, 9, 65, 25, 'oblique')
    assert set(c['special']) == {'xf_nan', 'xf_zero', 'xf_inf', 'fixed_nan', 'fixed_inf',
                                 'fixed_twice', 'moving_nan', 'moving_inf', 'moving_twice'}
    assert np.array_equal(c['moving'][6], c['moving'][7]) and not c['xf'][4].any()
    assert set(cases.SPECIAL_CASES) == {'all_nan_fixed', 'all_nan_moving'}


CASE_KEYS = cases.GPU_CASES + list(cases.SPECIAL_CASES)


@pytest.mark.parametrize('key', [(20, 9, 65, 25, 'oblique'), 'all_nan_fixed', 'all_nan_moving'],
                         ids=str)
def test_reference_on_the_special_inputs(key):
    """Against the reference alone: the NaN patterns the header states."""
    c, r = cases.get(key), cases.reference(key)
    s = c['special']
    rows, cols, cost = f64(r['row_min']), f64(r['col_min']), f64(r['cost'])
    for t in (s['xf_nan'], s['xf_inf']):                # no moving line takes part
        assert np.isnan(rows[t]).all() and np.isnan(cols[t]).all() and np.isnan(cost[t])
    if key == 'all_nan_fixed' or key == 'all_nan_moving':
        assert np.isnan(rows).all() and np.isnan(cols).all() and np.isnan(cost).all()
        return
    plain = [t for t in range(c['T']) if t not in (s['xf_nan'], s['xf_inf'])]
    assert np.isnan(rows[plain][:, [s['fixed_nan'], s['fixed_inf']]]).all()
    assert np.isnan(cols[plain][:, [s['moving_nan'], s['moving_inf']]]).all()
    assert np.isnan(rows[plain]).sum() == 2 * len(plain)
    assert np.isnan(cols[plain]).sum() == 2 * len(plain) and not np.isnan(cost[plain]).any()
    a, b = s['fixed_twice']
    assert np.array_equal(rows[:, a], rows[:, b], equal_nan=True)
    # the all-zero transform: every moving line is the point 0, every column the same
    z = cols[s['xf_zero']]
    assert len(set(z[~np.isnan(z)].tolist())) == 1


@pytest.fixture(scope='module', params=['rigid', 'affine'])
def cpu_fit(request):
    from tracktolearn_amd.bundle_register import register
    c = cases.recovery(request.param)
    evaluate = ref.evaluate(c['fixed_vox'], c['moving_vox'], c['affine'][:3, :3])
    return c, register(c['fixed_vox'], c['moving_vox'], c['affine'], kind=request.param,
                       evaluate=evaluate)


def _cost_at(c, matrix, fixed_vox=None):
    """The reference's longdouble cost of the mm ``matrix`` on the case."""
    from tracktolearn_amd.bundle_register import to_voxel
    fixed = c['fixed_vox'] if fixed_vox is None else fixed_vox
    got = ref.cost(fixed, c['moving_vox'], to_voxel(matrix, c['affine'])[None],
                   c['affine'][:3, :3])
    return float(got['cost'][0])


def test_driver_recovers_the_planted_transform(cpu_fit):
    """(a) the cost found is at or below the reference's cost at the planted
    transform, (b) no atlas station lies further than 2 sigma = 1 mm from where
    the planted transform puts it; every evaluation is one call."""
    c, fit = cpu_fit
    at_plant = _cost_at(c, c['planted'])
    shift = cases.displacement(c, fit['matrix'])
    print(fit['kind'], 'cost before', fit['cost_before'], 'after', fit['cost_after'], 'at the plant',
          at_plant, 'displacement mm', shift, 'evaluations', fit['evaluations'], fit['stages'])
    assert fit['cost_after'] <= at_plant
    assert shift <= CAP_MM
    assert abs(_cost_at(c, fit['matrix']) - fit['cost_after']) < 1e-9 * at_plant
    assert fit['cost_before'] > 5 * fit['cost_after']
    assert abs(_cost_at(c, np.eye(4)) - fit['cost_before']) < 1e-9 * fit['cost_before']
    from tracktolearn_amd.bundle_register import KINDS
    assert [s['kind'] for s in fit['stages']] == list(KINDS[:KINDS.index(fit['kind']) + 1])
    assert fit['matrix'].shape == (4, 4) and fit['params'].shape == (len(cases.PLANTED[fit['kind']]),)
    # the centre: the mean of the float32 voxel stations in mm, not of the case's float64 mm
    assert np.abs(fit['centre'] - c['centre']).max() < 1e-5
    assert fit['evaluations'] > len(fit['stages'])


def test_driver_counts_one_call_per_evaluation_and_can_skip_the_stages():
    from tracktolearn_amd.bundle_register import register
    c = cases.recovery('rigid')
    inner = ref.evaluate(c['fixed_vox'], c['moving_vox'], c['affine'][:3, :3])
    sizes = []

    def evaluate(mats):
        sizes.append(np.asarray(mats).shape)
        return inner(mats)
    fit = register(c['fixed_vox'], c['moving_vox'], c['affine'], kind='rigid', progressive=False,
                   evaluate=evaluate, max_iter=3)
    assert fit['evaluations'] == len(sizes) and [s['kind'] for s in fit['stages']] == ['rigid']
    assert sizes[0] == (1, 3, 4) and set(sizes[1:]) == {(13, 3, 4)}     # 2 * 6 + 1
    assert fit['cost_after'] < fit['cost_before']


@pytest.mark.parametrize('kind', ['rigid', 'affine'])
def test_recovery_case_needs_the_registration(kind):
    """By the reference: at least one in ten subject lines is nearest a line of
    another bundle before registration, none at the planted transform."""
    c = cases.recovery(kind)
    n = len(c['label'])
    before = cases.labels_by_reference(c, np.eye(4))[:n]
    planted = cases.labels_by_reference(c, c['planted'])[:n]
    assert (before != c['label']).mean() >= 0.1
    assert np.array_equal(planted, c['label'])


# ----------------------------------------------------------------- GPU tests
def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _cost(c, fixed=None, moving=None, xf=None):
    from tracktolearn_amd.bundle_register import bundle_register_cost
    got = bundle_register_cost(_dev(c['fixed'] if fixed is None else fixed, F32),
                               _dev(c['moving'] if moving is None else moving, F32),
                               _dev(c['xf'] if xf is None else xf, np.float64), c['lin'])
    return {k: v.cpu().numpy() for k, v in zip(('row_min', 'col_min', 'cost'), got)}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(I64)


def _inside(value, lo, hi):
    """NaN exactly where the interval is NaN, inside it elsewhere."""
    nan = np.isnan(f64(lo))
    assert np.array_equal(np.isnan(value), nan)
    v = value[~nan].astype(LD)
    return bool((lo[~nan] <= v).all() and (v <= hi[~nan]).all())


@pytest.mark.gpu
@pytest.mark.parametrize('key', CASE_KEYS, ids=str)
def test_kernel_is_the_reference(key):
    """row_min and col_min lie inside the reference's intervals on every entry, NaN
    exactly where it has none (the header's quiet NaN); the cost is within its
    bound, NaN exactly where the reference's is."""
    c, r = cases.get(key), cases.reference(key)
    got = _cost(c)
    assert got['row_min'].shape == (c['T'], c['A']) and got['col_min'].shape == (c['T'], c['B'])
    assert _inside(got['row_min'], r['row_lo'], r['row_hi'])
    assert _inside(got['col_min'], r['col_lo'], r['col_hi'])
    for k in ('row_min', 'col_min', 'cost'):
        nan = np.isnan(got[k])
        assert (_bits(got[k])[nan] == 0x7ff8000000000000).all()
    nan = np.isnan(f64(r['cost']))
    assert np.array_equal(np.isnan(got['cost']), nan)
    err = np.abs(got['cost'][~nan].astype(LD) - r['cost'][~nan])
    print(key, 'largest cost error / bound', float((err / r['cost_bound'][~nan]).max())
          if err.size else None)
    assert (err <= r['cost_bound'][~nan]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('key', [(20, 9, 65, 25, 'oblique'), (65, 7, 63, 64, 'anisotropic'),
                                 (256, 70, 65, 1, 'oblique'), (2, 70, 300, 2, 'axis')], ids=str)
def test_bits_do_not_depend_on_call_order_or_split(key):
    """The minima are the same bits in a repeated call, with the fixed or the
    moving lines permuted (indices mapped back) and with the transforms split into
    separate calls; the cost, a sum in line order, is the same bits where the
    order of the lines is the same."""
    c = cases.get(key)
    whole = _cost(c)
    again = _cost(c)
    for k in ('row_min', 'col_min', 'cost'):
        assert np.array_equal(_bits(again[k]), _bits(whole[k]))
    rng = np.random.default_rng(3)
    perm = rng.permutation(c['A'])
    got = _cost(c, fixed=c['fixed'][perm])
    assert np.array_equal(_bits(got['row_min']), _bits(whole['row_min'][:, perm]))
    assert np.array_equal(_bits(got['col_min']), _bits(whole['col_min']))
    perm = rng.permutation(c['B'])
    got = _cost(c, moving=c['moving'][perm])
    assert np.array_equal(_bits(got['row_min']), _bits(whole['row_min']))
    assert np.array_equal(_bits(got['col_min']), _bits(whole['col_min'][:, perm]))
    cut = c['T'] // 3 + 1
    parts = [_cost(c, xf=c['xf'][:cut])] + ([_cost(c, xf=c['xf'][cut:])] if cut < c['T'] else [])
    for k in ('row_min', 'col_min', 'cost'):
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k]))
    if c['T'] > 1:                                      # one transform a call
        one = _cost(c, xf=c['xf'][c['T'] - 1:])
        for k in ('row_min', 'col_min', 'cost'):
            assert np.array_equal(_bits(one[k][0]), _bits(whole[k][-1]))


def _straight(rng, n, K):
    """Axis-parallel lines of K points a power of two apart at quarter-voxel
    places: their stations at K are their points, exactly."""
    lines = np.zeros((n, K, 3), F32)
    for i in range(n):
        step = (0.125, 0.25, 0.5)[i % 3] * (1 if i % 2 else -1)
        lines[i] = rng.integers(0, 24, 3) / 4.0
        lines[i, :, i % 3] += step * np.arange(K)
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize('K,lin_name', [(3, 'axis'), (20, 'oblique'), (65, 'anisotropic')])
def test_identity_agrees_with_bundle_recognize(K, lin_name):
    """Under the identity row_min is ttl_bundle_recognize's mdf with the fixed
    lines as its rows and the moving set as its models, bit for bit: the two
    kernels run one statement of the tile walk (the same distance, sum order and
    flip rule), ((1 p0 + 0 p1) + 0 p2) + 0 is p0, and the rows are lines the
    resampler leaves as they are."""
    from ref_oracle_validator import resample_blocked
    from tracktolearn_amd.bundle_recognize import bundle_recognize
    rng = np.random.default_rng(K)
    fixed = _straight(rng, 70, K)
    for line in fixed[:6]:
        assert np.array_equal(resample_blocked(line, K), line)
    moving = cases.case(K, 9, 65, 2, lin_name)['moving'].copy()
    moving = moving[np.isfinite(moving).all((1, 2))]
    lin = cases.LINS[lin_name]
    c = {'fixed': fixed, 'moving': moving, 'xf': np.eye(4)[None, :3], 'lin': lin}
    got = _cost(c)
    r = ref.cost(fixed, moving, c['xf'], lin)
    offsets = np.arange(len(fixed) + 1, dtype=I64) * K
    mdf = bundle_recognize(_dev(fixed.reshape(-1, 3)), _dev(offsets), _dev(moving), lin)[2]
    mdf = mdf.cpu().numpy()
    assert not np.isnan(mdf).any()
    width = f64(r['row_hi'][0] - r['row_lo'][0])
    print('largest |row_min - mdf| / width', float((np.abs(got['row_min'][0] - mdf) / width).max()))
    assert np.array_equal(_bits(got['row_min'][0]), _bits(mdf))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['rigid', 'affine'])
def test_register_then_recognize_end_to_end(kind, tmp_path, capsys):
    """The command with --register on the recovery case: (a) the cost found is at
    or below the reference's at the planted transform (on the stations the fit
    used), (b) no atlas station is further than 1 mm from where the planted
    transform puts it; every subject line of a bundle gets its bundle with the
    moved atlas, and at least one in ten a wrong one with the unmoved atlas."""
    from tracktolearn_amd.bundle_recognize import BundleAtlas
    from tracktolearn_amd.bundle_register import fixed_stations, register_atlas
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_recognize_bundles as cmd
    from tracktolearn_amd.tractogram import Tractogram
    c = cases.recovery(kind)
    p = lambda name: str(tmp_path / name)
    sio.save(Tractogram([line.astype(F32) for line in c['fixed_mm']], affine_to_rasmm=np.eye(4)),
             p('subject.trk'), sio.create_tractogram_header(c['affine'], c['dims'], (2.0,) * 3))
    sio.save(Tractogram([line.astype(F32) for line in c['atlas_mm']], affine_to_rasmm=np.eye(4)),
             p('atlas.trk'), sio.create_tractogram_header(c['affine'], c['dims'], (2.0,) * 3))
    nifti.save(p('ref.nii.gz'), np.zeros(c['dims'], np.uint8), c['affine'])
    np.save(p('labels.npy'), c['label'])
    K, n = c['atlas_mm'].shape[1], len(c['label'])
    atlas = BundleAtlas.from_tractogram(p('ref.nii.gz'), p('atlas.trk'), c['label'], list('abc'), K,
                                        device=DEV)
    fit = register_atlas(atlas, p('subject.trk'), kind=kind)
    stations = fixed_stations(p('subject.trk'), c['affine'], K, device=DEV)
    assert stations.shape == (len(c['truth']), K, 3) == (fit['n_fixed'], K, 3)
    case = dict(c, moving_vox=atlas.models_vox)
    at_plant = _cost_at(case, c['planted'], stations)
    shift = cases.displacement(c, fit['matrix'])
    with capsys.disabled():
        print(kind, 'cost before', fit['cost_before'], 'after', fit['cost_after'], 'at the plant',
              at_plant, 'displacement mm', shift, 'evaluations', fit['evaluations'])
    assert fit['cost_after'] <= at_plant
    assert shift <= CAP_MM
    assert abs(_cost_at(case, fit['matrix'], stations) - fit['cost_after']) < 1e-9 * at_plant
    got = fit['atlas'].recognize(p('subject.trk'))
    assert np.array_equal(got['bundle'][:n], c['label'])
    unmoved = atlas.recognize(p('subject.trk'))
    assert (unmoved['bundle'][:n] != c['label']).mean() >= 0.1
    # the command: the same fit, written out, and the bundles of the moved atlas
    cmd.main([p('subject.trk'), p('ref.nii.gz'), p('atlas.trk'), p('out'), '--atlas_labels',
              p('labels.npy'), '--nb_points', str(K), '--register', kind])
    capsys.readouterr()
    record = json.load(open(p('out_registration.json')))
    assert set(record) == {'kind', 'matrix', 'params', 'centre', 'cost_before', 'cost_after',
                           'evaluations', 'n_fixed', 'n_moving'}
    assert record['kind'] == kind and record['evaluations'] == fit['evaluations']
    assert np.array_equal(np.asarray(record['matrix']), fit['matrix'])
    assert record['cost_after'] == fit['cost_after']
    assert np.array_equal(np.load(p('out_bundles.npy'))[:n], c['label'])
    cmd.main([p('subject.trk'), p('ref.nii.gz'), p('atlas.trk'), p('plain'), '--atlas_labels',
              p('labels.npy'), '--nb_points', str(K)])
    capsys.readouterr()
    assert not os.path.exists(p('plain_registration.json'))
    assert np.array_equal(np.load(p('plain_bundles.npy')), unmoved['bundle'])


@pytest.mark.gpu
def test_register_atlas_subsamples_the_fixed_set(tmp_path):
    from tracktolearn_amd.bundle_register import fixed_stations
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    c = cases.recovery('rigid')
    lines = [line.astype(F32) for line in c['fixed_mm']]
    lines[2] = lines[2][:1]                             # a single point: takes no part
    path = str(tmp_path / 'subject.trk')
    sio.save(Tractogram(lines, affine_to_rasmm=np.eye(4)), path,
             sio.create_tractogram_header(c['affine'], c['dims'], (2.0,) * 3))
    K = 12
    every = fixed_stations(path, c['affine'], K, device=DEV)
    assert every.shape == (len(lines) - 1, K, 3)
    some = fixed_stations(path, c['affine'], K, max_fixed=10, device=DEV)
    assert some.shape == (9, K, 3)                      # 35 lines, every 4th
    assert np.array_equal(some, every[::4])
