"""Weighted connectome edges (ttl_tract_sample_mean,
ttl_connectome_accumulate_metric, ``Connectome(metrics=...)``, ``ttl_track.py
--connectome_metric``, ``ttl_connectome.py --metric``) against
tests/ref_connectome_metric.py, the definition of include/ttl_hip.h as a literal
loop in numpy.longdouble, on the sets of tests/connectome_metric_cases.py.  Which
points are sampled and which rows have a mean is compared exactly, and so are the
integer matrices; mean and weight are held to the header's derived bound."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import connectome_metric_cases as cases
import ref_connectome_metric as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
LD = np.longdouble
SET_NAMES = sorted(cases.SETS)
WITNESS_SETS = ('normal_axis', 'holes_oblique', 'one_axis', 'slab_oblique')


# ------------------------------------------------------------------ CPU part
def test_definition_on_two_voxels():
    """A 1 x 1 x 2 volume holding 1 and 3, 1 mm voxels: the centres are at z = 0.5
    and 1.5; beyond them the border value is replicated."""
    volume = np.array([1.0, 3.0], F32).reshape(1, 1, 2)
    at = lambda z, mutant=None: ref.sample((0.5, 0.5, z), volume, mutant)
    assert [float(at(z)[0]) for z in (0.0, 0.5, 1.0, 1.25, 1.5, 2.0)] == \
        [1.0, 1.0, 2.0, 2.5, 3.0, 3.0]
    assert at(np.nextafter(F32(2.0), F32(3.0))) is None and at(-0.3) is None
    assert at(np.nextafter(F32(0.0), F32(-1.0))) is None and at(1e30) is None
    assert at(float('nan')) is None and ref.sample((1.5, 0.5, 0.5), volume) is None
    assert float(at(1.0, 'no_half_shift')[0]) == 3.0
    assert float(at(0.25, 'truncation')[0]) == 0.5          # extrapolated from f = -0.25
    assert float(at(0.25, 'zero_padding')[0]) == 0.75
    assert float(at(2.5, 'outside_clamped')[0]) == 3.0
    holes = np.array([1.0, np.nan], F32).reshape(1, 1, 2)
    assert ref.sample((0.5, 0.5, 0.5), holes) is None       # a corner of weight 0 counts
    assert float(ref.sample((0.5, 0.5, 1.0), holes, 'nonfinite_corner_zero')[0]) == 0.5
    # three points half a voxel apart: w = 1/4, 1/2, 1/4 mm at 1 mm voxels
    row = np.array([(0.5, 0.5, 0.5), (0.5, 0.5, 1.0), (0.5, 0.5, 1.5)], F32)
    mean, weight, b_mean, b_weight = ref.row_mean(row, volume, np.eye(3))
    assert (float(mean), float(weight)) == (2.0, 1.0) and 0 < b_mean < 1e-14 and b_weight > 0
    assert float(ref.row_mean(row, volume, np.diag([1.0, 1.0, 4.0]))[1]) == 4.0
    assert float(ref.row_mean(row, volume, np.eye(3), 'uniform_weights')[1]) == 3.0
    assert float(ref.row_mean(row, volume, np.eye(3), 'ends_not_halved')[0]) == 2.0
    assert float(ref.row_mean(row[:2], volume, np.eye(3), 'ends_not_halved')[1]) == 1.0
    # an unsampled middle point leaves the ends: (1/4 + 3/4) / (1/2)
    row[1, 0] = 1.5
    mean, weight, _, _ = ref.row_mean(row, volume, np.eye(3))
    assert float(weight) == float(np.sqrt(LD(1.25))) and float(mean) == 2.0
    for degenerate in (row[:1], row[:0], np.tile(row[:1], (3, 1)), row[1:2].repeat(2, 0)):
        mean, weight, _, _ = ref.row_mean(degenerate, volume, np.eye(3))
        assert np.isnan(mean) and weight == 0


def test_sets_hold_what_they_are_for():
    for name in SET_NAMES:
        c = cases.case(name)
        mean, weight, b_mean, b_weight = cases.expected(name)
        L = np.diff(c.offsets)
        assert set(cases.ROW_LENGTHS) <= set(L.tolist())
        assert np.isnan(mean[L < 2]).all() and (weight[np.isnan(mean)] == 0).all()
        assert 8 <= np.isnan(mean).sum() <= 9 and (weight[~np.isnan(mean)] > 0).all()
        assert (b_mean[~np.isnan(mean)] > 0).all() and (b_weight[~np.isnan(mean)] > 0).all()
    # the row whose only sampled point touches the NaN block has no mean there alone
    touch = len(cases.ROW_LENGTHS) + 3 + 9 + 2
    assert len(cases.case('holes_axis').rows[touch]) == 3
    assert np.isnan(cases.expected('holes_axis')[0][touch])
    assert not np.isnan(cases.expected('normal_axis')[0][touch])
    scales = {ref.scale_for(cases.volume_of(v)) for v in cases.VOLUMES}
    assert len(scales) >= 3                                 # several scales occur


def test_reference_gives_the_constant_and_the_analytic_value():
    for lin in cases.LINS:
        mean, _, bound, _ = cases.expected(f'constant_{lin}')
        ok = ~np.isnan(mean)
        assert (np.abs(mean[ok] - LD(F32(cases.CONSTANT))) <= bound[ok]).all()
        name = f'linear_{lin}'
        c = cases.case(name)
        points, offsets = cases.interior_rows(name)
        mean, _, bound, _ = ref.sample_mean(points, offsets, c.volume, c.lin)
        assert (np.abs(mean - cases.analytic_means(name)) <= bound).all()


@pytest.mark.parametrize('mutant', ref.SAMPLE_MUTANTS)
def test_every_sampling_mutant_has_a_witness(mutant):
    witnesses = [name for name in WITNESS_SETS if len(cases.differs(name, mutant))]
    assert witnesses, mutant


def accumulate_rows():
    """Chosen doubles at scale 2^3: ties at half a unit (to even), values just
    under and at 2^40 / scale, rows that do not count."""
    scale, limit = 8.0, 2.0 ** 37
    mean = [0.5 / 8, 1.5 / 8, 2.5 / 8, -0.5 / 8, -1.5 / 8, -2.5 / 8, 3.5 / 8, 2.4999 / 8,
            np.nextafter(limit, 0.0), limit, -np.nextafter(limit, 0.0), -limit,
            np.nan, np.inf, -np.inf, 1.0, 1.0, 1.0, 0.0, 5e-324]
    node = [[1, 2]] * 3 + [[3, 1]] * 3 + [[2, 1]] * 2 + [
        [2, 2], [2, 2], [3, 2], [3, 2], [1, 1], [1, 1], [1, 1],
        [-1, -1], [4, 1], [0, 3], [3, 0], [0, 0]]
    return np.array(node, np.int32), np.array(mean, np.float64), scale


def test_accumulate_definition_and_its_mutants():
    node, mean, scale = accumulate_rows()
    q, n = ref.accumulate_metric(node, mean, 3, scale)
    # 0 + 2 + 2 + 4 + 2 in cell (1, 2) and -0 - 2 - 2 in (1, 3): half to even both ways
    assert (q[1, 2], n[1, 2]) == (10, 5) and (q[1, 3], n[1, 3]) == (-4, 3)
    # 2^40 - 2^-13 rounds to 2^40 and counts; 2^40 itself is skipped
    assert q[2, 2] == 2 ** 40 and n[2, 2] == 1
    assert q[2, 3] == -q[2, 2] and n[2, 3] == 1
    assert n[1, 1] == 0 and q[1, 1] == 0                    # NaN, +Inf, -Inf
    assert (n[0, 3], q[0, 3]) == (2, 8) and (n[0, 0], q[0, 0]) == (1, 0)
    assert n.sum() == 13 and not np.tril(n, -1).any()
    for mutant in ref.ACCUMULATE_MUTANTS:
        wrong = ref.accumulate_metric(node, mean, 3, scale, mutant=mutant)
        assert not all(np.array_equal(a, b) for a, b in zip((q, n), wrong)), mutant
    away = ref.accumulate_metric(node, mean, 3, scale, mutant='half_away_from_zero')[0]
    assert (away[1, 2], away[1, 3]) == (12, -6)
    assert ref.accumulate_metric(node, mean, 3, scale, mutant='nan_rows_counted')[1][1, 1] == 3
    m, count = ref.edge_means(q, n, scale)
    assert m.shape == (3, 3) and m[0, 1] == m[1, 0] == 10 / 8 / 5 and count[0, 1] == 5
    assert np.isnan(m[0, 0]) and count[0, 0] == 0


def test_scale_rule():
    from tracktolearn_amd.connectome import metric_scale
    vol = lambda *v: np.array(v, np.float64).reshape(1, 1, -1)
    assert metric_scale(vol(0.0, 0.0)) == 2.0 ** 38                 # m = 1 < 2^1
    assert metric_scale(vol(np.nan, np.nan)) == 2.0 ** 38
    assert metric_scale(vol(np.inf, -np.inf, np.nan, 0.0)) == 2.0 ** 38
    assert metric_scale(vol(1.0)) == 2.0 ** 38 and metric_scale(vol(-1.0, 0.5)) == 2.0 ** 38
    assert metric_scale(vol(0.999)) == 2.0 ** 39 and metric_scale(vol(0.5)) == 2.0 ** 39
    assert metric_scale(vol(0.49, np.inf)) == 2.0 ** 40
    assert metric_scale(vol(-3.0e-3, 1e-3)) == 2.0 ** 47            # 2^-9 <= 3e-3 < 2^-8
    assert metric_scale(vol(1e4, np.nan)) == 2.0 ** 25              # 2^13 <= 1e4 < 2^14
    assert metric_scale(vol(1e38)) == 2.0 ** -60 and metric_scale(vol(1e-30)) == 2.0 ** 60
    for name in cases.VOLUMES:
        v = cases.volume_of(name)
        scale = metric_scale(v)
        assert scale == ref.scale_for(v)
        finite = np.abs(v[np.isfinite(v)]).astype(np.float64)
        assert finite.max() * scale < 2.0 ** 39 <= 2 * finite.max() * scale


def test_connectome_argument_errors():
    """Refused on the host, before the library or a device is touched."""
    from tracktolearn_amd.connectome import Connectome, check_metrics
    labels = np.ones((2, 3, 4), np.int32)
    good = np.zeros((2, 3, 4))
    for metrics in ({'': good}, {'a=b': good}, {'=': good}, {3: good},
                    {'fa': np.zeros((2, 3, 5))}, {'fa': np.zeros((2, 3))},
                    {'fa': np.zeros((2, 3, 4, 1))}, {'fa': good, 'md': np.zeros((4, 3, 2))}):
        with pytest.raises(ValueError, match='metric'):
            Connectome(labels, np.eye(4), metrics=metrics)
    out = check_metrics({'fa': np.asfortranarray(good), 'md': good.astype(np.int16)}, (2, 3, 4))
    assert list(out) == ['fa', 'md']
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in out.values())
    assert check_metrics(None, (2, 3, 4)) == {} and check_metrics({}, (2, 3, 4)) == {}


def _sample_args():
    """Arguments that pass every check of ttl_tract_sample_mean: the pointers are
    never followed, TTL_ERR_INVALID and n == 0 return before any HIP call."""
    p = C.c_void_p(4096)
    return dict(points=p, offsets=p, n=0, volume=p, dims=(C.c_int32 * 3)(5, 6, 7),
                lin=(C.c_double * 9)(*np.eye(3).reshape(-1)), mean=p, weight=p, stream=None)


@pytest.mark.parametrize('key,value', [(k, None) for k in (
    'points', 'offsets', 'volume', 'dims', 'lin', 'mean', 'weight')] + [
    ('n', -1), ('dims', (C.c_int32 * 3)(0, 6, 7)), ('dims', (C.c_int32 * 3)(5, 6, -2))])
def test_sample_mean_refuses_before_any_hip_call(key, value):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    args = _sample_args()
    assert lib.ttl_tract_sample_mean(*args.values()) == 0            # n == 0: a no-op
    args[key] = value
    assert lib.ttl_tract_sample_mean(*args.values()) == _lib.ERR_INVALID
    assert b'ttl_tract_sample_mean' in lib.ttl_last_error()


@pytest.mark.parametrize('key,value', [
    ('node', None), ('mean', None), ('metric_q', None), ('metric_n', None), ('n', -1),
    ('n_nodes', 0), ('n_nodes', 4097), ('scale', 0.0), ('scale', -1.0), ('scale', 3.0),
    ('scale', 0.75), ('scale', float('nan')), ('scale', float('inf')), ('scale', 2.0 ** 61),
    ('scale', 2.0 ** -61), ('scale', 5e-324)])
def test_accumulate_metric_refuses_before_any_hip_call(key, value):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    args = dict(node=p, mean=p, n=0, n_nodes=4096, scale=1.0, metric_q=p, metric_n=p,
                stream=None)
    for scale in (1.0, 2.0 ** 60, 2.0 ** -60, 2.0 ** 38):
        assert lib.ttl_connectome_accumulate_metric(*dict(args, scale=scale).values()) == 0
    args[key] = value
    assert lib.ttl_connectome_accumulate_metric(*args.values()) == _lib.ERR_INVALID
    assert b'ttl_connectome_accumulate_metric' in lib.ttl_last_error()


def test_header_announces_the_feature_and_keeps_the_abi():
    from tracktolearn_amd import _lib, connectome
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'^#define TTL_HAS_TRACT_SAMPLE 1$', header, re.M)
    assert re.search(r'^#define TTL_HAS_CONNECTOME_METRIC 1$', header, re.M)
    assert re.search(r'^#define TTL_ABI_VERSION 13$', header, re.M)
    for words in ('z pairs first, then y, then x', 'floor, not truncation',
                  'edge replicate', r'\(L \+ 9\) u A', r'\(L \+ 19\) M', 'half to even',
                  r'\|mean\[s\] \* scale\| >= 2\^40'):
        assert re.search(words, header), words
    assert (_lib.HAS_TRACT_SAMPLE, _lib.HAS_CONNECTOME_METRIC, _lib.ABI_VERSION) == (1, 1, 13)
    lib = _lib.load()
    for name in ('ttl_tract_sample_mean', 'ttl_connectome_accumulate_metric'):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert re.search(r'^TTL_API int %s\(' % name, header, re.M)
    from tracktolearn_amd.csrc import build
    assert any(s.endswith('ttl_tract_sample.hip') for s in build.SOURCES)
    for name in ('sample_mean', 'accumulate_metric', 'metric_scale'):
        assert name in connectome.__all__


def _track_parse(argv, tmp_path):
    from tracktolearn_amd.runners import ttl_track
    files = {}
    for name in ('fodf', 'seed', 'mask', 'labels', 'fa', 'md'):
        files[name] = str(tmp_path / f'{name}.nii.gz')
        open(files[name], 'wb').close()
    argv = [re.sub(r'\b(LABELS|FA|MD)\b', lambda m: files[m.group(1).lower()], a)
            .replace('PREFIX', str(tmp_path / 'con')) for a in argv]
    return ttl_track.parse_args([files['fodf'], files['seed'], files['mask'],
                                 str(tmp_path / 'out.trk'), '--odf_policy', 'det'] + argv)


def test_track_command_metric_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(SystemExit):
        ttl_track.parse_args(['--help'])
    assert '--connectome_metric NAME=FILE' in capsys.readouterr().out
    con = ['--connectome', 'LABELS', '--connectome_out', 'PREFIX']
    assert _track_parse(con, tmp_path).connectome_metric == []
    args = _track_parse(con + ['--connectome_metric', 'fa=FA', '--connectome_metric', 'md=MD'],
                        tmp_path)
    assert [n for n, _ in args.connectome_metric] == ['fa', 'md']
    assert args.connectome_metric[0][1].endswith('fa.nii.gz')
    for argv, word in ((['--connectome_metric', 'fa=FA'], 'only with --connectome'),
                       (con + ['--connectome_metric', 'FA'], 'NAME=FILE'),
                       (con + ['--connectome_metric', '=FA'], 'NAME=FILE'),
                       (con + ['--connectome_metric', 'fa='], 'NAME=FILE'),
                       (con + ['--connectome_metric', 'fa=nowhere.nii.gz'], 'does not exist'),
                       (con + ['--connectome_metric', 'fa=FA', '--connectome_metric', 'fa=MD'],
                        'more than once')):
        with pytest.raises(SystemExit) as e:
            _track_parse(argv, tmp_path)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_connectome_command_metric_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_connectome
    with pytest.raises(SystemExit):
        ttl_connectome.parse_args(['--help'])
    assert '--metric NAME=FILE' in capsys.readouterr().out
    for name in ('t.trk', 'labels.nii.gz', 'fa.nii.gz', 'md.nii.gz', 'held_mean_fa.npy',
                 'kept_fa_streamlines.npy'):
        (tmp_path / name).write_bytes(b'')
    p = lambda name: str(tmp_path / name)
    base = [p('t.trk'), p('labels.nii.gz')]
    assert ttl_connectome.parse_args(base + [p('out')]).metric == []
    args = ttl_connectome.parse_args(base + [p('out'), '--metric', 'fa=' + p('fa.nii.gz'),
                                             '--metric', 'md=' + p('md.nii.gz')])
    assert args.metric == [('fa', p('fa.nii.gz')), ('md', p('md.nii.gz'))]
    # a name may hold what a path holds; the first '=' splits
    assert ttl_connectome.metric_options(['a.b=c=d']) == [('a.b', 'c=d')]
    fa = ['--metric', 'fa=' + p('fa.nii.gz')]
    assert ttl_connectome.parse_args(base + [p('held'), '--metric', 'md=' + p('md.nii.gz')])
    assert ttl_connectome.parse_args(base + [p('kept')] + fa)       # not written without
    for argv, word in ((base + [p('out'), '--metric', p('fa.nii.gz')], 'NAME=FILE'),
                       (base + [p('out'), '--metric', '=' + p('fa.nii.gz')], 'NAME=FILE'),
                       (base + [p('out'), '--metric', 'fa=nowhere.nii.gz'], 'does not exist'),
                       (base + [p('out')] + fa + fa, 'more than once'),
                       (base + [p('held')] + fa, 'use -f'),
                       (base + [p('kept'), '--save_assignments'] + fa, 'use -f')):
        with pytest.raises(SystemExit) as e:
            ttl_connectome.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_a_metric_on_another_grid_is_an_error_that_names_both(tmp_path):
    """``load_metric``, through which both commands read a metric."""
    from tracktolearn_amd.connectome import load_metric
    from tracktolearn_amd.io import nifti
    affine = np.array([[2.0, 0, 0, -10], [0, 1.0, 0, 3], [0, 0, 1.5, 7], [0, 0, 0, 1]])
    moved = affine.copy()
    moved[0, 3] = -9.5
    data = np.random.RandomState(0).uniform(0, 1, (7, 5, 4))
    for name, vol, aff in (('same', data, affine), ('moved', data, moved),
                           ('larger', np.zeros((7, 5, 5)), affine),
                           ('four', data[..., None], affine)):
        nifti.save(str(tmp_path / f'{name}.nii.gz'), vol.astype(F32), aff)
    got = load_metric('fa', str(tmp_path / 'same.nii.gz'), (7, 5, 4), affine, 'labels.nii.gz')
    assert got.dtype == np.float32 and np.array_equal(got, data.astype(F32))
    got = load_metric('fa', str(tmp_path / 'four.nii.gz'), (7, 5, 4), affine, 'labels.nii.gz')
    assert got.shape == (7, 5, 4)
    with pytest.raises(ValueError) as e:
        load_metric('fa', str(tmp_path / 'larger.nii.gz'), (7, 5, 4), affine, 'labels.nii.gz')
    text = str(e.value)
    assert 'metric fa' in text and 'larger.nii.gz' in text and 'labels.nii.gz' in text
    assert '(7, 5, 5)' in text and '(7, 5, 4)' in text and 'resample' in text
    with pytest.raises(ValueError) as e:
        load_metric('md', str(tmp_path / 'moved.nii.gz'), (7, 5, 4), affine, 'labels.nii.gz')
    assert '-9.5' in str(e.value) and '-10.0' in str(e.value) and 'metric md' in str(e.value)


def test_metric_matrices_symmetrise_and_average():
    from tracktolearn_amd.connectome import metric_matrices_from
    q = np.array([[7, 1, 2], [0, 3 << 10, -(5 << 10)], [0, 0, 0]], np.int64)
    n = np.array([[4, 1, 1], [0, 2, 4], [0, 0, 0]], np.int64)
    mean, count = metric_matrices_from(q, n, 1024.0)
    assert count.tolist() == [[2, 4], [4, 0]] and count.dtype == np.int64
    assert mean[0, 0] == 1.5 and mean[0, 1] == mean[1, 0] == -1.25 and np.isnan(mean[1, 1])
    want = ref.edge_means(q, n, 1024.0)
    assert np.array_equal(mean, want[0], equal_nan=True) and np.array_equal(count, want[1])


# ------------------------------------------------------------------ GPU part
def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def gpu_sample(c, points, offsets, lin=None):
    from tracktolearn_amd import connectome as con
    mean, weight = con.sample_mean(_dev(points), _dev(offsets), _dev(np.array(c.volume)),
                                   c.lin if lin is None else lin)
    assert mean.dtype == weight.dtype and str(mean.dtype) == 'torch.float64'
    return mean.cpu().numpy(), weight.cpu().numpy()


def gpu_accumulate_metric(node, mean, n_nodes, scale, matrices=None):
    import torch
    from tracktolearn_amd import connectome as con
    side = n_nodes + 1
    if matrices is None:
        matrices = (torch.zeros((side, side), dtype=torch.int64, device=DEV),
                    torch.zeros((side, side), dtype=torch.int64, device=DEV))
    con.accumulate_metric(_dev(np.asarray(node, np.int32)), _dev(np.asarray(mean, np.float64)),
                          n_nodes, scale, *matrices)
    return matrices


def same_matrices(got, want):
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, 'cpu') else g
        assert g.dtype == np.int64 and np.array_equal(g, w)
        assert not np.tril(g, -1).any()                 # only the upper triangle is touched


def within_bounds(got, want, what=''):
    """The exact decisions, then the derived bounds, row by row: the largest
    error / bound of (mean, weight)."""
    mean, weight = got
    w_mean, w_weight, b_mean, b_weight = want
    nan = np.isnan(w_mean)
    assert np.array_equal(np.isnan(mean), nan), (what, np.flatnonzero(np.isnan(mean) != nan))
    assert (weight[nan] == 0.0).all() and (weight[~nan] > 0.0).all()
    worst = [0.0, 0.0]
    for s in np.flatnonzero(~nan):
        e_mean, e_weight = abs(LD(mean[s]) - w_mean[s]), abs(LD(weight[s]) - w_weight[s])
        worst = [max(worst[0], float(e_mean / b_mean[s])),
                 max(worst[1], float(e_weight / b_weight[s]))]
        assert e_mean <= b_mean[s], (what, s, float(e_mean), float(b_mean[s]))
        assert e_weight <= b_weight[s], (what, s, float(e_weight), float(b_weight[s]))
    return worst


@pytest.fixture(scope='module')
def sampled():
    """{set: (mean, weight)} of one launch per set, shared by the tests below."""
    out = {}
    for name in SET_NAMES:
        c = cases.case(name)
        out[name] = gpu_sample(c, c.points, c.offsets)
    return out


@pytest.mark.gpu
def test_means_and_weights_are_within_the_derived_bound(sampled, capsys):
    """Every row of every set, on the axis-aligned and the oblique ``lin``:
    |weight - definition| <= (L + 9) 2^-53 A and |mean - definition| <= 2^-53
    ((L + 19) M + (L + 9) A M / weight) / weight against the definition in
    longdouble (include/ttl_hip.h: derived, not measured).  The largest ratios
    observed on an MI355X are 0.067 (mean) and 0.134 (weight)."""
    worst = [0.0, 0.0]
    for name in SET_NAMES:
        got = within_bounds(sampled[name], cases.expected(name), name)
        worst = [max(a, b) for a, b in zip(worst, got)]
    with capsys.disabled():
        print(f'\nsample_mean: largest error / bound = {worst[0]:.4f} (mean), '
              f'{worst[1]:.4f} (weight)')
    assert worst[0] > 0.0 and worst[1] > 0.0            # some row was rounded at all


@pytest.mark.gpu
@pytest.mark.parametrize('lin', sorted(cases.LINS))
def test_constant_and_analytic_value(sampled, lin):
    mean, _ = sampled[f'constant_{lin}']
    w_mean, _, bound, _ = cases.expected(f'constant_{lin}')
    ok = ~np.isnan(w_mean)
    assert ok.sum() > 15
    assert (np.abs(mean[ok].astype(LD) - LD(F32(cases.CONSTANT))) <= bound[ok]).all()
    name = f'linear_{lin}'
    c = cases.case(name)
    points, offsets = cases.interior_rows(name)
    mean, weight = gpu_sample(c, points, offsets)
    want = ref.sample_mean(points, offsets, c.volume, c.lin)
    within_bounds((mean, weight), want, name)
    assert (np.abs(mean.astype(LD) - cases.analytic_means(name)) <= want[2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [0, 1, 2, 5])
def test_launch_sizes(n):
    c = cases.case('normal_oblique')
    mean, weight = gpu_sample(c, c.points[:c.offsets[n]], c.offsets[:n + 1])
    assert mean.shape == weight.shape == (n,)
    within_bounds((mean, weight), [w[:n] for w in cases.expected('normal_oblique')])


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid():
    """70 000 short rows: the grid is capped at 8192 workgroups of four waves, a
    wave per row."""
    name = 'normal_oblique'
    points, offsets, *want = cases.many_rows(name, 70000)
    got = gpu_sample(cases.case(name), points, offsets)
    within_bounds(got, want, name)
    assert np.isnan(want[0]).sum() == 0 and len(np.unique(got[0])) > 90


@pytest.mark.gpu
def test_accumulate_chosen_doubles():
    node, mean, scale = accumulate_rows()
    want = ref.accumulate_metric(node, mean, 3, scale)
    same_matrices(gpu_accumulate_metric(node, mean, 3, scale), want)
    # every scale the sets use, and the ends of the range
    rng = np.random.RandomState(1)
    node = rng.randint(-1, 6, (3000, 2)).astype(np.int32)          # above N = 4 among them
    for scale in (2.0 ** 60, 2.0 ** 47, 2.0 ** 38, 2.0 ** 25, 1.0, 2.0 ** -60):
        mean = rng.standard_normal(3000) * (2.0 ** 39 / scale)
        mean[::11] = np.rint(mean[::11] * scale) / scale + 0.5 / scale      # ties
        mean[::13] = np.nan
        mean[5::17] *= 4.0                                          # past 2^40 / scale
        want = ref.accumulate_metric(node, mean, 4, scale)
        assert 0 < want[1].sum() < (node.min(axis=1) >= 0).sum()
        same_matrices(gpu_accumulate_metric(node, mean, 4, scale), want)


@pytest.mark.gpu
def test_accumulate_does_not_depend_on_order_or_split_and_fills_a_cell():
    n = 2048 * 256 + 777                                # more rows than one pass of the grid
    rng = np.random.RandomState(9)
    node = rng.randint(0, 4, (n, 2)).astype(np.int32)
    node[rng.randint(0, n, 1000)] = -1
    scale = 2.0 ** 39
    mean = rng.uniform(-1.0, 1.0, n)
    mean[rng.randint(0, n, 1000)] = np.nan
    keep = (node[:, 0] >= 0) & np.isfinite(mean)
    a, b = node[keep].min(axis=1), node[keep].max(axis=1)
    q, count = np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int64)
    np.add.at(q, (a, b), np.rint(mean[keep] * scale).astype(np.int64))
    np.add.at(count, (a, b), 1)
    same_matrices(gpu_accumulate_metric(node, mean, 3, scale), (q, count))
    order = rng.permutation(n)
    same_matrices(gpu_accumulate_metric(node[order], mean[order], 3, scale), (q, count))
    half = gpu_accumulate_metric(node[:n // 3], mean[:n // 3], 3, scale)
    same_matrices(gpu_accumulate_metric(node[n // 3:], mean[n // 3:], 3, scale, half), (q, count))
    # 2^23 streamlines of the largest mean fit in a cell: 2^17 rows of 2^40 - 1 here
    rows = 1 << 17
    big = np.full(rows, np.nextafter(2.0 ** 40, 0.0))
    got = gpu_accumulate_metric(np.ones((rows, 2), np.int32), big, 1, 1.0)
    assert int(got[0][1, 1]) == rows * 2 ** 40 and int(got[1][1, 1]) == rows


def box_labels(dims, n_nodes=6, seed=4):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, n_nodes + 1, dims).astype(np.int32)
    labels.flat[0] = n_nodes
    return labels


@pytest.mark.gpu
def test_connectome_with_metrics_does_not_depend_on_the_batch_split(sampled):
    from tracktolearn_amd import connectome as con_module
    from tracktolearn_amd.connectome import Connectome
    c, other = cases.case('holes_oblique'), cases.case('large_oblique')
    affine = np.eye(4)
    affine[:3, :3] = c.lin
    affine[:3, 3] = (3.0, -2.0, 1.0)
    labels = box_labels(c.dims)
    metrics = {'holes': c.volume, 'large': other.volume}
    # the second volume along the rows of the first set, in one launch
    own = {'holes': sampled['holes_oblique'][0],
           'large': con_module.sample_mean(_dev(c.points), _dev(c.offsets),
                                           _dev(np.array(other.volume)), c.lin)[0].cpu().numpy()}
    n = len(c.rows)
    orders = [(1, None), (3, None), (17, None), (1, 0), (5, 1)]
    results, raw = [], []
    for parts, seed in orders:
        rows = np.arange(n) if seed is None else np.random.RandomState(seed).permutation(n)
        con = Connectome(labels, affine, radius_mm=2.0, device=DEV, metrics=metrics)
        cuts = np.linspace(0, n, parts + 1).astype(int)
        nodes, means = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = [c.rows[r] for r in rows[lo:hi]]
            offsets = np.concatenate([[0], np.cumsum([len(r) for r in part])]).astype(np.int64)
            nodes.append(con.add(_dev(np.concatenate(part)), _dev(offsets)).cpu().numpy())
            means.append(con.last_means['holes'][0].cpu().numpy())
        node, mean = np.concatenate(nodes), np.concatenate(means)
        back = np.argsort(rows)
        # a row's mean does not depend on its neighbours in the launch: the set's own bits
        assert np.array_equal(mean[back], own['holes'], equal_nan=True)
        for name, mean_of in own.items():
            m = con.metrics[name]
            assert m['scale'] == ref.scale_for(metrics[name])
            # metric_q exactly, given the kernel's own means
            same_matrices((m['q'], m['n']),
                          ref.accumulate_metric(node[back], mean_of, con.n_nodes, m['scale']))
        results.append(con.matrices())
        raw.append({k: (v['q'].cpu().numpy(), v['n'].cpu().numpy())
                    for k, v in con.metrics.items()})
    assert metrics['holes'].shape == labels.shape
    assert con.metrics['holes']['scale'] != con.metrics['large']['scale']
    first = results[0]
    assert {'mean_holes', 'holes_n', 'mean_large', 'large_n'} <= set(first)
    assert first['mean_holes'].shape == (con.n_nodes, con.n_nodes)
    assert np.array_equal(first['mean_holes'], first['mean_holes'].T, equal_nan=True)
    assert np.array_equal(np.isnan(first['mean_holes']), first['holes_n'] == 0)
    assert 0 < first['holes_n'].sum() <= first['large_n'].sum() <= first['count'].sum()
    # the row whose one sampled point touches the NaN block is scored and has no mean
    assert raw[0]['holes'][1].sum() < raw[0]['large'][1].sum() <= int(con.count.sum())
    for other_result, other_raw in zip(results[1:], raw[1:]):
        assert set(other_result) == set(first)
        for key in first:
            assert np.array_equal(first[key], other_result[key], equal_nan=True), key
        for key in raw[0]:
            assert all(np.array_equal(a, b) for a, b in zip(raw[0][key], other_raw[key]))
    # without metrics: the same counts and lengths, and no key more than before
    plain = Connectome(labels, affine, radius_mm=2.0, device=DEV)
    plain.add(_dev(c.points), _dev(c.offsets))
    m = plain.matrices()
    assert set(m) == {'count', 'length_sum_mm', 'mean_length_mm', 'unassigned_one_end',
                      'unassigned_both'}
    for key in m:
        assert np.array_equal(m[key], first[key]), key
    assert 'metrics' not in plain.totals() and plain.last_means == {}


@pytest.mark.gpu
def test_save_writes_the_metric_files(tmp_path):
    from tracktolearn_amd.connectome import Connectome
    c = cases.case('small_axis')
    con = Connectome(box_labels(c.dims), np.eye(4), device=DEV, metrics={'fa': c.volume})
    con.add(_dev(c.points), _dev(c.offsets))
    files = con.save(str(tmp_path / 'con'))
    assert [os.path.basename(f) for f in files] == [
        'con_count.npy', 'con_mean_length.npy', 'con_count.csv', 'con.json', 'con_mean_fa.npy']
    assert np.array_equal(np.load(files[4]), con.matrices()['mean_fa'], equal_nan=True)
    assert np.isfinite(np.load(files[4])).sum() > 4
    totals = json.load(open(files[3]))
    assert totals['metrics'] == {'fa': {'scale': ref.scale_for(c.volume)}}
    plain = Connectome(box_labels(c.dims), np.eye(4), device=DEV)
    plain.add(_dev(c.points), _dev(c.offsets))
    files = plain.save(str(tmp_path / 'plain'))
    assert sorted(os.listdir(tmp_path)) == sorted(
        ['con_count.npy', 'con_mean_length.npy', 'con_count.csv', 'con.json', 'con_mean_fa.npy',
         'plain_count.npy', 'plain_mean_length.npy', 'plain_count.csv', 'plain.json'])
    assert 'metrics' not in json.load(open(files[3]))


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """The synthetic subject of tests/test_connectome.py with two scalar maps."""
    import test_connectome as base
    from tracktolearn_amd.io import nifti
    root = tmp_path_factory.mktemp('connectome_metric')
    sh, mask, _ = base.subject()
    seed_mask = np.zeros(mask.shape, np.uint8)
    seed_mask[5:11, 5:11, 5:11] = 1
    rng = np.random.RandomState(8)
    fa = rng.uniform(0.0, 1.0, mask.shape).astype(F32)
    md = (rng.uniform(0.2, 3.0, mask.shape) * 1e-3).astype(F32)
    for name, vol in (('fodf', sh), ('mask', mask), ('seed', seed_mask),
                      ('labels', base.painted_labels(mask)), ('fa', fa), ('md', md),
                      ('other_grid', np.ones(mask.shape[:2] + (mask.shape[2] + 1,), F32))):
        nifti.save(str(root / f'{name}.nii.gz'), vol, np.eye(4))
    return root


@pytest.mark.gpu
def test_tracked_metrics_are_those_of_the_file_it_wrote(files, capsys):
    """``ttl_track.py --connectome_metric`` streams what ``ttl_connectome.py
    --metric`` computes from the .tck of the same run (identity affine: the file's
    points are the tracker's), and a run without metrics counts the same."""
    import test_connectome as base
    from tracktolearn_amd.runners import ttl_connectome, ttl_track
    labels = str(files / 'labels.nii.gz')
    fa, md = 'fa=' + str(files / 'fa.nii.gz'), 'md=' + str(files / 'md.nii.gz')
    ttl_track.main(base._argv(files, 'with.tck', '--connectome', labels, '--connectome_out',
                              str(files / 'with'), '--connectome_metric', fa,
                              '--connectome_metric', md))
    n_saved = int(re.search(r'Saved (\d+) streamlines to', capsys.readouterr().out).group(1))
    ttl_track.main(base._argv(files, 'plain.tck', '--connectome', labels, '--connectome_out',
                              str(files / 'plain')))
    capsys.readouterr()
    ttl_connectome.main([str(files / 'with.tck'), labels, str(files / 'cmd'), '--reference',
                         str(files / 'mask.nii.gz'), '--metric', fa, '--metric', md,
                         '--save_assignments'])
    totals = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert n_saved > 50 and totals['streamlines'] == n_saved
    assert set(totals['metrics']) == {'fa', 'md'}
    assert totals['metrics']['fa']['scale'] == 2.0 ** 39
    assert totals['metrics']['md']['scale'] == 2.0 ** 47
    streamed = json.load(open(str(files / 'with.json')))
    assert streamed['metrics'] == totals['metrics'] and streamed['streamlines'] == n_saved
    assert 'metrics' not in json.load(open(str(files / 'plain.json')))
    for suffix in ('_count.npy', '_mean_length.npy', '_mean_fa.npy', '_mean_md.npy'):
        tracked, from_file = np.load(str(files / 'with') + suffix), np.load(
            str(files / 'cmd') + suffix)
        assert np.array_equal(tracked, from_file, equal_nan=True), suffix
    for suffix in ('_count.npy', '_mean_length.npy'):
        assert np.array_equal(np.load(str(files / 'plain') + suffix),
                              np.load(str(files / 'with') + suffix)), suffix
    assert not os.path.exists(str(files / 'plain_mean_fa.npy'))
    count, mean_fa = np.load(str(files / 'cmd_count.npy')), np.load(str(files / 'cmd_mean_fa.npy'))
    assert mean_fa.shape == count.shape == (8, 8)
    assert np.array_equal(np.isfinite(mean_fa), count > 0)         # every streamline is inside
    assert (mean_fa[count > 0] > 0.0).all() and (mean_fa[count > 0] < 1.0).all()
    mean_md = np.load(str(files / 'cmd_mean_md.npy'))
    assert (mean_md[count > 0] > 1.9e-4).all() and (mean_md[count > 0] < 3.1e-3).all()
    # the per-streamline means and weights beside the nodes
    nodes = np.load(str(files / 'cmd_nodes.npy'))
    rows = np.load(str(files / 'cmd_fa_streamlines.npy'))
    assert rows.shape == (n_saved, 3) and np.array_equal(rows[:, 0], np.arange(n_saved))
    assert np.isfinite(rows[:, 1]).all() and (rows[:, 2] > 1.0).all()     # min_length 2 mm
    edge = (nodes[:, 1] == 1) & (nodes[:, 2] == 1)
    if edge.any():
        q = np.rint(rows[edge, 1] * 2.0 ** 39).sum() / 2.0 ** 39 / edge.sum()
        assert mean_fa[0, 0] == q
    with pytest.raises(ValueError, match='not on the grid'):
        ttl_track.main(base._argv(files, 'never.tck', '--connectome', labels, '--connectome_out',
                                  str(files / 'never'), '--connectome_metric',
                                  'fa=' + str(files / 'other_grid.nii.gz')))
    with pytest.raises(ValueError, match='not on the grid'):
        ttl_connectome.main([str(files / 'with.tck'), labels, str(files / 'never'),
                             '--reference', str(files / 'mask.nii.gz'), '--metric',
                             'fa=' + str(files / 'other_grid.nii.gz')])
