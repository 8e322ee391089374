"""Bundle recognition (include/ttl_hip.h, ttl_bundle_recognize): on
the CPU a hand-computed case, a witness for every named mutant, the decidedness
of the GPU cases, the header, the refusals, the Python layer's argument checks,
the gates on fabricated kernel outputs and the command's options; on the GPU the
kernel against the reference (winner and flip on every decided row and on the
built ties, mdf and runner_up inside the reference's intervals, NaN patterns
exactly), the independence of row order, split and model order bit for bit, the
agreement with ttl_bundle_orient, and the chain profile -> recognise -> profile
end to end."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bundle_recognize_cases as cases
import ref_bundle_profile
import ref_bundle_recognize as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
I64 = np.int64
LD = ref.LD


def _ref(c, mutant=None):
    return ref.recognize(c['points'], c['offsets'], c['models'], c['lin'], c['label'], mutant)


# ------------------------------------------------------------------ CPU part
def test_three_models_by_hand():
    """2 mm voxels, K = 3, stations = points.  Row 0 is model 0 backwards: F_0 = 0
    (D_0 = (4 + 0 + 4) / 3), model 1 is 2 mm away and of the same bundle, so the
    runner-up is model 2 at 3.5 voxels = 7 mm.  Row 1 is 1 voxel = 2 mm from model
    2 and 1.5 voxels = 3 mm from model 1 of the other bundle."""
    got = _ref(cases.hand())
    assert got['best'].tolist() == [0, 2] and got['flip'].tolist() == [1, 0]
    assert [float(v) for v in got['mdf']] == [0.0, 2.0]
    assert [float(v) for v in got['runner_up']] == [7.0, 3.0]
    assert got['decided'].all() and got['part'].all()
    assert float(got['D'][0, 0]) == float(LD(8) / LD(3)) and float(got['F'][0, 1]) == 2.0
    assert (got['mdf_lo'] <= got['mdf']).all() and (got['mdf'] <= got['mdf_hi']).all()
    assert (got['ru_lo'] <= got['runner_up']).all() and (got['runner_up'] <= got['ru_hi']).all()


def test_pair_distances_are_the_profile_references():
    c = cases.case(64, 63, 70, 'oblique', 'grouped')
    a = c['models'][0][::-1]
    for magnitudes in (False, True):
        every = ref.pair_distances(a, c['models'], c['lin'], magnitudes)
        for m in (0, 1, 5, 6, 62):
            one = ref_bundle_profile.distances(a, c['models'][m], c['lin'], magnitudes)
            assert np.array_equal(every[m], one, equal_nan=True)


WITNESS = {'highest_index_on_tie': ('best', 0), 'flip_on_tie': ('flip', 1),
           'distance_in_voxels': ('best', 2), 'squared_distances': ('best', 2),
           'direct_only': ('best', 3), 'flip_of_last_model': ('flip', 3),
           'runner_up_same_label': ('runner_up', 2), 'nan_wins': ('best', 0),
           'short_row_takes_part': ('best', 4)}


def test_every_mutant_is_named_once():
    assert set(WITNESS) == set(ref.MUTANTS) and len(ref.MUTANTS) == 9


def test_the_witness_set_by_the_definition():
    good = _ref(cases.witness())
    assert good['best'].tolist() == [0, 2, 3, 5, -1] and good['flip'].tolist() == [0, 0, 0, 1, 0]
    assert good['decided'].tolist() == [False, False, True, True, True]
    assert good['runner_up'][0] > good['mdf'][0]        # models 0 and 1 are one label
    assert not np.isnan(good['runner_up'][:4].astype(np.float64)).any()


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_mutants_have_a_witness(mutant):
    w = cases.witness()
    good, bad = _ref(w), _ref(w, mutant)
    key, row = WITNESS[mutant]
    assert good[key][row] != bad[key][row]


CASE_KEYS = cases.GPU_CASES + ['all_nan']


def _case(key):
    return cases.all_nan_case() if key == 'all_nan' else cases.case(*key)


@pytest.mark.parametrize('key', CASE_KEYS, ids=str)
def test_cases_leave_only_the_built_ties_undecided(key):
    """Against the reference alone: the only rows that are not decided are the
    ties built on purpose, and the reference resolves them as the header says --
    the lower index of a duplicated model (with runner_up == mdf when the two are
    of different labels), no flip for the row that reads the same both ways."""
    c = _case(key)
    r = cases.reference(key)
    s = c['special']
    assert np.flatnonzero(r['part'] & ~r['decided']).tolist() == cases.ties(c)
    for name in ('nan', 'inf', 'single'):
        if name in s:
            assert not r['part'][s[name]] and r['best'][s[name]] == -1
    if 'tie_same' in s:
        assert r['best'][s['tie_same']] == 1 and r['flip'][s['tie_same']] == 0
        assert np.array_equal(r['D'][:, 1], r['D'][:, 3], equal_nan=True)
    if 'tie_cross' in s:
        row = s['tie_cross']
        assert r['best'][row] == 2 and r['flip'][row] == 1
        assert r['runner_up'][row] == r['mdf'][row]
    if 'tie_flip' in s:
        row = s['tie_flip']
        assert r['best'][row] == 7 and r['flip'][row] == 0
        assert r['D'][row, 7] == r['F'][row, 7]
    if key == 'all_nan':
        assert (r['best'] == -1).all() and r['part'].any()
    elif c['M'] >= 8 and len(c['offsets']) > 16:
        assert not np.isin(r['best'], (5, 6)).any()     # the NaN and the Inf station
        assert np.isnan(r['D'][r['part']][:, 5].astype(np.float64)).all()
        assert (r['flip'][r['part']] == 1).any() and (r['flip'][r['part']] == 0).any()
        labelled_one = c['label'] is not None and len(set(c['label'].tolist())) == 1
        assert np.isnan(r['runner_up'][r['part']].astype(np.float64)).all() == labelled_one


def test_the_cases_cover_the_issue_ranges():
    keys = cases.GPU_CASES
    assert sorted({k[0] for k in keys}) == list(cases.KS)
    assert sorted({k[1] for k in keys}) == list(cases.MS)
    assert cases.TILE_MODELS + 1 in cases.MS            # one model more than the LDS tile
    assert sorted({k[2] for k in keys}) == list(cases.NS)
    assert 70 > 8 * cases.WORKGROUP_ROWS and 70 % cases.WORKGROUP_ROWS
    assert {k[3] for k in keys} == set(cases.LINS)
    assert {k[4] for k in keys} == {'null', 'grouped', 'one'}
    assert (2, 4096) in {k[:2] for k in keys}
    big = cases.case(65, 64, 300, 'axis', 'grouped')
    assert set(big['special']) == {'nan', 'inf', 'single', 'tie_same', 'tie_cross', 'tie_flip'}
    assert set(cases.LENGTHS) <= set(np.diff(big['offsets']).tolist())
    assert (big['label'] < 0).any() and len(set(big['label'].tolist())) < big['M']
    assert 'tie_flip' in cases.case(2, 4096, 70, 'axis', 'grouped')['special']


def test_header_announces_the_feature_and_keeps_the_abi():
    from tracktolearn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'^#define TTL_HAS_BUNDLE_RECOGNIZE 1$', header, re.M)
    assert re.search(r'^#define TTL_RECOGNIZE_MAX_MODELS 4096$', header, re.M)
    assert re.search(r'^#define TTL_ABI_VERSION 13$', header, re.M)
    assert header.index('TTL_HAS_BUNDLE_PROFILE 1') < header.index('TTL_HAS_BUNDLE_RECOGNIZE 1')
    assert (_lib.HAS_BUNDLE_RECOGNIZE, _lib.RECOGNIZE_MAX_MODELS, _lib.ABI_VERSION) == (1, 4096, 13)
    lib = _lib.load()
    name = 'ttl_bundle_recognize'
    assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    assert re.search(r'^TTL_API int ' + name + r'\(', header, re.M)
    from tracktolearn_amd.csrc import build
    assert any(s.endswith('ttl_bundle_recognize.hip') for s in build.SOURCES)


def _args():
    p = C.c_void_p(4096)                # never dereferenced: every call here is refused or a no-op
    return dict(points=p, offsets=p, n=0, models=p, label=p, n_models=21, nb_points=20,
                lin=(C.c_double * 9)(*np.eye(3).reshape(-1)), best=p, flip=p, mdf=p,
                runner_up=p, stream=None)


INVALID = [(k, None) for k in ('points', 'offsets', 'models', 'lin', 'best', 'flip', 'mdf')] + \
    [('n', -1), ('n_models', 0), ('n_models', 4097), ('nb_points', 1), ('nb_points', 257)]


def test_refusals_come_before_any_hip_call():
    from tracktolearn_amd import _lib
    lib = _lib.load()
    call = lib.ttl_bundle_recognize
    assert call(*_args().values()) == 0                 # n == 0: a no-op
    for ok in (dict(label=None), dict(runner_up=None), dict(n_models=1, nb_points=2),
               dict(n_models=4096, nb_points=256)):
        assert call(*dict(_args(), **ok).values()) == 0
    for key, value in INVALID:
        assert call(*dict(_args(), **{key: value}).values()) == _lib.ERR_INVALID, (key, value)
        assert b'ttl_bundle_recognize' in lib.ttl_last_error()


def test_python_layer_refuses_with_the_shape_wanted():
    import torch
    from tracktolearn_amd.bundle_recognize import BundleAtlas, bundle_recognize
    points = torch.zeros((4, 3), dtype=torch.float32)
    offsets = torch.tensor([0, 2, 4], dtype=torch.int64)
    models = torch.zeros((3, 5, 3), dtype=torch.float32)
    label = torch.zeros(3, dtype=torch.int32)
    lin = np.eye(3)
    for bad, word in (((points.double(), offsets, models, lin), r'\(P, 3\) float32'),
                      ((points, offsets.int(), models, lin), r'\(n \+ 1,\) int64'),
                      ((points, offsets, models.double(), lin), r'\(M, K, 3\) float32'),
                      ((points, offsets, models[:, :, :2].contiguous(), lin), r'\(M, K, 3\)'),
                      ((points, offsets, models[:, :1].contiguous(), lin), '2 .. 256 stations'),
                      ((points, offsets, torch.zeros((4097, 2, 3)), lin), '1 .. 4096 lines'),
                      ((points, offsets, models, lin, label[:2]), r'\(3,\) int32'),
                      ((points, offsets, models, lin, label.long()), r'\(3,\) int32'),
                      ((points, offsets, models, np.eye(4)), r'\(3, 3\)')):
        with pytest.raises(ValueError, match=word):
            bundle_recognize(*bad)
    best, flip, mdf, second = bundle_recognize(points[:0], offsets[:1], models, lin)
    assert best.shape == (0,) and second is None        # no rows: no launch
    dims, affine = (7, 6, 5), np.diag([2.0, 2.0, 2.0, 1.0])
    lines = np.zeros((3, 5, 3))
    for args, kw, word in (((dims, None, lines, list('abc')), {}, 'affine'),
                           ((dims, affine, lines[:, :1], list('abc')), {}, r'\(M, K, 3\)'),
                           ((dims, affine, lines, list('ab')), {}, 'as many names'),
                           ((dims, affine, lines, list('aab')), {}, 'distinct'),
                           ((dims, affine, lines, list('ab')), {'label': [0, 1, 2]}, '0 .. 1'),
                           ((dims, affine, lines, list('ab')), {'label': [0, 1]}, r'\(3,\)')):
        with pytest.raises(ValueError, match=word):
            BundleAtlas(*args, **kw)
    atlas = BundleAtlas(dims, affine, lines, list('ab'), label=[1, 0, 1], device='cpu')
    assert atlas.one_model_per_label() is None
    with pytest.raises(ValueError, match='comes before'):
        atlas.summary()
    one = BundleAtlas(dims, affine, np.arange(18.0).reshape(2, 3, 3), list('ab'), label=[1, 0],
                      device='cpu')
    assert np.array_equal(one.one_model_per_label(), one.models_vox[::-1])


def test_gates_on_fabricated_kernel_outputs():
    """The two gates in their order, a NaN runner_up passing the ratio gate, and
    the streamlines the intake dropped."""
    from tracktolearn_amd.bundle_recognize import BundleAtlas, apply_gates
    nan = np.nan
    atlas = BundleAtlas((7, 6, 5), np.diag([2.0, 2.0, 2.0, 1.0]), np.zeros((3, 4, 3)),
                        ['left', 'right'], label=[1, 0, 1], device='cpu')
    index = np.array([0, 1, 3, 4, 5, 7])                # inputs 2 and 6 were dropped
    best = np.array([0, 1, 2, -1, 0, 1], np.int32)
    flip = np.array([1, 0, 1, 0, 0, 1], np.int32)
    mdf = np.array([1.0, 6.0, 3.0, nan, 2.0, 4.0])
    second = np.array([8.0, 6.5, 3.5, nan, nan, 100.0])
    got = atlas.assemble(8, index, best, flip, mdf, second)
    assert got['bundle'].tolist() == [1, 0, -1, 1, -1, 1, -1, 0]
    assert got['model'].tolist() == [0, 1, -1, 2, -1, 0, -1, 1]
    assert got['flip'].tolist() == [1, 0, 0, 1, 0, 0, 0, 1]
    assert np.array_equal(got['mdf'], [1.0, 6.0, nan, 3.0, nan, 2.0, nan, 4.0], equal_nan=True)
    assert np.array_equal(got['runner_up'], [8.0, 6.5, nan, 3.5, nan, nan, nan, 100.0],
                          equal_nan=True)
    assert got['index'] is not None and got['index'].tolist() == index.tolist()
    assert atlas.summary() == {'left': {'n': 2, 'mdf_mean': 5.0, 'n_gated': 0},
                               'right': {'n': 3, 'mdf_mean': 2.0, 'n_gated': 0}}
    # max_mdf 5: input 1 goes; max_ratio 0.5: input 3 (3 > 1.75) goes, input 5 (NaN) stays
    got = atlas.assemble(8, index, best, flip, mdf, second, max_mdf=5.0, max_ratio=0.5)
    assert got['bundle'].tolist() == [1, -1, -1, -1, -1, 1, -1, 0]
    assert got['model'].tolist() == [0, 1, -1, 2, -1, 0, -1, 1]     # the winner is still told
    summary = atlas.summary()
    assert summary['left'] == {'n': 1, 'mdf_mean': 4.0, 'n_gated': 1}
    assert summary['right'] == {'n': 2, 'mdf_mean': 1.5, 'n_gated': 1}
    # the order: a row beyond max_mdf is gone before the ratio is asked
    bundle = np.array([0, 0, 0, -1], np.int32)
    d, s = np.array([6.0, 6.0, 1.0, nan]), np.array([nan, 7.0, 3.0, nan])
    assert apply_gates(bundle, d, s).tolist() == [0, 0, 0, -1]
    assert apply_gates(bundle, d, s, max_mdf=5.0).tolist() == [-1, -1, 0, -1]
    assert apply_gates(bundle, d, s, max_ratio=0.5).tolist() == [0, -1, 0, -1]
    assert apply_gates(bundle, d, s, max_ratio=0.25).tolist() == [0, -1, -1, -1]
    assert apply_gates(bundle, d, s, 6.0, 1.0).tolist() == [0, 0, 0, -1]    # both are strict


def test_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_recognize_bundles as cmd
    shim = open(os.path.join(ROOT, 'ttl_recognize_bundles.py')).read()
    assert 'from tracktolearn_amd.runners.ttl_recognize_bundles import main' in shim
    with pytest.raises(SystemExit) as e:
        cmd.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('in_tractogram', 'reference', 'atlas', 'out_prefix', '--atlas_labels IDS.npy',
                '--nb_points K', '--atlas_names NAMES.json', '--max_mdf MM', '--max_ratio R',
                '--save_bundles', '--profile NAME=MAP', '-f'):
        assert opt in text
    for name in ('t.trk', 't.txt', 'ref.nii.gz', 'fa.nii.gz', 'a_centroids.npy', 'a.trk',
                 'ids.npy', 'a.txt', 'held_bundles.npy', 'prof_profiles.json'):
        (tmp_path / name).write_bytes(b'')
    p = lambda name: str(tmp_path / name)
    base = [p('t.trk'), p('ref.nii.gz')]
    args = cmd.parse_args(base + [p('a_centroids.npy'), p('out')])
    assert args.profile == {} and args.max_mdf is None and args.max_ratio is None
    assert not args.save_bundles and args.atlas_labels is None
    args = cmd.parse_args(base + [p('a.trk'), p('out'), '--atlas_labels', p('ids.npy'),
                                  '--nb_points', '12', '--max_mdf', '8', '--max_ratio', '0.8',
                                  '--profile', 'fa=' + p('fa.nii.gz'), '--save_bundles'])
    assert (args.nb_points, args.max_mdf, args.max_ratio) == (12, 8.0, 0.8)
    assert args.profile == {'fa': p('fa.nii.gz')} and args.save_bundles
    assert cmd.parse_args(base + [p('a_centroids.npy'), p('held'), '-f'])
    assert cmd.parse_args(base + [p('a_centroids.npy'), p('prof')])    # no --profile: not written
    npy = p('a_centroids.npy')
    for argv, word in (
            ([p('t.txt'), p('ref.nii.gz'), npy, p('out')], '.trk or .tck'),
            ([p('t.trk'), p('no.nii.gz'), npy, p('out')], 'does not exist'),
            (base + [p('a.txt'), p('out')], '_centroids.npy'),
            (base + [p('a.trk'), p('out')], '--atlas_labels'),
            (base + [npy, p('out'), '--atlas_labels', p('ids.npy')], 'only with'),
            (base + [npy, p('out'), '--nb_points', '20'], 'only with'),
            (base + [p('a.trk'), p('out'), '--atlas_labels', p('ids.npy'), '--nb_points', '257'],
             '2 .. 256'),
            (base + [npy, p('out'), '--max_mdf', '0'], 'positive'),
            (base + [npy, p('out'), '--max_ratio', '-1'], 'positive'),
            (base + [npy, p('out'), '--profile', 'fa'], 'NAME=MAP'),
            (base + [npy, p('held')], 'use -f'),
            (base + [npy, p('prof'), '--profile', 'fa=' + p('fa.nii.gz')], 'use -f')):
        with pytest.raises(SystemExit) as e:
            cmd.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


# ----------------------------------------------------------------- GPU tests
def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _rows(c, rows):
    if rows is None:
        return c['points'], c['offsets']
    return cases.pack([c['points'][c['offsets'][s]:c['offsets'][s + 1]] for s in rows])


def _recognize(c, rows=None, models=None, label='case', runner_up=True):
    from tracktolearn_amd.bundle_recognize import bundle_recognize
    points, offsets = _rows(c, rows)
    label = c['label'] if isinstance(label, str) else label
    got = bundle_recognize(_dev(points), _dev(offsets),
                           _dev(c['models'] if models is None else models), c['lin'],
                           label=None if label is None else _dev(label, np.int32),
                           runner_up=runner_up)
    return {k: None if v is None else v.cpu().numpy()
            for k, v in zip(('best', 'flip', 'mdf', 'runner_up'), got)}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(I64)


def _inside(value, lo, hi):
    """NaN exactly where the interval is NaN, inside it elsewhere."""
    nan = np.isnan(lo.astype(np.float64))
    assert np.array_equal(np.isnan(value), nan)
    v = value[~nan].astype(LD)
    return bool((lo[~nan] <= v).all() and (v <= hi[~nan]).all())


@pytest.mark.gpu
@pytest.mark.parametrize('key', CASE_KEYS, ids=str)
def test_kernel_is_the_reference(key):
    """best and flip are the reference's on every decided row and on the built
    ties; mdf and runner_up lie inside the reference's intervals on every row, NaN
    exactly where it has none; a row without a winner is -1 / 0 / NaN / NaN; on the
    tie across two labels runner_up is mdf bit for bit; runner_up is optional."""
    c = _case(key)
    r = cases.reference(key)
    got = _recognize(c)
    check = r['decided'].copy()
    check[cases.ties(c)] = True
    assert np.array_equal(got['best'][check], r['best'][check])
    assert np.array_equal(got['flip'][check], r['flip'][check])
    assert _inside(got['mdf'], r['mdf_lo'], r['mdf_hi'])
    assert _inside(got['runner_up'], r['ru_lo'], r['ru_hi'])
    none = r['best'] == -1
    assert (got['best'][none] == -1).all() and not got['flip'][none].any()
    assert np.isnan(got['mdf'][none]).all() and np.isnan(got['runner_up'][none]).all()
    if 'tie_cross' in c['special']:
        row = c['special']['tie_cross']
        assert _bits(got['runner_up'][row]) == _bits(got['mdf'][row])
    again = _recognize(c, runner_up=False)
    assert again['runner_up'] is None
    for k in ('best', 'flip'):
        assert np.array_equal(again[k], got[k])
    assert np.array_equal(_bits(again['mdf']), _bits(got['mdf']))


@pytest.mark.gpu
@pytest.mark.parametrize('key', [(65, 64, 300, 'axis', 'grouped'), (2, 4096, 70, 'axis', 'grouped'),
                                 (256, 65, 70, 'anisotropic', 'one')], ids=str)
def test_bits_do_not_depend_on_row_order_split_or_model_order(key):
    c = cases.case(*key)
    whole = _recognize(c)
    n = len(c['offsets']) - 1
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)
    shuffled = _recognize(c, perm)
    for k in ('best', 'flip'):
        assert np.array_equal(shuffled[k], whole[k][perm])
    for k in ('mdf', 'runner_up'):
        assert np.array_equal(_bits(shuffled[k]), _bits(whole[k][perm]))
    first, second = np.arange(n)[:n // 3 + 1], np.arange(n)[n // 3 + 1:]
    parts = [_recognize(c, first), _recognize(c, second)]
    for k in ('best', 'flip'):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    for k in ('mdf', 'runner_up'):
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k]))
    # the models permuted: indices mapped back, on the rows without a built tie
    order = rng.permutation(c['M'])                      # new position j holds model order[j]
    moved = _recognize(c, models=c['models'][order],
                       label=None if c['label'] is None else c['label'][order])
    if c['label'] is None:                  # every model its own label either way
        moved = _recognize(c, models=c['models'][order], label=None)
    plain = np.ones(n, bool)
    plain[cases.ties(c)] = False
    back = np.where(moved['best'] >= 0, order[np.clip(moved['best'], 0, None)], -1)
    assert np.array_equal(back[plain], whole['best'][plain])
    assert np.array_equal(moved['flip'][plain], whole['flip'][plain])
    for k in ('mdf', 'runner_up'):
        assert np.array_equal(_bits(moved[k][plain]), _bits(whole[k][plain]))


@pytest.mark.gpu
@pytest.mark.parametrize('key', [k for k in cases.GPU_CASES if k[1] <= 64], ids=str)
def test_bundle_orient_agrees_on_the_winner(key):
    """ttl_bundle_orient with bundle = best: the same flip on the decided rows and
    an mdf within the sum of the two kernels' bounds of ours (each is within (K +
    8) u A of the exact value)."""
    import torch
    from tracktolearn_amd.bundle_profile import bundle_orient
    c = cases.case(*key)
    r = cases.reference(key)
    got = _recognize(c)
    M, K = c['M'], c['K']
    sums = (torch.zeros((M, K, 3), dtype=torch.int64, device=DEV),
            torch.zeros(M, dtype=torch.int64, device=DEV))
    flip, mdf = bundle_orient(_dev(c['points']), _dev(c['offsets']), _dev(got['best']), M, K,
                              _dev(c['models']), c['lin'], 2.0 ** 30, *sums)
    flip, mdf = flip.cpu().numpy(), mdf.cpu().numpy()
    assert np.array_equal(np.isnan(mdf), np.isnan(got['mdf']))
    assert np.array_equal(flip[r['decided']], got['flip'][r['decided']])
    won = np.flatnonzero(got['best'] >= 0)
    w = got['best'][won]
    bound = np.where(got['flip'][won] != 0, r['bound_f'][won, w], r['bound_d'][won, w])
    assert (np.abs(mdf[won].astype(LD) - got['mdf'][won].astype(LD)) <= 2 * bound).all()
    assert int(sums[1].sum().item()) == len(won)


def _planted():
    """Two crossing bundles of 20 streamlines each on a 12 x 8 x 8 grid of 2 mm
    voxels (ends spread by +-0.5 voxels, every second one stored backwards), 5
    noise streamlines far from both and one of a single point: RAS mm lines and
    the planted numbers."""
    rng = np.random.default_rng(4)
    ends = [((2.0, 4.0, 4.0), (10.0, 4.0, 4.0)), ((6.0, 1.5, 2.0), (6.0, 6.5, 6.0))]
    t = np.linspace(0.0, 1.0, 25)[:, None]
    lines, ids = [], []
    for i in range(40):
        b = i % 2
        a = np.asarray(ends[b][0]) + rng.uniform(-0.5, 0.5, 3)
        e = np.asarray(ends[b][1]) + rng.uniform(-0.5, 0.5, 3)
        ras = (((a + t * (e - a)) - 0.5) * 2.0).astype(F32)
        lines.append(ras[::-1] if (i // 2) % 2 else ras)
        ids.append(b)
        if i % 8 == 3:                      # noise: short lines in a corner, > 3 voxels away
            a = np.array([1.0, 7.0, 1.0]) + rng.uniform(-0.5, 0.5, 3)
            ras = (((a + t[:5] * (2.0, 0.0, 0.5)) - 0.5) * 2.0).astype(F32)
            lines.append(ras)
            ids.append(-1)
    lines.append(np.array([[3.0, 3.0, 3.0]], F32))
    ids.append(-1)
    return lines, np.asarray(ids, np.int64)


def _strict(path):
    def refuse(word):
        raise ValueError(f'{path}: {word} is not JSON')
    return json.load(open(path), parse_constant=refuse)


@pytest.mark.gpu
def test_profile_recognize_profile_end_to_end(tmp_path, capsys):
    """BundleProfiles makes the atlas from the planted numbers; the command
    recovers them with --max_mdf gating the noise; its _bundles.npy gives
    ttl_bundle_profile.py the profiles the planted numbers give, byte for byte,
    and --profile writes that file in the same run."""
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_bundle_profile as profile_cmd
    from tracktolearn_amd.runners import ttl_recognize_bundles as cmd
    from tracktolearn_amd.tractogram import Tractogram
    dims, affine = (12, 8, 8), np.diag([2.0, 2.0, 2.0, 1.0])
    lines, ids = _planted()
    p = lambda name: str(tmp_path / name)
    sio.save(Tractogram(lines, affine_to_rasmm=np.eye(4)), p('in.trk'),
             sio.create_tractogram_header(affine, dims, (2.0, 2.0, 2.0)))
    grid = np.stack(np.meshgrid(*(np.arange(d) + 0.5 for d in dims), indexing='ij'), -1)
    ramp = (1.0 + 0.125 * grid[..., 0] + 0.25 * grid[..., 1] + 0.375 * grid[..., 2]).astype(F32)
    nifti.save(p('ramp.nii.gz'), ramp, affine)
    nifti.save(p('ref.nii.gz'), np.zeros(dims, np.uint8), affine)
    np.save(p('planted.npy'), ids)
    metric = 'ramp=' + p('ramp.nii.gz')
    profile_cmd.main([p('in.trk'), p('ref.nii.gz'), p('atlas'), '--metric', metric, '--bundles',
                      p('planted.npy'), '--nb_points', '17'])
    gate = ['--max_mdf', '4']
    cmd.main([p('in.trk'), p('ref.nii.gz'), p('atlas_centroids.npy'), p('got'), '--atlas_names',
              p('atlas_profiles.json'), '--save_bundles', '--profile', metric] + gate)
    capsys.readouterr()
    bundles = np.load(p('got_bundles.npy'))
    assert bundles.dtype == np.int32 and np.array_equal(bundles, ids)
    record = np.load(p('got_recognized.npy'))
    assert record.dtype.names == ('model', 'flip', 'mdf', 'runner_up') and len(record) == len(ids)
    assert (record['model'][:-1] >= 0).all() and record['model'][-1] == -1   # the noise has a winner
    assert (record['mdf'][ids >= 0] < 4.0).all() and (record['mdf'][:-1][ids[:-1] < 0] > 4.0).all()
    assert np.isnan(record['mdf'][-1]) and not np.isnan(record['runner_up'][:-1]).any()
    backwards = np.array([(i // 2) % 2 for i in range(40)])
    # the atlas runs L -> R and P -> A (the canonical direction): a row stored backwards flips
    assert np.array_equal(record['flip'][ids >= 0], backwards)
    summary = _strict(p('got_recognized.json'))
    assert summary['bundle_0']['n'] == summary['bundle_1']['n'] == 20
    assert summary['bundle_0']['n_gated'] + summary['bundle_1']['n_gated'] == 5
    for b in (0, 1):
        assert len(sio.load_trk(p(f'got_bundle_{b}.trk'))[0].streamlines) == 20
    with_model = ['--metric', metric, '--nb_points', '17', '--model', p('atlas_centroids.npy')]
    profile_cmd.main([p('in.trk'), p('ref.nii.gz'), p('fed'), '--bundles', p('got_bundles.npy')] +
                     with_model + gate)
    profile_cmd.main([p('in.trk'), p('ref.nii.gz'), p('want'), '--bundles', p('planted.npy')] +
                     with_model + gate)
    capsys.readouterr()
    want = open(p('want_profiles.json'), 'rb').read()
    assert open(p('fed_profiles.json'), 'rb').read() == want
    assert open(p('got_profiles.json'), 'rb').read() == want
    assert _strict(p('want_profiles.json'))['bundle_1']['n'] == 20
    assert np.array_equal(np.load(p('got_centroids.npy')), np.load(p('want_centroids.npy')))
    with pytest.raises(SystemExit):         # the outputs exist now
        cmd.parse_args([p('in.trk'), p('ref.nii.gz'), p('atlas_centroids.npy'), p('got')])
    capsys.readouterr()
