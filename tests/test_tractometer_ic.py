"""The Tractometer's invalid connections and full scores
(experiment/tractometer_validator.py, ``ttl_tractometer_invalid`` of
csrc/ttl_tractometer.hip, runners/ttl_score_tractogram.py) against their NumPy
definition (tests/ref_tractometer_ic.py) on the case sets of
tests/tractometer_ic_cases.py.  Integers throughout: every comparison is exact.

On the CPU: the definition against hand-written pairs, a witness for every
named mutant in the sets the GPU tests launch, ``rois_and_pairs``, the packed
words, the score arithmetic, the unchanged default dict, the argument errors of
the new entry, the header and the command's ``--help``.  On the GPU: ``pair``
on every set, 40 000 rows, more rows than one pass of the capped grid holds, a
scoring directory end to end (memory, ``.trk``, command, ``--save_bundles``) and
the trainer's ``--tractometer_compute_ic``."""
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ref_tractometer as ref
import ref_tractometer_ic as ric
import tractometer_cases as tc
import tractometer_ic_cases as ic
from tractometer_cases import AFFINE, _box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
BIG_ROWS = 600000           # more than one pass of the capped grid (ic.GRID_PASS)


# ------------------------------------------------------------------ helpers
def _data(rois, valid, device=DEV):
    """A ScoringData that holds the ROI planes (its one bundle is not used)."""
    from tracktolearn_amd.experiment.tractometer_validator import ScoringData, limits_table
    none = np.zeros(ic.DIMS, bool)
    return ScoringData(ic.DIMS, [none], [none], [None], [None], [None],
                       limits_table([None], [None], [None], [None]), device,
                       roi_masks=rois, valid=valid)


def _run(c):
    """``pair`` of the library call on a case, as NumPy."""
    from tracktolearn_amd.experiment.tractometer_validator import invalid
    data = _data(c['rois'], c['valid'])
    pair = invalid(torch.from_numpy(c['points']).to(DEV), torch.from_numpy(c['offsets']).to(DEV),
                   torch.from_numpy(c['bundle']).to(DEV), data)
    torch.cuda.synchronize()
    return pair.cpu().numpy()


# ----------------------------------------------------------------- CPU tests
def test_definition_on_hand_written_pairs():
    """Four ROIs on a line of voxels, (0, 1) and (2, 3) valid: P = [(0, 2),
    (0, 3), (1, 2), (1, 3)]."""
    dims = (6, 1, 1)
    rois = [np.zeros(dims, bool) for _ in range(4)]
    rois[0][0:2] = rois[1][1:3] = rois[2][3:5] = rois[3][4:6] = True     # 0|01|1|2|23|3
    valid = np.eye(4, dtype=bool)
    valid[0, 1] = valid[1, 0] = valid[2, 3] = valid[3, 2] = True
    assert ric.pair_list(valid) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    assert ric.pair_list(valid, 'valid_kept') == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]

    def x(*xs):
        return np.array([(v, 0.5, 0.5) for v in xs], np.float32)

    lines = [x(0.5, 3.5),            # {0} -> {2}: (0, 2)
             x(3.5, 0.5),            # the other order: (0, 2)
             x(0.5, 2.5),            # {0} -> {1}: valid only
             x(1.5, 4.5),            # {0, 1} -> {2, 3}: (0, 2) is the first of four
             x(2.5, 4.5),            # {1} -> {2, 3}: (1, 2)
             x(2.5, 5.5),            # {1} -> {3}: (1, 3)
             x(1.5, 1.5),            # {0, 1} -> {0, 1}: (0, 1) is valid
             x(0.5, 0.9),            # {0} -> {0}
             x(4.5, 3.2, 4.9),       # {2, 3} -> {2, 3}: (2, 3) is valid
             x(5.5, 1.5),            # {3} -> {0, 1}: (0, 3)
             x(5.5, 1.5),            # ... but it carries a bundle
             x(0.5),                 # one point
             x(),                    # none
             x(-0.5, 3.5),           # floor(-0.5) = -1: outside
             x(0.5, np.nan, 5.5),    # the middle is not read: (0, 3)
             x(0.5, 6.0)]            # outside
    points, offsets = tc.pack(lines)
    bundle = np.full(len(lines), -1, np.int32)
    bundle[10] = 0
    got = ric.pairs(points, offsets, bundle, dims, rois, valid)
    R = 4
    assert got.tolist() == [0 * R + 2, 0 * R + 2, -1, 0 * R + 2, 1 * R + 2, 1 * R + 3, -1, -1, -1,
                            0 * R + 3, -1, -1, -1, -1, 0 * R + 3, -1]
    mutants = {m: ric.pairs(points, offsets, bundle, dims, rois, valid, m).tolist()
               for m in ric.MUTANTS}
    assert mutants['one_order'][1] == -1 and mutants['one_order'][9] == -1
    assert mutants['last_pair'][3] == 1 * R + 3
    assert mutants['valid_kept'][2] == 0 * R + 1
    assert mutants['assigned_kept'][10] == 0 * R + 3
    assert mutants['trunc_ends'][13] == 0 * R + 2


@pytest.mark.parametrize('R', ic.SETS)
def test_designed_rows_get_the_pair_worked_out_by_hand(R):
    c = ic.case(R)
    n_hand = 0
    for name, want, got in zip(c['names'], c['want'], c['pair']):
        if want is None:
            continue
        n_hand += 1
        assert got == want, (name, want, int(got))
    assert n_hand >= 20
    assert ((c['pair'] >= 0) & (c['bundle'] < 0)).any() and (c['pair'] < 0).any()
    assert (c['pair'][c['bundle'] >= 0] == -1).all()
    if R >= 64:      # the fillers take part: walks connect them
        fillers = set(range(R)) - set(ic.deciding(R))
        walks = c['pair'][[n.startswith('walk_') for n in c['names']]]
        hit = {(int(p) // R, int(p) % R) for p in walks if p >= 0}
        assert len(hit) > 10 and any(i in fillers and j in fillers for i, j in hit)
    if R >= 65:      # pairs with i in word 0 and j in word 1, and with both in word 1
        ij = {(int(p) // R, int(p) % R) for p in c['pair'] if p >= 0}
        assert any(i < 64 <= j for i, j in ij)
        assert R == 65 or any(i >= 64 for i, j in ij)      # R = 65 has one ROI in word 1


def test_every_mutant_has_a_witness_in_the_launched_sets():
    """Each named deviation changes ``pair`` of a case set the GPU tests launch
    and compare exactly."""
    for mutant in ric.MUTANTS:
        seen = []
        for R in ic.SETS:
            c = ic.case(R)
            got = ric.pairs(c['points'], c['offsets'], c['bundle'], ic.DIMS, c['rois'],
                            c['valid'], mutant)
            if not np.array_equal(got, c['pair']):
                seen.append(R)
        print(mutant, seen)
        assert seen, mutant
    # the word mutants show where they should
    assert ic.SETS[-1] == 128


def test_periodic_cases_cover_the_grid():
    """40 000 rows take many workgroups; GRID_PASS + 75 712 rows make every
    thread of the capped grid take a second row, which is another row of the
    period than its first."""
    c = ic.periodic_case(40000)
    assert len(c['pair']) == len(c['bundle']) == len(c['offsets']) - 1 == 40000
    assert (c['pair'] >= 0).sum() > 10000 and (c['pair'] < 0).sum() > 10000
    assert (c['bundle'] >= 0).any()
    assert len(set(c['pair'][:ic.PERIOD].tolist())) > 8
    assert ic.GRID_PASS % ic.PERIOD != 0 and BIG_ROWS > ic.GRID_PASS == 2048 * 256
    # the definition on a stretch far from the start equals the repeated period
    lo, hi = 39000, 39100
    o = c['offsets']
    part = ric.pairs(c['points'][o[lo]:o[hi]], o[lo:hi + 1] - o[lo], c['bundle'][lo:hi], ic.DIMS,
                     c['rois'], c['valid'])
    assert np.array_equal(part, c['pair'][lo:hi])


def test_rois_and_pairs():
    from tracktolearn_amd.experiment.tractometer_validator import roi_names, rois_and_pairs
    # config order: zeta, alpha, mid, beta, omega; zeta serves two bundles
    heads = ['d/zeta.nii.gz', 'd/zeta.nii.gz', 'd/beta.nii.gz']
    tails = ['d/alpha.nii.gz', 'd/mid.nii.gz', 'd/omega.nii.gz']
    rois, valid, pairs = rois_and_pairs(tails, heads)
    assert rois == ['d/alpha.nii.gz', 'd/beta.nii.gz', 'd/mid.nii.gz', 'd/omega.nii.gz',
                    'd/zeta.nii.gz']
    want_valid = np.eye(5, dtype=bool)
    for i, j in ((0, 4), (2, 4), (1, 3)):     # the head sorts last, first, first
        want_valid[i, j] = want_valid[j, i] = True
    assert valid.dtype == bool and np.array_equal(valid, want_valid)
    assert pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 4), (2, 3), (3, 4)]
    assert pairs == ric.pair_list(valid)
    assert roi_names(rois) == ['alpha', 'beta', 'mid', 'omega', 'zeta']
    # head and tail swapped between two bundles that name the same files: one pair
    rois, valid, pairs = rois_and_pairs(['a', 'b', 'c'], ['b', 'a', 'a'])
    assert rois == ['a', 'b', 'c'] and pairs == [(1, 2)]
    # compared as strings: 'B' < 'a', '10' < '9'
    assert rois_and_pairs(['a', '9'], ['B', '10'])[0] == ['10', '9', 'B', 'a']
    assert roi_names(['x/m.nii.gz', 'y/m.nii.gz', 't.trk']) == ['m_0', 'm_1', 't_2']


def test_packed_words():
    from tracktolearn_amd.experiment.tractometer_validator import (pack_roi_words,
                                                                   pack_valid_words)
    rng = np.random.default_rng(5)
    dims = (3, 4, 5)
    for R in (2, 64, 65, 128):
        masks = [rng.random(dims) < 0.3 for _ in range(R)]
        words = pack_roi_words(masks, dims)
        W = (R + 63) // 64
        assert words.dtype == np.uint64 and words.shape == (60, W)
        for r in {0, 1, 31, 32, 63, 64, 65, 127} & set(range(R)):
            bit = (words[:, r // 64] >> np.uint64(r % 64)) & np.uint64(1)
            assert np.array_equal(bit.reshape(dims) != 0, masks[r]), r
        # nothing at or above R
        if R % 64:
            assert not (words[:, -1] >> np.uint64(R % 64)).any()
        valid = rng.random((R, R)) < 0.2
        vw = pack_valid_words(valid)
        assert vw.shape == (R, W)
        for i, j in ((0, 0), (1, 0), (0, 1), (R - 1, R - 1), (R - 1, 0), (R // 2, R - 1)):
            bit = (int(vw[i, j // 64]) >> (j % 64)) & 1
            assert bit == int(valid[i, j] or i == j), (i, j)
    one = np.zeros(dims, bool)
    one[2, 1, 3] = True
    w = pack_roi_words([np.zeros(dims, bool)] * 70 + [one], dims)
    assert np.argwhere(w).tolist() == [[(2 * 4 + 1) * 5 + 3, 1]] and int(w.max()) == 1 << 6
    for R in (1, 129):
        with pytest.raises(ValueError, match='2 to 128'):
            pack_roi_words([one] * R, dims)
    with pytest.raises(ValueError, match='shape'):
        pack_roi_words([one, np.zeros((3, 4, 6), bool)], dims)


def test_score_arithmetic_from_integers():
    from tracktolearn_amd.experiment.tractometer_validator import full_scores, metrics
    names = ['full', 'empty_gt', 'no_streamline', 'no_gt']
    per_bundle = [6, 2, 0, 1]
    counts = [[30, 10], [0, 8], [0, 0], [0, 5]]       # (|M & G|, |M \ G|)
    gt_sizes = [40, 0, 25, None]
    wpc = [2, 0, 1, 0]
    got = full_scores(20, names, per_bundle, counts, gt_sizes, wpc,
                      {'a__b': 3, 'a__c': 1})
    assert got['bundles']['full'] == {'VS': 6, 'WPC': 2, 'TP': 30, 'FP': 10, 'FN': 10,
                                      'OL': 0.75, 'OR_gt': 0.25, 'OR_vs': 0.25, 'f1': 0.75}
    assert got['bundles']['empty_gt'] == {'VS': 2, 'WPC': 0, 'TP': 0, 'FP': 8, 'FN': 0,
                                          'OL': 0.0, 'OR_gt': 0.0, 'OR_vs': 1.0, 'f1': 0.0}
    assert got['bundles']['no_streamline'] == {'VS': 0, 'WPC': 1, 'TP': 0, 'FP': 0, 'FN': 25,
                                               'OL': 0.0, 'OR_gt': 0.0, 'OR_vs': 0.0, 'f1': 0.0}
    assert got['bundles']['no_gt'] == {'VS': 1, 'WPC': 0, 'TP': None, 'FP': None, 'FN': None,
                                       'OL': None, 'OR_gt': None, 'OR_vs': None, 'f1': None}
    totals = {k: v for k, v in got.items() if k not in ('bundles', 'invalid_bundles')}
    assert totals == {'n': 20, 'VS': 9, 'VC': 0.45, 'IC': 0.2, 'IS': 0.2 + 0.35, 'NC': 0.35,
                      'VB': 3, 'IB': 2, 'mean_OL': 0.25, 'mean_OR_gt': 0.25 / 3,
                      'mean_OR_vs': 1.25 / 3, 'mean_f1': 0.25}
    assert got['invalid_bundles'] == {'a__b': 3, 'a__c': 1}
    assert list(got) == ['n', 'VS', 'VC', 'IC', 'IS', 'NC', 'VB', 'IB', 'mean_OL', 'mean_OR_gt',
                         'mean_OR_vs', 'mean_f1', 'bundles', 'invalid_bundles']
    json.dumps(got)
    # not computed: as the default dict
    plain = full_scores(20, names, per_bundle, counts, gt_sizes, wpc)
    assert (plain['IC'], plain['IS'], plain['IB'], plain['NC']) == (0, 0, 0, 1 - 0.45)
    assert plain['invalid_bundles'] == {}
    # computed and none found
    none = full_scores(20, names, per_bundle, counts, gt_sizes, wpc, {})
    assert (none['IC'], none['IS'], none['IB'], none['NC']) == (0.0, 0.55, 0, 0.55)
    assert metrics(20, per_bundle, counts, gt_sizes, invalid=(4, 2)) == {
        'VC': 0.45, 'IC': 0.2, 'IS': 0.2 + 0.35, 'NC': 0.35, 'mean_OL': 0.25, 'VB': 3, 'IB': 2}
    # no bundle has a gt_mask: the means are 0
    bare = full_scores(4, ['a'], [1], [[0, 3]], [None], [0], {})
    assert [bare[k] for k in ('mean_OL', 'mean_OR_gt', 'mean_OR_vs', 'mean_f1')] == [0.0] * 4


def test_default_metrics_dict_is_unchanged():
    from tracktolearn_amd.experiment.tractometer_validator import metrics
    got = metrics(8, [3, 0, 1], [[5, 1], [0, 0], [2, 2]], [10, None, 0])
    assert got == {'VC': 0.5, 'IC': 0, 'IS': 0, 'NC': 0.5, 'mean_OL': 0.25, 'VB': 2, 'IB': 0}
    assert list(got) == ['VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB']
    assert all(type(got[k]) is int for k in ('IC', 'IS', 'IB'))
    for B in (3, 33):
        c = tc.case(B)
        sc = c['score']
        per_bundle = np.bincount(sc['bundle'] + 1, minlength=B + 1)[1:]
        sizes = [None if b['gt'] is None else int(b['gt'].sum()) for b in c['bundles']]
        assert metrics(len(sc['bundle']), per_bundle, sc['counts'], sizes) == sc['metrics']


def test_c_abi_rejects_bad_arguments():
    """The argument checks come before any device work: a null pointer, R
    outside 2 .. 128, a dim < 1, n < 0 and two-word sets that are not 16-byte
    aligned return TTL_ERR_INVALID."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    p = 4096                                      # never dereferenced
    dims = (C.c_int32 * 3)(12, 9, 7)

    def call(**kw):
        a = dict(points=p, offsets=p, n=1, bundle=p, dims=dims, R=3, roi=p, valid=p, pair=p)
        a.update(kw)
        return lib.ttl_tractometer_invalid(a['points'], a['offsets'], a['n'], a['bundle'],
                                           a['dims'], a['R'], a['roi'], a['valid'], a['pair'],
                                           None)

    for name in ('points', 'offsets', 'bundle', 'dims', 'roi', 'valid', 'pair'):
        assert call(**{name: None}) == _lib.ERR_INVALID, name
    assert b'ttl_tractometer_invalid' in lib.ttl_last_error()
    for R in (-1, 0, 1, 129, 1 << 20):
        assert call(R=R) == _lib.ERR_INVALID, R
    for d in ((0, 9, 7), (12, -1, 7), (12, 9, 0)):
        assert call(dims=(C.c_int32 * 3)(*d)) == _lib.ERR_INVALID
    assert call(n=-1) == _lib.ERR_INVALID
    assert call(R=65, roi=p + 8) == _lib.ERR_INVALID
    assert call(R=128, valid=p + 8) == _lib.ERR_INVALID
    for R in (2, 64, 65, 128):
        assert call(n=0, R=R) == 0                # nothing to do, nothing touched
    assert call(n=0, R=64, roi=p + 8) == 0        # one-word sets need 8 bytes only
    assert lib.ttl_abi_version() == 13
    assert _lib.TRACTOMETER_MAX_ROIS == 128


def test_python_wrapper_needs_the_roi_planes():
    from tracktolearn_amd.experiment.tractometer_validator import (ScoringData, invalid,
                                                                   limits_table)
    none = np.zeros(ic.DIMS, bool)
    data = ScoringData(ic.DIMS, [none], [none], [None], [None], [None],
                       limits_table([None], [None], [None], [None]), 'cpu')
    assert data.roi is None and data.valid is None and data.n_rois == 0
    with pytest.raises(ValueError, match='compute_ic'):
        invalid(torch.zeros((2, 3)), torch.tensor([0, 2]), torch.tensor([-1], dtype=torch.int32),
                data)


def test_header_states_the_entry():
    text = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert '#define TTL_HAS_TRACTOMETER_IC 1' in text
    assert '#define TTL_TRACTOMETER_MAX_ROIS 128' in text
    assert '#define TTL_ABI_VERSION 13' in text
    assert 'TTL_API int ttl_tractometer_invalid(' in text


def test_ttl_score_tractogram_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'ttl_score_tractogram.py'),
                          '--help'], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for word in ('in_tractogram', 'scoring_data', 'out_dir', '--reference',
                 '--dilate_endpoints', '--compute_ic', '--save_bundles', '-f'):
        assert word in out.stdout


def test_trainer_takes_the_flag():
    import argparse
    from tracktolearn_amd.trainers.train import add_tractometer_args
    parser = argparse.ArgumentParser()
    add_tractometer_args(parser)
    assert parser.parse_args([]).tractometer_compute_ic is False
    assert parser.parse_args(['--tractometer_compute_ic']).tractometer_compute_ic is True


# ----------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize('R', ic.SETS)
def test_pair_equals_the_definition(R):
    c = ic.case(R)
    got = _run(c)
    wrong = np.flatnonzero(got != c['pair'])
    assert len(wrong) == 0, [(c['names'][r], int(got[r]), int(c['pair'][r])) for r in wrong[:8]]
    assert got.dtype == np.int32 and (got >= 0).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('n_rows', [40000, BIG_ROWS])
def test_many_rows(n_rows):
    """40 000 rows: 157 workgroups.  600 000 rows: more than the 524 288 of one
    pass of the capped grid, so the first 75 712 threads take a second row."""
    c = ic.periodic_case(n_rows)
    got = _run(c)
    wrong = np.flatnonzero(got != c['pair'])
    assert len(wrong) == 0, (wrong[:8], got[wrong[:8]], c['pair'][wrong[:8]])


# ---- end to end
ROI_NAMES = ['alpha', 'beta', 'mid', 'omega', 'zeta']          # sorted; not the config's order
VALID_PAIRS = ((0, 4), (2, 4), (1, 3))


def _e2e_scoring():
    """(config, masks by file name, bundle dicts in the config's order with
    undilated heads and tails, ROI masks in sorted order)."""
    roi = {'zeta': _box((0, 2), (0, 9), (3, 5)), 'alpha': _box((10, 12), (0, 9), (3, 5)),
           'mid': _box((5, 7), (0, 4), (3, 5)), 'beta': _box((0, 2), (0, 9), (0, 2)),
           'omega': _box((10, 12), (0, 9), (0, 2))}
    gt_first, gt_third = _box((0, 12), (2, 5), (3, 5)), _box((2, 12), (0, 6), (0, 1))
    config = {      # the order of the keys is the order of the bundles
        'b_first': {'head': 'zeta.nii.gz', 'tail': 'alpha.nii.gz', 'gt_mask': 'gt_first.nii.gz',
                    'length': [15, 40]},
        'a_second': {'head': 'zeta.nii.gz', 'tail': 'mid.nii.gz'},
        'c_third': {'head': 'beta.nii.gz', 'tail': 'omega.nii.gz', 'gt_mask': 'gt_third.nii.gz'}}
    masks = {f'{k}.nii.gz': v for k, v in roi.items()}
    masks.update({'gt_first.nii.gz': gt_first, 'gt_third.nii.gz': gt_third})
    bundles = [ref.bundle(roi['zeta'], roi['alpha'], gt=gt_first, length=[15, 40]),
               ref.bundle(roi['zeta'], roi['mid']),
               ref.bundle(roi['beta'], roi['omega'], gt=gt_third)]
    return config, masks, bundles, [roi[k] for k in ROI_NAMES]


def _write_scoring_dir(path):
    from tracktolearn_amd.io import nifti
    config, masks, _, _ = _e2e_scoring()
    os.makedirs(path, exist_ok=True)
    nifti.save(os.path.join(path, 'ref.nii.gz'), np.zeros(tc.DIMS, np.uint8), AFFINE)
    for k, (name, mask) in enumerate(masks.items()):
        dtype = (np.uint8, np.int16, np.float32)[k % 3]
        nifti.save(os.path.join(path, name), (mask * (2 + k)).astype(dtype), AFFINE)
    with open(os.path.join(path, 'scil_scoring_config.json'), 'w') as f:
        json.dump(config, f)


def _e2e_lines():
    """Corner-origin voxel coordinates.  Rows of every kind, away from voxel
    faces and from the length limits (the file path rounds to float32 twice)."""
    rng = np.random.default_rng(33)
    L = []

    def add(*pts):
        L.append(np.array(pts, np.float32))

    for y in (2.5, 3.5, 4.5):
        add((0.5, y, 3.5), (11.5, y, 3.5))                    # b_first
    add((11.5, 3.5, 4.5), (0.5, 3.5, 4.5))                    # b_first, reversed
    add((2.5, 3.5, 3.5), (11.5, 3.5, 3.5))                    # b_first through the dilation
    add((0.5, 1.5, 4.5), (5.5, 1.5, 4.5))                     # a_second
    add((1.0, 1.0, 1.0))                                      # one point: not scored
    add((6.5, 2.5, 3.5), (3.5, 2.5, 4.2), (1.5, 2.5, 3.5))    # a_second, reversed
    for y in (1.5, 4.5, 7.5):
        add((0.5, y, 0.5), (11.5, y, 0.5))                    # c_third
    # wrong path connections of b_first: its ROIs, three times too long
    add((0.5, 1.5, 3.5), (11.5, 7.5, 3.5), (0.7, 7.5, 4.5), (11.5, 1.5, 4.5))
    add((11.5, 6.5, 3.5), (0.7, 2.5, 3.5), (11.5, 2.5, 4.5), (1.5, 6.5, 4.5))
    add((0.5, 5.5, 3.5), (1.5, 5.5, 3.5), (11.5, 5.5, 3.5), (2.5, 5.5, 4.5),
        (10.5, 5.5, 4.5))
    add((11.5, 1.5, 3.5), (5.5, 1.5, 3.5))                    # alpha - mid: (0, 2)
    add((5.5, 2.5, 4.5), (10.5, 2.5, 4.5))                    # mid - alpha: (0, 2)
    add((9.5, 1.5, 3.5), (6.5, 1.5, 3.5))                     # alpha through the dilation
    add((0.5, 4.5, 3.5), (11.5, 4.5, 0.5))                    # zeta - omega: (3, 4)
    add((0.5, 6.5, 0.5), (6.5, 8.5, 2.5), (11.5, 6.5, 4.5))   # beta - alpha: (0, 1)
    add((0.5, 2.5, 0.5), (1.5, 6.5, 4.5))                     # beta - zeta: (1, 4)
    add((5.5, 1.5, 3.5), (11.5, 1.5, 1.5))                    # mid - omega (dilated): (2, 3)
    # an end in dilated beta and dilated zeta (z = 2), too long for b_first (a wrong path
    # connection of it): (0, 1) comes before the valid (0, 4)
    add((0.5, 3.5, 2.5), (11.5, 7.5, 2.5), (0.7, 7.5, 3.5), (11.5, 3.5, 3.5))
    add((0.5, 3.5, 3.5), (1.5, 5.5, 4.5))                     # zeta - zeta
    add((5.5, 6.5, 5.5), (7.5, 6.5, 6.5))                     # nowhere
    walks = tc.random_walks(rng, 60, 2, 40, 12, step=(0.3, 1.9), start=(0, 7))
    L += [np.asarray(w, np.float32) for w in walks]
    return [s + rng.uniform(0.01, 0.05, 3).astype(np.float32) if len(s) > 1 else s for s in L]


def _strip(result):
    return {k: v for k, v in result.items() if k not in ('bundle', 'pair', 'index')}


@pytest.fixture(scope='module')
def e2e(tmp_path_factory):
    """The scoring directory, the tractogram in memory and as a .trk with an
    ``id`` per streamline, and the definition's result for both paths."""
    from scipy.ndimage import binary_dilation
    from tracktolearn_amd.tractogram import Tractogram
    root = tmp_path_factory.mktemp('tractometer_ic')
    scoring = str(root / 'scoring')
    _write_scoring_dir(scoring)
    lines = _e2e_lines()
    env = tc.env()
    tract = Tractogram([s - np.float32(0.5) for s in lines])
    path = str(root / 'v.trk')
    tc.save_trk(tract.streamlines, path,
                {'id': np.arange(len(lines), dtype=np.float32).reshape(-1, 1)})
    _, _, bundles, rois = _e2e_scoring()
    for b in bundles:
        b['head'], b['tail'] = binary_dilation(b['head']), binary_dilation(b['tail'])
    valid = np.eye(5, dtype=bool)
    for i, j in VALID_PAIRS:
        valid[i, j] = valid[j, i] = True
    return SimpleNamespace(scoring=scoring, reference=os.path.join(scoring, 'ref.nii.gz'),
                           lines=lines, env=env, tract=tract, path=path, bundles=bundles,
                           rois=[binary_dilation(m) for m in rois], valid=valid,
                           names=['b_first', 'a_second', 'c_third'], root=root)


def _want(e2e, points, offsets, compute_ic=True):
    lin = AFFINE[:3, :3]
    for r in range(len(offsets) - 1):
        rep = ref.margin_report(points[offsets[r]:offsets[r + 1]], tc.DIMS, e2e.bundles, lin)
        assert all(m[-1] for m in rep), [m for m in rep if not m[-1]]
    if not compute_ic:
        return ric.full_result(points, offsets, tc.DIMS, e2e.bundles, e2e.names, lin)
    return ric.full_result(points, offsets, tc.DIMS, e2e.bundles, e2e.names, lin, e2e.rois,
                           e2e.valid, ROI_NAMES)


@pytest.mark.gpu
def test_score_from_memory_and_from_a_trk(e2e):
    """``score()`` equals the definition's dict and arrays on both input paths
    (the definition is evaluated on the coordinates each path hands to the
    device); ``__call__`` with compute_ic equals its seven keys, by default
    today's dict."""
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    one_point = [i for i, s in enumerate(e2e.lines) if len(s) < 2]
    assert one_point == [6]
    index = np.array([i for i in range(len(e2e.lines)) if i != 6])
    val = TractometerValidator(e2e.scoring, e2e.reference, dilate_endpoints=1, device=DEV,
                               compute_ic=True)
    assert val.roi_names == ROI_NAMES and val.data.n_rois == 5
    wants = []
    for source, env in ((e2e.tract, e2e.env), (e2e.path, None)):
        points, offsets, idx, affine = val.corner_voxels(source, env)
        assert np.array_equal(idx, index) and np.allclose(affine, AFFINE, atol=1e-6)
        want = _want(e2e, points, offsets)
        wants.append(want)
        got = val.score(source, env)
        assert _strip(got) == _strip(want)
        assert np.array_equal(got['bundle'], want['bundle'])
        assert np.array_equal(got['pair'], want['pair'])
        assert np.array_equal(got['index'], index)
        assert got['bundle'].dtype == got['pair'].dtype == np.int32
        seven = val(source, e2e.env)
        assert seven == {k: want[k] for k in ('VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB')}
        assert list(seven) == ['VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB']
    assert _strip(wants[0]) == _strip(wants[1])
    w = wants[0]
    # the rows were built for these: every kind is there
    assert w['VB'] == 3 and w['IB'] >= 5 and w['n'] == len(e2e.lines) - 1
    assert set(w['invalid_bundles']) >= {'alpha__beta', 'alpha__mid', 'beta__zeta', 'mid__omega',
                                         'omega__zeta'}
    assert w['invalid_bundles']['alpha__mid'] >= 3 and w['invalid_bundles']['alpha__beta'] >= 2
    assert w['bundles']['b_first']['WPC'] >= 4 and w['bundles']['b_first']['VS'] >= 5
    assert w['bundles']['a_second']['TP'] is None and w['bundles']['a_second']['VS'] >= 2
    assert 0 < w['IC'] < 1 and 0 < w['NC'] < 1 and w['IC'] + w['NC'] + w['VC'] == pytest.approx(1)
    assert 0 < w['mean_OL'] < 1 and 0 < w['mean_f1'] < 1 and w['mean_OR_gt'] > 0
    # a .trk needs no reference either: its header supplies the space
    own = TractometerValidator(e2e.scoring, None, dilate_endpoints=1, device=DEV, compute_ic=True)
    points, offsets, _, affine = own.corner_voxels(e2e.path)
    assert np.allclose(affine, AFFINE, atol=1e-6)
    got = own.score(e2e.path)
    assert _strip(got) == _strip(_want(e2e, points, offsets))
    with pytest.raises(ValueError, match='give the env'):
        own.score(e2e.tract)
    # by default: today's dict from __call__, and score() without the invalid connections
    plain = TractometerValidator(e2e.scoring, e2e.reference, dilate_endpoints=1, device=DEV)
    assert plain.data.roi is None and plain.rois is None
    points, offsets, _, _ = plain.corner_voxels(e2e.tract, e2e.env)
    today = ref.score(points, offsets, tc.DIMS, e2e.bundles, AFFINE[:3, :3])['metrics']
    got = plain(e2e.tract, e2e.env)
    assert got == today and list(got) == list(today)
    assert type(got['IC']) is int and got['IC'] == got['IS'] == got['IB'] == 0
    got = plain.score(e2e.tract, e2e.env)
    want = _want(e2e, points, offsets, compute_ic=False)
    assert _strip(got) == _strip(want) and (got['pair'] == -1).all()
    assert got['invalid_bundles'] == {} and got['NC'] == today['NC']
    # without dilation the rows that reach an ROI through it connect nothing
    bare = TractometerValidator(e2e.scoring, e2e.reference, dilate_endpoints=0, device=DEV,
                                compute_ic=True).score(e2e.tract, e2e.env)
    assert bare['VS'] < w['VS'] and bare['invalid_bundles'].get('alpha__mid', 0) < \
        w['invalid_bundles']['alpha__mid']
    assert 'alpha__beta' not in bare['invalid_bundles'] or \
        bare['invalid_bundles']['alpha__beta'] < w['invalid_bundles']['alpha__beta']
    assert plain.score([np.ones((1, 3), np.float32)], e2e.env) == {}


@pytest.mark.gpu
@pytest.mark.parametrize('compute_ic', [True, False])
def test_summary_names_what_it_reads_back(e2e, compute_ic):
    """The one read-back of the device pass, name by name, against NumPy on the
    arrays the pass left and on the definition's; ``__call__`` is the seven
    keys of ``score``."""
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator, segment
    val = TractometerValidator(e2e.scoring, e2e.reference, dilate_endpoints=1, device=DEV,
                               compute_ic=compute_ic)
    points, offsets, _, affine = val.corner_voxels(e2e.tract, e2e.env)
    want = _want(e2e, points, offsets, compute_ic)
    seg = segment(points, offsets, val.data, affine[:3, :3], compute_ic)
    s = seg.summary(wpc=True, per_pair=True)
    bundle, connected = seg.bundle.cpu().numpy(), seg.connected.cpu().numpy().view(np.uint64)
    assert np.array_equal(bundle, want['bundle'])
    B, R = 3, 5
    per_bundle = np.bincount(bundle + 1, minlength=B + 1)[1:]
    assert s.per_bundle.tolist() == per_bundle.tolist()
    assert s.per_bundle.tolist() == [want['bundles'][k]['VS'] for k in e2e.names]
    assert s.counts.shape == (B, 2) and np.array_equal(s.counts, seg.counts.cpu().numpy())
    for b, name in enumerate(e2e.names):
        entry = want['bundles'][name]
        if entry['TP'] is not None:
            assert s.counts[b].tolist() == [entry['TP'], entry['FP']]
    wrong = connected[bundle < 0]
    wpc = [int(((wrong >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(B)]
    assert s.wpc.tolist() == wpc == [want['bundles'][k]['WPC'] for k in e2e.names]
    if compute_ic:
        pair = seg.pair.cpu().numpy()
        assert np.array_equal(pair, want['pair'])
        per_pair = np.bincount(pair + 1, minlength=R * R + 1)[1:]
        assert s.per_pair.tolist() == per_pair.tolist() and per_pair.sum() > 0
        assert {f'{ROI_NAMES[k // R]}__{ROI_NAMES[k % R]}': int(per_pair[k])
                for k in np.flatnonzero(per_pair)} == want['invalid_bundles']
        assert [int(v) for v in s.invalid] == [per_pair.sum(), (per_pair > 0).sum()]
    else:
        assert seg.pair is None and s.per_pair is None and s.invalid is None
    # the short summary of __call__: the same numbers, the totals of the pairs only
    short = seg.summary()
    assert short.wpc is None and short.per_pair is None
    assert short.per_bundle.tolist() == s.per_bundle.tolist()
    assert np.array_equal(short.counts, s.counts)
    assert (short.invalid is None) == (not compute_ic)
    assert not compute_ic or [int(v) for v in short.invalid] == [int(v) for v in s.invalid]
    for source in (e2e.tract, e2e.path):
        seven, full = val(source, e2e.env), val.score(source, e2e.env)
        assert seven == {k: full[k] for k in ('VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB')}
        assert list(seven) == ['VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB']


@pytest.mark.gpu
def test_command_writes_results_and_bundles(e2e, capsys):
    """``ttl_score_tractogram.py`` on the .trk: results.json is ``score()``
    without the arrays; with --save_bundles the files' streamlines partition
    the input (by their ``id`` property, points to float32 rounding), one file
    per non-empty class, with the counts of the result."""
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_score_tractogram as cmd
    out = str(e2e.root / 'out')
    cmd.main([e2e.path, e2e.scoring, out, '--reference', e2e.reference, '--compute_ic',
              '--save_bundles'])
    val = TractometerValidator(e2e.scoring, e2e.reference, dilate_endpoints=1, device=DEV,
                               compute_ic=True)
    result = val.score(e2e.path)
    want_json = json.loads(json.dumps(_strip(result)))
    assert json.load(open(os.path.join(out, 'results.json'))) == want_json
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])['IB'] == result['IB']

    files = {}
    for sub, _, names in os.walk(out):
        for name in names:
            if name.endswith('.trk'):
                files[os.path.relpath(os.path.join(sub, name), out)] = sio.load_trk(
                    os.path.join(sub, name))[0]
    want_files = {os.path.join('segmented_VB', f'{b}_VS.trk'): e['VS']
                  for b, e in result['bundles'].items() if e['VS']}
    want_files.update({os.path.join('segmented_IB', f'{p}_IC.trk'): k
                       for p, k in result['invalid_bundles'].items()})
    n_in = len(e2e.lines)
    n_ic = sum(result['invalid_bundles'].values())
    want_files['NC.trk'] = n_in - result['VS'] - n_ic     # the one-point row is in it
    assert {k: len(v) for k, v in files.items()} == want_files
    assert want_files['NC.trk'] == round(result['NC'] * result['n']) + 1
    source = sio.load_trk(e2e.path)[0]
    seen = []
    for name, part in files.items():
        ids = part.data_per_streamline['id'].reshape(-1).astype(int)
        seen += ids.tolist()
        for i, s in zip(ids, part.streamlines):
            assert s.shape == source.streamlines[i].shape
            assert np.allclose(s, source.streamlines[i], atol=1e-4)
        # the class of every streamline in the file is the file's
        scored = {int(i): r for r, i in enumerate(result['index'])}
        if name.startswith('segmented_VB'):
            b = list(result['bundles']).index(os.path.basename(name)[:-len('_VS.trk')])
            assert all(result['bundle'][scored[i]] == b for i in ids)
        elif name.startswith('segmented_IB'):
            assert all(result['pair'][scored[i]] >= 0 for i in ids)
            assert len({int(result['pair'][scored[i]]) for i in ids}) == 1
        else:
            assert all(i not in scored or (result['bundle'][scored[i]] < 0 and
                                           result['pair'][scored[i]] < 0) for i in ids)
    assert sorted(seen) == list(range(n_in))
    # a second run refuses to overwrite, -f overwrites; without --compute_ic no invalid bundles
    with pytest.raises(SystemExit):
        cmd.main([e2e.path, e2e.scoring, out])
    cmd.main([e2e.path, e2e.scoring, out, '-f'])           # the .trk's own space
    again = json.load(open(os.path.join(out, 'results.json')))
    assert again['IB'] == 0 and again['invalid_bundles'] == {} and again['VS'] == result['VS']


@pytest.mark.gpu
def test_sac_auto_train_compute_ic(tmp_path, capsys):
    """--tractometer_validator --tractometer_compute_ic end to end: the IC and
    IB monitors carry what the validator returned."""
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.trainers import sac_auto_train
    D = 20
    tc._write_dataset(str(tmp_path / 'ds.npz'), D)
    scoring = tmp_path / 'scoring'
    scoring.mkdir()
    vols = {k: np.zeros((D, D, D), np.uint8) for k in ('low', 'middle', 'high', 'whole')}
    vols['low'][:7], vols['middle'][7:13], vols['high'][13:], vols['whole'][:] = 1, 1, 1, 1
    for name, vol in vols.items():
        nifti.save(str(scoring / f'{name}.nii.gz'), vol, np.eye(4))
    (scoring / 'scil_scoring_config.json').write_text(json.dumps({
        'long': {'head': 'low.nii.gz', 'tail': 'high.nii.gz', 'gt_mask': 'whole.nii.gz'},
        'never': {'head': 'middle.nii.gz', 'tail': 'middle.nii.gz', 'length': [1e6, 2e6]}}))
    sac_auto_train.main(tc._train_args(tmp_path, [
        '--tractometer_validator', '--scoring_data', str(scoring), '--tractometer_dilate', '0',
        '--tractometer_compute_ic']))
    out = capsys.readouterr().out
    assert out.count("'IC':") == 4
    plots = tmp_path / 'exp' / 'plots'
    series = {k: np.load(plots / f'{k}.npy') for k in ('vc', 'ic', 'nc', 'ib')}
    for name, s in series.items():
        assert s.shape == (4, 2), name
    vc, icv, nc, ib = (series[k][:, 1] for k in ('vc', 'ic', 'nc', 'ib'))
    assert np.allclose(vc + icv + nc, 1) and ((icv >= 0) & (icv <= 1)).all()
    # every voxel lies in exactly one of low / middle / high, and only low - high is valid:
    # a streamline of 2 points or more connects an invalid pair unless it stays in one ROI
    assert (icv > 0).all() and (ib >= 1).all() and (ib <= 2).all() and (ib == np.round(ib)).all()
