"""The Tractometer validator (experiment/tractometer_validator.py,
csrc/ttl_tractometer.hip) against its NumPy definition
(tests/ref_tractometer.py) on the case sets of tests/tractometer_cases.py.

On the CPU: the config reader, the dilation, the bit planes and the limits
table, the definition against hand-computed answers, the preconditions under
which the kernel's float64 sums may be compared exactly (asserted on the
inputs, never skipped), and a witness for every named mutant in the sets the
GPU tests launch.  On the GPU: ``bundle``, ``connected``, ``counts`` and
``visited_bits`` bit for bit, the grid-stride loop, the validator end to end
(file and memory paths) and the trainer's ``--tractometer_validator``."""
import argparse
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import ref_tractometer as ref
import tractometer_cases as tc
from tractometer_cases import AFFINE

DEV = 'cuda:0'
SETS = (3, 33, 64)


# ------------------------------------------------------------------ helpers
def _scoring_data(bundles, device=DEV):
    from tracktolearn_amd.experiment.tractometer_validator import ScoringData, limits_table
    heads, tails, alls, anys, gts, lengths, angles, dirs, absdirs = tc.tables(bundles)
    return ScoringData(tc.DIMS, heads, tails, alls, anys, gts,
                       limits_table(lengths, angles, dirs, absdirs), device)


def _run(points, offsets, bundles, visited=None):
    """(bundle, connected, counts, visited) of the two library calls, as NumPy."""
    from tracktolearn_amd.experiment.tractometer_validator import classify, overlap
    data = _scoring_data(bundles)
    pts = torch.from_numpy(np.ascontiguousarray(points)).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(offsets)).to(DEV)
    bundle, connected = classify(pts, off, data, tc.LIN)
    if visited is not None:
        visited = torch.from_numpy(visited.reshape(-1).view(np.int64).copy()).to(DEV)
    counts, visited = overlap(pts, off, bundle, data, visited)
    torch.cuda.synchronize()
    return (bundle.cpu().numpy(), connected.cpu().numpy().view(np.uint64),
            counts.cpu().numpy(), visited.cpu().numpy().view(np.uint64).reshape(tc.DIMS))


@functools.lru_cache(maxsize=None)
def _margins(key):
    """Every decision of the case set ``key`` that rests on a float64 sum or on
    the winding, as (row, bundle, what, value, limit, ok)."""
    c = tc.grid_case() if key == 'grid' else tc.case(key)
    out = []
    for r in range(len(c['offsets']) - 1):
        row = c['points'][c['offsets'][r]:c['offsets'][r + 1]]
        out += [(r,) + rep for rep in ref.margin_report(row, tc.DIMS, c['bundles'], tc.LIN)]
    return out


def _assert_margins(key):
    """The kernel may order its float64 sums differently from NumPy, so an
    exact comparison of decisions needs: no quantity within 1e-9 (relative) of
    a limit it is compared with, unless the row's sums are exact in every
    order; under an angle, lambda2 - lambda3 >= 1e-3 lambda1 and no |p_j| below
    1e-9.  Asserted on the inputs; no case is left out."""
    bad = [m for m in _margins(key) if not m[-1]]
    assert not bad, bad[:5]


# ----------------------------------------------------------------- CPU tests
def _write_config(tmp_path, config):
    path = tmp_path / 'scil_scoring_config.json'
    path.write_text(json.dumps(config))
    return str(path)


def test_read_config_file(tmp_path):
    from tracktolearn_amd.experiment.tractometer_validator import (compute_endpoint_masks,
                                                                   read_config_file)
    cfg = {'CC': {'head': 'h.nii.gz', 'tail': 't.nii.gz', 'gt_mask': 'cc.nii.gz', 'angle': 300,
                  'length': [20, 180], 'length_x': [10, 100], 'length_z_abs': [0, 40]},
           'CST': {'tail': 'b.nii.gz', 'head': 'a.nii.gz', 'all_mask': 'all.nii.gz',
                   'any_mask': 'any.trk'}}
    out = read_config_file(_write_config(tmp_path, cfg), 'data')
    names, gts, alls, anys, rois, lengths, angles, dirs, absdirs = out
    assert names == ['CC', 'CST']
    assert gts == [os.path.join('data', 'cc.nii.gz'), None]
    assert alls == [None, os.path.join('data', 'all.nii.gz')]
    assert anys == [None, os.path.join('data', 'any.trk')]
    assert rois[0] == {'gt_head': os.path.join('data', 'h.nii.gz'),
                       'gt_tail': os.path.join('data', 't.nii.gz')}
    assert lengths == [[20, 180], None] and angles == [300, None]
    assert dirs == [[[10, 100], [0, np.inf], [0, np.inf]], None]
    assert absdirs == [[[0, np.inf], [0, np.inf], [0, 40]], None]
    tails, heads = compute_endpoint_masks(rois)
    assert heads == [os.path.join('data', 'h.nii.gz'), os.path.join('data', 'a.nii.gz')]
    assert tails == [os.path.join('data', 't.nii.gz'), os.path.join('data', 'b.nii.gz')]
    # no gt_dir: the names as written; gt masks as all masks
    out = read_config_file(_write_config(tmp_path, {'CC': cfg['CC']}), '', True)
    assert out[1] == ['cc.nii.gz'] and out[2] == ['cc.nii.gz']


@pytest.mark.parametrize('bundle_cfg,match', [
    ({'head': 'h', 'tail': 't', 'colour': 'red'}, 'Unrecognized value colour'),
    ({'head': 'h'}, 'not the tail'),
    ({'tail': 't'}, "misses 'endpoints' or 'head'/'tail'"),
    ({'gt_mask': 'g'}, "misses 'endpoints' or 'head'/'tail'"),
    ({'endpoints': 'e', 'head': 'h', 'tail': 't'}, 'confusing keywords'),
])
def test_read_config_file_errors(tmp_path, bundle_cfg, match):
    from tracktolearn_amd.experiment.tractometer_validator import read_config_file
    with pytest.raises(ValueError, match=match):
        read_config_file(_write_config(tmp_path, {'B': bundle_cfg}))


def test_config_all_mask_with_gt_as_all_masks(tmp_path):
    from tracktolearn_amd.experiment.tractometer_validator import read_config_file
    path = _write_config(tmp_path, {'B': {'head': 'h', 'tail': 't', 'all_mask': 'a'}})
    with pytest.raises(ValueError, match='use_gt_masks_as_all_masks'):
        read_config_file(path, '', True)


def test_endpoints_without_head_and_tail_says_so(tmp_path):
    from tracktolearn_amd.experiment.tractometer_validator import (compute_endpoint_masks,
                                                                   read_config_file)
    out = read_config_file(_write_config(tmp_path, {'B': {'endpoints': 'e.nii.gz'}}))
    assert out[4] == [{'gt_endpoints': 'e.nii.gz'}]
    with pytest.raises(ValueError, match="'endpoints' has no 'head' and 'tail'"):
        compute_endpoint_masks(out[4])


def test_validator_refuses_bad_scoring_data(tmp_path):
    """Raised before any mask is read or the device is touched."""
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    with pytest.raises(ValueError, match='scil_scoring_config.json'):
        TractometerValidator(str(tmp_path), None, device='cpu')
    _write_config(tmp_path, {f'b{i}': {'head': 'h.nii.gz', 'tail': 't.nii.gz'}
                             for i in range(65)})
    with pytest.raises(ValueError, match='at most 64'):
        TractometerValidator(str(tmp_path), None, device='cpu')
    _write_config(tmp_path, {'b': {'endpoints': 'e.nii.gz'}})
    with pytest.raises(ValueError, match="no 'head' and 'tail'"):
        TractometerValidator(str(tmp_path), None, device='cpu')


@pytest.mark.parametrize('k', [0, 1, 2])
def test_dilation_equals_scipy(k):
    from scipy.ndimage import binary_dilation
    from tracktolearn_amd.experiment.tractometer_validator import dilate
    rng = np.random.default_rng(3)
    mask = rng.random((9, 8, 7)) < 0.06
    mask[0, 0, 0] = mask[8, 7, 6] = True           # the volume's corners
    want = binary_dilation(mask, iterations=k) if k else mask
    got = dilate(mask.astype(np.uint8) * 3, k)     # non-zero counts as 1
    assert got.dtype == bool and np.array_equal(got, want)
    assert k == 0 or got.sum() > mask.sum()


def test_bit_planes_and_limits_table():
    from tracktolearn_amd.experiment.tractometer_validator import (bundle_word, limits_table,
                                                                   pack_bit_planes)
    rng = np.random.default_rng(4)
    dims = (3, 4, 5)
    masks = [rng.random(dims) < 0.4 if b % 3 else None for b in range(64)]
    masks[63] = np.ones(dims, np.int16) * 7
    planes = pack_bit_planes(masks, dims)
    filled = pack_bit_planes(masks, dims, missing=True)
    assert planes.dtype == np.uint64 and planes.shape == (60,)
    for b in (0, 1, 31, 32, 62, 63):
        bit = (planes.reshape(dims) >> np.uint64(b)) & np.uint64(1)
        fbit = (filled.reshape(dims) >> np.uint64(b)) & np.uint64(1)
        if masks[b] is None:
            assert not bit.any() and fbit.all()
        else:
            assert np.array_equal(bit != 0, np.asarray(masks[b]) != 0)
            assert np.array_equal(fbit, bit)
    # C order: the word of (x, y, z) is (x * Y + y) * Z + z
    one = np.zeros(dims, bool)
    one[2, 1, 3] = True
    assert np.flatnonzero(pack_bit_planes([one], dims)).tolist() == [(2 * 4 + 1) * 5 + 3]
    assert bundle_word(m is not None for m in masks) == sum(1 << b for b in range(64) if b % 3
                                                            or b == 63)
    with pytest.raises(ValueError, match='at most 64'):
        pack_bit_planes([one] * 65, dims)
    with pytest.raises(ValueError, match='shape'):
        pack_bit_planes([np.zeros((3, 4, 6), bool)], dims)
    t = limits_table([None, [20, 180]], [None, 300], [None, [[1, 2], [0, np.inf], [3, 4]]],
                     [[[0, np.inf], [5, 6], [0, np.inf]], None])
    inf = np.inf
    assert t.shape == (2, 16) and t.dtype == np.float64
    assert t[0].tolist() == [-inf, inf] * 4 + [0, inf, 5, 6, 0, inf] + [inf, 0]
    assert t[1].tolist() == [20, 180, 1, 2, 0, inf, 3, 4] + [-inf, inf] * 3 + [300, 0]


def test_definition_on_hand_computed_quantities():
    """Lengths and the winding of the reference against numbers worked out by
    hand."""
    length, d, a = ref.lengths([(0.5, 3.5, 4.5), (0.5, 5.5, 4.5), (11.5, 5.5, 5.5),
                                (10.5, 5.5, 4.5)], tc.LIN)
    # v = (1, 3, 0), (22, 0, 1.25), (-2, 0, -1.25)
    assert length == np.sqrt(10.0) + np.sqrt(22 * 22 + 1.5625) + np.sqrt(4 + 1.5625)
    assert d.tolist() == [21.0, 3.0, 0.0] and a.tolist() == [25.0, 3.0, 2.5]
    # a straight row: 180 degrees, all of it where the row passes its centroid
    assert abs(ref.winding(np.array([[0, 0, 0], [1, 0.5, 0], [2, 1, 0], [6, 3, 0]],
                                    np.float32)) - 180.0) < 1e-6
    # twice round a square seen from its middle: seven quarter turns
    square = np.array([[1, 1, 0], [-1, 1, 0], [-1, -1, 0], [1, -1, 0], [1, 1, 0],
                       [-1, 1, 0], [-1, -1, 0], [1, -1, 0]], np.float32)
    assert abs(ref.winding(square) - 7 * 90.0) < 1e-6
    assert ref.end_voxel((-0.3, 1.0, 2.99), (4, 4, 4)) is None
    assert ref.end_voxel((-0.3, 1.0, 2.99), (4, 4, 4), 'trunc_ends') == (0, 1, 2)
    assert ref.end_voxel((3.0, 0.0, 3.999), (4, 4, 4)) == (3, 0, 3)
    assert ref.end_voxel((4.0, 0.0, 0.0), (4, 4, 4)) is None


@pytest.mark.parametrize('B', SETS)
def test_definition_on_hand_built_streamlines(B):
    """The designed rows get the bundle worked out by hand (tractometer_cases:
    the role a row was built for, or none), with the connected sets that go
    with it."""
    c = tc.case(B)
    roles = tc.ROLES[B]
    got = c['score']
    n_hand = 0
    for r, (name, want) in enumerate(zip(c['names'], c['want'])):
        if want is None:
            continue
        n_hand += 1
        assert got['bundle'][r] == want, (name, want, got['bundle'][r])
        if want >= 0:
            assert int(got['connected'][r]) >> want & 1, name
    assert n_hand >= 39
    conn = dict(zip(c['names'], (int(v) for v in got['connected'])))
    L = 1 << roles['L']
    assert conn['head_to_tail'] == conn['tail_to_head'] == conn['nan_mid_row'] == L
    assert conn['length_below_lo'] == conn['straight_65_nan_last_lane'] == L
    for name in ('head_to_head', 'end_on_face_out', 'end_minus_third', 'end_outside',
                 'no_points', 'one_point'):
        assert conn[name] == 0, name
    assert conn['hole_by_walk_only'] == conn['touches_nothing'] == 1 << roles['AY']
    assert conn['deep_arc_200'] == 1 << roles['W']
    if 'P2' in roles:
        both = (1 << 2) | (1 << 5)
        assert conn['valid_for_2_and_5'] == conn['valid_for_5_only'] == both
    # the filler bundles take part: walks connect and join them
    if B > 3:
        designed = set(roles.values())
        assert any(b >= 0 and b not in designed for b in got['bundle'])
    assert got['metrics']['VB'] >= 3 and 0 < got['metrics']['VC'] < 1
    assert 0 < got['metrics']['mean_OL'] < 1


@pytest.mark.parametrize('key', SETS + ('grid',))
def test_sums_may_be_compared_exactly(key):
    _assert_margins(key)
    # the limits at their inclusive bounds are among the decisions
    if key != 'grid':
        at_bound = [m for m in _margins(key) if m[3] == m[4]]
        assert {m[2] for m in at_bound} >= {'length', 'dir0', 'dir1', 'absdir2'}
        assert any(m[2] == 'winding' for m in _margins(key))


def test_every_mutant_has_a_witness_in_the_launched_sets():
    """Each named deviation changes ``bundle``, ``connected`` or ``counts`` of
    a case set the GPU tests launch and compare exactly."""
    for mutant in ref.MUTANTS:
        seen = []
        for B in SETS:
            c = tc.case(B)
            got = ref.score(c['points'], c['offsets'], tc.DIMS, c['bundles'], tc.LIN, mutant)
            seen += [B for k in ('bundle', 'connected', 'counts')
                     if not np.array_equal(got[k], c['score'][k])]
        print(mutant, sorted(set(seen)))
        assert seen, mutant


def test_grid_case_takes_a_second_pass():
    c = tc.grid_case()
    lens = np.diff(c['offsets'])
    assert len(lens) == tc.GRID_ROWS > tc.GRID_PASS
    second = lens[tc.GRID_PASS:]
    first = lens[:len(second)]
    # one wave, two rows of different length back to back, both ways round
    assert ((first >= 65) & (second <= 3)).sum() > 20
    assert ((first <= 3) & (second >= 65)).sum() > 20
    b = c['score']['bundle']
    assert (b[tc.GRID_PASS:] >= 0).sum() > 100 and len(set(b.tolist())) == 4


def test_metrics_from_counts():
    from tracktolearn_amd.experiment.tractometer_validator import metrics
    for B in SETS:
        c = tc.case(B)
        sc = c['score']
        n = len(sc['bundle'])
        per_bundle = np.bincount(sc['bundle'] + 1, minlength=B + 1)[1:]
        sizes = [None if b['gt'] is None else int(b['gt'].sum()) for b in c['bundles']]
        assert metrics(n, per_bundle, sc['counts'], sizes) == sc['metrics']
    assert metrics(4, [0, 0], [[0, 0], [0, 0]], [None, 0]) == {
        'VC': 0.0, 'IC': 0, 'IS': 0, 'NC': 1.0, 'mean_OL': 0.0, 'VB': 0, 'IB': 0}


def test_trainer_needs_scoring_data(tmp_path):
    from tracktolearn_amd.trainers import sac_auto_train
    from tracktolearn_amd.trainers.train import add_training_args
    with pytest.raises(ValueError, match='needs --scoring_data'):
        sac_auto_train.main(tc._train_args(tmp_path, ['--tractometer_validator']))
    empty = tmp_path / 'scoring'
    empty.mkdir()
    with pytest.raises(ValueError, match='scil_scoring_config.json'):
        sac_auto_train.main(tc._train_args(tmp_path, ['--tractometer_validator',
                                                   '--scoring_data', str(empty)]))
    parser = argparse.ArgumentParser()
    add_training_args(parser)
    assert '(ignored)' not in parser.format_help()


def test_c_abi_rejects_bad_arguments():
    """The argument checks come before any device work: a null pointer, B
    outside 1 .. 64, a dim < 1 and n < 0 return TTL_ERR_INVALID."""
    from tracktolearn_amd import _lib
    lib = _lib.load()
    p = 4096                                      # never dereferenced
    dims = (C.c_int32 * 3)(12, 9, 7)
    lin = (C.c_double * 9)(*np.eye(3).reshape(-1))

    def classify(**kw):
        a = dict(points=p, offsets=p, n=1, dims=dims, B=3, head=p, tail=p, all=p, any=p,
                 has_all=0, has_any=0, limits=p, lin=lin, bundle=p, connected=p)
        a.update(kw)
        return lib.ttl_tractometer_classify(
            a['points'], a['offsets'], a['n'], a['dims'], a['B'], a['head'], a['tail'], a['all'],
            a['any'], a['has_all'], a['has_any'], a['limits'], a['lin'], a['bundle'],
            a['connected'], None)

    def overlap(**kw):
        a = dict(points=p, offsets=p, n=1, bundle=p, dims=dims, B=3, gt=p, visited=p, counts=p)
        a.update(kw)
        return lib.ttl_tractometer_overlap(a['points'], a['offsets'], a['n'], a['bundle'],
                                           a['dims'], a['B'], a['gt'], a['visited'], a['counts'],
                                           None)

    bad_dims = [(C.c_int32 * 3)(*d) for d in ((0, 9, 7), (12, -1, 7), (12, 9, 0))]
    for name in ('points', 'offsets', 'dims', 'head', 'tail', 'all', 'any', 'limits', 'lin',
                 'bundle', 'connected'):
        assert classify(**{name: None}) == _lib.ERR_INVALID, name
    for name in ('points', 'offsets', 'bundle', 'dims', 'gt', 'visited', 'counts'):
        assert overlap(**{name: None}) == _lib.ERR_INVALID, name
    for call in (classify, overlap):
        for B in (0, -1, 65):
            assert call(B=B) == _lib.ERR_INVALID
        for d in bad_dims:
            assert call(dims=d) == _lib.ERR_INVALID
        assert call(n=-1) == _lib.ERR_INVALID
    assert b'ttl_tractometer_overlap' in lib.ttl_last_error()
    assert classify(n=0) == 0                     # nothing to do, nothing touched
    assert lib.ttl_abi_version() == 13


# ----------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize('B', SETS)
def test_classify_and_overlap_equal_the_definition(B):
    """``bundle``, ``connected``, ``counts`` and ``visited_bits`` of the case
    set with the deciding bundles at the top bits of B, exactly."""
    _assert_margins(B)
    c = tc.case(B)
    want = c['score']
    bundle, connected, counts, visited = _run(c['points'], c['offsets'], c['bundles'])
    wrong = np.flatnonzero((bundle != want['bundle']) | (connected != want['connected']))
    assert len(wrong) == 0, [(c['names'][r], int(bundle[r]), int(want['bundle'][r]),
                              hex(int(connected[r])), hex(int(want['connected'][r])))
                             for r in wrong[:8]]
    assert np.array_equal(counts, want['counts']), (counts, want['counts'])
    assert np.array_equal(visited, want['visited'])
    assert counts.sum() > 0


@pytest.mark.gpu
def test_overlap_only_ors_ones_in():
    """A bit volume that already holds bits keeps them; rows with bundle -1 mark
    nothing (their voxels show only what was there)."""
    c = tc.case(64)
    want = c['score']
    rng = np.random.default_rng(9)
    before = rng.integers(0, 2 ** 63, tc.DIMS, dtype=np.uint64) & \
        rng.integers(0, 2 ** 63, tc.DIMS, dtype=np.uint64)
    before |= (rng.random(tc.DIMS) < 0.3).astype(np.uint64) << np.uint64(63)
    _, _, counts, visited = _run(c['points'], c['offsets'], c['bundles'], visited=before)
    assert np.array_equal(visited, before | want['visited'])
    unmarked = want['visited'] == 0
    assert unmarked.any() and np.array_equal(visited[unmarked], before[unmarked])
    # the counts are those of the whole bit volume
    full = before | want['visited']
    for b in (0, 5, 40, 63):
        bit = (full >> np.uint64(b)) & np.uint64(1) != 0
        gt = c['bundles'][b]['gt']
        gt = np.zeros(tc.DIMS, bool) if gt is None else gt
        assert counts[b].tolist() == [int((bit & gt).sum()), int((bit & ~gt).sum())]


@pytest.mark.gpu
def test_grid_stride_rows():
    """40 000 rows: above the 32 768 of one pass of the capped grid."""
    _assert_margins('grid')
    c = tc.grid_case()
    want = c['score']
    bundle, connected, counts, visited = _run(c['points'], c['offsets'], c['bundles'])
    wrong = np.flatnonzero((bundle != want['bundle']) | (connected != want['connected']))
    assert len(wrong) == 0, (wrong[:8], bundle[wrong[:8]], want['bundle'][wrong[:8]])
    assert np.array_equal(counts, want['counts'])
    assert np.array_equal(visited, want['visited'])


# ---- end to end
def _e2e_bundles():
    """The B = 3 set with limits that suit AFFINE's linear part."""
    bundles = [dict(b) for b in tc.scoring_set(3)]
    bundles[0].update(length=[21.8, 23.5], dir=None, absdir=[[0, np.inf], [0, 9.0], [0, np.inf]])
    # the angle bundle's ROIs one voxel thinner: dilated once they reach the arcs at
    # z = 5.9 but not the straight rows at z = 4.5, which span no plane to wind in
    for key in ('head', 'tail'):
        thin = bundles[2][key].copy()
        thin[:, :, :6] = False
        bundles[2][key] = thin
    return bundles


def _e2e_lines():
    """Designed rows that sit away from voxel faces and limits (the two input
    paths differ by float32 rounding of the file's coordinates), and walks."""
    rng = np.random.default_rng(21)
    skip = ('on_face', 'at_hi', 'nan', 'inf', 'no_points', 'one_point')
    lines = [r[1] for r in tc.designed_rows(3) if not any(s in r[0] for s in skip)]
    lines = [s + rng.uniform(0.01, 0.05, 3).astype(np.float32) for s in lines]
    lines += tc.random_walks(rng, 150, 8, 60, 12, step=(0.3, 1.9), start=(0, 7))
    return lines + [np.ones((1, 3), np.float32)]


def _write_scoring_dir(path, bundles, gt_as_trk=None):
    from tracktolearn_amd.io import nifti
    os.makedirs(path, exist_ok=True)
    nifti.save(os.path.join(path, 'ref.nii.gz'), np.zeros(tc.DIMS, np.uint8), AFFINE)
    config = {}
    for b, B in enumerate(bundles):
        entry = {}
        for key, name in (('head', 'head'), ('tail', 'tail'), ('all', 'all_mask'),
                          ('any', 'any_mask'), ('gt', 'gt_mask')):
            if B[key] is None:
                continue
            entry[name] = f'b{b}_{key}.nii.gz'
            dtype = (np.uint8, np.int16, np.float32)[b % 3]
            nifti.save(os.path.join(path, entry[name]), (B[key] * (2 + b)).astype(dtype), AFFINE)
        if gt_as_trk is not None and b == gt_as_trk[0]:
            entry['gt_mask'] = f'b{b}_gt.trk'
            tc.save_trk([s - np.float32(0.5) for s in gt_as_trk[1]],
                        os.path.join(path, entry['gt_mask']))
        if B['length'] is not None:
            entry['length'] = B['length']
        if B['angle'] is not None:
            entry['angle'] = B['angle']
        for key, suffix in (('dir', ''), ('absdir', '_abs')):
            if B[key] is not None:
                for axis, lim in zip('xyz', B[key]):
                    if lim != [0, np.inf]:
                        entry[f'length_{axis}{suffix}'] = lim
        config[f'bundle{b}'] = entry
    with open(os.path.join(path, 'scil_scoring_config.json'), 'w') as f:
        json.dump(config, f)


def _corner(points, M):
    """The stated arithmetic of the intake in float64, rounded to float32."""
    p = np.asarray(points, np.float64)
    return np.stack([(((M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2]) + M[i, 3])
                     + 0.5 for i in range(3)], 1).astype(np.float32)


def test_one_intake_serves_every_path(tmp_path):
    """Rows of 0, 1, 2 and 5 points as a list, a ``Tractogram``, a .trk and a
    .tck: the rows 2 and 3 are kept, and the points are the stated formula's, bit
    for bit, whichever validator asks."""
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels, reference_space
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    rng = np.random.default_rng(12)
    lines = [rng.uniform(0.0, 6.0, (k, 3)).astype(np.float32) for k in (0, 1, 2, 5)]
    kept = np.concatenate(lines[2:])
    trk, tck = str(tmp_path / 't.trk'), str(tmp_path / 't.tck')
    tc.save_trk(lines, trk)
    sio.save_tck(Tractogram(lines).apply_affine(AFFINE), tck)
    shifted = AFFINE.copy()                      # the tracker's grid half a voxel off
    shifted[:3, 3] += AFFINE[:3, :3] @ (0.5, 0.5, 0.5)
    inv = np.linalg.inv(AFFINE)

    def check(source, want, tracker=None):
        points, offsets, index = corner_voxels(source, AFFINE, tracker)
        assert index.dtype == np.int64 and index.tolist() == [2, 3]
        assert offsets.dtype == np.int64 and offsets.tolist() == [0, 2, 7]
        assert points.dtype == np.float32 and np.array_equal(points, want)

    for source in (lines, Tractogram(lines)):
        check(source, _corner(kept, np.eye(4)), AFFINE.copy())     # equal affines: p + 0.5
        assert np.array_equal(_corner(kept, np.eye(4)), kept + np.float32(0.5))
        check(source, _corner(kept, inv @ shifted), shifted)
        with pytest.raises(ValueError, match='give the env'):
            corner_voxels(source, AFFINE)
    for path, load in ((trk, sio.load_trk), (tck, sio.load_tck)):
        read = load(path)[0].streamlines
        assert [len(s) for s in read] == [0, 1, 2, 5] and read[3].dtype == np.float32
        check(path, _corner(np.concatenate(read[2:]), inv))
        check(os.fsencode(path), _corner(np.concatenate(read[2:]), inv))
    # the two validators hand the device the same arrays: each one's own call of the intake
    scoring = str(tmp_path / 'scoring')
    _write_scoring_dir(scoring, _e2e_bundles())
    val = TractometerValidator(scoring, None, device='cpu')
    env = tc.env()

    def same(got, want):
        assert len(got) == len(want) == 3
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)

    for source in (Tractogram(lines), trk, tck):     # the two __call__s
        same(corner_voxels(source, val.space(env)[0], env.affine_vox2rasmm),
             corner_voxels(source, reference_space(env)[0], env.affine_vox2rasmm))
    for source, its_env in ((Tractogram(lines), env), (trk, None)):     # score()
        *scored, affine = val.corner_voxels(source, its_env)
        assert np.allclose(affine, AFFINE, atol=1e-6)    # the .trk header's, in float32
        same(scored, corner_voxels(source, affine, env.affine_vox2rasmm))
    with pytest.raises(ValueError, match='a .tck needs a reference'):
        val.corner_voxels(tck)


def test_neither_trk_nor_tck_is_refused_in_one_place(tmp_path):
    """One dispatch reads tractogram files; every way in meets its error."""
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels, load_tractogram
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    scoring = str(tmp_path / 'scoring')
    _write_scoring_dir(scoring, _e2e_bundles())
    val = TractometerValidator(scoring, os.path.join(scoring, 'ref.nii.gz'), device='cpu')
    bad = str(tmp_path / 'tracks.vtk')
    for call in (lambda: val(bad, tc.env()), lambda: val.score(bad), lambda: val.load(bad),
                 lambda: load_tractogram(bad), lambda: corner_voxels(bad, AFFINE)):
        with pytest.raises(ValueError, match='.trk or .tck'):
            call()
    config = json.load(open(os.path.join(scoring, 'scil_scoring_config.json')))
    config['bundle0']['gt_mask'] = 'b0_gt.vtk'
    with open(os.path.join(scoring, 'scil_scoring_config.json'), 'w') as f:
        json.dump(config, f)
    with pytest.raises(ValueError, match='.trk or .tck'):
        TractometerValidator(scoring, None, device='cpu')


@pytest.mark.gpu
def test_validator_file_and_memory_paths(tmp_path):
    """A scoring directory of NIfTI masks (one gt_mask as a .trk bundle) and a
    config; a reference that is not axis-aligned; the tractogram from memory
    and as a .trk: the same dict, equal to the definition's.  The metrics are
    ratios of integers, so equality is exact."""
    from scipy.ndimage import binary_dilation
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    bundles = _e2e_bundles()
    gt_lines = [tc.arc(40, 2.0, 5), tc.arc(40, 3.0, 6)]
    scoring = str(tmp_path / 'scoring')
    _write_scoring_dir(scoring, bundles, gt_as_trk=(2, gt_lines))
    lines = _e2e_lines()
    env = tc.env()
    tract = Tractogram([s - np.float32(0.5) for s in lines])
    path = str(tmp_path / 'v.trk')
    tc.save_trk(tract.streamlines, path)

    # the definition, on the coordinates each path hands to the device
    want_bundles = [dict(b) for b in bundles]
    for b in want_bundles:
        b['head'], b['tail'] = binary_dilation(b['head']), binary_dilation(b['tail'])
    gt_path = os.path.join(scoring, 'b2_gt.trk')
    gp, go, gi = corner_voxels(gt_path, sio.load_trk(gt_path)[1]['voxel_to_rasmm'])
    assert gi.tolist() == [0, 1]
    want_bundles[2]['gt'] = np.zeros(tc.DIMS, bool)
    for r in range(len(go) - 1):
        for v in ref.voxels(gp[go[r]:go[r + 1]], tc.DIMS):
            want_bundles[2]['gt'][v] = True
    lin = AFFINE[:3, :3]
    wants = []
    for source in (tract, path):
        points, offsets, index = corner_voxels(source, AFFINE, env.affine_vox2rasmm)
        assert len(offsets) - 1 == len(lines) - 1       # the one-point row is dropped
        assert index.dtype == np.int64 and index.tolist() == list(range(len(lines) - 1))
        for r in range(len(offsets) - 1):
            rep = ref.margin_report(points[offsets[r]:offsets[r + 1]], tc.DIMS, want_bundles, lin)
            assert all(m[-1] for m in rep), [m for m in rep if not m[-1]]
        wants.append(ref.score(points, offsets, tc.DIMS, want_bundles, lin)['metrics'])
    assert wants[0] == wants[1]
    assert wants[0]['VB'] == 3 and 0 < wants[0]['mean_OL'] < 1

    for reference in (None, os.path.join(scoring, 'ref.nii.gz')):
        val = TractometerValidator(scoring, reference, dilate_endpoints=1, device=DEV)
        mem, disk = val(tract, env), val(path, env)
        assert list(mem) == ['VC', 'IC', 'IS', 'NC', 'mean_OL', 'VB', 'IB']
        assert mem == wants[0] and disk == wants[0]
    assert val(Tractogram([np.ones((1, 3), np.float32)]), env) == {}
    # without dilation fewer ends lie in an ROI
    points, offsets, _ = corner_voxels(tract, AFFINE, env.affine_vox2rasmm)
    for b, undilated in zip(want_bundles, bundles):
        b['head'], b['tail'] = undilated['head'], undilated['tail']
    want_plain = ref.score(points, offsets, tc.DIMS, want_bundles, lin)['metrics']
    assert want_plain['VC'] < wants[0]['VC']
    plain = TractometerValidator(scoring, None, dilate_endpoints=0, device=DEV)(tract, env)
    assert plain == want_plain
    # masks of other dimensions are refused
    from tracktolearn_amd.io import nifti
    nifti.save(os.path.join(scoring, 'b0_head.nii.gz'), np.ones((12, 9, 8), np.uint8), AFFINE)
    with pytest.raises(ValueError, match='dimensions'):
        TractometerValidator(scoring, os.path.join(scoring, 'ref.nii.gz'), device=DEV)


@pytest.mark.gpu
def test_sac_auto_train_tractometer_validator(tmp_path, capsys):
    """--tractometer_validator --scoring_data DIR end to end: the score dict is
    printed at every validation, the six monitors are written, and the note
    that the flag is ignored is gone."""
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.trainers import sac_auto_train
    D = 20
    tc._write_dataset(str(tmp_path / 'ds.npz'), D)
    scoring = tmp_path / 'scoring'
    scoring.mkdir()
    low, high, whole = (np.zeros((D, D, D), np.uint8) for _ in range(3))
    low[:D // 2], high[D // 2:], whole[:] = 1, 1, 1
    for name, vol in (('low', low), ('high', high), ('whole', whole)):
        nifti.save(str(scoring / f'{name}.nii.gz'), vol, np.eye(4))
    (scoring / 'scil_scoring_config.json').write_text(json.dumps({
        'long': {'head': 'low.nii.gz', 'tail': 'high.nii.gz', 'gt_mask': 'whole.nii.gz',
                 'length': [6, 1000]},
        'any': {'head': 'low.nii.gz', 'tail': 'high.nii.gz', 'gt_mask': 'whole.nii.gz'}}))
    sac_auto_train.main(tc._train_args(tmp_path, ['--tractometer_validator', '--scoring_data',
                                               str(scoring), '--tractometer_dilate', '0']))
    out = capsys.readouterr().out
    assert 'tractometer_validator is outside the scope' not in out
    assert out.count("'VC':") == 4 and out.count("'mean_OL':") == 4
    plots = tmp_path / 'exp' / 'plots'
    for name in ('vc', 'ic', 'nc', 'vb', 'ib', 'mean_ol'):
        series = np.load(plots / f'{name}.npy')
        assert series.shape == (4, 2), name
    vc, nc = np.load(plots / 'vc.npy')[:, 1], np.load(plots / 'nc.npy')[:, 1]
    assert ((vc >= 0) & (vc <= 1)).all() and np.allclose(vc + nc, 1)
    assert (np.load(plots / 'ic.npy')[:, 1] == 0).all()
    assert not (plots / 'oracle.npy').exists()
