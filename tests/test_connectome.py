"""The structural connectome (ttl_connectome_assign / ttl_connectome_accumulate,
connectome.py, ``Tracker(connectome=...)``, ``ttl_track.py --connectome``,
``ttl_connectome.py``) against tests/ref_connectome.py, the
definition of include/ttl_hip.h as a literal loop, on the sets of
tests/connectome_cases.py.  Nodes and matrices are compared exactly; the length
is held to a derived bound against the definition in numpy.longdouble."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import connectome_cases as cases
import ref_connectome as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
SET_NAMES = sorted(cases.SETS)


# ------------------------------------------------------------------ CPU part
def test_definition_on_a_line_of_voxels():
    """labels 1 0 0 2 0 5 along z with N = 2 (5 names no node), 2 mm voxels along
    z, radius 2 mm: reach (2, 2, 1)."""
    labels = np.array([1, 0, 0, 2, 0, 5], np.int32).reshape(1, 1, 6)
    lin = np.diag([1.0, 1.0, 2.0])
    reach = ref.reach_for(lin, 2.0)
    assert reach == [2, 2, 1]
    z_and_node = [
        (0.5, 1),       # inside node 1
        (1.5, 1),       # voxel 1 is empty; the centre of voxel 0 is 2 mm away: inclusive
        (2.5, 2),       # voxel 2 is empty; voxel 3 is 2 mm away, voxel 1 is empty
        (2.25, 0),      # ... 2.5 mm: beyond the radius
        (4.5, 2),       # between node 2 and the label above N
        (5.5, 0),       # inside the label above N, beside an empty voxel
        (-0.3, 1),      # voxel -1: outside, the centre of voxel 0 is 1.6 mm away
        (6.0, 0),       # dims exactly: outside, beside the label above N
        (1e30, 0),
    ]
    for z, want in z_and_node:
        assert ref.end_node((0.5, 0.5, z), labels, lin, 2.0, reach, 2) == want, z
    rows = [np.array([(0.5, 0.5, 0.5), (0.5, 0.5, 2.5)], F32),                 # 1 - 2, 4 mm
            np.array([(0.5, 0.5, 4.5), (0.25, 0.5, 3.0), (0.5, 0.5, -0.3)], F32),    # 2 - 1
            np.array([(0.5, 0.5, 5.5), (0.5, 0.5, 5.5)], F32),                 # 0 - 0, 0 mm
            np.array([(0.5, 0.5, 0.5)], F32),                                  # one point
            np.array([(0.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (0.5, 0.5, 0.5)], F32)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    node, length, exact = ref.assign(np.concatenate(rows), offsets, labels, lin, 2.0, reach, 2)
    assert node.tolist() == [[1, 2], [2, 1], [0, 0], [-1, -1], [-1, -1]]
    assert length[0] == 4.0 and length[2] == 0.0 and length[3] == 0.0 and length[4] == 0.0
    assert abs(float(exact[1]) - length[1]) < 1e-12 and 9.0 < length[1] < 9.7
    count, length_q = ref.accumulate(node, length, 2)
    assert count.tolist() == [[1, 0, 0], [0, 0, 2], [0, 0, 0]]
    assert length_q[1, 2] == 4 * 2 ** 20 + int(np.rint(length[1] * 2 ** 20))
    assert length_q[0, 0] == 0 and length_q.sum() == length_q[1, 2]


def test_sets_hold_what_they_are_for():
    """Every kind of end of the issue's list decides as intended somewhere."""
    box = dict(zip([tuple(float(F32(v)) for v in e) for e in cases.BOX_ENDS],
                   cases.end_nodes('box_diag_tie')))
    f = lambda *e: box[tuple(float(F32(v)) for v in e)]
    assert f(2.25, 2.5, 1.75) == 1 and f(3.5, 2.5, 1.5) == 1        # inside; tie: lower index
    assert f(-20.0, 2.0, 1.0) == 0 and f(1e30, 1.0, 1.0) == 0
    wide = dict(zip([tuple(float(F32(v)) for v in e) for e in cases.BOX_ENDS],
                    cases.end_nodes('box_diag_max')))
    assert wide[(3.5, 2.0, 1.5)] == 3                               # four-way tie: (2, 1, 1)
    assert wide[(3.25, 2.5, 1.5)] == 1
    assert wide[tuple(float(F32(v)) for v in (-0.3, 0.5, 0.5))] == 1
    for name in SET_NAMES:
        c = cases.case(name)
        node, length, _ = cases.expected(name)
        L = np.diff(c.offsets)
        assert set(cases.ROW_LENGTHS) | {0, 1} <= set(L.tolist())
        assert (node[L < 2] == -1).all() and (node[:, 0] >= 0).sum() > 60
        assert (node[:, 0] < 0).sum() >= 10                         # NaN rows, 2^40 mm, L < 2
        assert node.max() <= c.n_nodes and (c.labels > c.n_nodes).any() and (c.labels < 0).any()
        assert (np.array(c.reach) <= cases.MAX_REACH).all()
    assert max(cases.case('box_diag_max').reach) == cases.MAX_REACH
    assert np.array(cases.case('box_diag_max').reach).min() >= 4       # the box exceeds (7, 5, 4)


@pytest.mark.parametrize('mutant', ref.ASSIGN_MUTANTS)
def test_every_assign_mutant_has_a_witness(mutant):
    witnesses = [name for name in SET_NAMES
                 if cases.end_nodes(name, mutant) != cases.end_nodes(name)]
    assert witnesses, mutant


@pytest.mark.parametrize('mutant', ref.ACCUMULATE_MUTANTS)
def test_every_accumulate_mutant_has_a_witness(mutant):
    c = cases.case('box_diag_max')
    node, length, _ = cases.expected('box_diag_max')
    true = ref.accumulate(node, length, c.n_nodes)
    wrong = ref.accumulate(node, length, c.n_nodes, mutant=mutant)
    assert not all(np.array_equal(a, b) for a, b in zip(true, wrong))
    fast = ref.accumulate_fast(node, length, c.n_nodes)
    assert all(np.array_equal(a, b) for a, b in zip(true, fast))


def test_reach_for():
    from tracktolearn_amd.connectome import MAX_REACH, reach_for
    assert reach_for(np.eye(3), 0.0).tolist() == [0, 0, 0]
    assert reach_for(np.eye(3), 2.0).tolist() == [2, 2, 2]
    assert reach_for(np.eye(3), 2.0).dtype == np.int32
    assert reach_for(np.diag([2.0, 1.0, 1.5]), 2.0).tolist() == [1, 2, 2]
    assert reach_for(np.diag([-2.0, 1.0, 0.5]), 1.25).tolist() == [1, 2, 3]
    assert reach_for(cases.LINS['shear'], 1.0).tolist() == [2, 1, 1]     # sqrt(1.25), 1, 0.5
    assert reach_for(np.eye(3), 8.0).tolist() == [8, 8, 8] and MAX_REACH == 8
    for name in SET_NAMES:
        c = cases.case(name)
        assert reach_for(c.lin, c.radius_mm).tolist() == c.reach
    with pytest.raises(ValueError, match='largest radius for this voxel size is 4 mm'):
        reach_for(np.eye(3) * 0.5, 4.5)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            reach_for(np.eye(3), bad)


def test_matrices_symmetrise_and_average():
    from tracktolearn_amd.connectome import load_labels, matrices_from
    count = np.array([[5, 1, 2, 0], [0, 3, 4, 0], [0, 0, 0, 6], [0, 0, 0, 0]], np.int64)
    q = np.array([[99, 9, 9, 0], [0, 3 << 20, 6 << 20, 0], [0, 0, 0, 9 << 19], [0, 0, 0, 0]],
                 np.int64)
    m = matrices_from(count, q)
    assert m['count'].tolist() == [[3, 4, 0], [4, 0, 6], [0, 6, 0]] and m['count'].dtype == np.int64
    assert m['length_sum_mm'].tolist() == [[3.0, 6.0, 0.0], [6.0, 0.0, 4.5], [0.0, 4.5, 0.0]]
    assert m['mean_length_mm'].tolist() == [[1.0, 1.5, 0.0], [1.5, 0.0, 0.75], [0.0, 0.75, 0.0]]
    assert m['unassigned_one_end'].tolist() == [1, 2, 0] and m['unassigned_both'] == 5
    labels, n = load_labels(np.array([[[0.0, 2.0, -7.0]]]))
    assert n == 2 and labels.dtype == np.int32 and labels.tolist() == [[[0, 2, 0]]]
    # every integer dtype a parcellation comes in, the unsigned ones included
    for dtype in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32,
                  np.int64):
        labels, n = load_labels(np.array([[[0, 2, 1], [84, 0, 3]]], dtype))
        assert n == 84 and labels.dtype == np.int32 and labels.flags.c_contiguous
        assert labels.tolist() == [[[0, 2, 1], [84, 0, 3]]], dtype
    labels, n = load_labels(np.array([[[-(2 ** 40), 4096, -1]]], np.int64))
    assert n == 4096 and labels.tolist() == [[[0, 4096, 0]]]
    labels, n = load_labels(np.asfortranarray(np.arange(24, dtype=np.uint16).reshape(2, 3, 4)))
    assert n == 23 and labels.flags.c_contiguous and labels[1, 2, 3] == 23
    with pytest.raises(ValueError):
        load_labels(np.array([[[0, 2 ** 40]]], np.uint64))
    for bad in (np.zeros((2, 2, 2)), np.full((1, 1, 1), 4097), np.array([[[0.5, 1.0]]]),
                np.array([[[np.nan, 1.0]]]), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            load_labels(bad)


def _assign_args():
    """Arguments that pass every check of ttl_connectome_assign: the pointers are
    never followed, TTL_ERR_INVALID and n == 0 return before any HIP call."""
    p = C.c_void_p(4096)
    return dict(points=p, offsets=p, n=0, labels=p, dims=(C.c_int32 * 3)(7, 5, 4), n_nodes=3,
                lin=(C.c_double * 9)(*np.eye(3).reshape(-1)), radius_mm=2.0,
                reach=(C.c_int32 * 3)(2, 2, 2), node=p, length=p, stream=None)


ASSIGN_INVALID = [(k, None) for k in ('points', 'offsets', 'labels', 'dims', 'lin', 'reach',
                                      'node', 'length')] + [
    ('n', -1), ('n_nodes', 0), ('n_nodes', -3), ('n_nodes', 4097),
    ('dims', (C.c_int32 * 3)(0, 5, 4)), ('dims', (C.c_int32 * 3)(7, 5, -1)),
    ('reach', (C.c_int32 * 3)(-1, 0, 0)), ('reach', (C.c_int32 * 3)(0, 9, 0)),
    ('radius_mm', -0.5), ('radius_mm', float('nan')), ('radius_mm', float('inf'))]


@pytest.mark.parametrize('key,value', ASSIGN_INVALID)
def test_assign_refuses_before_any_hip_call(key, value):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    args = _assign_args()
    assert lib.ttl_connectome_assign(*args.values()) == 0            # n == 0: a no-op
    args[key] = value
    assert lib.ttl_connectome_assign(*args.values()) == _lib.ERR_INVALID
    assert b'ttl_connectome_assign' in lib.ttl_last_error()


@pytest.mark.parametrize('key,value', [('node', None), ('count', None), ('length_q', None),
                                       ('n', -1), ('n_nodes', 0), ('n_nodes', 4097)])
def test_accumulate_refuses_before_any_hip_call(key, value):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)
    args = dict(node=p, length=p, n=0, n_nodes=4096, count=p, length_q=p, stream=None)
    assert lib.ttl_connectome_accumulate(*args.values()) == 0
    assert lib.ttl_connectome_accumulate(*dict(args, length=None).values()) == 0
    args[key] = value
    assert lib.ttl_connectome_accumulate(*args.values()) == _lib.ERR_INVALID
    assert b'ttl_connectome_accumulate' in lib.ttl_last_error()


def test_header_announces_the_feature_and_keeps_the_abi():
    from tracktolearn_amd import _lib, connectome
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'^#define TTL_HAS_CONNECTOME 1$', header, re.M)
    assert re.search(r'^#define TTL_ABI_VERSION 13$', header, re.M)
    assert re.search(r'^#define TTL_CONNECTOME_MAX_NODES 4096$', header, re.M)
    assert re.search(r'^#define TTL_CONNECTOME_MAX_REACH 8$', header, re.M)
    assert re.search(r'^#define TTL_CONNECTOME_LENGTH_SCALE 1048576\.0\b', header, re.M)
    assert (_lib.HAS_CONNECTOME, _lib.ABI_VERSION) == (1, 13)
    assert (connectome.MAX_NODES, connectome.MAX_REACH, connectome.LENGTH_SCALE) == \
        (4096, 8, 2.0 ** 20) and ref.LENGTH_SCALE == 2.0 ** 20
    lib = _lib.load()
    for name in ('ttl_connectome_assign', 'ttl_connectome_accumulate'):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
    from tracktolearn_amd.csrc import build
    assert any(s.endswith('ttl_connectome.hip') for s in build.SOURCES)


def _track_parse(argv, tmp_path):
    from tracktolearn_amd.runners import ttl_track
    files = []
    for name in ('fodf', 'seed', 'mask', 'labels'):
        f = tmp_path / f'{name}.nii.gz'
        f.write_bytes(b'')
        files.append(str(f))
    argv = [a.replace('LABELS', files[3]).replace('PREFIX', str(tmp_path / 'con')) for a in argv]
    return ttl_track.parse_args(files[:3] + [str(tmp_path / 'out.trk'), '--odf_policy', 'det']
                                + argv)


def test_track_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(SystemExit) as e:
        ttl_track.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--connectome LABELS', '--connectome_out PREFIX', '--connectome_radius MM',
                '--connectome_only'):
        assert opt in text
    args = _track_parse([], tmp_path)
    assert args.connectome is None and not args.connectome_only
    args = _track_parse(['--connectome', 'LABELS', '--connectome_out', 'PREFIX'], tmp_path)
    assert args.connectome.endswith('labels.nii.gz') and args.connectome_radius is None
    args = _track_parse(['--connectome', 'LABELS', '--connectome_out', 'PREFIX',
                         '--connectome_radius', '3.5', '--connectome_only', '--bidirectional',
                         '--compress', '0.1'], tmp_path)
    assert args.connectome_radius == 3.5 and args.connectome_only


@pytest.mark.parametrize('argv,word', [
    (['--connectome', 'LABELS', '--connectome_out', 'PREFIX', '--direct_output'],
     'never makes'),
    (['--connectome_out', 'PREFIX'], 'only with --connectome'),
    (['--connectome_radius', '2'], 'only with --connectome'),
    (['--connectome_only'], 'only with --connectome'),
    (['--connectome', 'LABELS'], '--connectome_out'),
    (['--connectome', 'nowhere.nii.gz', '--connectome_out', 'PREFIX'], 'does not exist'),
    (['--connectome', 'LABELS', '--connectome_out', 'PREFIX', '--connectome_radius', '-1'],
     'must be >= 0 mm'),
])
def test_track_command_parser_errors(argv, word, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        _track_parse(argv, tmp_path)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_connectome_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_connectome
    shim = open(os.path.join(ROOT, 'ttl_connectome.py')).read()
    assert 'from tracktolearn_amd.runners.ttl_connectome import main' in shim
    assert len(shim.splitlines()) == 7
    with pytest.raises(SystemExit) as e:
        ttl_connectome.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('in_tractogram', 'labels', 'out_prefix', '--reference NIFTI', '--radius MM',
                '--save_assignments', '-f'):
        assert opt in text
    for name in ('t.trk', 't.tck', 't.txt', 'labels.nii.gz', 'ref.nii.gz', 'held_count.npy',
                 'nodes_nodes.npy'):
        (tmp_path / name).write_bytes(b'')
    p = lambda name: str(tmp_path / name)
    # a file the run would not write does not hold it up
    assert ttl_connectome.parse_args([p('t.trk'), p('labels.nii.gz'), p('nodes')])
    args = ttl_connectome.parse_args([p('t.trk'), p('labels.nii.gz'), p('out')])
    assert args.radius == 2.0 and args.reference is None and not args.save_assignments
    args = ttl_connectome.parse_args([p('t.tck'), p('labels.nii.gz'), p('held'), '--reference',
                                      p('ref.nii.gz'), '--radius', '0', '--save_assignments', '-f'])
    assert args.radius == 0.0 and args.save_assignments and args.overwrite
    for argv, word in (
            ([p('t.tck'), p('labels.nii.gz'), p('out')], 'needs --reference'),
            ([p('none.trk'), p('labels.nii.gz'), p('out')], 'does not exist'),
            ([p('t.trk'), p('none.nii.gz'), p('out')], 'does not exist'),
            ([p('t.trk'), p('labels.nii.gz'), p('out'), '--reference', p('no.nii.gz')],
             'does not exist'),
            ([p('t.txt'), p('labels.nii.gz'), p('out')], '.trk or .tck'),
            ([p('t.trk'), p('labels.nii.gz'), p('held')], 'use -f'),
            ([p('t.trk'), p('labels.nii.gz'), p('nodes'), '--save_assignments'], 'use -f'),
            ([p('t.trk'), p('labels.nii.gz'), p('out'), '--radius', '-2'], 'must be >= 0 mm'),
            ([p('t.trk'), p('labels.nii.gz')], 'required')):
        with pytest.raises(SystemExit) as e:
            ttl_connectome.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_connectome_command_checks_the_grid(tmp_path):
    """Shape and affine of the reference, or of the .trk's header, against the
    label image's own."""
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.runners.ttl_connectome import scoring_space
    affine = np.array([[2.0, 0, 0, -10], [0, 1.0, 0, 3], [0, 0, 1.5, 7], [0, 0, 0, 1]])
    flipped = affine.copy()
    flipped[0, 0], flipped[0, 3] = -2.0, 4.0
    for name, shape, aff in (('labels', (7, 5, 4), affine), ('same', (7, 5, 4), affine),
                             ('flipped', (7, 5, 4), flipped), ('larger', (7, 5, 5), affine)):
        nifti.save(str(tmp_path / f'{name}.nii.gz'), np.ones(shape, np.int16), aff)
    labels = nifti.load(str(tmp_path / 'labels.nii.gz'))
    header = {'dimensions': (7, 5, 4), 'voxel_to_rasmm': affine.astype(np.float32)}
    assert np.array_equal(scoring_space(labels, header, None, 't.trk'), affine)
    assert np.array_equal(scoring_space(labels, None, str(tmp_path / 'same.nii.gz'), 't.tck'),
                          affine)
    # a reference decides, whatever the .trk's header says
    assert np.array_equal(scoring_space(labels, dict(header, dimensions=(1, 1, 1)),
                                        str(tmp_path / 'same.nii.gz'), 't.trk'), affine)
    for name in ('flipped', 'larger'):
        with pytest.raises(ValueError, match='not on the grid'):
            scoring_space(labels, None, str(tmp_path / f'{name}.nii.gz'), 't.tck')
    for bad in (dict(header, dimensions=(7, 5, 5)), dict(header, voxel_to_rasmm=flipped)):
        with pytest.raises(ValueError, match='give a reference'):
            scoring_space(labels, bad, None, 't.trk')


class _Labels:
    dims = (4, 4, 4)


def test_tracker_refusals(monkeypatch):
    import torch.distributed as dist
    from tracktolearn_amd.tracking.tracker import Tracker
    con = _Labels()
    assert Tracker(None, 1).connectome is None
    assert Tracker(None, 1, connectome=con).connectome is con
    assert Tracker(None, 1, connectome=con, device_output=True).connectome is con
    with pytest.raises(ValueError, match='device_output'):
        Tracker(None, 1, connectome=con, device_output=False)
    with pytest.raises(ValueError, match='track_to_file'):
        Tracker(None, 1, connectome=con).track_to_file(None, 'out.trk')
    with pytest.raises(ValueError, match='connectome'):
        Tracker(None, 1).track_connectome(None)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_rank', lambda: 1)
    monkeypatch.setattr(dist, 'get_world_size', lambda: 2)
    assert Tracker(None, 1).group_size == 2
    with pytest.raises(ValueError, match='ranks'):
        Tracker(None, 1, connectome=con)


# ------------------------------------------------------------------ GPU part
def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def gpu_assign(c, points, offsets):
    from tracktolearn_amd import connectome as con
    node, length = con.assign_nodes(_dev(points), _dev(offsets), _dev(c.labels.reshape(-1)),
                                    c.dims, c.lin, c.radius_mm, c.n_nodes)
    return node.cpu().numpy(), length.cpu().numpy()


def gpu_accumulate(node, length, n_nodes, matrices=None):
    import torch
    from tracktolearn_amd import connectome as con
    side = n_nodes + 1
    if matrices is None:
        matrices = (torch.zeros((side, side), dtype=torch.int64, device=DEV),
                    torch.zeros((side, side), dtype=torch.int64, device=DEV))
    con.accumulate(_dev(np.asarray(node, np.int32)),
                   None if length is None else _dev(np.asarray(length, np.float64)),
                   n_nodes, *matrices)
    return matrices


def class_labels(c):
    """The set's labels as a ``Connectome`` takes them: its N is the largest
    label, so the values above the set's N become 0 -- no node either way."""
    labels = np.where(c.labels > c.n_nodes, 0, c.labels).astype(np.int32)
    assert labels.max() == c.n_nodes
    return labels


def same_matrices(got, want):
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, 'cpu') else g
        assert g.dtype == np.int64 and np.array_equal(g, w)
        assert not np.tril(g, -1).any()                 # only the upper triangle is touched


@pytest.fixture(scope='module')
def assigned():
    """{set: (node, length)} of one launch per set, shared by the tests below."""
    out = {}
    for name in SET_NAMES:
        c = cases.case(name)
        out[name] = gpu_assign(c, c.points, c.offsets)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', SET_NAMES)
def test_nodes_are_the_definitions(assigned, name):
    node, length = assigned[name]
    want, want_length, _ = cases.expected(name)
    assert node.dtype == np.int32 and node.shape == want.shape
    assert np.array_equal(node, want), np.flatnonzero((node != want).any(axis=1))[:10]
    assert np.array_equal(length == 0.0, want_length == 0.0)
    assert (length[want[:, 0] < 0] == 0.0).all()


@pytest.mark.gpu
def test_lengths_are_within_the_derived_bound(assigned, capsys):
    """Per streamline |length - longdouble definition| <= (L + 8) 2^-53 A_s
    (ref_connectome.length_bound: derived, not measured).  The largest ratio
    observed on an MI355X is 0.141."""
    worst = 0.0
    for name in SET_NAMES:
        c = cases.case(name)
        node, _, exact = cases.expected(name)
        length = assigned[name][1]
        for s in np.flatnonzero(node[:, 0] >= 0):
            row = c.points[c.offsets[s]:c.offsets[s + 1]]
            bound = ref.length_bound(row, c.lin)
            err = abs(np.longdouble(length[s]) - exact[s])
            if bound > 0:
                worst = max(worst, float(err / bound))
            assert err <= bound, (name, s, len(row), float(err), float(bound))
    with capsys.disabled():
        print(f'\nconnectome length: largest error / bound = {worst:.4f}')
    assert worst > 0.0                                   # some row was rounded at all


@pytest.mark.gpu
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65])
def test_launch_sizes(n):
    for name in ('box_diag_max', 'line_shear_tie'):
        c = cases.case(name)
        want = cases.expected(name)[0][:n]
        node, length = gpu_assign(c, c.points[:c.offsets[n]], c.offsets[:n + 1])
        assert node.shape == (n, 2) and length.shape == (n,)
        assert np.array_equal(node, want)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['box_diag_tie', 'box_neg_max'])
def test_more_rows_than_one_pass_of_the_grid(name):
    """70 000 two-point rows: the assign grid is capped at 8192 workgroups of four
    waves, a wave per row."""
    c = cases.case(name)
    points, offsets, want = cases.two_point_rows(name, 70000)
    node, length = gpu_assign(c, points, offsets)
    assert np.array_equal(node, want)
    assert len(np.unique(want)) >= 3 and np.isfinite(length).all()
    same_matrices(gpu_accumulate(node, length, c.n_nodes),
                  ref.accumulate_fast(node, length, c.n_nodes))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['box_diag_max', 'box_neg_tie', 'line_neg_max'])
def test_accumulate_of_the_kernels_own_rows(assigned, name):
    c = cases.case(name)
    node, length = assigned[name]
    want = ref.accumulate(node, length, c.n_nodes)
    assert want[0].sum() == (node[:, 0] >= 0).sum() > 60
    same_matrices(gpu_accumulate(node, length, c.n_nodes), want)
    # a null length leaves length_q alone
    got = gpu_accumulate(node, None, c.n_nodes)
    same_matrices(got, (want[0], np.zeros_like(want[1])))
    # two calls into the same matrices are one call on the concatenation
    half = len(node) // 2
    two = gpu_accumulate(node[:half], length[:half], c.n_nodes)
    same_matrices(gpu_accumulate(node[half:], length[half:], c.n_nodes, two), want)
    # any permutation of the rows
    for seed in (0, 1):
        order = np.random.RandomState(seed).permutation(len(node))
        same_matrices(gpu_accumulate(node[order], length[order], c.n_nodes), want)


@pytest.mark.gpu
@pytest.mark.parametrize('cell', [(1, 1), (0, 0)])
def test_accumulate_every_row_in_one_cell(cell):
    n = 100000
    rng = np.random.RandomState(3)
    node = np.tile(np.array(cell, np.int32), (n, 1))
    length = rng.uniform(0.0, 300.0, n)
    length[::7] = np.round(length[::7] * 2 ** 20) / 2 ** 20 + 2.0 ** -21     # halves: to even
    want = ref.accumulate_fast(node, length, 3)
    assert want[0][cell] == n and want[0].sum() == n
    same_matrices(gpu_accumulate(node, length, 3), want)


@pytest.mark.gpu
def test_accumulate_rounds_half_to_even():
    length = np.array([0.5, 1.5, 2.5, 3.5, 2.4999, 2.5001]) / 2 ** 20
    node = np.array([[1, 2], [2, 3], [3, 1], [1, 1], [2, 2], [3, 3]], np.int32)
    count, q = gpu_accumulate(node, length, 3)
    q = q.cpu().numpy()
    assert [q[1, 2], q[2, 3], q[1, 3], q[1, 1], q[2, 2], q[3, 3]] == [0, 2, 2, 4, 2, 3]
    same_matrices((count, q), ref.accumulate(node, length, 3))


@pytest.mark.gpu
def test_accumulate_every_cell_distinct_and_skipped_rows_interleaved():
    N = 40
    a, b = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing='ij')
    node = np.stack([a.reshape(-1), b.reshape(-1)], axis=1).astype(np.int32)     # both orders
    rng = np.random.RandomState(5)
    node = node[rng.permutation(len(node))]
    length = rng.uniform(0.0, 250.0, len(node))
    want = ref.accumulate(node, length, N)
    assert (want[0][np.triu_indices(N + 1, 1)] == 2).all() and (np.diag(want[0]) == 1).all()
    same_matrices(gpu_accumulate(node, length, N), want)
    # rows not scored between them change nothing
    mixed = np.full((3 * len(node), 2), -1, np.int32)
    mixed[1::3] = node
    mixed_length = np.zeros(len(mixed))
    mixed_length[1::3] = length
    same_matrices(gpu_accumulate(mixed, mixed_length, N), want)
    # N = 1
    one = np.array([[0, 0], [1, 0], [-1, -1], [0, 1], [1, 1], [1, 1]], np.int32)
    one_length = np.array([1.0, 2.25, 0.0, 3.5, 4.0, 5.0])
    want = ref.accumulate(one, one_length, 1)
    assert want[0].tolist() == [[1, 2], [0, 2]]
    same_matrices(gpu_accumulate(one, one_length, 1), want)


@pytest.mark.gpu
def test_accumulate_largest_node_count_touches_only_the_corners():
    import torch
    N = 4096
    node = np.array([[0, 0], [0, N], [N, 0], [N, N], [N, N], [-1, -1]] * 50, np.int32)
    length = np.arange(len(node), dtype=np.float64) / 8.0
    count, q = gpu_accumulate(node, length, N)
    want = ref.accumulate(np.where(node == N, 1, node), length, 1)      # the corners at N = 1
    corners = lambda m: [[int(m[0, 0]), int(m[0, -1])], [int(m[-1, 0]), int(m[-1, -1])]]
    assert corners(count) == want[0].tolist() == [[50, 100], [0, 100]]
    assert corners(q) == want[1].tolist()
    assert int(torch.count_nonzero(count)) == 3 and int(torch.count_nonzero(q)) == 3
    assert int(count.sum()) == 250


@pytest.mark.gpu
def test_accumulate_more_rows_than_one_pass_of_the_grid():
    """The accumulate grid is capped at 2048 workgroups of 256 rows."""
    n = 2048 * 256 + 777
    rng = np.random.RandomState(9)
    node = rng.randint(0, 4, (n, 2)).astype(np.int32)
    node[rng.randint(0, n, 1000)] = -1
    length = rng.uniform(0.0, 200.0, n)
    same_matrices(gpu_accumulate(node, length, 3), ref.accumulate_fast(node, length, 3))


@pytest.mark.gpu
def test_connectome_does_not_depend_on_the_batch_split(assigned):
    from tracktolearn_amd.connectome import Connectome
    name = 'box_neg_tie'
    c = cases.case(name)
    affine = np.eye(4)
    affine[:3, :3] = c.lin
    affine[:3, 3] = (3.0, -2.0, 1.0)
    node, length = assigned[name]
    want = ref.accumulate(node, length, c.n_nodes)
    n = len(c.rows)
    results = []
    for parts in (1, 3, 17):
        con = Connectome(class_labels(c), affine, radius_mm=c.radius_mm, device=DEV)
        assert con.n_nodes == c.n_nodes and con.dims == c.dims and con.reach.tolist() == c.reach
        cuts = np.linspace(0, n, parts + 1).astype(int)
        got = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            pts = c.points[c.offsets[lo]:c.offsets[hi]]
            got.append(con.add(_dev(pts), _dev(c.offsets[lo:hi + 1] - c.offsets[lo])).cpu().numpy())
        assert np.array_equal(np.concatenate(got), node)
        same_matrices((con.count, con.length_q), want)
        assert con.skipped == (node[:, 0] < 0).sum()
        results.append(con.matrices())
    m = results[0]
    assert m['count'].shape == (c.n_nodes, c.n_nodes) and np.array_equal(m['count'], m['count'].T)
    assert np.triu(m['count']).sum() + m['unassigned_one_end'].sum() + m['unassigned_both'] + \
        (node[:, 0] < 0).sum() == n
    for other in results[1:]:
        for key in m:
            assert np.array_equal(m[key], other[key]), key
    with pytest.raises(ValueError):
        Connectome(np.zeros(c.dims, np.int32), affine, device=DEV)
    with pytest.raises(ValueError):
        Connectome(class_labels(c), affine, radius_mm=100.0, device=DEV)


def _mm_lines(c, affine, n=120, seed=2):
    """Finite streamlines in RAS mm whose voxel coordinates cover the volume and
    its surroundings, with rows of 1 point among them."""
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        L = 1 if i % 40 == 7 else int(rng.randint(2, 30))
        vox = np.stack([rng.uniform(-2.0, d + 2.0, L) for d in c.dims], axis=1)
        lines.append((vox @ affine[:3, :3].T + affine[:3, 3]).astype(F32))
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize('ext', ['.trk', '.tck'])
def test_add_tractogram_goes_through_the_one_intake(tmp_path, ext):
    from tracktolearn_amd.connectome import Connectome
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    c = cases.case('box_diag_max')
    affine = np.eye(4)
    affine[:3, :3] = c.lin
    affine[:3, 3] = (-5.0, 2.0, 7.5)
    lines = _mm_lines(c, affine)
    path = str(tmp_path / ('lines' + ext))
    header = sio.create_tractogram_header(affine, c.dims, (2.0, 1.0, 1.5))
    assert sio.save(Tractogram(lines, {}), path, header) == len(lines)
    con = Connectome(class_labels(c), affine, radius_mm=c.radius_mm, device=DEV)
    node, index = con.add_tractogram(path)
    points, offsets, want_index = corner_voxels(path, affine)
    want_node, want_length, _ = ref.assign(points, offsets, c.labels, c.lin, c.radius_mm,
                                           c.reach, c.n_nodes)
    assert np.array_equal(index, want_index) and len(index) == len(lines) - 3
    assert np.array_equal(node.cpu().numpy(), want_node) and (want_node > 0).sum() > 40
    count, q = ref.accumulate(want_node, want_length, c.n_nodes)
    assert np.array_equal(con.count.cpu().numpy(), count)
    # the definition's own float64 sum may round a row to the neighbouring unit
    assert (np.abs(con.length_q.cpu().numpy() - q) <= count).all()
    assert con.skipped == 3
    # the in-memory tractogram of a tracker, in the voxel space of its env
    class Env:
        affine_vox2rasmm = affine
    vox_lines = [np.asarray(points[offsets[i]:offsets[i + 1]] - F32(0.5)) for i in range(len(index))]
    other = Connectome(class_labels(c), affine, radius_mm=c.radius_mm, device=DEV)
    other_node, _ = other.add_tractogram(Tractogram(vox_lines, {}), Env())
    again = corner_voxels(Tractogram(vox_lines, {}), affine, affine)
    want_node = ref.assign(again[0], again[1], c.labels, c.lin, c.radius_mm, c.reach,
                           c.n_nodes)[0]
    assert np.array_equal(other_node.cpu().numpy(), want_node)
    count = ref.accumulate(want_node, None, c.n_nodes)[0]
    assert np.array_equal(other.count.cpu().numpy(), count)
    files = other.save(str(tmp_path / 'sub' / 'con'))
    assert [os.path.basename(f) for f in files] == ['con_count.npy', 'con_mean_length.npy',
                                                    'con_count.csv', 'con.json']
    m = other.matrices()
    assert np.array_equal(np.load(files[0]), m['count'])
    assert np.array_equal(np.load(files[1]), m['mean_length_mm'])
    assert np.array_equal(np.loadtxt(files[2], delimiter=',', dtype=np.int64, ndmin=2), m['count'])
    totals = json.load(open(files[3]))
    assert totals['n_nodes'] == c.n_nodes and totals['radius_mm'] == c.radius_mm
    assert totals['scored'] == count.sum() and totals['skipped'] == 0


# ---- the tracker: the synthetic subject of utils/synthetic.py, tracked along its fODF
D, C_SH, ORDER = 16, 28, 6
N_SEEDS = 256


def subject():
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_volumes
    sh, mask, _ = synthetic_volumes(D, C_SH, peaks=False)
    return sh, mask, synthetic_seeds(mask, N_SEEDS, seed=4) + 0.0


def painted_labels(mask):
    """Eight nodes, the octants of the ball, on the outer voxels of the mask
    (2.5 voxels and more from its centre line planes are left to the search)."""
    g = np.indices(mask.shape).astype(np.float64) - (D - 1) / 2.0
    r = np.sqrt((g ** 2).sum(0))
    octant = 1 + (g[0] > 0) + 2 * (g[1] > 0) + 4 * (g[2] > 0)
    return np.where((mask > 0) & (r > 4.0), octant, 0).astype(np.int32)


def tissue_maps(mask):
    """include: the outer shell of the ball; exclude: a blob beside its centre."""
    g = np.indices(mask.shape).astype(np.float64) - (D - 1) / 2.0
    r = np.sqrt((g ** 2).sum(0))
    inc = ((mask > 0) & (r > 5.0)).astype(F32)
    exc = np.zeros(mask.shape, F32)
    exc[9:11, 7:9, 7:9] = 1.0
    return inc, exc


def make_env(act=False):
    import torch
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    sh, mask, seeds = subject()
    aff = np.eye(4, dtype=np.float32)
    dto = dict(n_dirs=2, theta=50.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=40.0, compute_reward=False, alignment_weighting=0.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=torch.device(DEV),
               target_sh_order=ORDER)
    if act:
        inc, exc = tissue_maps(mask)
        dto.update(act_include=inc, act_exclude=exc, act_mode='act')
    env = TrackingEnvironment((Vol(sh, aff), Vol(mask, aff), Vol(mask, aff), None, None),
                              'testing', dto)
    env.seeds = seeds.copy()
    return env, mask


def tracked(n_actor=N_SEEDS, only=False, record=None, monkeypatch=None, **options):
    """A det-tracked run with a connectome attached: (connectome, streamlines
    yielded).  ``record`` collects every ``select_tracts`` result."""
    from tracktolearn_amd import parallel
    from tracktolearn_amd.connectome import Connectome
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env, mask = make_env(act=options.get('act_filter') is not None)
    con = Connectome(painted_labels(mask), np.eye(4), radius_mm=2.0, device=DEV)
    if record is not None:
        inner = parallel.select_tracts

        def recording(*args, **kwargs):
            out = inner(*args, **kwargs)
            record.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
            return out
        monkeypatch.setattr(parallel, 'select_tracts', recording)
    np.random.seed(11)
    tracker = Tracker(OdfTracking(env, 'det', seed=5), n_actor, min_length=2.0, max_length=60.0,
                      connectome=con, **options)
    if only:
        assert tracker.track_connectome(env) is con
        return con, None
    return con, [np.asarray(item.streamline) for item in tracker.track(env, TrkFile)]


def matrices_of(con):
    return con.count.cpu().numpy(), con.length_q.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('options', [
    {}, {'compress': 0.1}, {'bidirectional': True},
    {'bidirectional': True, 'act_filter': 'exclude', 'compress': 0.1}],
    ids=['plain', 'compress', 'bidirectional', 'act_filter'])
def test_streamed_connectome_is_the_reference_on_the_output_stage(options, monkeypatch):
    record = []
    con, lines = tracked(record=record, monkeypatch=monkeypatch, **options)
    assert len(record) == 1 and len(lines) == len(record[0][1]) > N_SEEDS // 4
    if options.get('act_filter'):
        assert len(lines) < N_SEEDS                      # the filter dropped some
    points = record[0][0] + F32(0.5)
    offsets = np.concatenate([[0], np.cumsum(record[0][1])]).astype(np.int64)
    # what was written is what was counted (.trk at 1 mm: the same + 0.5)
    assert np.array_equal(np.concatenate(lines).astype(F32), points)
    labels = con.labels.cpu().numpy().reshape(con.dims)
    node, length, _ = ref.assign(points, offsets, labels, np.eye(3), 2.0, [2, 2, 2], 8)
    count, q = ref.accumulate_fast(node, length, 8)
    got_count, got_q = matrices_of(con)
    assert np.array_equal(got_count, count) and count.sum() == len(lines)
    assert (np.abs(got_q - q) <= count).all() and con.skipped == 0
    assert count[1:, 1:].sum() > len(lines) // 4 and np.count_nonzero(count) > 4


@pytest.mark.gpu
def test_connectome_does_not_depend_on_n_actor_and_needs_no_items():
    whole, lines = tracked(bidirectional=True, compress=0.1)
    small, small_lines = tracked(n_actor=64, bidirectional=True, compress=0.1)
    assert len(lines) == len(small_lines)
    for a, b in zip(matrices_of(whole), matrices_of(small)):
        assert np.array_equal(a, b)
    only, _ = tracked(n_actor=64, only=True, bidirectional=True, compress=0.1)
    for a, b in zip(matrices_of(whole), matrices_of(only)):
        assert np.array_equal(a, b)
    assert whole.count.sum().item() == len(lines)


@pytest.mark.gpu
def test_tracker_refuses_another_grid():
    from tracktolearn_amd.connectome import Connectome
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env, mask = make_env()
    con = Connectome(np.ones((D, D, D + 1), np.int32), np.eye(4), device=DEV)
    tracker = Tracker(OdfTracking(env, 'det', seed=5), N_SEEDS, min_length=2.0, connectome=con)
    with pytest.raises(ValueError, match='grid'):
        list(tracker.track(env, TrkFile))


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from tracktolearn_amd.io import nifti
    root = tmp_path_factory.mktemp('connectome')
    sh, mask, _ = subject()
    seed_mask = np.zeros(mask.shape, np.uint8)
    seed_mask[5:11, 5:11, 5:11] = 1
    for name, vol in (('fodf', sh), ('mask', mask), ('seed', seed_mask),
                      ('labels', painted_labels(mask)),
                      ('other_grid', np.ones((D, D, D + 1), np.int32))):
        nifti.save(str(root / f'{name}.nii.gz'), vol, np.eye(4))
    return root


def _argv(files, out, *more):
    return [str(files / 'fodf.nii.gz'), str(files / 'seed.nii.gz'), str(files / 'mask.nii.gz'),
            str(files / out), '--odf_policy', 'det', '--bidirectional', '--min_length', '2',
            '--max_length', '60', '--n_actor', '100', '-f'] + list(more)


@pytest.mark.gpu
def test_track_command_writes_the_connectome_and_no_tractogram(files, capsys):
    from tracktolearn_amd.runners import ttl_track
    prefix = str(files / 'only')
    ttl_track.main(_argv(files, 'never.trk', '--connectome', str(files / 'labels.nii.gz'),
                         '--connectome_out', prefix, '--connectome_only'))
    out = capsys.readouterr().out
    assert 'Saved the connectome' in out and 'streamlines to' not in out
    assert not os.path.exists(str(files / 'never.trk'))
    for suffix in ('_count.npy', '_mean_length.npy', '_count.csv', '.json'):
        assert os.path.isfile(prefix + suffix), suffix
    totals = json.load(open(prefix + '.json'))
    count = np.load(prefix + '_count.npy')
    assert count.shape == (8, 8) and np.array_equal(count, count.T)
    assert totals['n_nodes'] == 8 and totals['radius_mm'] == 2.0 and totals['skipped'] == 0
    assert np.triu(count).sum() == totals['connected'] > 20
    # with the tractogram: the same matrices, and as many streamlines as were counted
    ttl_track.main(_argv(files, 'with.trk', '--connectome', str(files / 'labels.nii.gz'),
                         '--connectome_out', str(files / 'with')))
    n_saved = int(re.search(r'Saved (\d+) streamlines to', capsys.readouterr().out).group(1))
    assert np.array_equal(np.load(str(files / 'with_count.npy')), count)
    assert json.load(open(str(files / 'with.json')))['streamlines'] == n_saved == \
        totals['streamlines']
    with pytest.raises(ValueError, match='--connectome'):
        ttl_track.main(_argv(files, 'never.trk', '--connectome', str(files / 'other_grid.nii.gz'),
                             '--connectome_out', prefix))


@pytest.mark.gpu
@pytest.mark.parametrize('ext', ['.trk', '.tck'])
def test_connectome_command_counts_every_streamline_of_the_file(files, capsys, ext):
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.runners import ttl_connectome, ttl_track
    tractogram = str(files / ('plain' + ext))
    ttl_track.main(_argv(files, 'plain' + ext))
    n_saved = int(re.search(r'Saved (\d+) streamlines to', capsys.readouterr().out).group(1))
    prefix = str(files / ('cmd' + ext[1:]))
    more = ['--reference', str(files / 'mask.nii.gz')] if ext == '.tck' else []
    ttl_connectome.main([tractogram, str(files / 'labels.nii.gz'), prefix,
                         '--save_assignments'] + more)
    totals = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    count = np.load(prefix + '_count.npy')
    m = json.load(open(prefix + '.json'))
    assert m == totals and n_saved > 50
    # count.sum() + skipped is every streamline of the file: the count over the whole
    # accumulated matrix, its unassigned row included (the (N, N) matrix is symmetric)
    scored = np.triu(count).sum() + totals['unassigned_one_end'] + totals['unassigned_both']
    assert scored == totals['scored'] and scored + totals['skipped'] == n_saved
    nodes = np.load(prefix + '_nodes.npy')
    assert nodes.shape == (n_saved, 3) and np.array_equal(nodes[:, 0], np.arange(n_saved))
    both = nodes[(nodes[:, 1] > 0) & (nodes[:, 2] > 0)]
    assert len(both) == np.triu(count).sum()
    # the streamed connectome of the same run is the one of its .tck, whose points are the
    # tracker's (identity affine); the .trk as written lies half a voxel further
    if ext == '.tck':
        ttl_track.main(_argv(files, 'again.tck', '--connectome', str(files / 'labels.nii.gz'),
                             '--connectome_out', str(files / 'again')))
        capsys.readouterr()
        assert np.array_equal(np.load(str(files / 'again_count.npy')), count)
    with pytest.raises(SystemExit):
        ttl_connectome.main([tractogram, str(files / 'labels.nii.gz'), prefix] + more)   # no -f
    capsys.readouterr()


@pytest.mark.gpu
def test_connectome_from_a_label_file_takes_the_files_own_affine(files):
    """``Connectome('labels.nii.gz', None)``: the class reads the image itself."""
    from tracktolearn_amd.connectome import Connectome
    _, mask, _ = subject()
    labels = painted_labels(mask)
    path = files / 'labels.nii.gz'
    from_file = Connectome(str(path), None, radius_mm=2.0, device=DEV)
    from_array = Connectome(labels, np.eye(4), radius_mm=2.0, device=DEV)
    assert from_file.n_nodes == from_array.n_nodes == 8 and from_file.dims == labels.shape
    assert np.array_equal(from_file.affine, np.eye(4))
    assert np.array_equal(from_file.labels.cpu().numpy(), labels.reshape(-1))
    # a path-like and an affine given beside the file; an unsigned array
    moved = np.eye(4)
    moved[:3, 3] = (1.0, 2.0, 3.0)
    assert np.array_equal(Connectome(path, moved, device=DEV).affine, moved)
    unsigned = Connectome(labels.astype(np.uint8), np.eye(4), device=DEV)
    assert np.array_equal(unsigned.labels.cpu().numpy(), labels.reshape(-1))
    with pytest.raises(ValueError, match='affine'):
        Connectome(labels, None, device=DEV)
    rng = np.random.RandomState(1)
    points = rng.uniform(0.0, D, (60, 3)).astype(F32)
    offsets = np.arange(0, 61, 3, dtype=np.int64)
    nodes = [c.add(_dev(points), _dev(offsets)).cpu().numpy() for c in (from_file, from_array)]
    assert np.array_equal(nodes[0], nodes[1]) and (nodes[0] > 0).any()
    same_matrices((from_file.count, from_file.length_q),
                  (from_array.count.cpu().numpy(), from_array.length_q.cpu().numpy()))
