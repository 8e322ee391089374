"""Track density maps (include/ttl_hip.h, ttl_tract_density):
the definition three ways on the CPU, witnesses for every named mutant and
the tier predictions; on the GPU the kernel against the ordered reference
(count, ends, status, length_q and dec_q exactly, as integers), the tiers, the
independence of order and split, the coverage cross-check, and everything
above the ABI (DensityMap, the Tracker, the commands)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import coverage_cases as cov
import density_cases as cases
import ref_density as ref
import ref_oracle_validator as walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
F32 = np.float32
MAP_KEYS = ('count', 'ends', 'length_q', 'dec_q')


# ------------------------------------------------------------------ CPU part
def test_definition_agrees_with_the_pinned_walk():
    """On 160 _walk rows (lengths 2 .. 300): statement (a)'s piece voxels are
    [floor(a) if inside] + walk_segment(a, b), no piece is negative, (a) and (b)
    are the same pieces bit for bit, and the fractions of a segment that stays
    inside sum to 1 within 1.2e-16."""
    dims = cov.ROW_VOLUME
    rows = cases.walk_rows()
    assert len(rows) == 160 and min(map(len, rows)) >= 2 and max(map(len, rows)) <= 300
    worst, reenter = 0.0, 0
    for row in rows:
        seen = ref.row_voxels(row, dims)
        reenter += _reenters_non_consecutively(seen)
        for j in range(len(row) - 1):
            a, b = row[j], row[j + 1]
            planes = ref.segment_pieces_planes(a, b, dims)
            assert planes == ref.segment_pieces(a, b, dims)
            fa, fb = ref._floor_voxel(ref._f64(a)), ref._floor_voxel(ref._f64(b))
            want = ([fa] if ref._inside(fa, dims) else []) + walk.walk_segment(a, b, dims)
            assert [p[0] for p in planes] == want
            assert all(p[2] >= p[1] >= 0.0 and p[2] <= 1.0 for p in planes)
            if ref._inside(fa, dims) and ref._inside(fb, dims):
                worst = max(worst, abs(sum(p[2] - p[1] for p in planes) - 1.0))
    assert worst <= 1.2e-16
    assert reenter == 158           # dedupe_consecutive_only has plenty to get wrong


def _reenters_non_consecutively(seen):
    last = {}
    for k, v in enumerate(seen):
        if v in last and last[v] != k - 1:
            return True
        last[v] = k
    return False


def test_a_diagonal_through_a_lattice_corner():
    """(1.5, 1.5, 1.5) -> (2.5, 2.5, 1.5) crosses x = 2 and y = 2 at t = 0.5: the
    lower axis first, so voxel (2, 1, 1) is visited with a piece of length 0 and
    still counts 1."""
    dims, lin = (4, 4, 4), np.diag([2.0, 2.0, 2.0])
    pieces = ref.segment_pieces((1.5, 1.5, 1.5), (2.5, 2.5, 1.5), dims)
    assert pieces == [((1, 1, 1), 0.0, 0.5), ((2, 1, 1), 0.5, 0.5), ((2, 2, 1), 0.5, 1.0)]
    assert pieces == ref.segment_pieces_planes((1.5, 1.5, 1.5), (2.5, 2.5, 1.5), dims)
    assert [(v, float(w)) for v, w in
            ref.segment_pieces_exact((1.5, 1.5, 1.5), (2.5, 2.5, 1.5), dims)] == \
        [((1, 1, 1), 0.5), ((2, 1, 1), 0.0), ((2, 2, 1), 0.5)]
    points = np.array([(1.5, 1.5, 1.5), (2.5, 2.5, 1.5)], F32)
    m = ref.density_final(points, np.array([0, 2]), dims, lin)
    assert m['count'].sum() == 3 and m['count'][2, 1, 1] == 1 and m['length_q'][2, 1, 1] == 0
    half = int(np.rint(0.5 * np.sqrt(8.0) * 2.0 ** 20))
    assert m['length_q'][1, 1, 1] == m['length_q'][2, 2, 1] == half
    assert m['dec_q'][1, 1, 1].tolist() == [2 ** 20, 2 ** 20, 0]
    assert m['ends'][1, 1, 1] == m['ends'][2, 2, 1] == 1 and m['ends'].sum() == 2
    assert m['status'].tolist() == [0] and m['n_voxels'].tolist() == [3]


def test_hand_rows():
    c = cases.sets()['hand']
    m = cases.reference('hand')
    assert m['status'].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert m['n_voxels'].tolist()[:8] == [0, 1, 1, 7, 8, 4, 7, 0]
    assert m['ends'][3, 4, 5] == 2 and m['ends'][3, 3, 3] == 3      # two ends in one voxel
    # the rows that stay inside leave their whole length: |lin d| 2^20, to a unit per piece
    for s in (1, 3):
        row = c.points[c.offsets[s]:c.offsets[s + 1]]
        one = ref.density_final(row, np.array([0, len(row)]), c.dims, c.lin)
        want = ref.segment_vector(row[0], row[1], [float(v) for v in c.lin.reshape(9)])[0]
        assert abs(one['length_q'].sum() - want * 2.0 ** 20) <= one['n_voxels'][0]
    # in through one face and out through another: 8 voxels of 2 mm each
    row = c.points[c.offsets[4]:c.offsets[5]]
    one = ref.density_final(row, np.array([0, 2]), c.dims, c.lin)
    assert one['length_q'][:, 4, 4].tolist() == [2 * 2 ** 20] * 8 and one['ends'].sum() == 0


def test_sets_hold_what_they_are_for():
    sets = cases.sets()
    assert set(sets) == set(cases.SET_NAMES) and len(sets) >= 30
    for name in cases.SET_NAMES:
        m = cases.reference(name)
        if name.startswith('rows_') and 'lengths' not in name:
            assert (m['status'] == -1).all() and m['count'].sum() == 0     # NaN / Inf rows
        elif name not in ('class_huge', 'length_threshold'):
            assert (m['status'] == 0).sum() >= 2 and m['count'].sum() > 20, name
    lengths = np.diff(sets['lengths_oblique'].offsets)
    assert sorted(set(lengths.tolist())) == list(cases.ROW_LENGTHS)
    assert cases.reference('needle')['n_voxels'].tolist() == [4096, 4096]
    assert cases.reference('class_huge')['status'].tolist() == [-1, -1, -1]
    # the length rule on its threshold, in the kernel's order of the sum: rows within 4 ulps
    # of 2^40 mm on both sides, some of which the sum in streamline order puts on the other
    rows = cases.threshold_rows()
    status = cases.reference('length_threshold')['status']
    assert status.tolist() == [0 if kernel < 0 else -1 for _, kernel, _ in rows]
    assert (status == 0).sum() >= 6 and (status == -1).sum() >= 6
    assert all(abs(kernel) <= 2.0 ** -10 for _, kernel, _ in rows)
    assert sum(kernel < 0 <= line for _, kernel, line in rows) >= 1
    assert sum(line < 0 <= kernel for _, kernel, line in rows) >= 1
    back = cases.reference('forth_and_back')
    assert (back['count'] <= 6).all() and back['count'].max() >= 2
    assert (back['length_q'][back['count'] > 0] > 0).all()


@pytest.mark.parametrize('name', ['hand', 'forth_and_back', 'lengths_oblique', 'class_grazing',
                                  'needle'])
def test_ordered_statement_is_within_the_derived_bound_of_exact_arithmetic(name, capsys):
    """(b) against (c): per voxel |length_q - exact| <= sum over its pieces of
    1 + 17 u B_j 2^20, |dec_q - exact| <= sum of 1 + 13 u B_jk 2^20 (header), each
    piece's tolerance once."""
    c = cases.sets()[name]
    q, q_bound, dq, dq_bound = ref.bounds(c.points, c.offsets, c.dims, c.lin)
    m = cases.reference(name)
    with capsys.disabled():
        print(f'\n{name}: largest |length_q - exact| / bound '
              f'{(np.abs(m["length_q"] - q) / np.maximum(q_bound, 1e-300)).max():.3f}, dec '
              f'{(np.abs(m["dec_q"] - dq) / np.maximum(dq_bound, 1e-300)).max():.3f}')
    assert (np.abs(m['length_q'] - q) <= q_bound).all()
    assert (np.abs(m['dec_q'] - dq) <= dq_bound).all()
    assert q.sum() > 0 and (q_bound[m['count'] > 0] >= 1.0).all()


MUTANT_SETS = {
    'nonfinite_row_partly_added': [n for n in cases.SET_NAMES if n.startswith('rows_')
                                   and 'lengths' not in n],
    'count_partial_on_overflow': None,          # the tier case, below
}


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_every_mutant_has_witnesses(mutant):
    """At least 5 cases of the launched sets whose maps a kernel with that
    mistake would change."""
    if mutant == 'count_partial_on_overflow':
        # the rows of the tier case, one by one, at the first of the three cases: each
        # status-2 row whose own count map the mistake changes is a witness
        c = cases.tier_case()
        spill = cases.TIER_SPILLS[0]
        witnesses = 0
        for s in np.flatnonzero(cases.tier_reference(spill)['status'] == 2):
            row = c.points[c.offsets[s]:c.offsets[s + 1]]
            one = [ref.density(row, np.array([0, len(row)]), c.dims, c.lin,
                               cases.TIER_WAVE_SLOTS, spill, mutant=which)
                   for which in (None, mutant)]
            assert one[0]['status'].tolist() == one[1]['status'].tolist() == [2]
            assert one[0]['count'].sum() == 0
            witnesses += not np.array_equal(one[0]['count'], one[1]['count'])
        assert witnesses >= 5
        return
    names = MUTANT_SETS.get(mutant) or [n for n in cases.SET_NAMES if n != 'needle']
    witnesses = 0
    for name in names:
        c = cases.sets()[name]
        want = cases.reference(name)
        # row by row where the set is small, else the set as one case
        got = cases.reference(name, mutant)
        if all(np.array_equal(got[k], want[k]) for k in MAP_KEYS):
            continue
        if len(c.offsets) - 1 > 30 or name.startswith('class_'):
            witnesses += 1
            continue
        for s in range(len(c.offsets) - 1):
            row = c.points[c.offsets[s]:c.offsets[s + 1]]
            off = np.array([0, len(row)])
            a = ref.density_final(row, off, c.dims, c.lin)
            b = ref.density_final(row, off, c.dims, c.lin, mutant)
            witnesses += not all(np.array_equal(a[k], b[k]) for k in MAP_KEYS)
    assert witnesses >= 5, (mutant, witnesses)


def test_tier_predictions():
    """At wave_slots = 64: at least 5 rows in each of status 0, 1 and 2, the
    thresholds exact (32 | 33 and 512 | 513 voxels), and the status a function of
    the number of distinct voxels alone."""
    assert [ref.tier(v, 64, 1024) for v in (1, 32, 33, 512, 513)] == [0, 0, 1, 1, 2]
    assert [ref.tier(v, 64, 64) for v in (32, 33)] == [0, 2]
    assert [ref.tier(v, 64, None) for v in (32, 33)] == [0, 2]
    first = cases.tier_reference(1024)
    for status in (0, 1, 2):
        assert (first['status'] == status).sum() >= 5
    for v in (32, 33, 512, 513):
        assert (first['n_voxels'] == v).sum() == 1
    for spill in cases.TIER_SPILLS:
        m = cases.tier_reference(spill)
        assert m['status'].tolist() == [ref.tier(int(v), 64, spill) for v in m['n_voxels']]
        assert (m['status'] == 2).sum() >= 5
    final = ref.density_final(*_args(cases.tier_case()))
    assert final['count'].sum() == final['n_voxels'].sum() > first['count'].sum()
    grid = cases.grid_reference()
    assert (grid['status'][:6] == 1).all() and (grid['status'][6:] == 0).all()


def _args(c):
    return c.points, c.offsets, c.dims, c.lin


def test_zoom_grid_and_argument_checks():
    from tracktolearn_amd import density
    affine = np.array([[2.0, 0.1, 0, -10], [0, 1.0, 0, 3], [0.2, 0, 1.5, 7], [0, 0, 0, 1]])
    dims, zoomed = density.zoom_grid((7, 5, 4), affine, 2)
    assert dims == (14, 10, 8)
    assert np.array_equal(zoomed[:3, :3], affine[:3, :3] / 2) and \
        np.array_equal(zoomed[:, 3], affine[:, 3])
    # the corner of voxel 0 stays, a reference voxel's far corner is zoom map voxels on
    assert np.allclose(zoomed @ [2.0, 2.0, 2.0, 1.0], affine @ [1.0, 1.0, 1.0, 1.0])
    assert density.zoom_grid((7, 5, 4), affine, 1)[0] == (7, 5, 4)
    for bad in (0, 9, 1.5, -1, True):
        with pytest.raises(ValueError, match='zoom'):
            density.zoom_grid((7, 5, 4), affine, bad)
    for bad in ((0, 5, 4), (7, 5), (2048, 2048, 512)):
        with pytest.raises(ValueError, match='dims'):
            density.check_dims(bad)
    assert density.check_dims((2048, 1024, 1023)) == (2048, 1024, 1023)
    assert density.check_slots(0, 0) == (0, 0) and density.check_slots(64, 1 << 26) == (64, 1 << 26)
    for wave, spill in ((32, 0), (96, 0), (16384, 0), (64, 32), (64, 100), (64, 1 << 27)):
        with pytest.raises(ValueError, match='slots'):
            density.check_slots(wave, spill)
    assert (density.MAX_WAVE_SLOTS, density.DEFAULT_WAVE_SLOTS, density.LENGTH_SCALE) == \
        (8192, 2048, 2.0 ** 20)
    with pytest.raises(ValueError, match='affine'):
        density.DensityMap((4, 4, 4), None)
    with pytest.raises(ValueError, match='zoom'):
        density.DensityMap((4, 4, 4), np.eye(4), zoom=9)


def _density_args():
    """Arguments that pass every check of ttl_tract_density: the pointers are never
    followed, TTL_ERR_INVALID and n == 0 return before any HIP call."""
    from tracktolearn_amd import _lib
    p = 4096
    desc = _lib.DensityDesc()
    desc.dims = (C.c_int32 * 3)(7, 5, 4)
    desc.lin = (C.c_double * 9)(*np.eye(3).reshape(-1))
    desc.count, desc.length_q, desc.dec_q, desc.ends = p, p, p, p
    desc.wave_slots, desc.spill_slots, desc.workspace, desc.workspace_bytes = 0, 0, None, 0
    return desc, dict(points=C.c_void_p(p), offsets=C.c_void_p(p), n=0, status=C.c_void_p(p),
                      stream=None)


def _call_density(desc, args):
    from tracktolearn_amd import _lib
    return _lib.load().ttl_tract_density(None if desc is None else C.byref(desc), *args.values())


DENSITY_INVALID = [('points', None), ('offsets', None), ('status', None), ('n', -1),
                   ('desc', None), ('dims', (0, 5, 4)), ('dims', (7, 5, -1)),
                   ('dims', (2048, 2048, 512)), ('dims', (65536, 65536, 1)), ('maps', None),
                   ('wave_slots', 32), ('wave_slots', 96), ('wave_slots', 16384),
                   ('spill_slots', 32), ('spill_slots', 100), ('spill_slots', 1 << 27),
                   ('workspace', 4096)]


@pytest.mark.parametrize('key,value', DENSITY_INVALID)
def test_density_refuses_before_any_hip_call(key, value):
    from tracktolearn_amd import _lib
    lib = _lib.load()
    desc, args = _density_args()
    assert _call_density(desc, args) == 0                            # n == 0: a no-op
    for only in ('count', 'length_q', 'dec_q', 'ends'):              # any one map is enough
        one, _ = _density_args()
        one.count, one.length_q, one.dec_q, one.ends = None, None, None, None
        setattr(one, only, 4096)
        assert _call_density(one, args) == 0
    if key == 'desc':
        desc = None
    elif key == 'dims':
        desc.dims = (C.c_int32 * 3)(*value)
    elif key == 'maps':
        desc.count, desc.length_q, desc.dec_q, desc.ends = None, None, None, None
    elif key == 'workspace':                     # a workspace without spill_slots
        desc.workspace, desc.workspace_bytes = value, 1 << 20
    elif key in ('wave_slots', 'spill_slots'):
        setattr(desc, key, value)
    else:
        args[key] = value
    assert _call_density(desc, args) == _lib.ERR_INVALID
    assert b'ttl_tract_density' in lib.ttl_last_error()


def test_workspace_bytes_and_a_workspace_too_small():
    from tracktolearn_amd import _lib
    lib = _lib.load()
    small, large = (lib.ttl_tract_density_workspace_bytes(1024, n) for n in (1, 100000))
    assert 0 < small < large and large - small >= 4 * 99999 - 64      # the list, to a line
    assert lib.ttl_tract_density_workspace_bytes(2048, 1) > small
    for spill, n in ((0, 1), (100, 1), (32, 1), (1 << 27, 1), (1024, 0), (1024, -1)):
        assert lib.ttl_tract_density_workspace_bytes(spill, n) == 0
    desc, args = _density_args()
    desc.spill_slots, desc.workspace, desc.workspace_bytes = 1024, 4096, small - 1
    assert _call_density(desc, dict(args, n=1)) == _lib.ERR_INVALID
    assert b'workspace' in lib.ttl_last_error()


def test_header_announces_the_feature_and_keeps_the_abi():
    from tracktolearn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'^#define TTL_HAS_TRACT_DENSITY 1$', header, re.M)
    assert re.search(r'^#define TTL_ABI_VERSION 13$', header, re.M)
    assert re.search(r'^#define TTL_DENSITY_MAX_WAVE_SLOTS 8192$', header, re.M)
    assert (_lib.HAS_TRACT_DENSITY, _lib.ABI_VERSION) == (1, 13)
    assert (_lib.DENSITY_MAX_WAVE_SLOTS, _lib.DENSITY_WAVE_SLOTS) == (8192, 2048)
    assert ref.LENGTH_SCALE == _lib.CONNECTOME_LENGTH_SCALE == 2.0 ** 20
    lib = _lib.load()
    for name in ('ttl_tract_density', 'ttl_tract_density_workspace_bytes'):
        assert name in _lib.SYMBOLS and getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert re.search(r'^TTL_API \w+ ' + name + r'\(', header, re.M)
    # the ctypes mirror of ttl_density_desc: 3 int32, pad, 9 doubles, 4 pointers, 2 int32,
    # pointer, size_t
    assert C.sizeof(_lib.DensityDesc) == 16 + 72 + 32 + 8 + 16
    from tracktolearn_amd.csrc import build
    assert any(s.endswith('ttl_tract_density.hip') for s in build.SOURCES)


def _track_parse(argv, tmp_path):
    from tracktolearn_amd.runners import ttl_track
    files = []
    for name in ('fodf', 'seed', 'mask'):
        f = tmp_path / f'{name}.nii.gz'
        f.write_bytes(b'')
        files.append(str(f))
    argv = [a.replace('PREFIX', str(tmp_path / 'tdi')) for a in argv]
    return ttl_track.parse_args(files + [str(tmp_path / 'out.trk'), '--odf_policy', 'det'] + argv)


def test_track_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_track
    with pytest.raises(SystemExit) as e:
        ttl_track.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('--density_map PREFIX', '--density_zoom K', '--density_dec', '--density_only'):
        assert opt in text
    args = _track_parse([], tmp_path)
    assert args.density_map is None and not args.density_only and not args.density_dec
    args = _track_parse(['--density_map', 'PREFIX'], tmp_path)
    assert args.density_map.endswith('tdi') and args.density_zoom is None
    args = _track_parse(['--density_map', 'PREFIX', '--density_zoom', '4', '--density_dec',
                         '--density_only', '--compress', '0.1'], tmp_path)
    assert args.density_zoom == 4 and args.density_dec and args.density_only
    for argv, word in ((['--density_zoom', '2'], 'only with --density_map'),
                       (['--density_dec'], 'only with --density_map'),
                       (['--density_only'], 'only with --density_map'),
                       (['--density_map', 'PREFIX', '--density_zoom', '9'], '1 .. 8'),
                       (['--density_map', 'PREFIX', '--density_zoom', '0'], '1 .. 8'),
                       (['--density_map', 'PREFIX', '--direct_output'], 'never makes')):
        with pytest.raises(SystemExit) as e:
            _track_parse(argv, tmp_path)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_density_command_options(tmp_path, capsys):
    from tracktolearn_amd.runners import ttl_density
    shim = open(os.path.join(ROOT, 'ttl_density.py')).read()
    assert 'from tracktolearn_amd.runners.ttl_density import main' in shim
    assert len(shim.splitlines()) == 7
    with pytest.raises(SystemExit) as e:
        ttl_density.parse_args(['--help'])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ('in_tractogram', 'reference', 'out_prefix', '--zoom K', '--dec', '-f'):
        assert opt in text
    for name in ('t.trk', 't.tck', 't.txt', 'ref.nii.gz', 'held_count.nii.gz',
                 'dec_dec.nii.gz'):
        (tmp_path / name).write_bytes(b'')
    p = lambda name: str(tmp_path / name)
    args = ttl_density.parse_args([p('t.trk'), p('ref.nii.gz'), p('out')])
    assert args.zoom == 1 and not args.dec and not args.overwrite
    assert ttl_density.parse_args([p('t.trk'), p('ref.nii.gz'), p('dec')])   # not written: no hold
    args = ttl_density.parse_args([p('t.tck'), p('ref.nii.gz'), p('held'), '--zoom', '4', '--dec',
                                   '-f'])
    assert args.zoom == 4 and args.dec and args.overwrite
    for argv, word in (([p('none.trk'), p('ref.nii.gz'), p('out')], 'does not exist'),
                       ([p('t.trk'), p('none.nii.gz'), p('out')], 'does not exist'),
                       ([p('t.txt'), p('ref.nii.gz'), p('out')], '.trk or .tck'),
                       ([p('t.trk'), p('ref.nii.gz'), p('held')], 'use -f'),
                       ([p('t.trk'), p('ref.nii.gz'), p('dec'), '--dec'], 'use -f'),
                       ([p('t.trk'), p('ref.nii.gz'), p('out'), '--zoom', '9'], '1 .. 8'),
                       ([p('t.trk'), p('ref.nii.gz')], 'required')):
        with pytest.raises(SystemExit) as e:
            ttl_density.parse_args(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


class _Map:
    ref_dims = (4, 4, 4)


def test_tracker_refusals(monkeypatch):
    import torch.distributed as dist
    from tracktolearn_amd.tracking.tracker import Tracker
    tdi = _Map()
    assert Tracker(None, 1).density is None
    assert Tracker(None, 1, density=tdi).density is tdi
    assert Tracker(None, 1, density=tdi, device_output=True).density is tdi
    with pytest.raises(ValueError, match='device_output'):
        Tracker(None, 1, density=tdi, device_output=False)
    with pytest.raises(ValueError, match='track_to_file'):
        Tracker(None, 1, density=tdi).track_to_file(None, 'out.trk')
    with pytest.raises(ValueError, match='density'):
        Tracker(None, 1).track_density(None)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_rank', lambda: 1)
    monkeypatch.setattr(dist, 'get_world_size', lambda: 2)
    with pytest.raises(ValueError, match='ranks'):
        Tracker(None, 1, density=tdi)


# ------------------------------------------------------------------ GPU part
def _dev(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def gpu_density(c, wave_slots=0, spill_slots=0, workspace=True, maps=None, rows=None,
                only_count=False):
    """One call of ttl_tract_density on case ``c`` (``rows``: those rows, in that
    order): (maps as device tensors -- added to when given --, status, the
    workspace after the call)."""
    import torch
    from tracktolearn_amd import density
    points, offsets = c.points, c.offsets
    if rows is not None:
        points, offsets = cov.pack([c.points[c.offsets[i]:c.offsets[i + 1]] for i in rows])
    words = int(np.prod(c.dims))
    if maps is None:
        maps = {'count': torch.zeros(words, dtype=torch.int32, device=DEV),
                'ends': torch.zeros(words, dtype=torch.int32, device=DEV),
                'length_q': torch.zeros(words, dtype=torch.int64, device=DEV),
                'dec_q': torch.zeros((words, 3), dtype=torch.int64, device=DEV)}
    ws = None
    if workspace and spill_slots:
        ws = torch.zeros(density.workspace_bytes(spill_slots, len(offsets) - 1), dtype=torch.uint8,
                         device=DEV)
    given = {'count': maps['count']} if only_count else maps
    status = density.tract_density(_dev(points), _dev(offsets), c.dims, c.lin,
                                   wave_slots=wave_slots, spill_slots=spill_slots, workspace=ws,
                                   **given)
    return maps, status.cpu().numpy(), ws


def host(maps, dims):
    return {'count': maps['count'].cpu().numpy().reshape(dims),
            'ends': maps['ends'].cpu().numpy().reshape(dims),
            'length_q': maps['length_q'].cpu().numpy().reshape(dims),
            'dec_q': maps['dec_q'].cpu().numpy().reshape(tuple(dims) + (3,))}


def same_maps(got, want):
    for key in MAP_KEYS:
        diff = np.argwhere(np.asarray(got[key]) != np.asarray(want[key]))
        assert len(diff) == 0, (key, len(diff), diff[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('name', cases.SET_NAMES)
def test_maps_are_the_ordered_reference(name):
    """count, ends and status exactly; length_q and dec_q equal statement (b) as
    integers.  At the default wave set, with a spill set of 8192 slots."""
    c = cases.sets()[name]
    want = cases.reference(name)
    maps, status, ws = gpu_density(c, spill_slots=8192)
    same_maps(host(maps, c.dims), want)
    predicted = [-1 if s < 0 else ref.tier(int(v), 2048, 8192)
                 for s, v in zip(want['status'], want['n_voxels'])]
    assert status.tolist() == predicted and 2 not in predicted
    assert not ws.any().item()


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in cases.SET_NAMES if n.startswith(
    ('class_', 'lengths_', 'forth', 'needle')) and n != 'class_huge'])
def test_count_is_the_coverage_map(name):
    """(count > 0) is ttl_tract_coverage's map on all-finite rows of >= 2 points."""
    from tracktolearn_amd.experiment.oracle_validator import tract_coverage
    c = cases.sets()[name]
    assert np.isfinite(c.points).all() and np.diff(c.offsets).min() >= 2
    maps, status, _ = gpu_density(c, spill_slots=8192)
    assert (status >= 0).all()
    visited = tract_coverage(_dev(c.points), _dev(c.offsets), c.dims)
    assert np.array_equal(visited.cpu().numpy() > 0, maps['count'].cpu().numpy() > 0)
    assert visited.sum().item() > 20


@pytest.mark.gpu
@pytest.mark.parametrize('spill', cases.TIER_SPILLS, ids=['spill1024', 'spill64', 'no_workspace'])
def test_tiers(spill):
    """The first call: predicted status row by row, count holds nothing of a
    status-2 row while length_q holds all of it, the workspace is zero; then the
    re-add through DensityMap.add gives the same final maps in all three cases."""
    from tracktolearn_amd.density import DensityMap
    c = cases.tier_case()
    want = cases.tier_reference(spill)
    final = ref.density_final(*_args(c))
    maps, status, ws = gpu_density(c, cases.TIER_WAVE_SLOTS, spill or 0)
    assert status.tolist() == want['status'].tolist()
    got = host(maps, c.dims)
    same_maps(got, want)
    assert np.array_equal(got['length_q'], final['length_q'])
    assert got['count'].sum() == want['n_voxels'][want['status'] != 2].sum()
    if ws is not None:
        assert not ws.any().item()
    # the caller's second call: the status-2 rows, count alone, a larger spill set
    left = np.flatnonzero(status == 2)
    _, again, ws = gpu_density(c, cases.TIER_WAVE_SLOTS, 8192, maps=maps, rows=left,
                               only_count=True)
    assert (again == 1).all() and not ws.any().item()
    same_maps(host(maps, c.dims), final)
    # ... which is what DensityMap.add does
    tdi = DensityMap(c.dims, np.vstack([np.c_[c.lin, [0, 0, 0]], [0, 0, 0, 1]]), device=DEV,
                     dec=True, wave_slots=cases.TIER_WAVE_SLOTS, spill_slots=spill or 0)
    out = tdi.add(_dev(c.points), _dev(c.offsets)).cpu().numpy()
    assert set(out.tolist()) == {0, 1} and (out == 0).sum() == (want['status'] == 0).sum()
    same_maps({'count': tdi.count.cpu().numpy().reshape(c.dims),
               'ends': tdi.ends.cpu().numpy().reshape(c.dims),
               'length_q': tdi.length_q.cpu().numpy().reshape(c.dims),
               'dec_q': tdi.dec_q.cpu().numpy().reshape(c.dims + (3,))}, final)
    assert tdi._workspace is None or not tdi._workspace.any().item()
    assert tdi.tiers() == {'not_added': 0, 'wave': int((out == 0).sum()),
                           'spill': int((out == 1).sum())} and tdi.skipped == 0


@pytest.mark.gpu
def test_maps_do_not_depend_on_order_or_split():
    """The same rows in one call, in three calls and permuted: identical maps."""
    c = cases.tier_case()
    n = len(c.offsets) - 1
    one, status, _ = gpu_density(c, cases.TIER_WAVE_SLOTS, 4096)
    assert 2 not in status.tolist() and {0, 1} <= set(status.tolist())
    want = host(one, c.dims)
    same_maps(want, ref.density_final(*_args(c)))
    maps = None
    for part in np.array_split(np.arange(n), 3):
        maps, _, _ = gpu_density(c, cases.TIER_WAVE_SLOTS, 4096, maps=maps, rows=part)
    same_maps(host(maps, c.dims), want)
    order = np.random.default_rng(36).permutation(n)
    permuted, p_status, _ = gpu_density(c, cases.TIER_WAVE_SLOTS, 4096, rows=order)
    same_maps(host(permuted, c.dims), want)
    assert p_status.tolist() == status[order].tolist()


@pytest.mark.gpu
def test_more_rows_than_one_pass_of_the_grid():
    """40 000 rows: 7 232 waves take a second row, six of them after a row that
    overflowed their set -- the sweep leaves the table empty either way."""
    c = cases.grid_case()
    want = cases.grid_reference()
    maps, status, ws = gpu_density(c, cases.TIER_WAVE_SLOTS, 1024)
    assert status.tolist() == want['status'].tolist()
    same_maps(host(maps, c.dims), want)
    assert not ws.any().item()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3, 4, 5, 63, 64, 65])
def test_launch_sizes(n):
    c = cases.sets()['lengths_oblique']
    rows = list(range(len(c.offsets) - 1)) * 5
    part = cases.case([c.points[c.offsets[i]:c.offsets[i + 1]] for i in rows[:n]], c.dims, c.lin)
    maps, status, _ = gpu_density(part, 64, 1024)
    same_maps(host(maps, c.dims), ref.density_final(*_args(part)))
    assert (status >= 0).all()


@pytest.mark.gpu
def test_single_maps_and_no_rows():
    """Any one map alone gives that map; n == 0 and empty points launch nothing."""
    import torch
    from tracktolearn_amd import density
    c = cases.sets()['lengths_aniso']
    want = cases.reference('lengths_aniso')
    words = int(np.prod(c.dims))
    for key, dtype, shape in (('count', torch.int32, (words,)), ('ends', torch.int32, (words,)),
                              ('length_q', torch.int64, (words,)),
                              ('dec_q', torch.int64, (words, 3))):
        t = torch.zeros(shape, dtype=dtype, device=DEV)
        status = density.tract_density(_dev(c.points), _dev(c.offsets), c.dims, c.lin, **{key: t})
        assert np.array_equal(t.cpu().numpy().reshape(want[key].shape), want[key]), key
        assert (status.cpu().numpy() == 0).all()
    empty = density.tract_density(_dev(np.zeros((0, 3), F32)), _dev(np.zeros(1, np.int64)),
                                  c.dims, c.lin, count=torch.zeros(words, dtype=torch.int32,
                                                                   device=DEV))
    assert empty.shape == (0,)
    with pytest.raises(ValueError, match='count'):
        density.tract_density(_dev(c.points), _dev(c.offsets), c.dims, c.lin,
                              count=torch.zeros(words, dtype=torch.int64, device=DEV))


# ---- above the ABI
def _affine(lin, origin=(-5.0, 2.0, 7.5)):
    affine = np.eye(4)
    affine[:3, :3] = lin
    affine[:3, 3] = origin
    return affine


@pytest.mark.gpu
@pytest.mark.parametrize('zoom', [1, 2])
def test_density_map_against_the_reference_on_scaled_points(zoom, tmp_path):
    """DensityMap at zoom 1 and 2: the maps of the float32 product points * zoom
    on the grid dims * zoom; save -> nifti.load: dtype, affine, values."""
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.io import nifti
    c = cases.sets()['lengths_oblique']
    affine = _affine(c.lin)
    tdi = DensityMap(c.dims, affine, zoom=zoom, device=DEV, dec=True)
    assert tdi.dims == tuple(d * zoom for d in c.dims)
    assert np.array_equal(tdi.affine[:3, :3], c.lin / zoom) and \
        np.array_equal(tdi.affine[:, 3], affine[:, 3])
    status = tdi.add(_dev(c.points), _dev(c.offsets)).cpu().numpy()
    scaled = c.points * F32(zoom)
    want = ref.density_final(scaled, c.offsets, tdi.dims, c.lin / zoom)
    m = tdi.maps()
    assert m['count'].dtype == np.int32 and m['ends'].dtype == np.int32
    assert np.array_equal(m['count'], want['count']) and np.array_equal(m['ends'], want['ends'])
    assert np.array_equal(m['length_mm'], want['length_q'] / 2.0 ** 20)
    assert np.array_equal(m['dec_mm'], want['dec_q'] / 2.0 ** 20)
    assert m['dec_mm'].shape == tdi.dims + (3,) and (status >= 0).all()
    # the mm of streamline do not depend on the grid: to a unit per piece
    assert abs(want['length_q'].sum() - cases.reference('lengths_oblique')['length_q'].sum()) \
        <= want['count'].sum() + cases.reference('lengths_oblique')['count'].sum()
    files = tdi.save(str(tmp_path / 'sub' / 'tdi'))
    assert [os.path.basename(f) for f in files] == [
        'tdi_count.nii.gz', 'tdi_length.nii.gz', 'tdi_ends.nii.gz', 'tdi_dec.nii.gz', 'tdi.json']
    for f, key, dtype in zip(files, ('count', 'length_mm', 'ends', 'dec_mm'),
                             (np.int32, F32, F32, F32)):
        img = nifti.load(f)
        assert img.dataobj.dtype == dtype and np.allclose(img.affine, tdi.affine, atol=1e-6)
        assert np.array_equal(np.asarray(img.dataobj), m[key].astype(dtype))
    totals = json.load(open(files[4]))
    n = len(c.offsets) - 1
    assert totals == {'added': n, 'skipped': 0, 'zoom': zoom, 'dims': list(tdi.dims),
                      'wave_slots': 2048, 'spill_slots': 8192,
                      'tiers': {'not_added': 0, 'wave': n, 'spill': 0}}
    # without dec, ends or length: those maps are not kept, not written
    plain = DensityMap(c.dims, affine, zoom=zoom, device=DEV, ends=False, length=False)
    plain.add(_dev(c.points), _dev(c.offsets))
    assert set(plain.maps()) == {'count'} and np.array_equal(plain.maps()['count'], want['count'])


def _mm_lines(dims, affine, n=120, seed=2):
    rng = np.random.RandomState(seed)
    lines = []
    for i in range(n):
        L = 1 if i % 40 == 7 else int(rng.randint(2, 30))
        vox = np.stack([rng.uniform(-2.0, d + 2.0, L) for d in dims], axis=1)
        lines.append((vox @ affine[:3, :3].T + affine[:3, 3]).astype(F32))
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize('ext', ['.trk', '.tck'])
def test_add_tractogram_goes_through_the_one_intake(tmp_path, ext):
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.experiment.oracle_validator import corner_voxels
    from tracktolearn_amd.io import nifti, streamlines as sio
    from tracktolearn_amd.runners import ttl_density
    from tracktolearn_amd.tractogram import Tractogram
    dims, lin = (7, 5, 4), cases.ANISO
    affine = _affine(lin)
    lines = _mm_lines(dims, affine)
    bad = int(ext == '.trk')                         # (a .tck ends a row at a NaN triplet)
    if bad:
        lines[3][1, 0] = np.nan                      # a row that adds nothing
    path = str(tmp_path / ('lines' + ext))
    header = sio.create_tractogram_header(affine, dims, (2.0, 1.0, 1.5))
    assert sio.save(Tractogram(lines, {}), path, header) == len(lines)
    tdi = DensityMap(dims, affine, zoom=2, device=DEV)
    status, index = tdi.add_tractogram(path)
    points, offsets, want_index = corner_voxels(path, affine)
    want = ref.density_final(points * F32(2), offsets, tdi.dims, lin / 2)
    assert np.array_equal(index, want_index) and len(index) == len(lines) - 3
    assert np.array_equal(status.cpu().numpy(), want['status']) and (want['status'] < 0).sum() == bad
    m = tdi.maps()
    assert np.array_equal(m['count'], want['count']) and want['count'].sum() > 500
    assert np.array_equal(m['length_mm'], want['length_q'] / 2.0 ** 20)
    assert tdi.skipped == 3 + bad
    # the command on the same file
    ref_file = str(tmp_path / 'ref.nii.gz')
    nifti.save(ref_file, np.zeros(dims, np.uint8), affine)
    prefix = str(tmp_path / 'cmd')
    ttl_density.main([path, ref_file, prefix, '--zoom', '2', '--dec'])
    assert np.array_equal(np.asarray(nifti.load(prefix + '_count.nii.gz').dataobj), want['count'])
    assert np.array_equal(np.asarray(nifti.load(prefix + '_dec.nii.gz').dataobj),
                          (want['dec_q'] / 2.0 ** 20).astype(F32))
    totals = json.load(open(prefix + '.json'))
    assert totals['added'] == len(lines) - 3 - bad and totals['skipped'] == 3 + bad and \
        totals['zoom'] == 2
    with pytest.raises(SystemExit):
        ttl_density.main([path, ref_file, prefix])                    # no -f
    if ext == '.trk':
        other = str(tmp_path / 'other.nii.gz')
        nifti.save(other, np.zeros((7, 5, 5), np.uint8), affine)
        with pytest.raises(ValueError, match='not on the grid'):
            ttl_density.main([path, other, str(tmp_path / 'never')])


def tracked(n_actor=None, only=False, record=None, monkeypatch=None, zoom=1, **options):
    """A det-tracked run of test_connectome's synthetic subject with a density
    map attached: (map, env, streamlines yielded)."""
    import test_connectome as tc
    from tracktolearn_amd import parallel
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env, mask = tc.make_env()
    tdi = DensityMap(mask.shape, np.eye(4), zoom=zoom, device=DEV, dec=True)
    if record is not None:
        inner = parallel.select_tracts

        def recording(*args, **kwargs):
            out = inner(*args, **kwargs)
            record.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
            return out
        monkeypatch.setattr(parallel, 'select_tracts', recording)
    np.random.seed(11)
    tracker = Tracker(OdfTracking(env, 'det', seed=5), n_actor or tc.N_SEEDS, min_length=2.0,
                      max_length=60.0, density=tdi, **options)
    if only:
        assert tracker.track_density(env) is tdi
        return tdi, env, None
    return tdi, env, [np.asarray(item.streamline) for item in tracker.track(env, TrkFile)]


def _tdi_maps(tdi):
    return [t.cpu().numpy() for t in (tdi.count, tdi.ends, tdi.length_q, tdi.dec_q)]


@pytest.mark.gpu
@pytest.mark.parametrize('options', [{}, {'compress': 0.1, 'bidirectional': True, 'zoom': 2}],
                         ids=['plain', 'compress_bidirectional_zoom2'])
def test_streamed_density_is_add_tractogram_of_what_track_returned(options, monkeypatch):
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.tractogram import Tractogram
    record = []
    tdi, env, lines = tracked(record=record, monkeypatch=monkeypatch, **options)
    assert len(record) == 1 and len(lines) == len(record[0][1]) > 64
    points, counts = record[0]
    # what was written is what was mapped (.trk at 1 mm: the same + 0.5)
    assert np.array_equal(np.concatenate(lines).astype(F32), points + F32(0.5))
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    vox_lines = [points[offsets[i]:offsets[i + 1]] for i in range(len(counts))]
    other = DensityMap(tdi.ref_dims, np.eye(4), zoom=tdi.zoom, device=DEV, dec=True)
    other.add_tractogram(Tractogram(vox_lines, {}), env)
    for a, b in zip(_tdi_maps(tdi), _tdi_maps(other)):
        assert np.array_equal(a, b)
    want = ref.density_final((points + F32(0.5)) * F32(tdi.zoom), offsets, tdi.dims,
                             np.eye(3) / tdi.zoom)
    assert np.array_equal(tdi.maps()['count'], want['count'])
    assert np.array_equal(tdi.maps()['ends'], want['ends']) and want['ends'].sum() > len(lines)
    assert np.array_equal(tdi.length_q.cpu().numpy().reshape(tdi.dims), want['length_q'])
    assert tdi.skipped == 0 and tdi.totals()['added'] == len(lines)


@pytest.mark.gpu
def test_density_does_not_depend_on_n_actor_and_needs_no_items():
    whole, _, lines = tracked(bidirectional=True)
    small, _, small_lines = tracked(n_actor=64, bidirectional=True)
    assert len(lines) == len(small_lines)
    only, _, _ = tracked(n_actor=64, only=True, bidirectional=True)
    for other in (small, only):
        for a, b in zip(_tdi_maps(whole), _tdi_maps(other)):
            assert np.array_equal(a, b)
    assert whole.totals()['added'] == len(lines)


@pytest.mark.gpu
def test_tracker_refuses_another_grid_and_host_buffers():
    import test_connectome as tc
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.tracking.odf_policy import OdfTracking
    from tracktolearn_amd.tracking.tracker import Tracker, TrkFile
    env, mask = tc.make_env()
    tdi = DensityMap((tc.D, tc.D, tc.D + 1), np.eye(4), device=DEV)
    tracker = Tracker(OdfTracking(env, 'det', seed=5), tc.N_SEEDS, min_length=2.0, density=tdi)
    with pytest.raises(ValueError, match='grid'):
        list(tracker.track(env, TrkFile))
    ok = DensityMap(mask.shape, np.eye(4), device=DEV)
    tracker = Tracker(OdfTracking(env, 'det', seed=5), tc.N_SEEDS, min_length=2.0, density=ok)
    tracker._device_output = lambda env: False           # an env with host buffers
    with pytest.raises(ValueError, match='host buffers'):
        tracker._check_products(env)


@pytest.mark.gpu
def test_track_command_writes_the_maps(tmp_path, capsys):
    import test_connectome as tc
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.runners import ttl_density, ttl_track
    sh, mask, _ = tc.subject()
    seed_mask = np.zeros(mask.shape, np.uint8)
    seed_mask[5:11, 5:11, 5:11] = 1
    for name, vol in (('fodf', sh), ('mask', mask), ('seed', seed_mask)):
        nifti.save(str(tmp_path / f'{name}.nii.gz'), vol, np.eye(4))
    prefix = str(tmp_path / 'only')
    ttl_track.main(tc._argv(tmp_path, 'never.trk', '--density_map', prefix, '--density_zoom', '2',
                            '--density_dec', '--density_only'))
    out = capsys.readouterr().out
    assert 'Saved the density maps' in out and 'streamlines to' not in out
    assert not os.path.exists(str(tmp_path / 'never.trk'))
    count = np.asarray(nifti.load(prefix + '_count.nii.gz').dataobj)
    totals = json.load(open(prefix + '.json'))
    assert count.shape == (2 * tc.D,) * 3 and count.dtype == np.int32 and count.max() >= 2
    assert totals['zoom'] == 2 and totals['added'] > 20 and totals['skipped'] == 0
    assert nifti.load(prefix + '_dec.nii.gz').dataobj.shape == (2 * tc.D,) * 3 + (3,)
    # with the tractogram, as a .tck (whose points are the tracker's): the same maps, and
    # ttl_density.py on that file gives them again
    ttl_track.main(tc._argv(tmp_path, 'with.tck', '--density_map', str(tmp_path / 'with'),
                            '--density_zoom', '2'))
    n_saved = int(re.search(r'Saved (\d+) streamlines to', capsys.readouterr().out).group(1))
    assert n_saved == totals['added']
    assert np.array_equal(np.asarray(nifti.load(str(tmp_path / 'with_count.nii.gz')).dataobj), count)
    assert not os.path.exists(str(tmp_path / 'with_dec.nii.gz'))
    ttl_density.main([str(tmp_path / 'with.tck'), str(tmp_path / 'mask.nii.gz'),
                      str(tmp_path / 'cmd'), '--zoom', '2'])
    capsys.readouterr()
    assert np.array_equal(np.asarray(nifti.load(str(tmp_path / 'cmd_count.nii.gz')).dataobj), count)
