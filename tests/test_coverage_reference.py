"""``ttl_tract_coverage`` held to its definition where its merge logic runs
(DESIGN 3.8): segments that cross many planes per axis, enter and leave the
volume, tie, graze lattice points from afar and end 10^38 voxels away, each
launched alone and compared byte for byte with ``walk_segment_planes``; the
same classes as ragged tractograms; streamline lengths, non-finite points,
the score gate and the grid-stride loop against ``coverage_map``.  On the CPU:
the three statements of the walk agree on every case, the case set reaches the
walk's difficult parts, and every named mutant of the restatement
(tests/ref_oracle_validator.py) changes what the GPU tests compare."""
import numpy as np
import pytest
import torch

import coverage_cases as cc
import ref_oracle_validator as ref
from ref_oracle_validator import HAND, random_walks

DEV = 'cuda:0'


def _case_set(a, b, dims, walk):
    """The marked set of the two-point streamline a -> b (what one launch reports)."""
    return cc.first_voxel(a, dims) | set(walk)


def _as_map(voxels, dims):
    m = np.zeros(dims, np.uint8)
    for v in voxels:
        m[v] = 1
    return m


# ----------------------------------------------------------------- CPU tests
@pytest.mark.parametrize('dims', cc.VOLUMES + (cc.RAGGED_VOLUME,))
def test_three_statements_agree(dims):
    """Bounded walk == crossing-by-crossing definition == planes definition,
    as ordered lists, on every segment case; 10^38 voxels away (where the
    naive walk cannot run) bounded == planes."""
    cases, walks = cc.segment_cases(dims), cc.segment_walks(dims)
    for name in cc.CLASSES:
        A, B = cases[name]
        for a, b, want in zip(A, B, walks[name]):
            assert ref.walk_segment(a, b, dims) == want, (name, a, b, dims)
            if name != 'huge':
                assert ref.walk_segment_naive(a, b, dims) == want, (name, a, b, dims)


def test_planes_definition_on_hand_built():
    for a, b, dims, want in HAND:
        assert ref.walk_segment_planes(a, b, dims) == want, (a, b)


def test_case_set_reaches_the_walk():
    """Asserted on the reference alone: in every (class, volume) cell at least
    a quarter of the cases mark a voxel by a crossing and at least a tenth
    mark three or more.  Every volume here has an axis an index can move
    along, so no cell is exempt; in (2, 3, 1) three voxels are half the
    volume, and the generators of the axis-aligned, diagonal and huge classes
    start just outside and aim across it to get there."""
    for dims in cc.VOLUMES:
        walks = cc.segment_walks(dims)
        for name in cc.CLASSES:
            n = len(walks[name])
            some = sum(len(w) >= 1 for w in walks[name])
            three = sum(len(set(w)) >= 3 for w in walks[name])
            print(f'{dims} {name}: {some}/{n} mark, {three}/{n} mark >= 3')
            assert 4 * some >= n, (dims, name, some, n)
            assert 10 * three >= n, (dims, name, three, n)


def test_rows_restatement_equals_definition():
    """coverage_rows (the kernel's outer loop) == streamline_voxels over the
    accepted rows == coverage_map, on the row cases and the 40 000-row batch."""
    for name, dims, points, offsets, scores, thr in cc.row_cases():
        accept = None if scores is None else scores > np.float32(thr)
        got = ref.coverage_rows(points, offsets, dims, scores, thr)
        want = set()
        for r in range(len(offsets) - 1):
            if accept is None or accept[r]:
                want |= ref.streamline_voxels(points[offsets[r]:offsets[r + 1]], dims,
                                              ref.walk_segment_planes)
        assert np.array_equal(got, _as_map(want, dims)), name
        assert np.array_equal(got, ref.coverage_map(points, offsets, dims, accept)), name
        assert got.any(), name
    dims, points, offsets, scores = cc.grid_batch()
    accept = scores > np.float32(0.5)
    assert np.flatnonzero(accept).tolist() == list(cc.GRID_ACCEPTED)
    got = ref.coverage_rows(points, offsets, dims, scores, 0.5)
    assert np.array_equal(got, ref.coverage_map(points, offsets, dims, accept))
    assert 0 < got.sum() < got.size // 50


def _segment_witnesses(cases, mutants=ref.SEGMENT_MUTANTS):
    """{mutant: number of (a, b, dims) whose two-point streamline's marked set
    the mutant changes}."""
    count = dict.fromkeys(mutants, 0)
    for a, b, dims in cases:
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        with np.errstate(invalid='ignore'):
            if np.array_equal(np.floor(a), np.floor(b)):
                continue                         # no crossing: no statement of the walk runs
        first = cc.first_voxel(a, dims)
        good = first | set(ref.walk_segment(a, b, dims))
        for m in mutants:
            count[m] += (first | set(ref.walk_segment(a, b, dims, m))) != good
    return count


def _launched_segments():
    return [(a, b, dims) for dims in cc.VOLUMES
            for A, B in cc.segment_cases(dims).values() for a, b in zip(A, B)]


def _row_witnesses(mutant):
    """The row cases, and the accepted rows of the 40 000-row batch, whose
    voxels the mutant changes."""
    n = 0
    for _, dims, points, offsets, scores, thr in cc.row_cases():
        n += not np.array_equal(ref.coverage_rows(points, offsets, dims, scores, thr, mutant),
                                ref.coverage_rows(points, offsets, dims, scores, thr))
    dims, points, offsets, scores = cc.grid_batch()
    bad = ref.coverage_rows(points, offsets, dims, scores, 0.5, mutant)
    for r in cc.GRID_ACCEPTED:
        own = ref.streamline_voxels(points[offsets[r]:offsets[r + 1]], dims)
        n += any(bad[v] != 1 for v in own)
    return n


def test_every_mutant_has_witnesses():
    """Each named mutant changes the marked set of at least 5 cases that the
    GPU tests launch and compare exactly."""
    seg = _segment_witnesses(_launched_segments())
    rows = {m: _row_witnesses(m) for m in ref.ROW_MUTANTS}
    for m, n in {**seg, **rows}.items():
        print(f'{m}: {n} witnesses')
    assert all(n >= 5 for n in seg.values()), seg
    assert all(n >= 5 for n in rows.values()), rows


def test_former_inputs_leave_mutants_without_witness():
    """The record of DESIGN 3.8: on the inputs of test_coverage_hand_built_and_random
    (HAND and the seed-4 walks of 0.5-0.75 voxel, here the first 300 of them)
    a segment crosses at most one plane per axis, and some mutants have no
    witness at all; the new case set (above) leaves none."""
    lines = random_walks(np.random.default_rng(4), 300, 2, 120, 40, start=(-4, 44))
    assert max(np.abs(np.floor(s[1:]) - np.floor(s[:-1])).max() for s in lines) <= 1
    old = [(a, b, dims) for a, b, dims, _ in HAND]
    old += [(s[j], s[j + 1], (40, 40, 40)) for s in lines for j in range(len(s) - 1)]
    count = _segment_witnesses(old)
    for m, n in count.items():
        print(f'{m}: {n} witnesses on the former inputs')
    none = [m for m, n in count.items() if n == 0]
    print(f'{len(none)} of {len(count)} mutants without a witness: {none}')
    assert len(none) >= 3 and {'t_float32', 'd_float32'} <= set(none)


# ----------------------------------------------------------------- GPU tests
def _dev(points, offsets):
    return torch.from_numpy(points).to(DEV), torch.from_numpy(offsets).to(DEV)


def _gpu_map(points, offsets, dims, scores=None, threshold=0.5, visited=None):
    from tracktolearn_amd.experiment.oracle_validator import tract_coverage
    p, o = _dev(points, offsets)
    sc = None if scores is None else torch.from_numpy(scores).to(DEV)
    v = tract_coverage(p, o, dims, sc, threshold, visited).cpu().numpy()
    assert ((v == 0) | (v == 1)).all()
    return v.reshape(dims)


@pytest.mark.gpu
@pytest.mark.parametrize('dims', cc.VOLUMES)
def test_every_segment_alone_equals_definition(dims):
    """One launch per segment case (a two-point streamline) into its own row
    of one zeroed [cases, X Y Z] tensor, read back once: every row is the
    definition's set, byte for byte."""
    from tracktolearn_amd.experiment.oracle_validator import tract_coverage
    cases, walks = cc.segment_cases(dims), cc.segment_walks(dims)
    A = np.concatenate([cases[c][0] for c in cc.CLASSES])
    B = np.concatenate([cases[c][1] for c in cc.CLASSES])
    want = [w for c in cc.CLASSES for w in walks[c]]
    names = [c for c in cc.CLASSES for _ in walks[c]]
    n, vol = len(A), int(np.prod(dims))
    points = torch.from_numpy(np.stack([A, B], 1).reshape(-1, 3).copy()).to(DEV)
    offsets = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    visited = torch.zeros(n, vol, dtype=torch.uint8, device=DEV)
    for k in range(n):
        tract_coverage(points[2 * k:2 * k + 2], offsets, dims, visited=visited[k])
    got = visited.cpu().numpy()
    assert ((got == 0) | (got == 1)).all()
    expect = np.zeros((n,) + tuple(dims), np.uint8)
    for k in range(n):
        for v in _case_set(A[k], B[k], dims, want[k]):
            expect[(k,) + v] = 1
    bad = np.flatnonzero((got != expect.reshape(n, vol)).any(1))
    for k in bad[:10]:
        g = sorted(zip(*np.nonzero(got[k].reshape(dims))))
        print(f'{names[k]} a={A[k].tolist()} b={B[k].tolist()} dims={dims}\n'
              f'  kernel     {[tuple(int(x) for x in v) for v in g]}\n'
              f'  definition {sorted(_case_set(A[k], B[k], dims, want[k]))}')
    assert len(bad) == 0, f'{len(bad)} of {n} segments differ'


@pytest.mark.gpu
@pytest.mark.parametrize('name', cc.CLASSES)
def test_class_as_ragged_tractogram(name):
    """The class's segments grouped into streamlines of 1-130 segments by
    concatenation (jumps between cases are segments too): the map of one
    launch equals coverage_map exactly."""
    dims = cc.RAGGED_VOLUME
    A, B = cc.segment_cases(dims)[name]
    A, B = np.tile(A, (3, 1)), np.tile(B, (3, 1))
    perm = np.random.default_rng(26).permutation(len(A))
    lines = cc.ragged_from_segments(A[perm], B[perm], cc.CLASSES.index(name))
    assert max(len(s) for s in lines) > 130      # more segments than a wave has lanes
    points, offsets = cc.pack(lines)
    want = ref.coverage_map(points, offsets, dims)
    assert want.any()
    assert np.array_equal(_gpu_map(points, offsets, dims), want)


@pytest.mark.gpu
def test_row_cases_equal_definition():
    """Lengths 0 .. 130 with empty rows between, NaN / +-Inf points in every
    position, scores at the threshold, next to it, NaN and +-Inf (thresholds
    0.5 and 0.0), and the same rows with scores=None."""
    for name, dims, points, offsets, scores, thr in cc.row_cases():
        accept = None if scores is None else scores > np.float32(thr)
        want = ref.coverage_map(points, offsets, dims, accept)
        got = _gpu_map(points, offsets, dims, scores, thr)
        assert np.array_equal(got, want), name


@pytest.mark.gpu
def test_grid_stride_and_score_gate_on_40000_rows():
    dims, points, offsets, scores = cc.grid_batch()
    want = ref.coverage_map(points, offsets, dims, scores > np.float32(0.5))
    got = _gpu_map(points, offsets, dims, scores)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_only_ones_are_written():
    """A visited buffer that already holds ones keeps them: the result is the
    union of what it held and what the streamlines mark."""
    name, dims, points, offsets, scores, thr = cc.row_cases()[0]
    rng = np.random.default_rng(27)
    held = (rng.random(dims) < 0.1).astype(np.uint8)
    visited = torch.from_numpy(held.reshape(-1).copy()).to(DEV)
    got = _gpu_map(points, offsets, dims, scores, thr, visited)
    want = ref.coverage_map(points, offsets, dims)
    assert (held & ~want.astype(bool)).any()
    assert np.array_equal(got, held | want)
