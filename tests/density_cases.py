"""The case sets of tests/test_density.py (test infrastructure only), shared
by its CPU and GPU tests: seeded, deterministic, float32 before anything looks
at them.  ``SETS``: name -> Case(dims, lin, points, offsets).  The segment
classes and row cases are those of coverage_cases, imported and not edited:
their NaN / +-Inf rows are now rows that add nothing."""
import collections
import functools

import numpy as np

import coverage_cases as cov
import ref_density as ref

F32 = np.float32
Case = collections.namedtuple('Case', 'dims lin points offsets')

IDENTITY = np.eye(3)
ANISO = np.diag([2.0, 1.0, 1.5])
OBLIQUE = np.array([[1.9, 0.3, -0.2], [-0.25, 1.1, 0.4], [0.15, -0.35, 1.4]])
ROW_LENGTHS = (2, 3, 64, 65, 66, 129, 130)
WALK_ROWS = 160                  # the CPU check of the definition: lengths 2 .. 300
TIER_WAVE_SLOTS = 64
TIER_SPILLS = (1024, 64, None)   # spill_slots of the three tier cases; None: no workspace


def case(lines, dims, lin=IDENTITY):
    points, offsets = cov.pack([np.asarray(s, F32).reshape(-1, 3) for s in lines])
    return Case(tuple(dims), np.asarray(lin, np.float64), points, offsets)


@functools.lru_cache(maxsize=None)
def walk_rows():
    """160 rows of coverage_cases._walk, lengths 2 .. 300, in ROW_VOLUME."""
    rng = np.random.default_rng(31)
    return [cov._walk(rng, int(L), cov.ROW_VOLUME) for L in rng.integers(2, 301, WALK_ROWS)]


def _forth_and_back(rng, dims):
    """A row that runs over some voxels and back over the same ones, twice."""
    there = cov._walk(rng, 24, dims, step=(0.4, 1.2))
    return np.concatenate([there, there[-2::-1], there[1:], there[-2::-1]])


THRESHOLD_LIN = np.diag([2.0 ** 30, 2.0 ** 20, 16.0])


@functools.lru_cache(maxsize=None)
def threshold_rows():
    """[(row, kernel-order length - 2^40, streamline-order length - 2^40)]: rows of
    130 points whose length sits within 4 ulps of 2^40 mm on either side, among
    them rows that the sum in streamline order would put on the other side.  127
    long moves along x (2^30 mm per voxel) bring the sum to within 2^23 mm, one
    along y (2^20 mm per voxel) to within 16 mm, the last along z (16 mm per
    voxel) is searched in steps of a quarter ulp of 2^40."""
    m = [float(v) for v in THRESHOLD_LIN.reshape(9)]
    T, out = ref.MAX_LENGTH, []
    for seed in range(6):
        rng = np.random.default_rng([37, seed])
        row = np.stack([rng.uniform(4.0, 12.0, 130), rng.uniform(0.5, 1.5, 130),
                        rng.uniform(0.25, 0.75, 130)], 1).astype(F32)
        row[-3:, 1:] = 0.0
        for _ in range(4):
            row[-3:, 0] = row[-4, 0]
            f = (T - 2.0 ** 23) / ref.kernel_length(row, m)
            row[:-3, 0] = (F32(8) + (row[:-3, 0] - F32(8)) * F32(f)).astype(F32)
        row[-3:, 0] = row[-4, 0]
        rest = T - ref.kernel_length(row, m)
        assert 2.0 ** 21 < rest < 1.5e7
        row[-2:, 1] = F32((rest - 8.0) / 2.0 ** 20)
        rest = T - ref.kernel_length(row, m)
        assert 1.0 < rest < 15.0
        seen = set()
        for k in range(-48, 49):
            r = row.copy()
            r[-1, 2] = F32(rest / 16.0 + k * 2.0 ** -18)
            kernel, line = ref.kernel_length(r, m) - T, ref.streamline_order_length(r, m) - T
            key = (kernel < 0, line < 0)
            if abs(kernel) <= 4 * np.spacing(T) and key not in seen:
                seen.add(key)
                out.append((r, kernel, line))
    return out


@functools.lru_cache(maxsize=None)
def sets():
    out = {}
    # the segment classes, each as one ragged tractogram
    for k, (name, (A, B)) in enumerate(cov.segment_cases(cov.RAGGED_VOLUME).items()):
        lin = (IDENTITY, ANISO, OBLIQUE)[k % 3]
        out['class_' + name] = case(cov.ragged_from_segments(A, B, k), cov.RAGGED_VOLUME, lin)
    # the row cases: every length, empty rows, non-finite points
    for name, dims, points, offsets, scores, _ in cov.row_cases():
        if scores is None and not name.startswith('noscores'):
            out['rows_' + name] = Case(tuple(dims), ANISO, points, offsets)
    # every length under an oblique and an anisotropic lin
    for name, lin in (('oblique', OBLIQUE), ('aniso', ANISO)):
        rng = np.random.default_rng([32, len(name)])
        lines = [cov._walk(rng, L, cov.ROW_VOLUME) for L in ROW_LENGTHS for _ in range(2)]
        out['lengths_' + name] = case(lines, cov.ROW_VOLUME, lin)
    rng = np.random.default_rng(33)
    out['forth_and_back'] = case([_forth_and_back(rng, cov.ROW_VOLUME) for _ in range(6)],
                                 cov.ROW_VOLUME, OBLIQUE)
    # one lane, 4096 visits: far above any wave set; and the same the other way
    out['needle'] = case([[(0.5, 0.5, -3.0), (0.25, 0.75, 4100.0)],
                          [(0.5, 0.5, 4099.5), (0.5, 0.5, 0.5)]], (1, 1, 4096), ANISO)
    hand = [
        [(3.5, 3.5, 3.5), (1e30, 3.5, 3.5)],            # skipped by the length rule
        [(3.25, 4.5, 5.5), (3.75, 4.25, 5.75)],         # both ends in one voxel
        [(3.5, 3.5, 3.5), (3.5, 3.5, 3.5)],             # ... and in one point
        [(1.5, 1.5, 1.5), (3.5, 3.5, 3.5)],             # through two lattice corners
        [(-2.0, 4.5, 4.5), (20.0, 4.5, 4.5)],           # in through one face, out through another
        [(6.5, 6.5, 6.5), (6.5, 6.5, 30.0)],            # starts inside, leaves
        [(6.5, -9.0, 6.5), (6.25, 6.5, 6.75)],          # enters, ends inside
        [(-1.0, -1.0, 3.0), (-3.0, 5.0, 3.0)],          # never inside
        [(0.0, 0.0, 0.0), (8.0, 9.0, 10.0), (0.0, 9.0, 0.0)],
    ]
    out['hand'] = case(hand, (8, 9, 10), ANISO)
    out['length_threshold'] = case([r for r, _, _ in threshold_rows()], cov.ROW_VOLUME,
                                   THRESHOLD_LIN)
    return out


SET_NAMES = tuple(sorted(
    ['class_' + c for c in cov.CLASSES] +
    ['rows_' + n for n, _, _, _, s, _ in cov.row_cases() if s is None and not n.startswith('noscores')] +
    ['lengths_oblique', 'lengths_aniso', 'forth_and_back', 'needle', 'hand', 'length_threshold']))


@functools.lru_cache(maxsize=None)
def reference(name, mutant=None):
    """``ref.density_final`` of a set: the maps once every row is counted."""
    c = sets()[name]
    return ref.density_final(c.points, c.offsets, c.dims, c.lin, mutant)


# ----------------------------------------------------------------- the tiers
def snake(k, dims):
    """k voxel centres in boustrophedon order (z fastest): a row of k points that
    visits exactly k distinct voxels, one plane per segment."""
    out = []
    for x in range(dims[0]):
        ys = range(dims[1]) if x % 2 == 0 else range(dims[1] - 1, -1, -1)
        for n_y, y in enumerate(ys):
            zs = range(dims[2]) if (x * dims[1] + n_y) % 2 == 0 else range(dims[2] - 1, -1, -1)
            out += [(x + 0.5, y + 0.5, z + 0.5) for z in zs]
    assert k <= len(out)
    return np.array(out[:k], F32)


@functools.lru_cache(maxsize=None)
def tier_case():
    """Rows for wave_slots = 64 (32 voxels): short rows that fit, rows of 64 ..
    130 points that leave the wave set, and rows of 1400 points that visit more
    than 512 voxels and leave a spill set of 1024 too, and four rows that sit
    exactly on the thresholds."""
    rng = np.random.default_rng(34)
    lines = [cov._walk(rng, int(L), cov.ROW_VOLUME, step=(0.2, 1.0)) for L in rng.integers(2, 16, 12)]
    lines += [cov._walk(rng, L, cov.ROW_VOLUME) for L in (64, 65, 66, 129, 130) for _ in range(3)]
    lines += [cov._walk(rng, 1400, cov.ROW_VOLUME, step=(1.5, 2.5)) for _ in range(6)]
    # exactly on either side of both thresholds: 32 | 33 and 512 | 513 voxels
    lines += [snake(k, cov.ROW_VOLUME) for k in (32, 33, 512, 513)]
    order = rng.permutation(len(lines))
    return case([lines[i] for i in order], cov.ROW_VOLUME, OBLIQUE)


@functools.lru_cache(maxsize=None)
def tier_reference(spill_slots):
    """The first call's maps and status at TIER_WAVE_SLOTS and ``spill_slots``."""
    c = tier_case()
    return ref.density(c.points, c.offsets, c.dims, c.lin, TIER_WAVE_SLOTS, spill_slots)


# ------------------------------------------------------------ the long batch
@functools.lru_cache(maxsize=None)
def grid_case():
    """The 40 000 short rows of coverage_cases.grid_batch(): more rows than the
    capped grid has waves (32 768), so 7 232 waves take a second row.  Rows 0 ..
    5 are replaced by rows that overflow a wave set of 64 slots: the waves that
    take them pass their table on to rows 32 768 .. 32 773."""
    dims, points, offsets, _ = cov.grid_batch()
    rng = np.random.default_rng(35)
    lines = [points[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
    for i in range(6):
        lines[i] = cov._walk(rng, 130, dims)
    return case(lines, dims, ANISO)


@functools.lru_cache(maxsize=None)
def grid_reference():
    c = grid_case()
    return ref.density(c.points, c.offsets, c.dims, c.lin, TIER_WAVE_SLOTS, 1024)
