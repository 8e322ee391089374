"""Case sets of tests/test_connectome.py.  Coordinates are dyadic (multiples of
1/8, plus float32(-0.3)) and so are the entries of every ``lin``: each d2 of the
definition is exact in float64 and the ties below are real ties."""
import functools

import numpy as np

import ref_connectome as ref

F32 = np.float32
MAX_REACH = 8

LINS = {
    'diag': np.array([[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.5]]),
    'shear': np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]]),
    'neg': np.array([[-2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.5]]),
}
BOX, LINE = (7, 5, 4), (1, 1, 9)

# name: (dims, lin, N, radius: 0.0, 'tie' or 'max')
SETS = {
    'box_diag_r0': (BOX, 'diag', 3, 0.0),
    'box_diag_tie': (BOX, 'diag', 3, 'tie'),
    'box_diag_max': (BOX, 'diag', 200, 'max'),
    'box_shear_tie': (BOX, 'shear', 3, 'tie'),
    'box_shear_max': (BOX, 'shear', 1, 'max'),
    'box_neg_tie': (BOX, 'neg', 200, 'tie'),
    'box_neg_max': (BOX, 'neg', 3, 'max'),
    'line_diag_r0': (LINE, 'diag', 3, 0.0),
    'line_shear_tie': (LINE, 'shear', 200, 'tie'),
    'line_neg_max': (LINE, 'neg', 1, 'max'),
}
ROW_LENGTHS = (2, 3, 63, 64, 65, 129, 1000)


def max_radius(lin):
    """The largest float64 radius whose reach stays within MAX_REACH."""
    rows = np.sqrt((np.linalg.inv(lin) ** 2).sum(axis=1))
    r = MAX_REACH / rows.max()
    while np.ceil(r * rows).max() > MAX_REACH:
        r = np.nextafter(r, 0.0)
    return float(r)


def radius_of(dims, lin, radius):
    """'tie': the distance of the two-way tie of the set's volume, the length of
    the column of ``lin`` along which its two candidates lie (exact)."""
    if radius == 'max':
        return max_radius(lin)
    if radius == 'tie':
        col = lin[:, 0] if dims == BOX else lin[:, 2]
        return float(np.sqrt((col ** 2).sum()))      # 2, 1, 2 / 1.5, 2, 1.5: exact
    return float(radius)


def box_labels(N):
    """(7, 5, 4).  Round (3, 2, 1): a two-way tie along x and a four-way tie
    across the face y = 2; round (5, 2, 2): a pair where mm and voxel distance
    disagree; a label above N and a negative one with ends inside them; a
    random top layer at x <= 3 with labels from -2 to N + 2."""
    lab = lambda k: min(k, N)
    v = np.zeros(BOX, np.int32)
    v[2, 2, 1], v[4, 2, 1] = lab(1), lab(2)
    v[2, 1, 1], v[4, 1, 1] = lab(3), lab(3)
    v[6, 2, 2], v[5, 3, 2] = lab(2), lab(3)
    v[0, 0, 0] = lab(1)
    v[1, 4, 0], v[1, 3, 0] = N + 1, -2
    v[6, 4, 3] = N                                   # the last word of the volume
    rng = np.random.RandomState(7)
    v[:4, :, 3] = rng.randint(-2, N + 3, (4, 5))
    return v


def line_labels(N):
    lab = lambda k: min(k, N)
    v = np.zeros(LINE, np.int32)
    v[0, 0] = [lab(1), 0, lab(2), 0, 0, lab(3), N + 1, -1, lab(1)]
    return v


BOX_ENDS = [
    (2.25, 2.5, 1.75),          # inside a node
    (3.25, 2.5, 1.5),           # beside one
    (3.5, 2.5, 1.5),            # equidistant from two
    (3.5, 2.0, 1.5),            # equidistant from four (diag, neg)
    (5.5, 2.25, 2.5),           # mm and voxel distance disagree
    (-0.3, 0.5, 0.5),           # -0.3: voxel -1, beside the node in (0, 0, 0)
    (0.5, -0.3, -0.3),
    (-1.5, 2.5, 1.5), (7.75, 2.5, 2.5), (3.5, 2.5, -2.0),        # outside, within reach
    (-20.0, 2.0, 1.0), (30.0, 2.0, 1.0), (3.5, 2.5, 40.0),       # outside, beyond it
    (7.0, 2.5, 2.5), (3.5, 5.0, 1.5), (3.5, 2.5, 4.0), (7.0, 5.0, 4.0),    # dims exactly
    (6.875, 4.875, 3.875),      # the last voxel
    (1.5, 4.5, 0.5),            # inside a label above N
    (1.5, 3.5, 0.5),            # inside a negative label
    (0.0, 0.0, 0.0), (0.125, 0.125, 0.125),
    (1e30, 1.0, 1.0), (-1e30, 1.0, 1.0),
]
LINE_ENDS = [
    (0.25, 0.75, 0.5),          # inside a node
    (0.5, 0.5, 1.25),           # beside one
    (0.5, 0.5, 1.5),            # equidistant from two
    (0.5, 0.5, 3.75), (0.5, 0.5, 4.0),
    (0.5, 0.5, -0.3), (-0.3, 0.5, 0.5), (0.5, 0.5, -3.0),
    (0.5, 0.5, 9.0), (0.5, 0.5, 12.25), (0.5, 3.0, 4.5), (1.0, 1.0, 9.0),
    (0.5, 0.5, 40.0), (0.5, -30.0, 2.5),
    (0.5, 0.5, 6.5), (0.5, 0.5, 7.5),        # inside a label above N, a negative one
    (0.5, 0.5, 8.875),
    (0.5, 0.5, 1e30), (1e30, 1e30, 1e30),
]


class Case:
    """One set: labels (X, Y, Z) int32, lin, N, radius_mm, reach, the ragged
    rows, and ``ends``, the distinct finite end points among them."""


def _rows(dims, seed):
    rng = np.random.RandomState(seed)
    special = [np.array(e, F32) for e in (BOX_ENDS if dims == BOX else LINE_ENDS)]
    near = [np.array([rng.randint(-24, 8 * d + 24) / 8.0 for d in dims], F32) for _ in range(24)]
    ends = special + near
    rows = []
    for i in range(2 * len(ends)):
        a, b = ends[i % len(ends)], ends[(5 * i + 2) % len(ends)]
        if max(abs(a).max(), abs(b).max()) > 1e6:
            b = a                   # an end at 1e30 pairs with itself: length 0, scored
        L = ROW_LENGTHS[i % len(ROW_LENGTHS)] if i % 3 == 0 else 2 + i % 2
        inner = np.stack([rng.randint(0, 8 * d + 1, L - 2) / 8.0 for d in dims], axis=1)
        rows.append(np.concatenate([a[None], inner.astype(F32), b[None]]))
    rows.append(np.array([ends[0], (1e30, 1.0, 1.0)], F32))         # 2^40 mm and more
    rows.append(np.zeros((0, 3), F32))                              # L = 0
    rows.append(ends[0][None].copy())                               # L = 1
    for L, at in ((5, 0), (5, 2), (5, 4), (130, 0), (130, 64), (130, 129), (2, 1)):
        row = np.stack([rng.randint(0, 8 * d + 1, L) / 8.0 for d in dims], axis=1).astype(F32)
        row[at, at % 3] = np.nan if L != 2 else np.inf
        rows.append(row)
    rows.append(np.zeros((0, 3), F32))
    rows.append(np.array([ends[2], ends[0]], F32))                  # a last, scored row
    return rows, [e for e in ends]


@functools.lru_cache(maxsize=None)
def case(name):
    dims, lin_name, N, radius = SETS[name]
    c = Case()
    c.name, c.dims, c.n_nodes = name, dims, N
    c.lin = LINS[lin_name].copy()
    c.radius_mm = radius_of(dims, c.lin, radius)
    c.reach = ref.reach_for(c.lin, c.radius_mm)
    c.labels = box_labels(N) if dims == BOX else line_labels(N)
    rows, c.ends = _rows(dims, 100 + sorted(SETS).index(name))
    c.rows = rows
    c.offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=c.offsets[1:])
    c.points = np.concatenate(rows).astype(F32)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """(node, length float64, length longdouble) of the definition, once per set."""
    c = case(name)
    out = ref.assign(c.points, c.offsets, c.labels, c.lin, c.radius_mm, c.reach, c.n_nodes)
    for a in out:
        a.setflags(write=False)
    return out


def end_nodes(name, mutant=None):
    """The node of every end of the set under ``mutant``."""
    c = case(name)
    return [ref.end_node(e, c.labels, c.lin, c.radius_mm, c.reach, c.n_nodes, mutant)
            for e in c.ends]


def two_point_rows(name, n):
    """n two-point rows that cycle through the set's ends (first end i, last
    end 3 i + 1): (points, offsets, node of the definition)."""
    c = case(name)
    finite = [k for k, e in enumerate(c.ends) if np.abs(e).max() < 1e6]
    nodes = np.array(end_nodes(name), np.int32)[finite]
    ends = np.stack([c.ends[k] for k in finite])
    i = np.arange(n)
    first, last = i % len(finite), (3 * i + 1) % len(finite)
    points = np.empty((2 * n, 3), F32)
    points[0::2], points[1::2] = ends[first], ends[last]
    return points, 2 * np.arange(n + 1, dtype=np.int64), np.stack([nodes[first], nodes[last]], 1)
