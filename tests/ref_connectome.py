"""The structural connectome's definition (include/ttl_hip.h,
ttl_connectome_assign / ttl_connectome_accumulate) as a literal loop over
streamlines and box voxels: Python floats are IEEE float64 and every expression
is written in the header's order, so the nodes and every d2 are the kernel's
bit for bit; the length is also taken in numpy.longdouble, the yardstick of the
kernel's butterfly sum.

``mutant`` names one deliberate misreading of the definition; the tests show a
witness for each inside the sets the GPU tests launch, so a kernel that made
that mistake could not pass them."""
import math

import numpy as np

LENGTH_SCALE = 1048576.0
MAX_LENGTH = 2.0 ** 40

ASSIGN_MUTANTS = ('trunc_ends', 'corner_centre', 'exclusive_radius', 'last_on_tie',
                  'voxel_distance', 'own_voxel_searched', 'clamped_outside',
                  'label_above_n_kept')
ACCUMULATE_MUTANTS = ('ordered_cell', 'length_truncated')
MUTANTS = ASSIGN_MUTANTS + ACCUMULATE_MUTANTS


def reach_for(lin, radius_mm):
    """ceil(radius * ||row i of inv(lin)||_2), as connectome.reach_for (no limit)."""
    inv = np.linalg.inv(np.asarray(lin, np.float64).reshape(3, 3))
    return [int(math.ceil(float(radius_mm) * math.sqrt(float((inv[i] ** 2).sum()))))
            for i in range(3)]


def _apply(m, d):
    """lin d, each row ((m0 x + m1 y) + m2 z); m: 9 Python floats."""
    return [(m[3 * r] * d[0] + m[3 * r + 1] * d[1]) + m[3 * r + 2] * d[2] for r in range(3)]


def end_node(p, labels, lin, radius_mm, reach, n_nodes, mutant=None):
    """The node of the end ``p`` (three finite floats): header, steps 1 and 2."""
    dims = labels.shape
    m = [float(v) for v in np.asarray(lin, np.float64).reshape(9)]
    p = [float(v) for v in p]

    def is_node(label):
        return label >= 1 and (label <= n_nodes or mutant == 'label_above_n_kept')

    e = [int(math.trunc(c)) if mutant == 'trunc_ends' else int(math.floor(c)) for c in p]
    if mutant == 'clamped_outside':
        e = [min(max(e[i], 0), dims[i] - 1) for i in range(3)]
    inside = all(0 <= e[i] < dims[i] for i in range(3))
    if inside and mutant != 'own_voxel_searched':
        own = int(labels[e[0], e[1], e[2]])
        if is_node(own):
            return own
    r2 = float(radius_mm) * float(radius_mm)
    best = None                                  # (d2, index, label)
    lo = [max(e[i] - int(reach[i]), 0) for i in range(3)]
    hi = [min(e[i] + int(reach[i]), dims[i] - 1) for i in range(3)]
    for x in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for z in range(lo[2], hi[2] + 1):
                label = int(labels[x, y, z])
                if not is_node(label):
                    continue
                half = 0.0 if mutant == 'corner_centre' else 0.5
                d = [p[0] - (float(x) + half), p[1] - (float(y) + half),
                     p[2] - (float(z) + half)]
                w = d if mutant == 'voxel_distance' else _apply(m, d)
                d2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
                if not (d2 < r2 if mutant == 'exclusive_radius' else d2 <= r2):
                    continue
                index = (x * dims[1] + y) * dims[2] + z
                if best is None or d2 < best[0] or \
                        (d2 == best[0] and (index > best[1] if mutant == 'last_on_tie'
                                            else index < best[1])):
                    best = (d2, index, label)
    return 0 if best is None else best[2]


def segment_lengths(row, lin, dtype):
    """|lin (c_{j+1} - c_j)| per segment in ``dtype``, the header's expressions."""
    c = np.asarray(row, np.float32).astype(dtype)
    m = np.asarray(lin, np.float64).reshape(9).astype(dtype)
    d = c[1:] - c[:-1]
    v = [(m[3 * r] * d[:, 0] + m[3 * r + 1] * d[:, 1]) + m[3 * r + 2] * d[:, 2]
         for r in range(3)]
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def length_bound(row, lin):
    """(L + 8) * 2^-53 * A_s, A_s = sum_j || |lin| |c_{j+1} - c_j| ||_2: one rounding of the
    difference, three products and two sums per component, the norm (about 3
    roundings), and at most L - 2 roundings of a sum taken in any order."""
    c = np.asarray(row, np.float32).astype(np.longdouble)
    a = np.abs(np.asarray(lin, np.float64).reshape(3, 3)).astype(np.longdouble)
    d = np.abs(c[1:] - c[:-1])
    v = d @ a.T
    A = np.sqrt((v * v).sum(axis=1)).sum()
    return (len(c) + 8) * np.longdouble(2.0) ** -53 * A


def assign(points, offsets, labels, lin, radius_mm, reach, n_nodes, mutant=None):
    """(node (n, 2) int32, length (n,) float64, length in longdouble (n,)) of
    the ragged rows.  The float64 length is the sum in streamline order."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(offsets) - 1
    node = np.full((n, 2), -1, np.int32)
    length = np.zeros(n, np.float64)
    exact = np.zeros(n, np.longdouble)
    for s in range(n):
        row = points[offsets[s]:offsets[s + 1]]
        if len(row) < 2 or not np.isfinite(row).all():
            continue
        total = 0.0
        for seg in segment_lengths(row, lin, np.float64):
            total += float(seg)
        if not total < MAX_LENGTH:
            continue
        length[s] = total
        exact[s] = segment_lengths(row, lin, np.longdouble).sum()
        node[s, 0] = end_node(row[0], labels, lin, radius_mm, reach, n_nodes, mutant)
        node[s, 1] = end_node(row[-1], labels, lin, radius_mm, reach, n_nodes, mutant)
    return node, length, exact


def accumulate(node, length, n_nodes, count=None, length_q=None, mutant=None):
    """count and length_q ((N + 1, N + 1) int64), added to when given."""
    side = n_nodes + 1
    count = np.zeros((side, side), np.int64) if count is None else count
    length_q = np.zeros((side, side), np.int64) if length_q is None else length_q
    for s in range(len(node)):
        n0, n1 = int(node[s, 0]), int(node[s, 1])
        if n0 < 0:
            continue
        a, b = (n0, n1) if mutant == 'ordered_cell' else (min(n0, n1), max(n0, n1))
        count[a, b] += 1
        if length is not None:
            scaled = float(length[s]) * LENGTH_SCALE
            # numpy.rint rounds half to even, like llrint in the default mode
            length_q[a, b] += int(math.trunc(scaled)) if mutant == 'length_truncated' \
                else int(np.rint(scaled))
    return count, length_q


def accumulate_fast(node, length, n_nodes):
    """``accumulate`` for the long launches: the same sums by numpy.add.at."""
    side = n_nodes + 1
    node = np.asarray(node)
    keep = node[:, 0] >= 0
    a, b = node[keep].min(axis=1), node[keep].max(axis=1)
    count = np.zeros((side, side), np.int64)
    length_q = np.zeros((side, side), np.int64)
    np.add.at(count, (a, b), 1)
    if length is not None:
        np.add.at(length_q, (a, b),
                  np.rint(np.asarray(length, np.float64)[keep] * LENGTH_SCALE).astype(np.int64))
    return count, length_q
