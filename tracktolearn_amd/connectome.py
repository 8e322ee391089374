"""Structural connectome: the parcellation x parcellation matrices of a
tractogram, on the GPU.

``ttl_connectome_assign`` names the node of a label image at either end of
every streamline (the end's own voxel, or the nearest labelled voxel centre
within ``radius_mm``) and measures its length in mm; ``ttl_connectome_accumulate``
adds the rows into two integer matrices with device atomics (include/ttl_hip.h
states both).  Every matrix is an integer sum, so the connectome of a
tractogram does not depend on the batch split or on the order of arrival:

    con = Connectome('labels.nii.gz', None, radius_mm=2.0)
    con.add_tractogram('tracts.trk')            # or Tracker(..., connectome=con)
    con.matrices()['count']                     # (N, N) int64, symmetric

With ``metrics={'fa': fa_volume}`` every edge also gets the mean of that scalar
map along its streamlines: ``ttl_tract_sample_mean`` samples the
volume trilinearly at every point and takes the arc-length weighted mean per
streamline, ``ttl_connectome_accumulate_metric`` sums those means per edge in
fixed point, and ``matrices()`` gains ``mean_fa`` and ``fa_n``.  That is one more
pass over the points per metric.

There is no NumPy fallback: like the rest of the product path this needs the
library.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from tracktolearn_amd import _lib

MAX_NODES = _lib.CONNECTOME_MAX_NODES
MAX_REACH = _lib.CONNECTOME_MAX_REACH
LENGTH_SCALE = _lib.CONNECTOME_LENGTH_SCALE


def reach_for(lin, radius_mm):
    """reach_i = ceil(radius_mm * ||row i of inv(lin)||_2): the extent along voxel
    axis i of the ball of ``radius_mm`` mm, (3,) int32.  ValueError above
    ``MAX_REACH``, naming the largest radius this voxel size allows."""
    lin = np.asarray(lin, np.float64).reshape(3, 3)
    radius_mm = float(radius_mm)
    if not np.isfinite(radius_mm) or radius_mm < 0:
        raise ValueError(f'radius_mm must be finite and >= 0, not {radius_mm!r}')
    rows = np.sqrt((np.linalg.inv(lin) ** 2).sum(axis=1))
    reach = np.ceil(radius_mm * rows)
    if reach.max() > MAX_REACH:
        raise ValueError(f'radius_mm = {radius_mm:g} reaches {int(reach.max())} voxels, more '
                         f'than the {MAX_REACH} the search covers: the largest radius for this '
                         f'voxel size is {MAX_REACH / rows.max():g} mm')
    return reach.astype(np.int32)


def assign_nodes(points, offsets, labels_dev, dims, lin, radius_mm, n_nodes):
    """``ttl_connectome_assign`` on device tensors: (node (n, 2) int32, length
    (n,) float64) of the ragged rows ``points`` (M, 3) float32 / ``offsets``
    (n + 1,) int64 in corner-origin voxel coordinates of the label grid;
    ``labels_dev`` (X * Y * Z,) int32 on the same device, ``lin`` the (3, 3)
    linear part of voxel -> RAS mm."""
    from tracktolearn_amd.experiment.oracle_validator import launch_ragged
    n = max(int(offsets.shape[0]) - 1, 0)
    dev = points.device
    node = torch.empty((n, 2), dtype=torch.int32, device=dev)
    length = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0 or points.shape[0] == 0:      # no launch: an empty tensor has no pointer
        return node.fill_(-1), length.zero_()
    lin = np.ascontiguousarray(np.asarray(lin, np.float64).reshape(9))
    reach = reach_for(lin, radius_mm)
    if labels_dev.dtype != torch.int32 or not labels_dev.is_contiguous() or \
            labels_dev.numel() != int(dims[0]) * int(dims[1]) * int(dims[2]):
        raise ValueError('labels_dev must be a contiguous int32 tensor of X * Y * Z words')
    launch_ragged('ttl_connectome_assign', points, offsets, dims,
                  before=(labels_dev.data_ptr(),),
                  after=(int(n_nodes), _lib.lin9(lin), float(radius_mm),
                         (C.c_int32 * 3)(*(int(r) for r in reach)), node.data_ptr(),
                         length.data_ptr()))
    return node, length


def accumulate(node, length, n_nodes, count, length_q):
    """``ttl_connectome_accumulate``: the rows of ``node`` (n, 2) int32 and
    ``length`` (n,) float64 or None added into ``count`` and ``length_q``
    ((N + 1, N + 1) int64, device), on the current stream of their device."""
    dev = node.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_connectome_accumulate(
            node.data_ptr(), None if length is None else length.data_ptr(),
            int(node.shape[0]), int(n_nodes), count.data_ptr(), length_q.data_ptr(),
            _lib.stream_of(dev)), 'ttl_connectome_accumulate')


def _lin_of(affine):
    a = np.asarray(affine, np.float64)
    if a.shape == (4, 4):
        a = a[:3, :3]
    return np.ascontiguousarray(a.reshape(9))


def sample_mean(points, offsets, volume, affine):
    """``ttl_tract_sample_mean`` on device tensors: (mean, weight), each (n,)
    float64, of the ragged rows ``points`` (M, 3) float32 / ``offsets`` (n + 1,)
    int64 in corner-origin voxel coordinates of the grid of ``volume`` (an
    (X, Y, Z) float32 tensor on the device of ``points``; an array is uploaded).
    ``affine``: the (4, 4) voxel -> RAS mm of that grid, or its (3, 3) linear
    part.  mean: the trapezoid-rule mean over the arc length in mm of the
    trilinear samples; NaN (and weight 0) for a row without one."""
    from tracktolearn_amd.experiment.oracle_validator import launch_ragged
    n = max(int(offsets.shape[0]) - 1, 0)
    dev = points.device
    if not torch.is_tensor(volume):
        volume = torch.from_numpy(np.ascontiguousarray(np.asarray(volume, np.float32))).to(dev)
    if volume.dim() != 3 or volume.numel() == 0:
        raise ValueError(f'a scalar map is a 3-D volume, not of shape {tuple(volume.shape)}')
    if volume.dtype != torch.float32 or not volume.is_contiguous() or volume.device != dev:
        raise ValueError('volume must be a contiguous float32 tensor on the device of points')
    mean = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
    weight = torch.zeros(n, dtype=torch.float64, device=dev)
    if n == 0 or points.shape[0] == 0:      # no launch: an empty tensor has no pointer
        return mean, weight
    launch_ragged('ttl_tract_sample_mean', points, offsets, volume.shape,
                  before=(volume.data_ptr(),),
                  after=(_lib.lin9(_lin_of(affine)), mean.data_ptr(),
                         weight.data_ptr()))
    return mean, weight


def accumulate_metric(node, mean, n_nodes, scale, metric_q, metric_n):
    """``ttl_connectome_accumulate_metric``: llrint(mean * scale) of the scored
    rows with a finite mean added into ``metric_q``, and 1 into ``metric_n``
    ((N + 1, N + 1) int64, device), on the current stream of their device."""
    dev = node.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_connectome_accumulate_metric(
            node.data_ptr(), mean.data_ptr(), int(node.shape[0]), int(n_nodes), float(scale),
            metric_q.data_ptr(), metric_n.data_ptr(), _lib.stream_of(dev)),
            'ttl_connectome_accumulate_metric')


def metric_scale(volume):
    """The fixed-point scale of a metric volume (float32, as uploaded): with m the
    largest finite |value| (1 for an all-zero or all-NaN volume) and e the smallest
    integer with m < 2^e, 2^(39 - e): |mean| * scale < 2^40, and 2^23 streamlines
    fit in a cell.  The exponent is held to the -60 .. 60 the library takes."""
    v = np.abs(np.asarray(volume, np.float32).astype(np.float64))
    v = v[np.isfinite(v)]
    m = float(v.max()) if v.size and v.max() > 0 else 1.0
    e = math.frexp(m)[1]                # m = f * 2^e with 0.5 <= f < 1
    return 2.0 ** min(max(39 - e, -60), 60)


def metric_matrices_from(metric_q_upper, metric_n_upper, scale):
    """(mean (N, N) float64, symmetric, NaN where no streamline contributed; n
    (N, N) int64) of the two accumulated matrices of one metric."""
    def symmetric(m):
        inner = np.asarray(m, np.int64)[1:, 1:]
        return inner + inner.T - np.diag(np.diag(inner))
    q, n = symmetric(metric_q_upper), symmetric(metric_n_upper)
    mean = np.full(q.shape, np.nan)
    np.divide(q.astype(np.float64) / scale, n, out=mean, where=n > 0)
    return mean, n


def check_metrics(metrics, dims):
    """name -> contiguous (X, Y, Z) float32 array of the ``metrics`` argument of
    ``Connectome``: ValueError for an empty name, one with ``=`` (the commands
    split NAME=FILE there) or a volume that is not of the labels' shape."""
    out = {}
    for name, volume in (metrics or {}).items():
        if not isinstance(name, str) or not name or '=' in name:
            raise ValueError(f'a metric name is a non-empty string without "=", not {name!r}')
        data = np.asarray(volume)
        if data.shape != tuple(dims):
            raise ValueError(f'metric {name} has shape {data.shape}, the label image '
                             f'{tuple(dims)}: there is no resampling')
        out[name] = np.ascontiguousarray(data.astype(np.float32))
    return out


def parse_metric(text):
    """(name, file) of a ``NAME=FILE`` option; ValueError otherwise."""
    name, eq, filename = str(text).partition('=')
    if not eq or not name or not filename:
        raise ValueError(f'{text!r}: a metric is given as NAME=FILE')
    return name, filename


def load_metric(name, filename, shape, affine, grid_of):
    """The (X, Y, Z) float32 volume of the NIfTI ``filename``, which must be on
    the grid (``shape``, ``affine`` to 1e-3) of ``grid_of``: there is no
    resampling, and the error names both grids."""
    from tracktolearn_amd.io import nifti
    img = nifti.load(filename)
    got = tuple(int(v) for v in img.shape[:3])
    data = np.asarray(img.get_fdata(dtype=np.float64))
    if data.ndim == 4 and data.shape[3] == 1:
        data = data[..., 0]
    shape = tuple(int(v) for v in shape)
    affine = np.asarray(affine, np.float64)
    if data.ndim != 3 or got != shape or not np.allclose(img.affine, affine, atol=1e-3):
        raise ValueError(
            f'metric {name} ({filename}: shape {tuple(img.shape)}, affine '
            f'{np.asarray(img.affine).round(4).tolist()}) is not on the grid of {grid_of} '
            f'(shape {shape}, affine {affine.round(4).tolist()}): resample it')
    return data.astype(np.float32)


def matrices_from(count_upper, length_q_upper):
    """The public matrices of the two accumulated ones ((N + 1, N + 1) int64,
    upper triangle, row 0 = unassigned): ``count`` (N, N) int64, symmetric;
    ``length_sum_mm`` and ``mean_length_mm`` (N, N) float64 (sum_q / 2^20; 0
    where the count is 0); ``unassigned_one_end`` (N,) int64 and
    ``unassigned_both``."""
    u = np.asarray(count_upper, np.int64)
    q = np.asarray(length_q_upper, np.int64)

    def symmetric(m):
        inner = m[1:, 1:]
        return inner + inner.T - np.diag(np.diag(inner))
    count, sum_q = symmetric(u), symmetric(q)
    length_sum = sum_q.astype(np.float64) / LENGTH_SCALE
    mean = np.zeros_like(length_sum)
    np.divide(length_sum, count, out=mean, where=count > 0)
    return {'count': count, 'length_sum_mm': length_sum, 'mean_length_mm': mean,
            'unassigned_one_end': u[0, 1:].copy(), 'unassigned_both': int(u[0, 0])}


def load_labels(labels):
    """(labels (X, Y, Z) int32, N) of an integer array or the data of a NIfTI
    image as read: ValueError for non-integer values, N = max < 1 or N >
    ``MAX_NODES``.  Values below 1 are no node."""
    data = np.asarray(labels)
    if data.ndim == 4 and data.shape[3] == 1:
        data = data[..., 0]
    if data.ndim != 3 or data.size == 0:
        raise ValueError(f'a label image is a 3-D volume, not of shape {data.shape}')
    if not np.issubdtype(data.dtype, np.integer):
        if not np.array_equal(data, np.rint(data)):       # a NaN fails too
            raise ValueError('a label image holds integers')
    n_nodes = int(data.max())
    if n_nodes < 1:
        raise ValueError('the label image names no node (its largest value is below 1)')
    if n_nodes > MAX_NODES:
        raise ValueError(f'the label image names {n_nodes} nodes, more than {MAX_NODES}')
    # the range is known now: everything below 1 is no node, whatever the dtype (an
    # unsigned array has no -1 to compare with, an int64 one may not fit int32)
    return np.ascontiguousarray(np.where(data < 1, 0, data).astype(np.int32)), n_nodes


class Connectome:
    """``Connectome(labels, affine, radius_mm=2.0, device='cuda', metrics=None)``:
    the two device matrices of a label image and what streams into them.
    ``labels``: an integer (X, Y, Z) array or a NIfTI file name; ``affine``: the
    (4, 4) voxel -> RAS mm of its grid (None: the file's own).  ``metrics``: a
    dict of name -> scalar map, a 3-D array on the labels' grid, uploaded once as
    float32; each adds two matrices and one sampling pass over the points of
    every ``add``."""

    def __init__(self, labels, affine, radius_mm=2.0, device='cuda', metrics=None):
        if isinstance(labels, (str, bytes, os.PathLike)):
            from tracktolearn_amd.io import nifti
            img = nifti.load(os.fsdecode(labels))
            if affine is None:
                affine = img.affine
            labels = img.get_fdata(dtype=np.float64)
        if affine is None:
            raise ValueError('an array of labels needs the affine of its grid')
        data, self.n_nodes = load_labels(labels)
        self.dims = tuple(int(v) for v in data.shape)
        self.affine = np.asarray(affine, np.float64).reshape(4, 4)
        self.lin = np.ascontiguousarray(self.affine[:3, :3])
        self.radius_mm = float(radius_mm)
        self.reach = reach_for(self.lin, self.radius_mm)
        volumes = check_metrics(metrics, self.dims)
        _lib.load()
        self.device = torch.device(device)
        self.labels = torch.from_numpy(data.reshape(-1)).to(self.device)
        side = self.n_nodes + 1
        self.count = torch.zeros((side, side), dtype=torch.int64, device=self.device)
        self.length_q = torch.zeros((side, side), dtype=torch.int64, device=self.device)
        self._skipped = torch.zeros((), dtype=torch.int64, device=self.device)
        self._dropped = 0           # rows the intake left out (fewer than 2 points)
        #: name -> {'volume': (X, Y, Z) float32 on the device, 'scale', 'q', 'n'}
        self.metrics = {}
        #: name -> (mean, weight) per row of the latest ``add``
        self.last_means = {}
        for name, data in volumes.items():
            self.metrics[name] = {
                'volume': torch.from_numpy(data).to(self.device), 'scale': metric_scale(data),
                'q': torch.zeros((side, side), dtype=torch.int64, device=self.device),
                'n': torch.zeros((side, side), dtype=torch.int64, device=self.device)}

    def add(self, points, offsets):
        """Device tensors in corner-origin voxel coordinates of the label
        grid: assign, then accumulate; then, per metric, sample and accumulate
        (one more pass over the points each).  Returns ``node`` (n, 2) int32."""
        node, length = assign_nodes(points, offsets, self.labels, self.dims, self.lin,
                                    self.radius_mm, self.n_nodes)
        if node.shape[0]:
            accumulate(node, length, self.n_nodes, self.count, self.length_q)
            self._skipped += (node[:, 0] < 0).sum()
        for name, m in self.metrics.items():
            mean, weight = sample_mean(points, offsets, m['volume'], self.lin)
            if node.shape[0]:
                accumulate_metric(node, mean, self.n_nodes, m['scale'], m['q'], m['n'])
            self.last_means[name] = (mean, weight)
        return node

    def add_tractogram(self, tractogram_or_filename, env=None, in_rasmm=False):
        """A .trk / .tck file, or the tracker's in-memory tractogram (voxel
        coordinates of ``env``; ``in_rasmm``: one that ``load_tractogram``
        read), through the validators' one intake.  Returns (node (n, 2) int32
        on the device, index (n,) int64: the rows' numbers in the input)."""
        from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                                  load_tractogram)
        from tracktolearn_amd.tractogram import Tractogram
        source = tractogram_or_filename
        if isinstance(source, FILENAME):
            # read here, not by the intake: ``skipped`` needs the file's row count, which
            # the intake's ``index`` (the rows it kept) does not tell
            source, in_rasmm = load_tractogram(source)[0], True
        lines = source.streamlines if isinstance(source, Tractogram) else source
        points, offsets, index = corner_voxels(
            source, self.affine, getattr(env, 'affine_vox2rasmm', None), in_rasmm=in_rasmm)
        self._dropped += len(lines) - len(index)
        node = self.add(torch.from_numpy(points).to(self.device),
                        torch.from_numpy(offsets).to(self.device))
        return node, index

    @property
    def skipped(self):
        """The number of rows not scored: fewer than 2 points, a non-finite
        point, a length of 2^40 mm or more."""
        return int(self._skipped.item()) + self._dropped

    def matrices(self):
        """``matrices_from`` and, per metric, ``mean_<name>`` ((N, N) float64,
        symmetric: the mean over an edge's streamlines of their means, NaN where
        none contributed) and ``<name>_n`` (how many did)."""
        out = matrices_from(self.count.cpu().numpy(), self.length_q.cpu().numpy())
        for name, m in self.metrics.items():
            out['mean_' + name], out[name + '_n'] = metric_matrices_from(
                m['q'].cpu().numpy(), m['n'].cpu().numpy(), m['scale'])
        return out

    def totals(self):
        """What ``prefix.json`` holds."""
        m = self.matrices()
        scored = int(np.triu(m['count']).sum() + m['unassigned_one_end'].sum()
                     + m['unassigned_both'])
        out = {'n_nodes': self.n_nodes, 'radius_mm': self.radius_mm,
               'reach': [int(r) for r in self.reach], 'streamlines': scored + self.skipped,
               'scored': scored, 'skipped': self.skipped,
               'connected': int(np.triu(m['count']).sum()),
               'unassigned_one_end': int(m['unassigned_one_end'].sum()),
               'unassigned_both': m['unassigned_both']}
        if self.metrics:
            out['metrics'] = {name: {'scale': v['scale']} for name, v in self.metrics.items()}
        return out

    def save(self, prefix):
        """``prefix_count.npy``, ``prefix_mean_length.npy``, ``prefix_count.csv``
        and ``prefix.json`` (the totals, radius and node count; the metrics' names
        and scales); per metric ``prefix_mean_<name>.npy``."""
        m = self.matrices()
        folder = os.path.dirname(os.path.abspath(prefix))
        os.makedirs(folder, exist_ok=True)
        np.save(prefix + '_count.npy', m['count'])
        np.save(prefix + '_mean_length.npy', m['mean_length_mm'])
        np.savetxt(prefix + '_count.csv', m['count'], fmt='%d', delimiter=',')
        with open(prefix + '.json', 'w') as f:
            json.dump(self.totals(), f, indent=2)
        for name in self.metrics:
            np.save(f'{prefix}_mean_{name}.npy', m['mean_' + name])
        return [prefix + s for s in ('_count.npy', '_mean_length.npy', '_count.csv', '.json')] \
            + [f'{prefix}_mean_{name}.npy' for name in self.metrics]


__all__ = ['Connectome', 'assign_nodes', 'accumulate', 'sample_mean', 'accumulate_metric',
           'metric_scale', 'metric_matrices_from', 'check_metrics', 'parse_metric',
           'load_metric', 'reach_for', 'matrices_from', 'load_labels', 'MAX_NODES', 'MAX_REACH',
           'LENGTH_SCALE']
