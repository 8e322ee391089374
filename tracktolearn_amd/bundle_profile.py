"""Bundle profiles: orient, centroid and along-tract statistics, on the GPU
(DESIGN 3.18).

A tract profile is the mean and the spread of a scalar map (FA, MD, AFD) at K
stations along a bundle: AFQ's tractometry, ``scil_bundle_mean_std
--per_point``.  ``ttl_bundle_orient`` resamples every streamline of a bundle to
K stations (the library's one resampler), orients it against the bundle's
model line and sums the oriented stations into the centroid;
``ttl_bundle_profile`` samples a volume at the oriented stations and sums value
and square per station (include/ttl_hip.h states both).  Every sum is an
integer, so the result does not depend on the batch split, the order of
arrival or the sorting by bundle:

    prof = BundleProfiles('fa.nii.gz', None, ['CST_L', 'CST_R'], nb_points=100)
    prof.add_tractogram('bundles.trk', bundle_ids)     # or prof.fit(points, offsets, bundle)
    prof.add_metric('fa', fa_volume)
    prof.profiles()['CST_L']['fa']['mean']             # K floats
    prof.save('out/profile')

The stations are equidistant in arc length in VOXEL units (the resampler's
bits): on an anisotropic grid they are not equidistant in mm.  There is no
NumPy fallback: like the rest of the product path this needs the library.
"""
import ctypes as C
import json
import math
import os
import warnings

import numpy as np
import torch

from tracktolearn_amd import _lib

MAX_POINTS = _lib.PROFILE_MAX_POINTS
MAX_BUNDLES = _lib.PROFILE_MAX_BUNDLES
#: a seed model is a row of at most this many points (the padded resampler keeps
#: a row's cumulative arc length in LDS)
SEED_MAX_POINTS = 4096


def _is_scale(scale):
    if not (isinstance(scale, (int, float)) and math.isfinite(scale) and scale > 0):
        return False
    m, e = math.frexp(scale)
    return m == 0.5 and -60 <= e - 1 <= 60


def _check_rows(points, offsets, bundle, n_bundles, nb_points):
    n = _lib.ragged_rows(points, offsets)
    if not (torch.is_tensor(bundle) and bundle.dtype == torch.int32 and bundle.is_contiguous() and
            tuple(bundle.shape) == (n,) and bundle.device == points.device):
        raise ValueError(f'bundle must be a contiguous ({n},) int32 tensor on the device of points')
    if not 1 <= int(n_bundles) <= MAX_BUNDLES:
        raise ValueError(f'n_bundles must be in 1 .. {MAX_BUNDLES}, not {n_bundles}')
    if not 2 <= int(nb_points) <= MAX_POINTS:
        raise ValueError(f'nb_points must be in 2 .. {MAX_POINTS}, not {nb_points}')
    return n


def _check_sum(name, t, shape, dev, dtype=torch.int64):
    if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and
            t.is_contiguous() and t.device == dev):
        raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on '
                         'the device of points')


def bundle_orient(points, offsets, bundle, n_bundles, nb_points, model, lin, scale, sum_q, sum_n):
    """``ttl_bundle_orient`` on device tensors: the ragged rows ``points`` (P, 3)
    float32 / ``offsets`` (n + 1,) int64 with their bundle numbers ``bundle``
    (n,) int32, oriented against ``model`` (B, K, 3) float32; the oriented
    stations are added into ``sum_q`` (B, K, 3) int64 at the power of two
    ``scale`` and the rows into ``sum_n`` (B,) int64.  ``lin``: the (3, 3) linear
    part of voxel -> RAS mm.  Returns (flip (n,) int32, mdf (n,) float64)."""
    n = _check_rows(points, offsets, bundle, n_bundles, nb_points)
    B, K, dev = int(n_bundles), int(nb_points), points.device
    _check_sum('model', model, (B, K, 3), dev, torch.float32)
    _check_sum('sum_q', sum_q, (B, K, 3), dev)
    _check_sum('sum_n', sum_n, (B,), dev)
    if not _is_scale(scale):
        raise ValueError(f'scale must be a power of two in 2^-60 .. 2^60, not {scale!r}')
    lin_c = _lib.lin9(lin)
    flip = torch.zeros(n, dtype=torch.int32, device=dev)
    mdf = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
    if n == 0 or points.shape[0] == 0:      # no launch: an empty tensor has no pointer
        return flip, mdf
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_bundle_orient(
            points.data_ptr(), offsets.data_ptr(), n, bundle.data_ptr(), B, K, model.data_ptr(),
            lin_c, float(scale), flip.data_ptr(), mdf.data_ptr(), sum_q.data_ptr(),
            sum_n.data_ptr(), _lib.stream_of(dev)), 'ttl_bundle_orient')
    return flip, mdf


def bundle_profile(points, offsets, bundle, flip, n_bundles, nb_points, volume, scale, scale_sq,
                   sum_q, sum_qq, count, values=False):
    """``ttl_bundle_profile`` on device tensors: ``volume`` (X, Y, Z) float32
    sampled at the K stations of every row, reversed where ``flip`` (n,) int32
    is not 0; value, square and 1 are added into ``sum_q``, ``sum_qq`` and
    ``count`` ((B, K) int64) at the powers of two ``scale`` / ``scale_sq``.
    ``values``: also return the (n, K) float64 samples (NaN where not sampled);
    None otherwise."""
    n = _check_rows(points, offsets, bundle, n_bundles, nb_points)
    B, K, dev = int(n_bundles), int(nb_points), points.device
    _check_sum('flip', flip, (n,), dev, torch.int32)
    if not (torch.is_tensor(volume) and volume.dtype == torch.float32 and volume.dim() == 3 and
            volume.numel() > 0 and volume.is_contiguous() and volume.device == dev):
        raise ValueError('volume must be a contiguous (X, Y, Z) float32 tensor on the device of '
                         'points')
    for name, t in (('sum_q', sum_q), ('sum_qq', sum_qq), ('count', count)):
        _check_sum(name, t, (B, K), dev)
    if not (_is_scale(scale) and _is_scale(scale_sq)):
        raise ValueError('scale and scale_sq must be powers of two in 2^-60 .. 2^60, not '
                         f'{scale!r}, {scale_sq!r}')
    out = torch.full((n, K), float('nan'), dtype=torch.float64, device=dev) if values else None
    if n == 0 or points.shape[0] == 0:
        return out
    dims_c = (C.c_int32 * 3)(*(int(v) for v in volume.shape))
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_bundle_profile(
            points.data_ptr(), offsets.data_ptr(), n, bundle.data_ptr(), flip.data_ptr(), B, K,
            volume.data_ptr(), dims_c, float(scale), float(scale_sq), sum_q.data_ptr(),
            sum_qq.data_ptr(), count.data_ptr(), out.data_ptr() if values else None,
            _lib.stream_of(dev)), 'ttl_bundle_profile')
    return out


def coordinate_scale(dims):
    """The fixed-point scale of station coordinates on a grid: with e the
    smallest integer with max(dims) < 2^e, 2^(37 - e).  Coordinates up to 8 times
    the grid pass the library's 2^40 gate and 2^23 rows fit in an int64 sum."""
    e = math.frexp(float(max(int(v) for v in dims)))[1]
    return 2.0 ** (37 - e)


def metric_scales(volume):
    """(scale, scale_sq) of a metric volume, chosen as ``connectome.metric_scale``
    chooses its scale: from the largest finite |value| m, |v| * scale < 2^40 and
    v^2 * scale_sq < 2^40, both exponents held to -60 .. 60."""
    from tracktolearn_amd.connectome import metric_scale
    scale = metric_scale(volume)
    e = 39 - int(round(math.log2(scale)))               # m < 2^e
    return scale, 2.0 ** min(max(39 - 2 * e, -60), 60)


def canonical_reverse(centroid, lin):
    """Whether a centroid ((K, 3), voxel coordinates) runs against the RAS
    convention: with e = lin (c_{K-1} - c_0), the component of largest |e| (the
    lower axis on a tie) must be positive -- L -> R, P -> A, I -> S.  False for a
    centroid with a non-finite end."""
    c = np.asarray(centroid, np.float64)
    e = np.asarray(lin, np.float64).reshape(3, 3) @ (c[-1] - c[0])
    if not np.all(np.isfinite(e)):
        return False
    return bool(e[int(np.argmax(np.abs(e)))] <= 0.0)


def mdf_gate(bundle, mdf, max_mdf):
    """The bundle numbers of the profile pass: -1 for the rows further than
    ``max_mdf`` mm from their model (None: no gate), and how many rows of each
    bundle that leaves out.  NumPy arrays or tensors; a NaN distance is no
    outlier (such a row takes no part anyway)."""
    tensor = torch.is_tensor(bundle)
    b = bundle.cpu().numpy() if tensor else np.asarray(bundle)
    d = mdf.cpu().numpy() if torch.is_tensor(mdf) else np.asarray(mdf, np.float64)
    out = np.array(b, np.int32)
    if max_mdf is not None:
        out[d > float(max_mdf)] = -1
    gone = b[(out != b) & (b >= 0)]
    counts = np.bincount(gone, minlength=int(b.max()) + 1 if b.size else 0)
    return (torch.from_numpy(out).to(bundle.device) if tensor else out), counts


def json_ready(value):
    """``value`` (nested dicts, lists, numbers) with every non-finite float
    replaced by None: strict JSON has no NaN, ``json.dump`` writes null."""
    if isinstance(value, dict):
        return {k: json_ready(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [json_ready(v) for v in value]
    if isinstance(value, float) and not math.isfinite(value):
        return None
    return value


class BundleProfiles:
    """``BundleProfiles(dims_or_reference_nifti, affine, bundle_names,
    nb_points=100, device='cuda', n_iter=2, max_mdf=None, model=None)``: the
    centroids and profiles of the bundles of a segmented tractogram.
    ``dims_or_reference_nifti``: (X, Y, Z) of the grid, or a NIfTI file on it;
    ``affine``: its (4, 4) voxel -> RAS mm (None: the file's own).  ``fit``
    orients the rows and computes the centroids, ``add_metric`` the profile of
    one scalar map on the grid.  ``model`` ((B, K, 3), corner-origin voxel
    coordinates): the model lines to orient against, instead of seeding them
    from the rows; it is never updated, so ``fit`` runs one pass with it
    whatever ``n_iter`` says (batches of a stream agree on it).  ``max_mdf`` (mm): rows whose ``mdf``
    of the last pass -- the distance to the model THAT pass oriented against: the
    centroid of the pass before or the given model, not the centroid the pass
    itself produces -- exceeds it are left out of the profiles."""

    def __init__(self, dims_or_reference_nifti, affine, bundle_names, nb_points=100,
                 device='cuda', n_iter=2, max_mdf=None, model=None):
        from tracktolearn_amd.density import check_dims
        ref = dims_or_reference_nifti
        if isinstance(ref, (str, bytes, os.PathLike)):
            from tracktolearn_amd.io import nifti
            img = nifti.load(os.fsdecode(ref))
            if affine is None:
                affine = img.affine
            ref = tuple(int(v) for v in img.shape[:3])
        if affine is None:
            raise ValueError('dims need the affine of their grid')
        self.dims = check_dims(ref)
        self.affine = np.asarray(affine, np.float64).reshape(4, 4)
        self.lin = np.ascontiguousarray(self.affine[:3, :3])
        self.names = [str(v) for v in bundle_names]
        self.B, self.K = len(self.names), int(nb_points)
        if not 1 <= self.B <= MAX_BUNDLES or len(set(self.names)) != self.B:
            raise ValueError(f'1 .. {MAX_BUNDLES} distinct bundle names, not {self.names}')
        if not 2 <= self.K <= MAX_POINTS:
            raise ValueError(f'nb_points must be in 2 .. {MAX_POINTS}, not {nb_points}')
        self.n_iter = int(n_iter)
        if model is None and self.n_iter < 2:
            raise ValueError('n_iter must be >= 2 without a model: a seed row is no centroid')
        if self.n_iter < 1:
            raise ValueError('n_iter must be >= 1')
        if model is not None:
            self.n_iter = 1         # a given model is never updated: more passes repeat the first
        self.max_mdf = None if max_mdf is None else float(max_mdf)
        self.user_model = None
        if model is not None:
            self.user_model = np.ascontiguousarray(np.asarray(model, np.float32))
            if self.user_model.shape != (self.B, self.K, 3):
                raise ValueError(f'model must have shape {(self.B, self.K, 3)}, not '
                                 f'{self.user_model.shape}')
        _lib.load()
        self.device = torch.device(device)
        self.scale = coordinate_scale(self.dims)
        self.metrics = {}
        self._rows = None
        self._dropped = 0

    # -- fit -------------------------------------------------------------
    def _seed_model(self, points, offsets, bundle):
        """(B, K, 3) float32: per bundle its first row that takes part (of at most
        SEED_MAX_POINTS points), resampled by ``ttl_resample_streamlines``; NaN for
        a bundle without one."""
        from tracktolearn_amd.density import gather_rows
        from tracktolearn_amd.oracles.oracle import resample_streamlines
        n, dev = bundle.shape[0], points.device
        lens = offsets[1:] - offsets[:-1]
        ok_pt = torch.isfinite(points).all(1) & \
            ((points.double().abs() * self.scale).amax(1) < 2.0 ** 40)
        bad = torch.zeros(points.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum((~ok_pt).to(torch.int64), 0, out=bad[1:])
        ok = (lens >= 2) & (lens <= SEED_MAX_POINTS) & (bad[offsets[1:]] == bad[offsets[:-1]]) & \
            (bundle >= 0) & (bundle < self.B)
        first = torch.full((self.B,), n, dtype=torch.int64, device=dev)
        rows = torch.nonzero(ok).squeeze(1)
        first.scatter_reduce_(0, bundle[rows].to(torch.int64), rows, 'amin')
        first = first.cpu().numpy()
        unseeded = np.flatnonzero((first == n) & (np.bincount(
            bundle[(bundle >= 0) & (bundle < self.B)].cpu().numpy(), minlength=self.B) > 0))
        if unseeded.size:
            warnings.warn('no seed model for ' + ', '.join(self.names[b] for b in unseeded) +
                          f': no row takes part with at most {SEED_MAX_POINTS} points; the first '
                          'pass sums these bundles unoriented (give a model)')
        model = torch.full((self.B, self.K, 3), float('nan'), dtype=torch.float32, device=dev)
        have = np.flatnonzero(first < n)
        if have.size:
            seeds = torch.from_numpy(first[have]).to(dev)
            pts, off = gather_rows(points, offsets, seeds)
            seed_len = off[1:] - off[:-1]
            longest = int(seed_len.max().item())
            pad = torch.zeros((have.size, longest, 3), dtype=torch.float32, device=dev)
            owner = torch.repeat_interleave(torch.arange(have.size, device=dev), seed_len)
            pad[owner, torch.arange(pts.shape[0], device=dev) - off[:-1][owner]] = pts
            model[torch.from_numpy(have).to(dev)] = resample_streamlines(pad, seed_len, self.K)
        return model

    def _canonical(self, lines):
        """``lines`` (B, K, 3) float64 with every line that runs against the RAS
        convention reversed, and which ones were."""
        turned = np.array([canonical_reverse(c, self.lin) for c in lines], bool)
        out = np.array(lines, np.float64)
        out[turned] = out[turned, ::-1]
        return out, turned

    def fit(self, points, offsets, bundle):
        """Device tensors: the ragged rows in corner-origin voxel coordinates of
        the grid and their bundle numbers (n,) (-1, or a number >= B: in no
        bundle).  Sorts the rows by bundle, then ``n_iter`` passes of orient ->
        centroid -> canonical direction -> next model.  Keeps the last pass's
        ``flip`` and ``mdf`` per row (input order)."""
        from tracktolearn_amd.density import gather_rows
        dev = self.device
        points = points.to(dev, torch.float32).contiguous()
        offsets = offsets.to(dev, torch.int64).contiguous()
        bundle = bundle.to(dev, torch.int32).contiguous()
        n = _check_rows(points, offsets, bundle, self.B, self.K)
        order = torch.argsort(bundle, stable=True)
        if n:
            points, offsets = gather_rows(points, offsets, order)
            points = points.contiguous()
        bundle = bundle[order].contiguous()
        if self.user_model is not None:
            model = torch.from_numpy(self.user_model).to(dev)
        elif n and points.shape[0]:
            seed = self._seed_model(points, offsets, bundle).cpu().numpy()
            model = torch.from_numpy(self._canonical(seed)[0].astype(np.float32)).to(dev)
        else:
            model = torch.full((self.B, self.K, 3), float('nan'), dtype=torch.float32, device=dev)
        for _ in range(self.n_iter):
            sum_q = torch.zeros((self.B, self.K, 3), dtype=torch.int64, device=dev)
            sum_n = torch.zeros(self.B, dtype=torch.int64, device=dev)
            flip, mdf = bundle_orient(points, offsets, bundle, self.B, self.K, model, self.lin,
                                      self.scale, sum_q, sum_n)
            count = sum_n.cpu().numpy()
            with np.errstate(invalid='ignore', divide='ignore'):
                centroid = sum_q.cpu().numpy().astype(np.float64) / self.scale / \
                    count[:, None, None]
            centroid[count == 0] = np.nan
            centroid, turned = self._canonical(centroid)
            if self.user_model is None:
                model = torch.from_numpy(centroid.astype(np.float32)).to(dev)
        if self.user_model is not None:
            # the model states the direction: the centroid is kept as the rows were summed
            centroid[turned] = centroid[turned, ::-1]
        elif turned.any():
            # the last centroid was reversed: so are the rows that made it
            rev = torch.from_numpy(turned).to(dev)
            took = ~torch.isnan(mdf) & (bundle >= 0) & (bundle < self.B)
            took &= rev[bundle.clamp(0, self.B - 1).to(torch.int64)]
            flip = torch.where(took, 1 - flip, flip).contiguous()
        gated, outliers = mdf_gate(bundle, mdf, self.max_mdf)
        self._rows = {'points': points, 'offsets': offsets, 'bundle': bundle,
                      'gated': gated.contiguous(), 'flip': flip, 'mdf': mdf, 'order': order}
        self.centroids_vox = centroid
        self.n = count
        self.n_outliers = np.zeros(self.B, np.int64)
        self.n_outliers[:min(len(outliers), self.B)] = outliers[:self.B]
        # mdf_mean: over every row that took part, the max_mdf outliers included
        took = ~torch.isnan(mdf) & (bundle >= 0) & (bundle < self.B)
        total = torch.zeros(self.B, dtype=torch.float64, device=dev)
        total.index_add_(0, bundle[took].to(torch.int64), mdf[took])
        with np.errstate(invalid='ignore', divide='ignore'):
            self.mdf_mean = total.cpu().numpy() / count
        self.metrics = {}
        return self

    def _unsorted(self, t):
        out = torch.empty_like(t)
        out[self._rows['order']] = t
        return out

    @property
    def flip(self):
        """(n,) int32, input order: 1 where the row is read backwards."""
        return self._unsorted(self._rows['flip'])

    @property
    def mdf(self):
        """(n,) float64, input order: the mean distance to the model in mm."""
        return self._unsorted(self._rows['mdf'])

    def add_tractogram(self, file_or_tractogram, bundle, env=None, in_rasmm=False):
        """A .trk / .tck file, or the tracker's in-memory tractogram (voxel
        coordinates of ``env``), through the validators' one intake; ``bundle``:
        the bundle number of every streamline of the input.  Returns the index
        (n,) int64 of the rows taken, and fits them."""
        from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                                  load_tractogram)
        from tracktolearn_amd.tractogram import Tractogram
        source = file_or_tractogram
        if isinstance(source, FILENAME):
            source, in_rasmm = load_tractogram(source)[0], True
        lines = source.streamlines if isinstance(source, Tractogram) else source
        bundle = np.asarray(bundle.cpu() if torch.is_tensor(bundle) else bundle)
        if bundle.shape != (len(lines),):
            raise ValueError(f'{len(lines)} streamlines need as many bundle numbers, not '
                             f'{bundle.shape}')
        points, offsets, index = corner_voxels(
            source, self.affine, getattr(env, 'affine_vox2rasmm', None), in_rasmm=in_rasmm)
        self._dropped = len(lines) - len(index)
        self.fit(torch.from_numpy(points), torch.from_numpy(offsets),
                 torch.from_numpy(bundle[index].astype(np.int32)))
        return index

    # -- profiles --------------------------------------------------------
    def add_metric(self, name, volume, per_streamline=False):
        """The profile pass of one scalar map on the grid ((X, Y, Z); another
        shape is refused: there is no resampling)."""
        if self._rows is None:
            raise ValueError('fit() comes before add_metric()')
        if not isinstance(name, str) or not name or '=' in name:
            raise ValueError(f'a metric name is a non-empty string without "=", not {name!r}')
        data = np.ascontiguousarray(np.asarray(volume.cpu() if torch.is_tensor(volume) else volume,
                                               dtype=np.float32))
        if data.shape != self.dims:
            raise ValueError(f'metric {name} has shape {data.shape}, the grid {self.dims}: '
                             'there is no resampling')
        scale, scale_sq = metric_scales(data)
        dev, r = self.device, self._rows
        sums = [torch.zeros((self.B, self.K), dtype=torch.int64, device=dev) for _ in range(3)]
        values = bundle_profile(r['points'], r['offsets'], r['gated'], r['flip'], self.B, self.K,
                                torch.from_numpy(data).to(dev), scale, scale_sq, *sums,
                                values=per_streamline)
        q, qq, count = (s.cpu().numpy() for s in sums)
        self.metrics[name] = {'sum_q': q, 'sum_qq': qq, 'count': count, 'scale': scale,
                              'scale_sq': scale_sq,
                              'values': None if values is None else
                              self._unsorted(values).cpu().numpy()}
        return self

    @staticmethod
    def statistics(sum_q, sum_qq, count, scale, scale_sq):
        """(mean, std) per station: mean = sum_q / scale / count, std =
        sqrt(max(sum_qq / scale_sq / count - mean^2, 0)); NaN at count 0."""
        count = np.asarray(count, np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = np.asarray(sum_q, np.float64) / scale / count
            var = np.asarray(sum_qq, np.float64) / scale_sq / count - mean * mean
            std = np.sqrt(np.maximum(var, 0.0))
        mean[count == 0] = np.nan
        std[count == 0] = np.nan
        return mean, std

    def profiles(self):
        """{bundle: {'n', 'n_outliers', 'mdf_mean', metric: {'mean', 'std',
        'count'}}}, lists of K per metric.  ``n`` and ``mdf_mean`` are of every
        row that took part in the last orient pass, the ``n_outliers`` rows that
        ``max_mdf`` keeps out of the profiles included.  NaN for an empty
        bundle's ``mdf_mean`` and at a station with count 0 (``json_ready``
        turns them into null for a file)."""
        if self._rows is None:
            raise ValueError('fit() comes before profiles()')
        out = {}
        for b, name in enumerate(self.names):
            entry = {'n': int(self.n[b]), 'n_outliers': int(self.n_outliers[b]),
                     'mdf_mean': float(self.mdf_mean[b])}
            for metric, m in self.metrics.items():
                mean, std = self.statistics(m['sum_q'][b], m['sum_qq'][b], m['count'][b],
                                            m['scale'], m['scale_sq'])
                entry[metric] = {'mean': mean.tolist(), 'std': std.tolist(),
                                 'count': m['count'][b].tolist()}
            out[name] = entry
        return out

    def centroids_rasmm(self):
        """(B, K, 3) float64, RAS mm: affine (c - 0.5) of the voxel centroids."""
        return (self.centroids_vox - 0.5) @ self.lin.T + self.affine[:3, 3]

    def save(self, prefix, per_streamline=False):
        """``prefix_profiles.json`` (strict JSON: null where ``profiles()`` has a
        NaN), ``prefix_centroids.npy`` (RAS mm, float64),
        ``prefix_centroids.trk`` (the bundles that have a centroid) and, with
        ``per_streamline``, ``prefix_<metric>_streamlines.npy`` ((n, K) float64)
        for the metrics added with ``per_streamline=True``."""
        from tracktolearn_amd.io import streamlines as sio
        from tracktolearn_amd.tractogram import Tractogram
        folder = os.path.dirname(os.path.abspath(prefix))
        os.makedirs(folder, exist_ok=True)
        written = [prefix + '_profiles.json', prefix + '_centroids.npy',
                   prefix + '_centroids.trk']
        with open(written[0], 'w') as f:
            json.dump(json_ready(self.profiles()), f, indent=2, allow_nan=False)
        ras = self.centroids_rasmm()
        np.save(written[1], ras)
        lines = [c.astype(np.float32) for c in ras if np.all(np.isfinite(c))]
        header = sio.create_tractogram_header(
            self.affine, self.dims, np.sqrt((self.lin * self.lin).sum(0)))
        sio.save(Tractogram(lines, affine_to_rasmm=np.eye(4)), written[2], header)
        if per_streamline:
            for metric, m in self.metrics.items():
                if m['values'] is not None:
                    written.append(f'{prefix}_{metric}_streamlines.npy')
                    np.save(written[-1], m['values'])
        return written


__all__ = ['BundleProfiles', 'bundle_orient', 'bundle_profile', 'coordinate_scale', 'json_ready',
           'metric_scales', 'canonical_reverse', 'mdf_gate', 'MAX_POINTS', 'MAX_BUNDLES',
           'SEED_MAX_POINTS']
