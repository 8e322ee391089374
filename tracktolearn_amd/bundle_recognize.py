"""Bundle recognition: the nearest model line by MDF for every streamline, on
the GPU.

The assignment step of RecoBundles / QuickBundles: ``ttl_bundle_recognize``
resamples every streamline to K stations (the library's one resampler) and
finds, among the M model lines of an atlas, the one with the smallest
minimum-average-direct-flip distance, whether the streamline runs with it or
against it, and how far the nearest model of another bundle is
(include/ttl_hip.h states it).  With it the chain track -> recognise -> profile
needs no scoring masks:

    atlas = BundleAtlas.from_centroids('t1.nii.gz', 'atlas_centroids.npy', 'atlas_profiles.json')
    got = atlas.recognize('subject.trk', max_mdf=8.0, max_ratio=0.8)
    got['bundle']                       # (streamlines of the file,) int32, -1: in no bundle
    atlas.summary()                     # per bundle n, mdf_mean, n_gated

The atlas is taken to be in the subject's space; one that is not is fitted first
by ``bundle_register.register_atlas`` and moved with
``BundleAtlas.transformed``.  There is no NumPy fallback: like the rest of the product path this needs the
library.
"""
import json
import os

import numpy as np
import torch

from tracktolearn_amd import _lib

MAX_POINTS = _lib.PROFILE_MAX_POINTS
MAX_MODELS = _lib.RECOGNIZE_MAX_MODELS
#: a model line of an atlas tractogram has at most this many points (the padded
#: resampler keeps a row's cumulative arc length in LDS)
MODEL_MAX_POINTS = 4096


def bundle_recognize(points, offsets, models, lin, label=None, runner_up=False):
    """``ttl_bundle_recognize`` on device tensors: the ragged rows ``points``
    (P, 3) float32 / ``offsets`` (n + 1,) int64 against ``models`` (M, K, 3)
    float32 in the rows' coordinates; ``label`` (M,) int32, the bundle of every
    model (None: every model is its own); ``lin``: the (3, 3) linear part of
    voxel -> RAS mm.  Returns (best (n,) int32, flip (n,) int32, mdf (n,)
    float64, runner_up (n,) float64 or None)."""
    n, dev = _lib.ragged_rows(points, offsets), points.device
    if not (torch.is_tensor(models) and models.dtype == torch.float32 and models.dim() == 3 and
            models.shape[2] == 3 and models.is_contiguous() and models.device == dev):
        raise ValueError('models must be a contiguous (M, K, 3) float32 tensor on the device of '
                         'points')
    M, K = int(models.shape[0]), int(models.shape[1])
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f'models must have 1 .. {MAX_MODELS} lines, not {M}')
    if not 2 <= K <= MAX_POINTS:
        raise ValueError(f'models must have 2 .. {MAX_POINTS} stations, not {K}')
    if label is not None and not (
            torch.is_tensor(label) and label.dtype == torch.int32 and label.is_contiguous() and
            tuple(label.shape) == (M,) and label.device == dev):
        raise ValueError(f'label must be a contiguous ({M},) int32 tensor on the device of points')
    lin_c = _lib.lin9(lin)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    flip = torch.zeros(n, dtype=torch.int32, device=dev)
    mdf = torch.full((n,), float('nan'), dtype=torch.float64, device=dev)
    second = torch.full((n,), float('nan'), dtype=torch.float64, device=dev) if runner_up else None
    if n == 0 or points.shape[0] == 0:      # no launch: an empty tensor has no pointer
        return best, flip, mdf, second
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_bundle_recognize(
            points.data_ptr(), offsets.data_ptr(), n, models.data_ptr(),
            None if label is None else label.data_ptr(), M, K, lin_c, best.data_ptr(),
            flip.data_ptr(), mdf.data_ptr(), second.data_ptr() if runner_up else None,
            _lib.stream_of(dev)), 'ttl_bundle_recognize')
    return best, flip, mdf, second


def apply_gates(bundle, mdf, runner_up, max_mdf=None, max_ratio=None):
    """The two gates of ``BundleAtlas.recognize`` on host arrays, in this order:
    a row is -1 when ``mdf > max_mdf``, then when ``runner_up`` is not NaN and
    ``mdf > max_ratio * runner_up``.  None: no such gate.  Returns the gated copy
    of ``bundle``; a NaN ``mdf`` passes both (such a row is -1 already)."""
    out = np.array(bundle, np.int32)
    mdf = np.asarray(mdf, np.float64)
    with np.errstate(invalid='ignore'):
        if max_mdf is not None:
            out[mdf > float(max_mdf)] = -1
        if max_ratio is not None:
            second = np.asarray(runner_up, np.float64)
            out[~np.isnan(second) & (mdf > float(max_ratio) * second)] = -1
    return out


def _reference_grid(dims_or_reference_nifti, affine):
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
    return check_dims(ref), np.asarray(affine, np.float64).reshape(4, 4)


class BundleAtlas:
    """``BundleAtlas(dims_or_reference_nifti, affine, models_vox, names,
    label=None, device='cuda')``: M model lines of K stations and the bundle
    each belongs to.  ``dims_or_reference_nifti``: (X, Y, Z) of the subject's
    grid, or a NIfTI file on it; ``affine``: its (4, 4) voxel -> RAS mm (None: the
    file's own).  ``models_vox``: (M, K, 3), corner-origin voxel coordinates of
    that grid; a model with a non-finite station never wins.  ``names``: the
    names of the labels; ``label``: (M,) the index into ``names`` of every model
    (None: model m is label m, one name per model)."""

    def __init__(self, dims_or_reference_nifti, affine, models_vox, names, label=None,
                 device='cuda'):
        self.dims, self.affine = _reference_grid(dims_or_reference_nifti, affine)
        self.lin = np.ascontiguousarray(self.affine[:3, :3])
        models = np.asarray(models_vox)
        if models.ndim != 3 or models.shape[2] != 3 or not 1 <= models.shape[0] <= MAX_MODELS or \
                not 2 <= models.shape[1] <= MAX_POINTS:
            raise ValueError(f'models_vox must be (M, K, 3) with M in 1 .. {MAX_MODELS} and K in '
                             f'2 .. {MAX_POINTS}, not {models.shape}')
        self.models_vox = np.ascontiguousarray(models, np.float32)
        self.M, self.K = int(models.shape[0]), int(models.shape[1])
        self.names = [str(v) for v in names]
        if not self.names or len(set(self.names)) != len(self.names):
            raise ValueError(f'names must be distinct and not empty, not {self.names}')
        if label is None:
            if len(self.names) != self.M:
                raise ValueError(f'{self.M} models without label need as many names, not '
                                 f'{len(self.names)}')
            label = np.arange(self.M)
        label = np.asarray(label)
        if label.shape != (self.M,) or label.dtype.kind not in 'iu' or \
                (label.size and (label.min() < 0 or label.max() >= len(self.names))):
            raise ValueError(f'label must be ({self.M},) integers in 0 .. {len(self.names) - 1}')
        self.label = np.ascontiguousarray(label, np.int32)
        _lib.load()
        self.device = torch.device(device)
        self._last = None

    # -- constructors ------------------------------------------------------
    @classmethod
    def from_centroids(cls, reference, centroids_npy, profiles_json=None, device='cuda'):
        """The atlas ``BundleProfiles.save`` wrote: ``PREFIX_centroids.npy``
        ((bundles, K, 3), RAS mm, one model per bundle) on the grid of the NIfTI
        ``reference``; the names are the keys of ``PREFIX_profiles.json`` when
        given, else bundle_0, bundle_1, ...  A bundle without a centroid (NaN) is
        kept: its number stays, its model never wins."""
        dims, affine = _reference_grid(reference, None)
        ras = np.asarray(np.load(os.fsdecode(centroids_npy)), np.float64)
        if ras.ndim != 3 or ras.shape[2] != 3:
            raise ValueError(f'{centroids_npy}: {ras.shape} is not (bundles, K, 3)')
        names = [f'bundle_{b}' for b in range(ras.shape[0])]
        if profiles_json is not None:
            with open(os.fsdecode(profiles_json)) as f:
                names = read_names(json.load(f))
            if len(names) != ras.shape[0]:
                raise ValueError(f'{profiles_json} names {len(names)} bundles, {centroids_npy} '
                                 f'has {ras.shape[0]}')
        inv = np.linalg.inv(affine)
        return cls(dims, affine, ras @ inv[:3, :3].T + inv[:3, 3] + 0.5, names, device=device)

    @classmethod
    def from_tractogram(cls, reference, file, label, names, nb_points, device='cuda'):
        """An atlas .trk / .tck with several model lines per bundle: ``label``
        the index into ``names`` of every streamline of the file.  The lines
        (2 .. MODEL_MAX_POINTS points each) are resampled to ``nb_points``
        stations by ``resample_streamlines``."""
        from tracktolearn_amd.experiment.oracle_validator import corner_voxels
        from tracktolearn_amd.oracles.oracle import resample_streamlines
        dims, affine = _reference_grid(reference, None)
        if not 2 <= int(nb_points) <= MAX_POINTS:
            raise ValueError(f'nb_points must be in 2 .. {MAX_POINTS}, not {nb_points}')
        points, offsets, index = corner_voxels(file, affine)
        label = np.asarray(label)
        lens = np.diff(offsets)
        if label.ndim != 1 or len(index) != label.shape[0]:
            raise ValueError(f'{file}: every model line needs 2 points or more and a label; '
                             f'{len(index)} such lines, {label.shape} labels')
        if not 1 <= len(index) <= MAX_MODELS or lens.max() > MODEL_MAX_POINTS:
            raise ValueError(f'{file}: 1 .. {MAX_MODELS} model lines of at most '
                             f'{MODEL_MAX_POINTS} points, not {len(index)} lines of up to '
                             f'{int(lens.max()) if lens.size else 0}')
        dev = torch.device(device)
        pad = np.zeros((len(index), int(lens.max()), 3), np.float32)
        owner = np.repeat(np.arange(len(index)), lens)
        pad[owner, np.arange(points.shape[0]) - offsets[:-1][owner]] = points
        models = resample_streamlines(torch.from_numpy(pad).to(dev),
                                      torch.from_numpy(lens).to(dev), int(nb_points))
        return cls(dims, affine, models.cpu().numpy(), names, label=label, device=device)

    # -- recognise -----------------------------------------------------------
    def assemble(self, n_input, index, best, flip, mdf, runner_up, max_mdf=None, max_ratio=None):
        """The result of ``recognize`` from the kernel's outputs for the rows
        ``index`` of ``n_input`` streamlines (host arrays): per input streamline
        ``model``, ``flip``, ``mdf``, ``runner_up`` (-1 / 0 / NaN / NaN for a
        streamline the intake dropped) and ``bundle``, the label of the winning
        model after the gates (``apply_gates``), -1 without one."""
        index = np.asarray(index, np.int64)
        best = np.asarray(best, np.int32)
        model = np.full(n_input, -1, np.int32)
        out_flip = np.zeros(n_input, np.int32)
        out_mdf, out_second = np.full(n_input, np.nan), np.full(n_input, np.nan)
        model[index] = best
        out_flip[index] = flip
        out_mdf[index] = mdf
        out_second[index] = runner_up
        won = np.where(model >= 0, self.label[np.clip(model, 0, self.M - 1)], -1).astype(np.int32)
        bundle = apply_gates(won, out_mdf, out_second, max_mdf, max_ratio)
        self._last = {'bundle': bundle, 'won': won, 'mdf': out_mdf}
        return {'bundle': bundle, 'model': model, 'flip': out_flip, 'mdf': out_mdf,
                'runner_up': out_second, 'index': index}

    def recognize(self, file_or_tractogram, env=None, in_rasmm=False, max_mdf=None,
                  max_ratio=None):
        """A .trk / .tck file, or the tracker's in-memory tractogram (voxel
        coordinates of ``env``), through the validators' one intake.  Returns a
        dict of NumPy arrays: ``bundle`` (N_input,) int32, the label of the
        winning model or -1; ``model``, ``flip``, ``mdf``, ``runner_up`` per input
        streamline; ``index``, the intake's.  Gates, in this order: -1 when
        ``mdf > max_mdf``; -1 when ``runner_up`` is not NaN and ``mdf >
        max_ratio * runner_up``."""
        from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                                  load_tractogram)
        from tracktolearn_amd.tractogram import Tractogram
        source = file_or_tractogram
        if isinstance(source, FILENAME):
            source, in_rasmm = load_tractogram(source)[0], True
        lines = source.streamlines if isinstance(source, Tractogram) else source
        points, offsets, index = corner_voxels(
            source, self.affine, getattr(env, 'affine_vox2rasmm', None), in_rasmm=in_rasmm)
        dev = self.device
        best, flip, mdf, second = bundle_recognize(
            torch.from_numpy(points).to(dev), torch.from_numpy(offsets).to(dev),
            torch.from_numpy(self.models_vox).to(dev), self.lin,
            label=torch.from_numpy(self.label).to(dev), runner_up=True)
        return self.assemble(len(lines), index, best.cpu().numpy(), flip.cpu().numpy(),
                             mdf.cpu().numpy(), second.cpu().numpy(), max_mdf, max_ratio)

    def summary(self):
        """{name: {'n', 'mdf_mean', 'n_gated'}} of the last ``recognize``: the
        streamlines a label keeps, their mean distance (NaN without one) and those
        a label won and a gate took away."""
        if self._last is None:
            raise ValueError('recognize() comes before summary()')
        last, out = self._last, {}
        for b, name in enumerate(self.names):
            kept = last['bundle'] == b
            out[name] = {'n': int(kept.sum()),
                         'mdf_mean': float(last['mdf'][kept].mean()) if kept.any() else
                         float('nan'),
                         'n_gated': int(((last['won'] == b) & ~kept).sum())}
        return out

    def transformed(self, matrix_ras):
        """A new atlas on the same grid with every model line moved by the (4, 4)
        RAS-mm ``matrix_ras`` (``bundle_register.register_atlas``'s ``matrix``): the
        same labels and names, the stations computed in float64 and stored as
        float32."""
        from tracktolearn_amd.bundle_register import to_voxel
        v = to_voxel(np.asarray(matrix_ras, np.float64).reshape(4, 4), self.affine)
        moved = self.models_vox.astype(np.float64) @ v[:, :3].T + v[:, 3]
        return BundleAtlas(self.dims, self.affine, moved, self.names, label=self.label,
                           device=self.device)

    def one_model_per_label(self):
        """(labels, K, 3) float32, the model of every label in label order, when
        every label has exactly one model; None otherwise."""
        if self.M != len(self.names) or sorted(self.label.tolist()) != list(range(self.M)):
            return None
        return self.models_vox[np.argsort(self.label, kind='stable')]


def read_names(value):
    """The label names of a JSON value: a list of names, or a dict whose keys are
    the names in order (a ``PREFIX_profiles.json``)."""
    if isinstance(value, dict):
        return [str(k) for k in value]
    if isinstance(value, list) and all(isinstance(v, str) for v in value):
        return list(value)
    raise ValueError('names are a JSON list of strings or the keys of a profiles.json')


__all__ = ['BundleAtlas', 'bundle_recognize', 'apply_gates', 'read_names', 'MAX_POINTS',
           'MAX_MODELS', 'MODEL_MAX_POINTS']
