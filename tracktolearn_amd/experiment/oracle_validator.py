"""OracleValidator: TractOracle accuracy and coverage of a validation
tractogram, on the GPU.

Mirror of TrackToLearn/experiment/oracle_validator.py.  The reference loads
the saved .trk into the reference anatomy's voxel space (corner origin),
scores it with ``OracleSingleton.predict`` in slices of 4 096 (every
streamline is scored) and builds the binarised tract-count map of the
accepted streamlines with scilpy on the CPU.  Here the tractogram is packed
once on the host and uploaded once; the scores come from
``OracleSingleton.predict_packed`` (ragged resampling + the network) and the
map from one ``ttl_tract_coverage`` launch; the host reads back two counts.

    Oracle   = #{scores > 0.5} / n
    Coverage = #{voxels visited by accepted streamlines} / #{tracking-mask voxels}

The voxel walk that defines "visited" is stated in include/ttl_hip.h
(scilpy's ``compute_tract_counts_map`` is absent: restated, parity unpinned;
DESIGN 3.8).  ``__call__`` takes the reference's filename (.trk / .tck) or the
in-memory ``Tractogram`` of ``Tracker.track_and_validate`` (tracker voxel
coordinates), which skips the file round trip.

Both validators take their tractogram through the one intake here,
``corner_voxels`` (file or memory, rows of >= 2 points, packed, corner-origin
voxels of the scoring space), read files through ``load_tractogram`` and launch
the library's ragged-row entries through ``launch_ragged``.
"""
import ctypes as C
import os

import numpy as np
import torch

from tracktolearn_amd.experiment.validators import Validator
from tracktolearn_amd.oracles.oracle import OracleSingleton
from tracktolearn_amd.tractogram import Tractogram


def reference_space(env):
    """(ref_affine (4, 4) float64, dims (3,)) of the reference anatomy, falling
    back to the tracking mask (env.py:236-239, ttl_track_from_hdf5.run)."""
    ref = getattr(env, 'reference', None)
    affine = dims = None
    if isinstance(ref, dict):
        affine, dims = ref.get('affine'), ref.get('shape')
    elif ref is not None and hasattr(ref, 'affine'):
        affine, dims = ref.affine, getattr(ref, 'shape', None)
    mask = env.tracking_mask
    if affine is None:
        affine = getattr(mask, 'affine_vox2rasmm', None)
        if affine is None:
            affine = env.affine_vox2rasmm
    if dims is None:
        dims = mask.data.shape
    return np.asarray(affine, np.float64), tuple(int(v) for v in tuple(dims)[:3])


def _affine_corner(pts, M):
    """float32 (M[:3, :3] p + M[:3, 3]) + 0.5, in float64, with a fixed order
    of operations (no BLAS): ((m0 x + m1 y) + m2 z) + m3, then + 0.5."""
    p = np.asarray(pts, np.float64)
    out = np.empty(p.shape, np.float32)
    for i in range(3):
        out[:, i] = (((M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2])
                     + M[i, 3]) + 0.5
    return out


def pack(lines):
    """Ragged layout: points (M, 3) float32 and offsets (n + 1,) int64."""
    offsets = np.zeros(len(lines) + 1, np.int64)
    if lines:
        np.cumsum([len(s) for s in lines], out=offsets[1:])
        points = np.concatenate(lines).astype(np.float32, copy=False)
    else:
        points = np.zeros((0, 3), np.float32)
    return points.reshape(-1, 3), offsets


def corner_voxels_from_rasmm(points_rasmm, ref_affine):
    """RAS+mm points (a .trk / .tck as read) -> float32 voxel coordinates of
    the reference anatomy, corner origin: inv(ref_affine) in float64, + 0.5."""
    return _affine_corner(points_rasmm, np.linalg.inv(np.asarray(ref_affine, np.float64)))


def corner_voxels_from_tracker(points_vox, vox2rasmm, ref_affine):
    """Tracker voxel coordinates -> the same space: inv(ref_affine) @ vox2rasmm
    in float64, + 0.5.  When the two affines are equal this is exactly the
    float32 ``p + 0.5``."""
    ref = np.asarray(ref_affine, np.float64)
    own = np.asarray(vox2rasmm, np.float64)
    if np.array_equal(ref, own):
        return np.asarray(points_vox, np.float32) + np.float32(0.5)
    return _affine_corner(points_vox, np.linalg.inv(ref) @ own)


FILENAME = (str, bytes, os.PathLike)


def load_tractogram(filename):
    """The one reader of a tractogram file: (tractogram in RAS+mm, the .trk's
    header dict, or None for a .tck)."""
    from tracktolearn_amd.io import streamlines as sio
    filename = os.fsdecode(filename)
    lower = filename.lower()
    if lower.endswith('.trk'):
        return sio.load_trk(filename)
    if lower.endswith('.tck'):
        return sio.load_tck(filename)[0], None
    raise ValueError(f'{filename}: a tractogram is read from a .trk or .tck file')


def corner_voxels(source, ref_affine, tracker_affine=None, in_rasmm=False):
    """The one intake of a validator: (points (M, 3) float32, offsets (n + 1,)
    int64, index (n,) int64) of the streamlines with >= 2 points, packed, in
    the voxel space of ``ref_affine``, corner origin; ``index`` their numbers
    in the input.  ``source``: a .trk / .tck file name (RAS+mm), or the
    in-memory ``Tractogram`` (or list of streamlines) of the tracker, in the
    voxel coordinates of ``tracker_affine``; ``in_rasmm``: an in-memory source
    that ``load_tractogram`` read."""
    if isinstance(source, FILENAME):
        source, in_rasmm = load_tractogram(source)[0], True
    elif not in_rasmm and tracker_affine is None:
        raise ValueError('an in-memory tractogram is in the voxel space of its env: '
                         'give the env')
    lines = source.streamlines if isinstance(source, Tractogram) else source
    index = np.flatnonzero(np.fromiter((len(s) >= 2 for s in lines), bool, len(lines)))
    index = index.astype(np.int64, copy=False)
    # a tracker's output keeps every row: no second list then
    points, offsets = pack(lines if len(index) == len(lines) else
                           [lines[i] for i in index.tolist()])
    if in_rasmm:
        return corner_voxels_from_rasmm(points, ref_affine), offsets, index
    return corner_voxels_from_tracker(points, tracker_affine, ref_affine), offsets, index


def launch_ragged(entry, points, offsets, dims, before=(), after=()):
    """The one launch of a library entry that walks ragged rows:
    ``entry(points, offsets, n, *before, dims, *after, stream)`` on the
    device and current stream of ``points``, float32 points and int64 offsets
    contiguous, n = max(len(offsets) - 1, 0), its status checked."""
    from tracktolearn_amd import _lib
    pts = points.to(torch.float32).contiguous()
    off = offsets.to(torch.int64).contiguous()
    dims_c = (C.c_int32 * 3)(*(int(v) for v in dims))
    dev = pts.device
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), entry)(
            pts.data_ptr(), off.data_ptr(), max(int(off.shape[0]) - 1, 0), *before, dims_c,
            *after, _lib.stream_of(dev)), entry)


def tract_coverage(points, offsets, dims, scores=None, threshold=0.5, visited=None):
    """``ttl_tract_coverage`` on device tensors: visited (X * Y * Z,) uint8,
    1 where an accepted streamline (scores > threshold; every one when scores
    is None) passes (include/ttl_hip.h).  ``visited`` (zeroed) may be given."""
    X, Y, Z = (int(v) for v in dims)
    if visited is None:
        visited = torch.zeros(X * Y * Z, dtype=torch.uint8, device=points.device)
    if len(offsets) <= 1:
        return visited
    sc = None if scores is None else scores.to(torch.float32).contiguous()
    launch_ragged('ttl_tract_coverage', points, offsets, dims,
                  (None if sc is None else sc.data_ptr(), float(threshold)),
                  (visited.data_ptr(),))
    return visited


class OracleValidator(Validator):
    """``OracleValidator(checkpoint, device)(tractogram_or_filename, env)`` ->
    ``{'Oracle': float, 'Coverage': float}``, ``{}`` without a streamline of
    >= 2 points."""

    def __init__(self, checkpoint, device):
        self.name = 'Oracle'
        if not checkpoint or not os.path.isfile(checkpoint) or \
                os.path.getsize(checkpoint) == 0:
            # the reference accepts it here and fails later, on self.model
            raise ValueError(f'OracleValidator needs an oracle checkpoint, got {checkpoint!r}')
        self.checkpoint = checkpoint
        self.device = torch.device(device)
        self.model = OracleSingleton(checkpoint, self.device)

    def __call__(self, tractogram_or_filename, env):
        ref_affine, dims = reference_space(env)
        points, offsets, _ = corner_voxels(tractogram_or_filename, ref_affine,
                                           env.affine_vox2rasmm)
        n = len(offsets) - 1
        if n == 0:
            return {}
        mask_count = int(np.count_nonzero(env.tracking_mask.data))
        dev = self.model.device
        pts = torch.from_numpy(points).to(dev)
        off = torch.from_numpy(offsets).to(dev)
        scores = self.model.predict_packed(pts, off)
        visited = tract_coverage(pts, off, dims, scores, 0.5)
        counts = torch.stack([(scores > 0.5).sum(), torch.count_nonzero(visited)]).cpu()
        accepted, covered = (int(v) for v in counts)
        return {'Oracle': float(accepted / n),
                'Coverage': float(covered / mask_count) if mask_count else 0.0}
