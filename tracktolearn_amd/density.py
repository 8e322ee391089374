"""Track density maps: streamlines, length and ends per voxel, on the GPU
(DESIGN 3.17).

``ttl_tract_density`` walks every streamline through the voxels of a grid
(the walk of ``ttl_tract_coverage``) and adds, per voxel, 1 to ``count`` for
every streamline that passes (once, however often it comes back), the mm of
streamline lying inside to ``length_q`` and, per RAS axis, to ``dec_q`` (the
direction-encoded density), and 1 to ``ends`` per streamline end
(include/ttl_hip.h states it).  Every map is an integer sum, so the maps of a
tractogram do not depend on the batch split or on the order of arrival:

    tdi = DensityMap('fa.nii.gz', None, zoom=2, dec=True)
    tdi.add_tractogram('tracts.trk')            # or Tracker(..., density=tdi)
    tdi.maps()['count']                         # (2X, 2Y, 2Z) int32
    tdi.save('out/tdi')                         # out/tdi_count.nii.gz, ...

There is no NumPy fallback: like the rest of the product path this needs the
library.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from tracktolearn_amd import _lib

LENGTH_SCALE = _lib.CONNECTOME_LENGTH_SCALE
MAX_WAVE_SLOTS = _lib.DENSITY_MAX_WAVE_SLOTS
DEFAULT_WAVE_SLOTS = _lib.DENSITY_WAVE_SLOTS
MAX_SPILL_SLOTS = 1 << 26
MAX_ZOOM = 8
#: where ``DensityMap`` starts its spill table: rows of up to 4096 voxels
DEFAULT_SPILL_SLOTS = 8192


def _power_of_two(v):
    return v > 0 and (v & (v - 1)) == 0


def check_slots(wave_slots, spill_slots):
    """ValueError unless ``wave_slots`` is 0 (the library's default) or a power
    of two in 64 .. MAX_WAVE_SLOTS and ``spill_slots`` 0 (no spill pass) or a
    power of two in 64 .. MAX_SPILL_SLOTS: what the library takes."""
    wave_slots, spill_slots = int(wave_slots), int(spill_slots)
    if wave_slots and not (_power_of_two(wave_slots) and 64 <= wave_slots <= MAX_WAVE_SLOTS):
        raise ValueError(f'wave_slots must be 0 or a power of two in 64 .. {MAX_WAVE_SLOTS}, '
                         f'not {wave_slots}')
    if spill_slots and not (_power_of_two(spill_slots) and 64 <= spill_slots <= MAX_SPILL_SLOTS):
        raise ValueError(f'spill_slots must be 0 or a power of two in 64 .. {MAX_SPILL_SLOTS}, '
                         f'not {spill_slots}')
    return wave_slots, spill_slots


def check_dims(dims):
    """(X, Y, Z) ints, each >= 1 with X * Y * Z < 2^31 - 1; ValueError otherwise."""
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31 - 1:
        raise ValueError(f'a density map has three dims >= 1 with X * Y * Z < 2^31 - 1, '
                         f'not {dims}')
    return dims


def zoom_grid(dims, affine, zoom):
    """(dims * zoom, the map's affine) of a super-resolution map: ``zoom`` an
    integer in 1 .. MAX_ZOOM; the linear part of ``affine`` divided by it, the
    translation kept (corner origin: the corner of voxel 0 does not move)."""
    if isinstance(zoom, bool) or int(zoom) != zoom or not 1 <= int(zoom) <= MAX_ZOOM:
        raise ValueError(f'zoom must be an integer in 1 .. {MAX_ZOOM}, not {zoom!r}')
    zoom = int(zoom)
    affine = np.array(affine, np.float64).reshape(4, 4)
    affine[:3, :3] /= zoom
    return check_dims(int(v) * zoom for v in dims), affine


def workspace_bytes(spill_slots, n_max):
    """``ttl_tract_density_workspace_bytes``."""
    return int(_lib.load().ttl_tract_density_workspace_bytes(int(spill_slots), int(n_max)))


def tract_density(points, offsets, dims, lin, count=None, length_q=None, dec_q=None, ends=None,
                  wave_slots=0, spill_slots=0, workspace=None):
    """``ttl_tract_density`` on device tensors: the ragged rows ``points``
    (M, 3) float32 / ``offsets`` (n + 1,) int64, in corner-origin voxel
    coordinates of the map's grid ``dims``, added into the maps that are given
    (``count``, ``ends``: int32 [X * Y * Z]; ``length_q``: int64 [X * Y * Z];
    ``dec_q``: int64 [X * Y * Z, 3]); ``lin`` the (3, 3) linear part of voxel
    -> RAS mm.  ``workspace``: a zeroed uint8 device tensor of at least
    ``workspace_bytes(spill_slots, n)`` bytes, or None.  Returns ``status``
    (n,) int32: 0 / 1 counted, 2 left out of ``count``, -1 not added."""
    n = max(int(offsets.shape[0]) - 1, 0)
    dev = points.device
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if n == 0 or points.shape[0] == 0:      # no launch: an empty tensor has no pointer
        return status
    dims = check_dims(dims)
    words = dims[0] * dims[1] * dims[2]
    desc = _lib.DensityDesc()
    desc.dims = (C.c_int32 * 3)(*dims)
    desc.lin = _lib.lin9(lin)
    for name, t, dtype, numel in (('count', count, torch.int32, words),
                                  ('length_q', length_q, torch.int64, words),
                                  ('dec_q', dec_q, torch.int64, 3 * words),
                                  ('ends', ends, torch.int32, words)):
        if t is None:
            continue
        if t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'{name} must be a contiguous {dtype} tensor of {numel} words on '
                             'the device of points')
        setattr(desc, name, t.data_ptr())
    desc.wave_slots, desc.spill_slots = int(wave_slots), int(spill_slots)
    if workspace is not None:
        if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or \
                workspace.device != dev:
            raise ValueError('workspace must be a contiguous uint8 tensor on the device of points')
        desc.workspace, desc.workspace_bytes = workspace.data_ptr(), workspace.numel()
    pts = points.to(torch.float32).contiguous()
    off = offsets.to(torch.int64).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_tract_density(C.byref(desc), pts.data_ptr(), off.data_ptr(), n,
                                                 status.data_ptr(), _lib.stream_of(dev)),
                   'ttl_tract_density')
    return status


def gather_rows(points, offsets, rows):
    """The ragged rows ``rows`` (int64 tensor) of (points, offsets), packed:
    torch on the device of ``points``."""
    lens = (offsets[1:] - offsets[:-1])[rows]
    out = torch.zeros(rows.shape[0] + 1, dtype=torch.int64, device=offsets.device)
    torch.cumsum(lens, 0, out=out[1:])
    total = int(out[-1].item())
    owner = torch.repeat_interleave(torch.arange(rows.shape[0], device=offsets.device), lens,
                                    output_size=total)
    src = offsets[rows][owner] + (torch.arange(total, device=offsets.device) - out[:-1][owner])
    return points[src], out


class DensityMap:
    """``DensityMap(dims_or_reference_nifti, affine, zoom=1, device='cuda',
    dec=False, ends=True, length=True)``: the device maps of a grid and what
    streams into them.  ``dims_or_reference_nifti``: (X, Y, Z) of the reference
    grid, or a NIfTI file on it; ``affine``: the (4, 4) voxel -> RAS mm of that
    grid (None: the file's own).  ``zoom`` (1 .. 8): the map's grid is ``dims *
    zoom`` and its affine the reference's with the linear part divided by zoom
    (``zoom_grid``).  ``count`` is always kept; ``length``, ``dec`` and ``ends``
    choose the other maps.  ``wave_slots`` / ``spill_slots``: the set sizes of
    ``ttl_tract_density`` (0: the library's default / ``DEFAULT_SPILL_SLOTS``)."""

    def __init__(self, dims_or_reference_nifti, affine, zoom=1, device='cuda', dec=False,
                 ends=True, length=True, wave_slots=0, spill_slots=DEFAULT_SPILL_SLOTS):
        ref = dims_or_reference_nifti
        if isinstance(ref, (str, bytes, os.PathLike)):
            from tracktolearn_amd.io import nifti
            img = nifti.load(os.fsdecode(ref))
            if affine is None:
                affine = img.affine
            ref = tuple(int(v) for v in img.shape[:3])
        if affine is None:
            raise ValueError('dims need the affine of their grid')
        self.ref_dims = check_dims(ref)
        self.ref_affine = np.asarray(affine, np.float64).reshape(4, 4)
        self.dims, self.affine = zoom_grid(self.ref_dims, self.ref_affine, zoom)
        self.zoom = int(zoom)
        self.lin = np.ascontiguousarray(self.affine[:3, :3])
        self.wave_slots, self.spill_slots = check_slots(wave_slots, spill_slots)
        _lib.load()
        self.device = torch.device(device)
        words = self.dims[0] * self.dims[1] * self.dims[2]

        def zeros(dtype, *shape):
            return torch.zeros(shape, dtype=dtype, device=self.device)
        self.count = zeros(torch.int32, words)
        self.length_q = zeros(torch.int64, words) if length else None
        self.dec_q = zeros(torch.int64, words, 3) if dec else None
        self.ends = zeros(torch.int32, words) if ends else None
        self._workspace = None
        self._tiers = torch.zeros(4, dtype=torch.int64, device=self.device)   # status -1, 0, 1, 2
        self._dropped = 0           # rows the intake left out (fewer than 2 points)

    def _room(self, spill_slots, n):
        """The zeroed workspace for ``n`` rows at ``spill_slots`` (None at 0),
        kept while it is large enough: every call leaves it zeroed."""
        if not spill_slots:
            return None
        need = workspace_bytes(spill_slots, n)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def add(self, points, offsets):
        """Device tensors in corner-origin voxel coordinates of the REFERENCE
        grid.  The float32 points are multiplied by ``zoom`` in float32; the map
        is of that product (at zoom 1: of the points as given).  Returns
        ``status`` (n,) int32: 0 and 1 name the set that counted the row, -1 a
        row that was not added.  While a row comes back with status 2 (its
        voxels fit neither set) the spill table is doubled (to at least
        ``DEFAULT_SPILL_SLOTS``) and those rows, gathered with torch, are added
        again with ``count`` alone; the test for that reads one small value per
        call (the only host read of ``add``)."""
        n = max(int(offsets.shape[0]) - 1, 0)
        pts = points.to(torch.float32)
        if self.zoom != 1:
            pts = pts * float(self.zoom)
        status = tract_density(pts, offsets, self.dims, self.lin, self.count, self.length_q,
                               self.dec_q, self.ends, self.wave_slots, self.spill_slots,
                               self._room(self.spill_slots, n))
        if n == 0:
            return status
        spill = self.spill_slots
        left = torch.nonzero(status == 2).squeeze(1)
        rows_pts, rows_off = pts, offsets
        while left.numel():                  # .numel() of a nonzero: the one host read
            if spill >= MAX_SPILL_SLOTS:
                raise _lib.TTLError(f'{left.numel()} rows visit more than {spill // 2} voxels')
            spill = max(2 * spill, DEFAULT_SPILL_SLOTS)
            rows_pts, rows_off = gather_rows(rows_pts, rows_off, left)
            again = tract_density(rows_pts, rows_off, self.dims, self.lin, count=self.count,
                                  wave_slots=self.wave_slots, spill_slots=spill,
                                  workspace=self._room(spill, left.numel()))
            owner = torch.nonzero(status == 2).squeeze(1)
            status[owner] = again
            left = torch.nonzero(again == 2).squeeze(1)
        self._tiers += torch.bincount((status + 1).to(torch.int64), minlength=4)[:4]
        return status

    def add_tractogram(self, tractogram_or_filename, env=None, in_rasmm=False):
        """A .trk / .tck file, or the tracker's in-memory tractogram (voxel
        coordinates of ``env``; ``in_rasmm``: one that ``load_tractogram``
        read), through the validators' one intake.  Returns (status (n,) int32
        on the device, index (n,) int64: the rows' numbers in the input)."""
        from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                                  load_tractogram)
        from tracktolearn_amd.tractogram import Tractogram
        source = tractogram_or_filename
        if isinstance(source, FILENAME):
            source, in_rasmm = load_tractogram(source)[0], True
        lines = source.streamlines if isinstance(source, Tractogram) else source
        points, offsets, index = corner_voxels(
            source, self.ref_affine, getattr(env, 'affine_vox2rasmm', None), in_rasmm=in_rasmm)
        self._dropped += len(lines) - len(index)
        status = self.add(torch.from_numpy(points).to(self.device),
                          torch.from_numpy(offsets).to(self.device))
        return status, index

    def tiers(self):
        """{'not_added', 'wave', 'spill'}: how many rows each status took."""
        t = [int(v) for v in self._tiers.cpu()]
        return {'not_added': t[0], 'wave': t[1], 'spill': t[2]}

    @property
    def skipped(self):
        """The number of rows left out: fewer than 2 points, a non-finite
        point, a length of 2^40 mm or more."""
        return int(self._tiers[0].item()) + self._dropped

    def maps(self):
        """``count`` and ``ends`` ((X, Y, Z) int32), ``length_mm`` ((X, Y, Z)
        float64 = length_q / 2^20) and ``dec_mm`` ((X, Y, Z, 3) float64), of the
        maps that are kept."""
        out = {'count': self.count.cpu().numpy().reshape(self.dims)}
        if self.ends is not None:
            out['ends'] = self.ends.cpu().numpy().reshape(self.dims)
        if self.length_q is not None:
            out['length_mm'] = self.length_q.cpu().numpy().reshape(self.dims) / LENGTH_SCALE
        if self.dec_q is not None:
            out['dec_mm'] = self.dec_q.cpu().numpy().reshape(self.dims + (3,)) / LENGTH_SCALE
        return out

    def totals(self):
        """What ``prefix.json`` holds."""
        tiers = self.tiers()
        return {'added': tiers['wave'] + tiers['spill'], 'skipped': self.skipped,
                'zoom': self.zoom, 'dims': list(self.dims),
                'wave_slots': self.wave_slots or DEFAULT_WAVE_SLOTS,
                'spill_slots': self.spill_slots, 'tiers': tiers}

    def save(self, prefix):
        """``prefix_count.nii.gz`` (int32), ``prefix_length.nii.gz``,
        ``prefix_ends.nii.gz`` and ``prefix_dec.nii.gz`` (float32; of the maps
        that are kept) with the map's affine, and ``prefix.json`` (``totals``)."""
        from tracktolearn_amd.io import nifti
        m = self.maps()
        folder = os.path.dirname(os.path.abspath(prefix))
        os.makedirs(folder, exist_ok=True)
        written = []
        for key, suffix, dtype in (('count', '_count', np.int32), ('length_mm', '_length', np.float32),
                                   ('ends', '_ends', np.float32), ('dec_mm', '_dec', np.float32)):
            if key in m:
                nifti.save(prefix + suffix + '.nii.gz', m[key].astype(dtype), self.affine)
                written.append(prefix + suffix + '.nii.gz')
        with open(prefix + '.json', 'w') as f:
            json.dump(self.totals(), f, indent=2)
        return written + [prefix + '.json']


__all__ = ['DensityMap', 'tract_density', 'workspace_bytes', 'gather_rows', 'zoom_grid',
           'check_dims', 'check_slots', 'LENGTH_SCALE', 'MAX_WAVE_SLOTS', 'DEFAULT_WAVE_SLOTS',
           'MAX_SPILL_SLOTS', 'MAX_ZOOM', 'DEFAULT_SPILL_SLOTS']
