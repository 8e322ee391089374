"""TractometerValidator: bundle segmentation and overlap of a validation
tractogram, on the GPU.

Mirror of TrackToLearn/experiment/tractometer_validator.py.  The reference
hands the saved .trk to scilpy on the CPU (``segment_tractogram_from_roi``,
then ``compute_tractometry`` with ``compute_ic=False, unique=True``): every
streamline's ends against the head and tail ROIs of every bundle, the length /
orientation / angle / all_mask / any_mask criteria, a tract-count map per valid
bundle and its intersection with the ground-truth mask.  Here the scoring data
is packed once, at construction, into bit planes (bit b of a voxel's 64-bit
word = bundle b) and a table of limits; a call uploads the tractogram once,
runs ``ttl_tractometer_classify`` and ``ttl_tractometer_overlap`` and reads
back a few hundred bytes.

    VC = #{streamlines with a bundle} / n      NC = 1 - VC
    VB = #{bundles with a streamline}          IC = IS = IB = 0
    OL_b = |M_b & G_b| / |G_b|                 mean_OL over bundles with a gt_mask

The definitions (ends, voxel walk, lengths, winding) are stated in
include/ttl_hip.h (scilpy's source is absent: restated, parity unpinned;
DESIGN 3.12).  ``__call__`` takes the reference's filename (.trk / .tck) or the
in-memory ``Tractogram`` of ``Tracker.track_and_validate``.

With ``compute_ic=True`` the streamlines left without a bundle are tested
against the distinct head / tail ROIs (``rois_and_pairs``,
``ttl_tractometer_invalid``): one that connects two ROIs no bundle joins is an
invalid connection, and IC / IS / IB / NC are filled.  ``score`` returns the
full result (per-bundle VS, WPC, TP, FP, FN, OL, OR, f1, the invalid bundles and
the per-streamline ``bundle`` / ``pair`` arrays) that
``ttl_score_tractogram.py`` writes.

``__call__`` and ``score`` share the intake of experiment/oracle_validator.py
(``corner_voxels``) and the one device pass here: ``segment`` (classify, overlap,
invalid) and its ``summary``, the single read-back, which names what it holds.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from tracktolearn_amd import _lib
from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                          corner_voxels_from_rasmm,
                                                          launch_ragged, load_tractogram, pack,
                                                          reference_space, tract_coverage)
from tracktolearn_amd.experiment.validators import Validator

def_len = [0, np.inf]
MAX_BUNDLES = 64
MAX_ROIS = 128          # TTL_TRACTOMETER_MAX_ROIS
CONFIG_NAME = 'scil_scoring_config.json'
# columns of a bundle's row of limits (TTL_TRACTOMETER_LIMITS doubles, ttl_hip.h)
LIM_LENGTH, LIM_DIR, LIM_ABSDIR, LIM_ANGLE, LIM_COLUMNS = 0, 2, 8, 14, 16


# ------------------------------------------------------------------- config
def read_config_file(gt_config, gt_dir='', use_gt_masks_as_all_masks=False):
    """tractometer_validator.py:69-229: (bundles, gt_masks, all_masks,
    any_masks, roi_options, lengths, angles, orientation_lengths,
    abs_orientation_lengths), one entry per bundle in the file's order, None
    where the config sets nothing; file names joined to ``gt_dir``."""
    def path(name):
        return os.path.join(gt_dir, name) if gt_dir else name

    with open(gt_config, 'r') as json_file:
        config = json.load(json_file)
    bundles = list(config.keys())
    out = {k: [] for k in ('gt', 'all', 'any', 'roi', 'length', 'angle', 'dir', 'absdir')}
    for bundle in bundles:
        cfg = config[bundle]
        if 'endpoints' not in cfg and 'head' not in cfg:
            raise ValueError("Bundle configuration for bundle {} misses 'endpoints' or "
                             "'head'/'tail'".format(bundle))
        scalars = {}
        gt_mask = all_mask = any_mask = roi_option = None
        for key in cfg.keys():
            if key in ('angle', 'length', 'length_x', 'length_y', 'length_z', 'length_x_abs',
                       'length_y_abs', 'length_z_abs'):
                scalars[key] = cfg[key]
            elif key == 'gt_mask':
                gt_mask = path(cfg['gt_mask'])
                if use_gt_masks_as_all_masks:
                    all_mask = gt_mask
            elif key == 'all_mask':
                if use_gt_masks_as_all_masks:
                    raise ValueError('With the option --use_gt_masks_as_all_masks, you should '
                                     'not add any all_mask in the config file.')
                all_mask = path(cfg['all_mask'])
            elif key == 'endpoints':
                if 'head' in cfg or 'tail' in cfg:
                    raise ValueError('Bundle {} has confusing keywords in the config file. '
                                     'Please choose either endpoints OR head/tail.'
                                     .format(bundle))
                roi_option = {'gt_endpoints': path(cfg['endpoints'])}
            elif key == 'head':
                if 'tail' not in cfg:
                    raise ValueError('You have provided the head for bundle {}, but not the '
                                     'tail'.format(bundle))
                roi_option = {'gt_head': path(cfg['head']), 'gt_tail': path(cfg['tail'])}
            elif key == 'tail':
                pass    # dealt with at head
            elif key == 'any_mask':
                any_mask = path(cfg['any_mask'])
            else:
                raise ValueError('Unrecognized value {} in the config file for bundle {}'
                                 .format(key, bundle))
        if roi_option is None:      # a tail without a head
            raise ValueError("Bundle configuration for bundle {} misses 'endpoints' or "
                             "'head'/'tail'".format(bundle))
        out['angle'].append(scalars.get('angle'))
        out['length'].append(scalars.get('length'))
        for name, suffix in (('dir', ''), ('absdir', '_abs')):
            xyz = [scalars.get(f'length_{a}{suffix}') for a in 'xyz']
            out[name].append(None if all(v is None for v in xyz) else
                             [v if v is not None else def_len for v in xyz])
        out['gt'].append(gt_mask)
        out['all'].append(all_mask)
        out['any'].append(any_mask)
        out['roi'].append(roi_option)
    return (bundles, out['gt'], out['all'], out['any'], out['roi'], out['length'],
            out['angle'], out['dir'], out['absdir'])


def compute_endpoint_masks(roi_options):
    """(tails, heads) file names per bundle (tractometer_validator.py:232-261).
    A bundle given as ``endpoints`` has no head and tail to return: the
    reference fails on it with a KeyError, here the error says why."""
    for opt in roi_options:
        if 'gt_head' not in opt or 'gt_tail' not in opt:
            raise ValueError(
                "a bundle configured with 'endpoints' has no 'head' and 'tail': the "
                'Tractometer validator needs the two ROIs as separate masks '
                f"(got {opt.get('gt_endpoints')!r})")
    return [o['gt_tail'] for o in roi_options], [o['gt_head'] for o in roi_options]


def rois_and_pairs(gt_tails, gt_heads):
    """(rois, valid, pairs) of the invalid connections (ttl_hip.h,
    ttl_tractometer_invalid): ``rois`` the distinct head / tail files sorted as
    strings, ``valid`` bool (R, R), True where some bundle joins the two ROIs
    and on the diagonal, ``pairs`` the invalid (i, j), i < j, in lexicographic
    order."""
    rois = sorted(set(list(gt_tails) + list(gt_heads)))
    index = {name: r for r, name in enumerate(rois)}
    valid = np.eye(len(rois), dtype=bool)
    for tail, head in zip(gt_tails, gt_heads):
        valid[index[tail], index[head]] = valid[index[head], index[tail]] = True
    pairs = [(i, j) for i in range(len(rois)) for j in range(i + 1, len(rois))
             if not valid[i, j]]
    return rois, valid, pairs


def roi_names(rois):
    """The ROI files' names without directory and extension; when two files
    share one, every name gets its index."""
    names = []
    for path in rois:
        name = os.path.basename(str(path))
        for ext in ('.nii.gz', '.nii', '.trk', '.tck'):
            if name.lower().endswith(ext):
                name = name[:-len(ext)]
                break
        names.append(name)
    if len(set(names)) != len(names):
        names = [f'{name}_{r}' for r, name in enumerate(names)]
    return names


# -------------------------------------------------------------- host packing
def dilate(mask, iterations):
    """``scipy.ndimage.binary_dilation(mask, iterations=k)`` with its default
    structure (the 6-neighbour cross; outside the volume counts as 0), written
    with shifts.  k = 0: no dilation."""
    m = np.asarray(mask) != 0
    for _ in range(int(iterations)):
        out = m.copy()
        for axis in range(m.ndim):
            lo = [slice(None)] * m.ndim
            hi = [slice(None)] * m.ndim
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            out[hi] |= m[lo]
            out[lo] |= m[hi]
        m = out
    return m


def pack_bit_planes(masks, dims, missing=False):
    """uint64 [X * Y * Z], C order: bit b is set where ``masks[b]`` is non-zero;
    a bundle whose mask is None has its bit set everywhere when ``missing``."""
    if len(masks) > MAX_BUNDLES:
        raise ValueError(f'{len(masks)} bundles: the bit planes hold at most {MAX_BUNDLES}')
    dims = tuple(int(v) for v in dims)
    planes = np.zeros(dims, np.uint64)
    for b, mask in enumerate(masks):
        bit = np.uint64(1) << np.uint64(b)
        if mask is None:
            if missing:
                planes |= bit
            continue
        mask = np.asarray(mask)
        if mask.shape != dims:
            raise ValueError(f'mask of bundle {b} has shape {mask.shape}, expected {dims}')
        planes[mask != 0] |= bit
    return planes.reshape(-1)


def pack_roi_words(masks, dims):
    """uint64 [X * Y * Z][W], W = (R + 63) // 64: bit r % 64 of word r // 64 is
    set where ``masks[r]`` is non-zero; the words of a voxel are adjacent."""
    R = len(masks)
    if not 2 <= R <= MAX_ROIS:
        raise ValueError(f'{R} distinct head / tail ROIs: the invalid connections take 2 to '
                         f'{MAX_ROIS}')
    dims = tuple(int(v) for v in dims)
    words = np.zeros(dims + ((R + 63) // 64,), np.uint64)
    for r, mask in enumerate(masks):
        mask = np.asarray(mask)
        if mask.shape != dims:
            raise ValueError(f'mask of ROI {r} has shape {mask.shape}, expected {dims}')
        word = words[..., r // 64]
        word[mask != 0] |= np.uint64(1) << np.uint64(r % 64)
    return words.reshape(-1, words.shape[-1])


def pack_valid_words(valid):
    """uint64 [R][W]: bit j of row i where ``valid[i, j]`` or i == j."""
    valid = np.asarray(valid, bool) | np.eye(len(valid), dtype=bool)
    words = np.zeros((len(valid), (len(valid) + 63) // 64), np.uint64)
    for i, j in zip(*np.nonzero(valid)):
        words[i, j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return words


def bundle_word(flags):
    """The uint64 whose bit b is ``bool(flags[b])``."""
    return sum(1 << b for b, f in enumerate(flags) if f)


def limits_table(lengths, angles, orientation_lengths, abs_orientation_lengths):
    """float64 [B][16] (ttl_hip.h): {length lo, hi; dir x, y, z lo, hi; absdir
    x, y, z lo, hi; angle; unused}, -inf / +inf where nothing is set."""
    B = len(lengths)
    table = np.empty((B, LIM_COLUMNS), np.float64)
    table[:, 0:LIM_ANGLE:2] = -np.inf
    table[:, 1:LIM_ANGLE:2] = np.inf
    table[:, LIM_ANGLE] = np.inf
    table[:, LIM_ANGLE + 1] = 0.0
    for b in range(B):
        if lengths[b] is not None:
            table[b, LIM_LENGTH:LIM_LENGTH + 2] = lengths[b]
        for col, per_axis in ((LIM_DIR, orientation_lengths[b]),
                              (LIM_ABSDIR, abs_orientation_lengths[b])):
            if per_axis is not None:
                for k in range(3):
                    table[b, col + 2 * k:col + 2 * k + 2] = per_axis[k]
        if angles[b] is not None:
            table[b, LIM_ANGLE] = angles[b]
    return table


def metrics(n, per_bundle, counts, gt_sizes, invalid=None):
    """The returned dict from integers: n streamlines, ``per_bundle[b]``
    streamlines of bundle b, ``counts[b] = (|M_b & G_b|, |M_b \\ G_b|)``,
    ``gt_sizes[b]`` = |G_b| or None without a gt_mask.  ``invalid`` (compute_ic):
    (streamlines with an invalid pair, invalid pairs with a streamline); then
    IC = the former / n, IB = the latter, NC = (n - VS - #IC) / n, IS = IC + NC."""
    vs = int(sum(int(c) for c in per_bundle))
    vc = vs / n
    ols = []
    for b, size in enumerate(gt_sizes):
        if size is None:
            continue
        ols.append(int(counts[b][0]) / size if size else 0.0)
    out = {'VC': vc, 'IC': 0, 'IS': 0, 'NC': 1 - vc,
           'mean_OL': float(sum(ols) / len(ols)) if ols else 0.0,
           'VB': int(sum(1 for c in per_bundle if int(c) > 0)), 'IB': 0}
    if invalid is not None:
        n_ic, n_ib = (int(v) for v in invalid)
        out['IC'], out['NC'], out['IB'] = n_ic / n, (n - vs - n_ic) / n, n_ib
        out['IS'] = out['IC'] + out['NC']
    return out


def _ratio(num, den):
    return num / den if den else 0.0


def full_scores(n, names, per_bundle, counts, gt_sizes, wpc, invalid_bundles=None):
    """The full result from integers: the totals ``n, VS, VC, IC,
    IS, NC, VB, IB, mean_OL, mean_OR_gt, mean_OR_vs, mean_f1``, per bundle
    ``bundles[name] = {VS, WPC, TP, FP, FN, OL, OR_gt, OR_vs, f1}`` with TP =
    |M & G|, FP = |M \\ G|, FN = |G \\ M|, OL = TP / |G|, OR_gt = FP / |G|, OR_vs =
    FP / |M|, f1 = 2 TP / (|M| + |G|) (a ratio with a zero denominator is 0; None
    for a bundle without a gt_mask, which no mean counts), and
    ``invalid_bundles`` = {'<roiA>__<roiB>': streamlines}, given with its positive
    counts only, or None when the invalid connections were not computed (IC = IB
    = 0 and NC = 1 - VC, as ``metrics`` without them)."""
    invalid = None if invalid_bundles is None else \
        (sum(int(c) for c in invalid_bundles.values()), len(invalid_bundles))
    m = metrics(n, per_bundle, counts, gt_sizes, invalid)
    bundles, per_gt = {}, {'OR_gt': [], 'OR_vs': [], 'f1': []}
    for b, name in enumerate(names):
        entry = {'VS': int(per_bundle[b]), 'WPC': int(wpc[b])}
        size = gt_sizes[b]
        if size is None:
            entry.update(dict.fromkeys(('TP', 'FP', 'FN', 'OL', 'OR_gt', 'OR_vs', 'f1')))
        else:
            tp, fp = int(counts[b][0]), int(counts[b][1])
            entry.update(TP=tp, FP=fp, FN=size - tp, OL=_ratio(tp, size),
                         OR_gt=_ratio(fp, size), OR_vs=_ratio(fp, tp + fp),
                         f1=_ratio(2 * tp, tp + fp + size))
            for key in per_gt:
                per_gt[key].append(entry[key])
        bundles[name] = entry
    means = {key: float(sum(v) / len(v)) if v else 0.0 for key, v in per_gt.items()}
    return {'n': int(n), 'VS': int(sum(int(c) for c in per_bundle)), 'VC': m['VC'],
            'IC': m['IC'], 'IS': m['IS'], 'NC': m['NC'], 'VB': m['VB'], 'IB': m['IB'],
            'mean_OL': m['mean_OL'], 'mean_OR_gt': means['OR_gt'], 'mean_OR_vs': means['OR_vs'],
            'mean_f1': means['f1'], 'bundles': bundles,
            'invalid_bundles': dict(invalid_bundles or {})}


# ------------------------------------------------------------ device wrappers
def _as_device_words(array, device):
    """A uint64 NumPy array as an int64 device tensor (the same bits)."""
    return torch.from_numpy(np.ascontiguousarray(array, np.uint64).view(np.int64)).to(device)


class ScoringData(object):
    """The packed scoring set on the device: bit planes head / tail / all / any
    / gt (uint64 words held in int64 tensors), the limits table, and the words
    naming the bundles with an all_mask / any_mask.  For the invalid
    connections, when ``roi_masks`` (the dilated masks of ``rois_and_pairs``'
    ROIs) and ``valid`` are given: the ROI planes ``roi`` [X * Y * Z][W] and
    the matrix ``valid`` [R][W]; otherwise both are None."""

    def __init__(self, dims, heads, tails, all_masks, any_masks, gt_masks, limits, device,
                 roi_masks=None, valid=None):
        self.dims = tuple(int(v) for v in dims)
        self.n_bundles = len(heads)
        if not 1 <= self.n_bundles <= MAX_BUNDLES:
            raise ValueError(f'{self.n_bundles} bundles: the Tractometer validator takes 1 to '
                             f'{MAX_BUNDLES}')
        self.device = torch.device(device)
        self.head = _as_device_words(pack_bit_planes(heads, dims), device)
        self.tail = _as_device_words(pack_bit_planes(tails, dims), device)
        self.all = _as_device_words(pack_bit_planes(all_masks, dims, missing=True), device)
        self.any = _as_device_words(pack_bit_planes(any_masks, dims), device)
        self.gt = _as_device_words(pack_bit_planes(gt_masks, dims), device)
        self.has_all = bundle_word(m is not None for m in all_masks)
        self.has_any = bundle_word(m is not None for m in any_masks)
        limits = np.ascontiguousarray(limits, np.float64)
        assert limits.shape == (self.n_bundles, LIM_COLUMNS), limits.shape
        self.limits = torch.from_numpy(limits).to(device)
        self.gt_sizes = [None if m is None else int(np.count_nonzero(m)) for m in gt_masks]
        self.n_rois, self.roi, self.valid = 0, None, None
        if roi_masks is not None:
            self.n_rois = len(roi_masks)
            valid = np.asarray(valid, bool)
            assert valid.shape == (self.n_rois, self.n_rois), valid.shape
            self.roi = _as_device_words(pack_roi_words(roi_masks, dims), device)
            self.valid = _as_device_words(pack_valid_words(valid), device)


def classify(points, offsets, data, lin):
    """``ttl_tractometer_classify`` on device tensors: (bundle int32 [n],
    connected int64 [n] holding the uint64 bit sets)."""
    n = max(len(offsets) - 1, 0)
    bundle = torch.empty(n, dtype=torch.int32, device=points.device)
    connected = torch.empty(n, dtype=torch.int64, device=points.device)
    if n:
        launch_ragged('ttl_tractometer_classify', points, offsets, data.dims, after=(
            data.n_bundles, data.head.data_ptr(), data.tail.data_ptr(), data.all.data_ptr(),
            data.any.data_ptr(), data.has_all, data.has_any, data.limits.data_ptr(),
            _lib.lin9(lin), bundle.data_ptr(), connected.data_ptr()))
    return bundle, connected


def overlap(points, offsets, bundle, data, visited_bits=None):
    """``ttl_tractometer_overlap`` on device tensors: (counts int64 [B][2],
    visited_bits int64 [X * Y * Z] holding the uint64 words).  ``visited_bits``
    (zeroed) may be given."""
    X, Y, Z = data.dims
    if visited_bits is None:
        visited_bits = torch.zeros(X * Y * Z, dtype=torch.int64, device=points.device)
    counts = torch.empty((data.n_bundles, 2), dtype=torch.int64, device=points.device)
    # no row still launches: the counts are written
    launch_ragged('ttl_tractometer_overlap', points, offsets, data.dims, (bundle.data_ptr(),),
                  (data.n_bundles, data.gt.data_ptr(), visited_bits.data_ptr(),
                   counts.data_ptr()))
    return counts, visited_bits


def invalid(points, offsets, bundle, data):
    """``ttl_tractometer_invalid`` on device tensors: pair int32 [n], i * R + j
    of the first invalid pair of ROIs a row without a bundle connects, else -1.
    ``data`` holds the ROI planes (``ScoringData(..., roi_masks, valid)``)."""
    if data.roi is None:
        raise ValueError('the scoring data was packed without the ROI planes of the invalid '
                         'connections (compute_ic)')
    pair = torch.empty(max(len(offsets) - 1, 0), dtype=torch.int32, device=points.device)
    if len(pair):
        launch_ragged('ttl_tractometer_invalid', points, offsets, data.dims, (bundle.data_ptr(),),
                      (data.n_rois, data.roi.data_ptr(), data.valid.data_ptr(), pair.data_ptr()))
    return pair


def segment(points, offsets, data, lin, compute_ic=False):
    """The one device pass on the intake's arrays: upload, classify, overlap
    and, when ``compute_ic`` and ``data`` holds the ROI planes, invalid."""
    points = torch.from_numpy(points).to(data.device)
    offsets = torch.from_numpy(offsets).to(data.device)
    bundle, connected = classify(points, offsets, data, lin)
    counts, _ = overlap(points, offsets, bundle, data)
    pair = invalid(points, offsets, bundle, data) if compute_ic and data.roi is not None else None
    return Segmentation(data, bundle, connected, counts, pair)


class Segmentation(object):
    """What the device pass left on the device: ``bundle`` int32 [n],
    ``connected`` int64 [n], ``counts`` int64 [B][2] and ``pair`` int32 [n], or
    None when the invalid connections were not computed."""

    def __init__(self, data, bundle, connected, counts, pair=None):
        self.data, self.bundle, self.connected = data, bundle, connected
        self.counts, self.pair = counts, pair

    def summary(self, wpc=False, per_pair=False):
        """The one read-back, as named host integers: ``per_bundle`` [B]
        streamlines per bundle, ``counts`` [B][2], ``wpc`` [B] (when asked, else
        None) the rows without a bundle that connect a bundle's ROIs, ``invalid``
        = (streamlines with an invalid pair, invalid pairs with a streamline) and,
        when asked, ``per_pair`` [R * R] streamlines per pair i * R + j; both None
        without ``pair``."""
        B, R, dev = self.data.n_bundles, self.data.n_rois, self.bundle.device
        parts = {'per_bundle': torch.bincount(self.bundle.to(torch.int64) + 1,
                                              minlength=B + 1)[1:],
                 'counts': self.counts.reshape(-1)}
        if wpc:
            wrong = self.connected[(self.bundle < 0) & (self.connected != 0)]
            parts['wpc'] = ((wrong[:, None] >> torch.arange(B, device=dev)) & 1).sum(0)
        if self.pair is not None:
            pairs = torch.bincount(self.pair.to(torch.int64) + 1, minlength=R * R + 1)[1:]
            if per_pair:
                parts['per_pair'] = pairs
            else:
                parts['invalid'] = torch.stack([pairs.sum(), (pairs > 0).sum()])
        back = torch.cat(list(parts.values())).cpu().numpy()
        cuts = np.cumsum([len(part) for part in parts.values()])[:-1]
        back = dict(zip(parts, np.split(back, cuts)))
        if per_pair and self.pair is not None:
            back['invalid'] = (back['per_pair'].sum(), np.count_nonzero(back['per_pair']))
        return SimpleNamespace(per_bundle=back['per_bundle'], counts=back['counts'].reshape(B, 2),
                               wpc=back.get('wpc'), invalid=back.get('invalid'),
                               per_pair=back.get('per_pair'))


# ---------------------------------------------------------------- validator
def _load_image(path):
    from tracktolearn_amd.io import nifti
    return nifti.load(path)


class TractometerValidator(Validator):
    """``TractometerValidator(base_dir, reference, dilate_endpoints, device)
    (tractogram_or_filename, env)`` -> ``{'VC', 'IC', 'IS', 'NC', 'mean_OL',
    'VB', 'IB'}``, ``{}`` without a streamline of >= 2 points.  ``reference``:
    the NIfTI file of the Tractometer's reference anatomy, or None to score in
    the env's reference space (``reference_space``).  ``compute_ic``: also
    segment the invalid connections; ``__call__`` then fills IC, IS, IB and NC.
    ``score`` gives the full result."""

    def __init__(self, base_dir, reference, dilate_endpoints=1, device='cuda',
                 compute_ic=False):
        self.name = 'Tractometer'
        self.compute_ic = bool(compute_ic)
        self.gt_config = os.path.join(base_dir, CONFIG_NAME)
        if not os.path.isfile(self.gt_config):
            raise ValueError(f'the Tractometer validator needs {CONFIG_NAME} in the scoring '
                             f'data, {self.gt_config} does not exist')
        self.gt_dir = base_dir
        self.reference = reference
        self.dilation_factor = int(dilate_endpoints)
        self.device = torch.device(device)
        self.ref_affine = self.dims = None
        if reference is not None:
            img = _load_image(reference)
            self.ref_affine = np.asarray(img.affine, np.float64)
            self.dims = tuple(int(v) for v in img.shape[:3])

        (self.bundle_names, gt_files, all_files, any_files, roi_options, self.bundle_lengths,
         self.angles, self.orientation_lengths, self.abs_orientation_lengths) = \
            read_config_file(self.gt_config, self.gt_dir, False)
        if len(self.bundle_names) > MAX_BUNDLES:
            raise ValueError(f'{len(self.bundle_names)} bundles in {self.gt_config}: the '
                             f'Tractometer validator takes at most {MAX_BUNDLES}')
        if not self.bundle_names:
            raise ValueError(f'{self.gt_config} names no bundle')
        self.gt_tails, self.gt_heads = compute_endpoint_masks(roi_options)

        cache = {}
        heads = [dilate(self._mask(f, cache), self.dilation_factor) for f in self.gt_heads]
        tails = [dilate(self._mask(f, cache), self.dilation_factor) for f in self.gt_tails]
        optional = [[None if f is None else self._mask(f, cache) for f in files]
                    for files in (all_files, any_files, gt_files)]
        limits = limits_table(self.bundle_lengths, self.angles, self.orientation_lengths,
                              self.abs_orientation_lengths)
        self.rois = self.roi_names = roi_masks = valid = None
        if self.compute_ic:
            self.rois, valid, _ = rois_and_pairs(self.gt_tails, self.gt_heads)
            if len(self.rois) < 2:
                raise ValueError(f'{self.gt_config} names one head / tail ROI only: there is '
                                 'no pair of ROIs to connect (compute_ic)')
            self.roi_names = roi_names(self.rois)
            roi_masks = [dilate(self._mask(f, cache), self.dilation_factor) for f in self.rois]
        self.data = ScoringData(self.dims, heads, tails, *optional, limits, self.device,
                                roi_masks=roi_masks, valid=valid)

    def _mask(self, path, cache):
        """A scoring file as a boolean volume of the reference's dims: a NIfTI
        mask (non-zero = 1), or a .trk / .tck bundle turned into the map of the
        voxels it passes through (``ttl_tract_coverage``)."""
        if path in cache:
            return cache[path]
        if str(path).lower().endswith(('.nii', '.nii.gz')):
            img = _load_image(path)
            mask = np.asarray(img.dataobj) != 0
            if self.dims is None:
                self.dims = tuple(int(v) for v in mask.shape[:3])
        else:
            mask = self._mask_from_bundle(path)
        if tuple(mask.shape) != tuple(self.dims):
            raise ValueError(f'{path}: dimensions {tuple(mask.shape)} differ from the '
                             f"reference's {tuple(self.dims)}")
        cache[path] = mask
        return mask

    def _mask_from_bundle(self, path):
        tract, header = load_tractogram(path)
        if header is not None:                   # a .trk: its own header is its reference
            affine = np.asarray(header['voxel_to_rasmm'], np.float64)
            dims = tuple(int(v) for v in header['dimensions'])
        elif self.ref_affine is None:
            raise ValueError(f'{path}: a .tck bundle needs --tractometer_reference')
        else:
            affine, dims = self.ref_affine, self.dims
        if self.dims is None:
            self.dims = dims
        # not the intake: a one-point row of a bundle still marks its voxel
        points, offsets = pack([np.asarray(s) for s in tract.streamlines if len(s) >= 1])
        points = corner_voxels_from_rasmm(points, affine)
        visited = tract_coverage(torch.from_numpy(points).to(self.device),
                                 torch.from_numpy(offsets).to(self.device), dims)
        return visited.cpu().numpy().reshape(dims) != 0

    def space(self, env):
        """(vox -> RAS mm affine, dims) the streamlines are scored in."""
        if self.ref_affine is not None:
            return self.ref_affine, self.dims
        affine, dims = reference_space(env)
        if tuple(dims) != tuple(self.dims):
            raise ValueError(f"the env's reference has dimensions {tuple(dims)}, the scoring "
                             f'data {tuple(self.dims)}: give --tractometer_reference')
        return affine, dims

    def __call__(self, tractogram_or_filename, env):
        ref_affine, _ = self.space(env)
        points, offsets, _ = corner_voxels(tractogram_or_filename, ref_affine,
                                           env.affine_vox2rasmm)
        n = len(offsets) - 1
        if n == 0:
            return {}
        s = segment(points, offsets, self.data, ref_affine[:3, :3], self.compute_ic).summary()
        return metrics(n, s.per_bundle, s.counts, self.data.gt_sizes, invalid=s.invalid)

    # ---- the full result
    def load(self, filename):
        """A .trk / .tck for ``score_loaded``: (tractogram in RAS+mm, the .trk's
        header dict or None, the vox -> RAS mm affine it is scored in: the
        reference's when one was given, else the .trk's own)."""
        tract, header = load_tractogram(filename)
        if self.ref_affine is not None:
            return tract, header, self.ref_affine
        if header is None:
            raise ValueError(f'{filename}: a .tck needs a reference')
        if tuple(int(v) for v in header['dimensions']) != tuple(self.dims):
            raise ValueError(f"{filename}: its header's dimensions "
                             f"{tuple(header['dimensions'])} differ from the scoring data's "
                             f'{tuple(self.dims)}: give a reference')
        return tract, header, np.asarray(header['voxel_to_rasmm'], np.float64)

    def corner_voxels(self, tractogram_or_filename, env=None):
        """(points, offsets, index, affine): the streamlines with >= 2 points
        in the voxel space they are scored in, corner origin, packed; ``index``
        their numbers in the input; ``affine`` that space's vox -> RAS mm."""
        if isinstance(tractogram_or_filename, FILENAME):
            tract, _, affine = self.load(os.fsdecode(tractogram_or_filename))
            return corner_voxels(tract, affine, in_rasmm=True) + (affine,)
        # without an env the intake raises before it looks at the affine
        affine = None if env is None else self.space(env)[0]
        return corner_voxels(tractogram_or_filename, affine,
                             getattr(env, 'affine_vox2rasmm', None)) + (affine,)

    def score(self, tractogram_or_filename, env=None):
        """The full result of ``full_scores`` plus ``bundle`` and ``pair`` (int32
        per streamline with >= 2 points; pair = -1 everywhere without
        compute_ic) and ``index``, those streamlines' numbers in the input.
        A file needs no env when a reference was given, a .trk none at all.
        ``{}`` without a streamline of >= 2 points."""
        return self._score(*self.corner_voxels(tractogram_or_filename, env))

    def score_loaded(self, tractogram, affine, return_intake=False):
        """``score`` of what ``load`` returned.  ``return_intake``: (result,
        (points, offsets, index)) -- the rows that were scored, for a caller that
        goes on with them (``bundle`` of the result numbers these rows)."""
        intake = corner_voxels(tractogram, affine, in_rasmm=True)
        result = self._score(*intake, affine)
        return (result, intake) if return_intake else result

    def _score(self, points, offsets, index, affine):
        n = len(offsets) - 1
        if n == 0:
            return {}
        seg = segment(points, offsets, self.data, affine[:3, :3], self.compute_ic)
        s = seg.summary(wpc=True, per_pair=True)
        invalid_bundles, pair = None, np.full(n, -1, np.int32)
        if seg.pair is not None:
            R, pair = self.data.n_rois, seg.pair.cpu().numpy()
            invalid_bundles = {
                f'{self.roi_names[k // R]}__{self.roi_names[k % R]}': int(s.per_pair[k])
                for k in np.flatnonzero(s.per_pair)}
        out = full_scores(n, self.bundle_names, s.per_bundle, s.counts, self.data.gt_sizes,
                          s.wpc, invalid_bundles)
        out.update(bundle=seg.bundle.cpu().numpy(), pair=pair, index=index)
        return out


__all__ = ['TractometerValidator', 'ScoringData', 'read_config_file', 'compute_endpoint_masks',
           'dilate', 'pack_bit_planes', 'limits_table', 'metrics', 'classify', 'overlap',
           'rois_and_pairs', 'roi_names', 'pack_roi_words', 'pack_valid_words', 'full_scores',
           'invalid', 'segment', 'Segmentation']
