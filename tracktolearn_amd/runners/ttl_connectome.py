#!/usr/bin/env python3
"""ttl_connectome.py -- the structural connectome of a tractogram on the MI355X.

    ttl_connectome.py in_tractogram labels out_prefix
        [--reference NIFTI] [--radius MM] [--metric NAME=FILE ...]
        [--save_assignments] [-f]

``labels`` is an integer image (.nii.gz): the values 1 .. N name the nodes.
Every streamline of 2 points or more gets the node at either end -- the label
of the end's own voxel or, outside every node, the nearest labelled voxel
centre within ``--radius`` mm -- and its length in mm (connectome.py, DESIGN
3.15).  Written: ``out_prefix_count.npy`` ((N, N) int64, symmetric),
``out_prefix_mean_length.npy`` (mm; 0 where the count is 0),
``out_prefix_count.csv`` and ``out_prefix.json`` (totals, radius, node count);
with ``--save_assignments`` also ``out_prefix_nodes.npy``: rows of (index in
the input, node of the first point, node of the last), 0 = no node, -1 = not
scored.  Every ``--metric NAME=FILE`` (a scalar map on the labels' grid: FA, MD,
AFD; there is no resampling) adds ``out_prefix_mean_NAME.npy``: per edge the mean
over its streamlines of the map's arc-length weighted mean along each (DESIGN
3.16; NaN where no streamline contributed), and with ``--save_assignments``
``out_prefix_NAME_streamlines.npy``: rows of (index in the input, mean, weight
in mm), NaN and 0 without a mean.  A .tck input needs ``--reference``, the
anatomy whose grid the labels are on; a .trk is read in its header's space
unless one is given.
"""
import argparse
import json
import os
from argparse import RawTextHelpFormatter

import numpy as np

from tracktolearn_amd.utils.torch_utils import get_device

OUTPUTS = ('_count.npy', '_mean_length.npy', '_count.csv', '.json')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawTextHelpFormatter)
    parser.add_argument('in_tractogram', help='Tractogram (.trk or .tck).')
    parser.add_argument('labels', help='Label image (.nii.gz), integers 1 .. N.')
    parser.add_argument('out_prefix', help='Prefix of the files written.')
    parser.add_argument('--reference', default=None, metavar='NIFTI',
                        help='Reference anatomy: the grid of the label image.')
    parser.add_argument('--radius', default=2.0, type=float, metavar='MM',
                        help='Search radius round an end outside every node. [%(default)s]')
    parser.add_argument('--metric', action='append', default=[], metavar='NAME=FILE',
                        help='Scalar map (.nii.gz) on the grid of the label image; writes\n'
                             'out_prefix_mean_NAME.npy. May be given several times.')
    parser.add_argument('--save_assignments', action='store_true',
                        help='Write out_prefix_nodes.npy: (index, node0, node1) per streamline,\n'
                             'and per metric out_prefix_NAME_streamlines.npy: (index, mean, '
                             'weight).')
    parser.add_argument('-f', dest='overwrite', action='store_true',
                        help='Force overwriting of the output files.')
    args = parser.parse_args(argv)
    try:
        args.metric = metric_options(args.metric)
    except ValueError as e:
        parser.error(str(e))
    for f in (args.in_tractogram, args.labels) + ((args.reference,) if args.reference else ()) \
            + tuple(f for _, f in args.metric):
        if not os.path.isfile(f):
            parser.error(f'{f} does not exist')
    lower = args.in_tractogram.lower()
    if not lower.endswith(('.trk', '.tck')):
        parser.error(f'{args.in_tractogram}: a tractogram is read from a .trk or .tck file')
    if lower.endswith('.tck') and args.reference is None:
        parser.error(f'{args.in_tractogram}: a .tck needs --reference')
    if not (np.isfinite(args.radius) and args.radius >= 0):
        parser.error('--radius must be >= 0 mm')
    written = OUTPUTS + (('_nodes.npy',) if args.save_assignments else ())
    for name, _ in args.metric:
        written += (f'_mean_{name}.npy',) + \
            ((f'_{name}_streamlines.npy',) if args.save_assignments else ())
    held = [args.out_prefix + s for s in written if os.path.exists(args.out_prefix + s)]
    if held and not args.overwrite:
        parser.error(f'{held[0]} exists; use -f to overwrite')
    return args


def metric_options(values):
    """[(name, file)] of the ``NAME=FILE`` options; ValueError for a malformed
    one or a name given twice."""
    from tracktolearn_amd.connectome import parse_metric
    pairs = [parse_metric(v) for v in values or ()]
    names = [name for name, _ in pairs]
    for name in names:
        if names.count(name) > 1:
            raise ValueError(f'metric {name} is given more than once')
    return pairs


def scoring_space(labels_img, header, reference, in_tractogram):
    """The voxel -> RAS mm affine the streamlines are read in: the reference's
    when one is given, else the .trk's own; either must be the label image's
    grid, shape and affine (to 1e-3, as ``ttl_track.load_on_mask_grid``)."""
    from tracktolearn_amd.io import nifti
    shape = tuple(int(v) for v in labels_img.shape[:3])
    if reference is not None:
        ref = nifti.load(reference)
        what, dims, affine = reference, tuple(int(v) for v in ref.shape[:3]), ref.affine
    else:
        what, dims = f"{in_tractogram}'s header", tuple(int(v) for v in header['dimensions'])
        affine = header['voxel_to_rasmm']
    affine = np.asarray(affine, np.float64)
    if dims != shape or not np.allclose(affine, labels_img.affine, atol=1e-3):
        raise ValueError(f'the label image (shape {shape}) is not on the grid of {what} '
                         f'(shape {dims}): '
                         + ('resample it' if reference is not None else 'give a reference'))
    return affine


def main(argv=None):
    args = parse_args(argv)
    from tracktolearn_amd.connectome import Connectome, load_metric
    from tracktolearn_amd.experiment.oracle_validator import load_tractogram
    from tracktolearn_amd.io import nifti
    labels_img = nifti.load(args.labels)
    tract, header = load_tractogram(args.in_tractogram)
    affine = scoring_space(labels_img, header, args.reference, args.in_tractogram)
    metrics = {name: load_metric(name, f, labels_img.shape[:3], labels_img.affine,
                                 f'the label image {args.labels}') for name, f in args.metric}
    connectome = Connectome(labels_img.get_fdata(dtype=np.float64), affine,
                            radius_mm=args.radius, device=get_device(), metrics=metrics)
    node, index = connectome.add_tractogram(tract, in_rasmm=True)
    connectome.save(args.out_prefix)
    if args.save_assignments:
        rows = np.full((len(tract.streamlines), 3), -1, np.int64)
        rows[:, 0] = np.arange(len(rows))
        rows[index, 1:] = node.cpu().numpy()
        np.save(args.out_prefix + '_nodes.npy', rows)
        for name, (mean, weight) in connectome.last_means.items():
            rows = np.zeros((len(tract.streamlines), 3), np.float64)
            rows[:, 0], rows[:, 1] = np.arange(len(rows)), np.nan
            rows[index, 1], rows[index, 2] = mean.cpu().numpy(), weight.cpu().numpy()
            np.save(f'{args.out_prefix}_{name}_streamlines.npy', rows)
    print(json.dumps(connectome.totals()))


if __name__ == '__main__':
    main()
