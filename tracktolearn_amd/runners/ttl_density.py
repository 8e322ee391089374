#!/usr/bin/env python3
"""ttl_density.py -- the track density maps of a tractogram on the MI355X.

    ttl_density.py in_tractogram reference out_prefix [--zoom K] [--dec] [-f]

``reference`` is the anatomy (.nii.gz) whose grid the maps are on; with
``--zoom K`` (1 .. 8) the maps are K times finer along every axis
(super-resolution: the affine's linear part divided by K).  Every streamline
of 2 points or more, all finite, is walked through the voxels (density.py,
DESIGN 3.17).  Written: ``out_prefix_count.nii.gz`` (int32: streamlines per
voxel, each counted once however often it comes back),
``out_prefix_length.nii.gz`` (float32: mm of streamline in the voxel),
``out_prefix_ends.nii.gz`` (float32: streamline ends in the voxel), with
``--dec`` ``out_prefix_dec.nii.gz`` ((X, Y, Z, 3) float32: the mm along x, y
and z), and ``out_prefix.json`` (rows added and skipped, zoom, dims, set sizes,
rows per set).  A .trk whose header is on another grid than the reference is
an error.
"""
import argparse
import json
import os
from argparse import RawTextHelpFormatter

import numpy as np

from tracktolearn_amd.utils.torch_utils import get_device

OUTPUTS = ('_count.nii.gz', '_length.nii.gz', '_ends.nii.gz', '.json')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawTextHelpFormatter)
    parser.add_argument('in_tractogram', help='Tractogram (.trk or .tck).')
    parser.add_argument('reference', help='Reference anatomy (.nii.gz): the grid of the maps.')
    parser.add_argument('out_prefix', help='Prefix of the files written.')
    parser.add_argument('--zoom', default=1, type=int, metavar='K',
                        help='Super-resolution factor, 1 .. 8. [%(default)s]')
    parser.add_argument('--dec', action='store_true',
                        help='Also out_prefix_dec.nii.gz: the mm per voxel along x, y and z.')
    parser.add_argument('-f', dest='overwrite', action='store_true',
                        help='Force overwriting of the output files.')
    args = parser.parse_args(argv)
    for f in (args.in_tractogram, args.reference):
        if not os.path.isfile(f):
            parser.error(f'{f} does not exist')
    if not args.in_tractogram.lower().endswith(('.trk', '.tck')):
        parser.error(f'{args.in_tractogram}: a tractogram is read from a .trk or .tck file')
    if not 1 <= args.zoom <= 8:
        parser.error('--zoom must be in 1 .. 8')
    written = OUTPUTS + (('_dec.nii.gz',) if args.dec else ())
    held = [args.out_prefix + s for s in written if os.path.exists(args.out_prefix + s)]
    if held and not args.overwrite:
        parser.error(f'{held[0]} exists; use -f to overwrite')
    return args


def main(argv=None):
    args = parse_args(argv)
    from tracktolearn_amd.density import DensityMap
    from tracktolearn_amd.experiment.oracle_validator import load_tractogram
    from tracktolearn_amd.io import nifti
    ref = nifti.load(args.reference)
    dims = tuple(int(v) for v in ref.shape[:3])
    tract, header = load_tractogram(args.in_tractogram)
    if header is not None and (
            tuple(int(v) for v in header['dimensions']) != dims or
            not np.allclose(np.asarray(header['voxel_to_rasmm'], np.float64), ref.affine,
                            atol=1e-3)):
        raise ValueError(f"{args.in_tractogram}'s header (shape "
                         f"{tuple(int(v) for v in header['dimensions'])}) is not on the grid of "
                         f'{args.reference} (shape {dims})')
    density = DensityMap(dims, ref.affine, zoom=args.zoom, device=get_device(), dec=args.dec)
    density.add_tractogram(tract, in_rasmm=True)
    density.save(args.out_prefix)
    print(json.dumps(density.totals()))


if __name__ == '__main__':
    main()
