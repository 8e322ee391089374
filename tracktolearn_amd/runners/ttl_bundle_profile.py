#!/usr/bin/env python3
"""ttl_bundle_profile.py -- the tract profiles of segmented bundles on the MI355X.

    ttl_bundle_profile.py in_tractogram reference out_prefix --metric NAME=MAP [--metric ...]
        [--bundles IDS.npy] [--nb_points K] [--model CENTROIDS.npy] [--max_mdf MM]
        [--per_streamline] [-f]

``reference`` is the anatomy (.nii.gz) whose grid the maps are on.  ``--bundles``
names an int array with the bundle number of every streamline of the file (-1:
in no bundle); without it the whole file is one bundle.  Every streamline of 2
points or more, all finite, is resampled to K stations equidistant in arc length
in voxel units, oriented against its bundle's model and summed into the centroid;
every map is sampled at the oriented stations (bundle_profile.py).
``--model`` gives the model lines ((bundles, K, 3) float64, RAS mm: an
``out_prefix_centroids.npy`` of an earlier run) instead of seeding them from the
file.  Written: ``out_prefix_profiles.json`` (per bundle n, n_outliers, mdf_mean
and per map the mean, std and count at the K stations; null where there is none),
``out_prefix_centroids.npy`` (RAS mm, float64), ``out_prefix_centroids.trk`` and,
with ``--per_streamline``, ``out_prefix_<name>_streamlines.npy`` ((streamlines
of 2 points or more, K) float64, NaN where a station is not sampled).  A .trk
whose header is on another grid than the reference is an error.
"""
import argparse
import json
import os
from argparse import RawTextHelpFormatter

import numpy as np

from tracktolearn_amd.runners.ttl_score_tractogram import parse_metrics
from tracktolearn_amd.utils.torch_utils import get_device

OUTPUTS = ('_profiles.json', '_centroids.npy', '_centroids.trk')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawTextHelpFormatter)
    parser.add_argument('in_tractogram', help='Tractogram (.trk or .tck).')
    parser.add_argument('reference', help='Reference anatomy (.nii.gz): the grid of the maps.')
    parser.add_argument('out_prefix', help='Prefix of the files written.')
    parser.add_argument('--metric', action='append', default=[], metavar='NAME=MAP',
                        help='A scalar map (.nii.gz on the reference grid); repeatable.')
    parser.add_argument('--bundles', default=None, metavar='IDS.npy',
                        help='Bundle number of every streamline. [one bundle]')
    parser.add_argument('--nb_points', default=100, type=int, metavar='K',
                        help='Stations per bundle, 2 .. 256. [%(default)s]')
    parser.add_argument('--model', default=None, metavar='CENTROIDS.npy',
                        help='Model lines (bundles, K, 3) in RAS mm. [seeded from the file]')
    parser.add_argument('--max_mdf', default=None, type=float, metavar='MM',
                        help='Leave streamlines further than MM mm from the model they were\n'
                             'oriented against (the centroid of the pass before, or --model)\n'
                             'out of the profiles.')
    parser.add_argument('--per_streamline', action='store_true',
                        help='Also out_prefix_<name>_streamlines.npy: the samples of every row.')
    parser.add_argument('-f', dest='overwrite', action='store_true',
                        help='Force overwriting of the output files.')
    args = parser.parse_args(argv)
    for f in (args.in_tractogram, args.reference, args.bundles, args.model):
        if f is not None and not os.path.isfile(f):
            parser.error(f'{f} does not exist')
    if not args.in_tractogram.lower().endswith(('.trk', '.tck')):
        parser.error(f'{args.in_tractogram}: a tractogram is read from a .trk or .tck file')
    if not args.metric:
        parser.error('at least one --metric NAME=MAP is required')
    args.metric = parse_metrics(parser, args.metric)
    if not 2 <= args.nb_points <= 256:
        parser.error('--nb_points must be in 2 .. 256')
    written = OUTPUTS + (tuple(f'_{m}_streamlines.npy' for m in args.metric)
                         if args.per_streamline else ())
    held = [args.out_prefix + s for s in written if os.path.exists(args.out_prefix + s)]
    if held and not args.overwrite:
        parser.error(f'{held[0]} exists; use -f to overwrite')
    return args


def main(argv=None):
    args = parse_args(argv)
    from tracktolearn_amd.bundle_profile import BundleProfiles, json_ready
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
    if args.bundles is None:
        bundle = np.zeros(len(tract), np.int32)
    else:
        bundle = np.load(args.bundles)
        if bundle.shape != (len(tract),) or bundle.dtype.kind not in 'iu':
            raise ValueError(f'{args.bundles}: {len(tract)} streamlines need as many integer '
                             f'bundle numbers, not {bundle.dtype} {bundle.shape}')
        bundle = bundle.astype(np.int32)
    n_bundles = max(int(bundle.max()) + 1 if bundle.size else 1, 1)
    model = None
    if args.model is not None:
        ras = np.load(args.model).astype(np.float64)
        if ras.shape != (n_bundles, args.nb_points, 3):
            raise ValueError(f'{args.model}: {ras.shape} is not (bundles, K, 3) = '
                             f'{(n_bundles, args.nb_points, 3)}')
        inv = np.linalg.inv(np.asarray(ref.affine, np.float64))
        model = ras @ inv[:3, :3].T + inv[:3, 3] + 0.5
    profiles = BundleProfiles(dims, ref.affine, [f'bundle_{b}' for b in range(n_bundles)],
                              nb_points=args.nb_points, device=get_device(),
                              n_iter=1 if model is not None else 2, max_mdf=args.max_mdf,
                              model=model)
    profiles.add_tractogram(tract, bundle, in_rasmm=True)
    for name, path in args.metric.items():
        profiles.add_metric(name, np.asarray(nifti.load(path).get_fdata(), np.float32),
                            per_streamline=args.per_streamline)
    profiles.save(args.out_prefix, per_streamline=args.per_streamline)
    print(json.dumps(json_ready({name: {k: p[k] for k in ('n', 'n_outliers', 'mdf_mean')}
                                 for name, p in profiles.profiles().items()})))


if __name__ == '__main__':
    main()
