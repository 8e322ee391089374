#!/usr/bin/env python3
"""ttl_score_tractogram.py -- score a tractogram with the Tractometer on the MI355X.

    ttl_score_tractogram.py in_tractogram scoring_data out_dir
        [--reference NIFTI] [--dilate_endpoints K] [--compute_ic] [--save_bundles] [-f]
        [--profile NAME=MAP ...] [--profile_points K] [--profile_max_mdf MM]

``scoring_data`` holds ``scil_scoring_config.json`` and its masks, as for
``sac_auto_train.py --tractometer_validator``.  The streamlines are segmented
into the valid bundles and, with ``--compute_ic``, into the invalid
connections (experiment/tractometer_validator.py; scilpy's
segment-and-score restated, parity unpinned).  ``out_dir/results.json`` holds
the totals (VS, VC, IC, IS, NC, VB, IB, mean OL / OR / f1), the scores of every
bundle and the streamline count of every invalid bundle.  ``--save_bundles``
also writes the segmented streamlines, in the input's space and format and with
its data_per_streamline: ``segmented_VB/<bundle>_VS``,
``segmented_IB/<roiA>__<roiB>_IC`` and ``NC`` (everything else, rows of fewer
than 2 points included, which are not scored); empty files are not written.
A .tck input needs ``--reference``; a .trk is scored in its header's space
unless one is given.  With ``--profile NAME=MAP`` (repeatable; MAP a .nii.gz on
the scoring grid) the valid bundles are also profiled from the same intake
(bundle_profile.py): ``out_dir/profiles.json`` (per bundle the
mean, std and count of every map at K stations; null where there is none) and
``out_dir/profiles_centroids.npy`` ((bundles, K, 3) float64, RAS mm).
"""
import argparse
import json
import os
import shutil
from argparse import RawTextHelpFormatter

import numpy as np

from tracktolearn_amd.utils.torch_utils import get_device

ARRAYS = ('bundle', 'pair', 'index')        # of score(): not part of results.json


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawTextHelpFormatter)
    parser.add_argument('in_tractogram', help='Tractogram to score (.trk or .tck).')
    parser.add_argument('scoring_data',
                        help='Location of the tractometer scoring data.')
    parser.add_argument('out_dir', help='Directory of results.json and the bundles.')
    parser.add_argument('--reference', default=None, metavar='NIFTI',
                        help='Reference anatomy of the scoring data.')
    parser.add_argument('--dilate_endpoints', default=1, type=int, metavar='K',
                        help='Dilation factor for the ROIs. [%(default)s]')
    parser.add_argument('--compute_ic', action='store_true',
                        help='Also segment the invalid connections (IC, IS, IB).')
    parser.add_argument('--save_bundles', action='store_true',
                        help='Write the segmented streamlines next to results.json.')
    parser.add_argument('--profile', action='append', default=[], metavar='NAME=MAP',
                        help='Also profile the valid bundles along their length on the scalar\n'
                             'map MAP (.nii.gz on the scoring grid); repeatable.')
    parser.add_argument('--profile_points', default=None, type=int, metavar='K',
                        help='Stations per bundle, 2 .. 256. [100]')
    parser.add_argument('--profile_max_mdf', default=None, type=float, metavar='MM',
                        help='Leave streamlines further than MM mm from the model they were\n'
                             'oriented against (the centroid of the pass before) out of the\n'
                             'profiles.')
    parser.add_argument('-f', dest='overwrite', action='store_true',
                        help='Force overwriting of the output files.')
    args = parser.parse_args(argv)
    if not os.path.isfile(args.in_tractogram):
        parser.error(f'{args.in_tractogram} does not exist')
    if not args.profile and (args.profile_points is not None or
                             args.profile_max_mdf is not None):
        parser.error('--profile_points and --profile_max_mdf go only with --profile')
    args.profile = parse_metrics(parser, args.profile)
    if args.profile_points is None:
        args.profile_points = 100
    if not 2 <= args.profile_points <= 256:
        parser.error('--profile_points must be in 2 .. 256')
    if os.path.exists(os.path.join(args.out_dir, 'results.json')) and not args.overwrite:
        parser.error(f'{args.out_dir} holds results already; use -f to overwrite')
    return args


def parse_metrics(parser, pairs):
    """{name: file} of the NAME=MAP arguments; a parser error for a malformed or
    repeated name or a file that does not exist."""
    out = {}
    for pair in pairs:
        name, eq, path = pair.partition('=')
        if not (name and eq and path):
            parser.error(f'{pair}: a map is given as NAME=MAP')
        if name in out:
            parser.error(f'{name}: given twice')
        if not os.path.isfile(path):
            parser.error(f'{path} does not exist')
        out[name] = path
    return out


def split(result, n_input):
    """{relative file name without extension: input streamline numbers} of a
    ``score()`` result: a partition of range(n_input)."""
    bundle, pair, index = (result[k] for k in ARRAYS)
    names = list(result['bundles'])
    groups, rest = {}, np.ones(n_input, bool)
    for b in np.unique(bundle[bundle >= 0]):
        groups[os.path.join('segmented_VB', f'{names[b]}_VS')] = index[bundle == b]
    pair_names = list(result['invalid_bundles'])      # ascending pair numbers
    for name, p in zip(pair_names, np.unique(pair[pair >= 0])):
        groups[os.path.join('segmented_IB', f'{name}_IC')] = index[pair == p]
    for rows in groups.values():
        rest[rows] = False
    if rest.any():
        groups['NC'] = np.flatnonzero(rest)
    return groups


def save_bundles(tract, header, groups, out_dir, ext):
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
    for sub in ('segmented_VB', 'segmented_IB'):
        shutil.rmtree(os.path.join(out_dir, sub), ignore_errors=True)
        os.makedirs(os.path.join(out_dir, sub))
    if os.path.exists(os.path.join(out_dir, 'NC' + ext)):
        os.remove(os.path.join(out_dir, 'NC' + ext))
    for name, rows in groups.items():
        part = Tractogram([tract.streamlines[i] for i in rows],
                          {k: v[rows] for k, v in tract.data_per_streamline.items()})
        sio.save(part, os.path.join(out_dir, name + ext), header)


def write_profiles(args, validator, affine, intake, result):
    """profiles.json and profiles_centroids.npy of the valid bundles of ``result``,
    from the rows ``intake`` = (points, offsets, index) that were scored."""
    import torch

    from tracktolearn_amd.bundle_profile import BundleProfiles, json_ready
    from tracktolearn_amd.io import nifti
    profiles = BundleProfiles(validator.dims, affine, list(result['bundles']),
                              nb_points=args.profile_points, device=get_device(),
                              max_mdf=args.profile_max_mdf)
    profiles.fit(torch.from_numpy(intake[0]), torch.from_numpy(intake[1]),
                 torch.from_numpy(np.asarray(result['bundle'], np.int32)))
    for name, path in args.profile.items():
        profiles.add_metric(name, np.asarray(nifti.load(path).get_fdata(), np.float32))
    with open(os.path.join(args.out_dir, 'profiles.json'), 'w') as f:
        json.dump(json_ready(profiles.profiles()), f, indent=2, allow_nan=False)
    np.save(os.path.join(args.out_dir, 'profiles_centroids.npy'), profiles.centroids_rasmm())


def main(argv=None):
    args = parse_args(argv)
    from tracktolearn_amd.experiment.tractometer_validator import TractometerValidator
    validator = TractometerValidator(args.scoring_data, args.reference,
                                     dilate_endpoints=args.dilate_endpoints,
                                     device=get_device(), compute_ic=args.compute_ic)
    tract, header, affine = validator.load(args.in_tractogram)
    profiled = None
    if args.profile:        # one intake for the scores and the profiles
        result, profiled = validator.score_loaded(tract, affine, return_intake=True)
    else:
        result = validator.score_loaded(tract, affine)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, 'results.json'), 'w') as f:
        json.dump({k: v for k, v in result.items() if k not in ARRAYS}, f, indent=2)
    if result and args.profile:
        write_profiles(args, validator, affine, profiled, result)
    if not result:
        print(f'{args.in_tractogram}: no streamline of 2 points or more, nothing scored')
    elif args.save_bundles:
        ext = os.path.splitext(args.in_tractogram)[1].lower()
        save_bundles(tract, header, split(result, len(tract)), args.out_dir, ext)
    print(json.dumps({k: v for k, v in result.items()
                      if k not in ARRAYS + ('bundles', 'invalid_bundles')}))


if __name__ == '__main__':
    main()
