#!/usr/bin/env python3
"""ttl_recognize_bundles.py -- the bundle of every streamline, from an atlas of model
lines, on the MI355X.

    ttl_recognize_bundles.py in_tractogram reference atlas out_prefix
        [--atlas_labels IDS.npy --nb_points K] [--atlas_names NAMES.json] [--max_mdf MM]
        [--max_ratio R] [--save_bundles] [--profile NAME=MAP ...]
        [--register {rigid,similarity,affine} [--register_max_fixed N]
         [--register_no_progressive]] [-f]

``reference`` is the subject's anatomy (.nii.gz); the atlas is taken to be in its
space unless ``--register`` fits it to the tractogram first (bundle_register.py,
DESIGN 3.20: the transform that minimises the bundle-minimum distance between at
most ``--register_max_fixed`` streamlines and the model lines, through translation,
rigid and similarity up to the kind asked for unless ``--register_no_progressive``);
what follows then uses the moved atlas, and ``out_prefix_registration.json`` holds
the matrix (atlas mm -> subject mm), the parameters, the kind, the centre, the costs
before and after and the number of evaluations.  ``atlas`` is an ``out_prefix_centroids.npy`` of ttl_bundle_profile.py
((bundles, K, 3) float64, RAS mm: one model line per bundle), or a .trk / .tck of
model lines with ``--atlas_labels`` (the bundle number of every line) resampled to
``--nb_points`` stations.  ``--atlas_names``: a JSON list of bundle names, or a
``_profiles.json`` whose keys are the names; bundle_0, bundle_1, ... without it.
Every streamline of 2 points or more, all finite, gets the bundle of the model line
at the smallest minimum-average-direct-flip distance (bundle_recognize.py, DESIGN
3.19); it gets -1 when that distance exceeds ``--max_mdf`` mm, or ``--max_ratio``
times the distance to the nearest model of another bundle.  Written:
``out_prefix_bundles.npy`` (int32, one number per streamline of the file: what
ttl_bundle_profile.py --bundles reads), ``out_prefix_recognized.npy`` (a structured
array, one record per streamline of the file: model i4, flip i4, mdf f8, runner_up
f8; -1 / 0 / NaN / NaN where there is none), ``out_prefix_recognized.json`` (per
bundle n, mdf_mean, n_gated; null where there is none) and, with ``--save_bundles``,
``out_prefix_<name>.trk`` per bundle that has a streamline.  ``--profile`` runs the
tract profiles of the recognised bundles on the maps given (atlases of one model line
per bundle): the files of ttl_bundle_profile.py --bundles out_prefix_bundles.npy
--model atlas, in the same run.  A .trk whose header is on another grid than the
reference is an error.
"""
import argparse
import json
import os
from argparse import RawTextHelpFormatter

import numpy as np

from tracktolearn_amd.runners.ttl_score_tractogram import parse_metrics
from tracktolearn_amd.utils.torch_utils import get_device

OUTPUTS = ('_bundles.npy', '_recognized.npy', '_recognized.json')
PROFILE_OUTPUTS = ('_profiles.json', '_centroids.npy', '_centroids.trk')
REGISTER_OUTPUT = '_registration.json'
RECORD = np.dtype([('model', '<i4'), ('flip', '<i4'), ('mdf', '<f8'), ('runner_up', '<f8')])


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=RawTextHelpFormatter)
    parser.add_argument('in_tractogram', help='Tractogram (.trk or .tck).')
    parser.add_argument('reference', help='Reference anatomy (.nii.gz) of the subject.')
    parser.add_argument('atlas', help='Model lines: a _centroids.npy, or a .trk / .tck with\n'
                                      '--atlas_labels.')
    parser.add_argument('out_prefix', help='Prefix of the files written.')
    parser.add_argument('--atlas_labels', default=None, metavar='IDS.npy',
                        help='Bundle number of every line of a .trk / .tck atlas.')
    parser.add_argument('--nb_points', default=None, type=int, metavar='K',
                        help='Stations of a .trk / .tck atlas, 2 .. 256. [20]')
    parser.add_argument('--atlas_names', default=None, metavar='NAMES.json',
                        help='Bundle names: a JSON list, or a _profiles.json. [bundle_<number>]')
    parser.add_argument('--max_mdf', default=None, type=float, metavar='MM',
                        help='No bundle for a streamline further than MM mm from its model.')
    parser.add_argument('--max_ratio', default=None, type=float, metavar='R',
                        help='No bundle when the distance exceeds R times the distance to the\n'
                             'nearest model of another bundle.')
    parser.add_argument('--save_bundles', action='store_true',
                        help='Also out_prefix_<name>.trk per bundle that has a streamline.')
    parser.add_argument('--profile', action='append', default=[], metavar='NAME=MAP',
                        help='Also the tract profiles of a scalar map (.nii.gz on the\n'
                             'reference grid); repeatable.')
    parser.add_argument('--register', default=None, choices=('rigid', 'similarity', 'affine'),
                        help='Fit the atlas to the tractogram first (streamline-based linear\n'
                             'registration); also out_prefix_registration.json.')
    parser.add_argument('--register_max_fixed', default=None, type=int, metavar='N',
                        help='Streamlines of the tractogram the fit uses at most. [4096]')
    parser.add_argument('--register_no_progressive', action='store_true',
                        help='Fit --register at once, not translation -> rigid -> ... first.')
    parser.add_argument('-f', dest='overwrite', action='store_true',
                        help='Force overwriting of the output files.')
    args = parser.parse_args(argv)
    if args.register is None and (args.register_max_fixed is not None or
                                  args.register_no_progressive):
        parser.error('--register_max_fixed and --register_no_progressive only with --register')
    if args.register_max_fixed is None:
        args.register_max_fixed = 4096
    if args.register_max_fixed < 1:
        parser.error('--register_max_fixed must be 1 or more')
    for f in (args.in_tractogram, args.reference, args.atlas, args.atlas_labels,
              args.atlas_names):
        if f is not None and not os.path.isfile(f):
            parser.error(f'{f} does not exist')
    if not args.in_tractogram.lower().endswith(('.trk', '.tck')):
        parser.error(f'{args.in_tractogram}: a tractogram is read from a .trk or .tck file')
    lines = args.atlas.lower().endswith(('.trk', '.tck'))
    if not lines and not args.atlas.lower().endswith('.npy'):
        parser.error(f'{args.atlas}: an atlas is a _centroids.npy, or a .trk or .tck file')
    if lines and args.atlas_labels is None:
        parser.error(f'{args.atlas}: an atlas of lines needs --atlas_labels IDS.npy')
    if not lines and (args.atlas_labels is not None or args.nb_points is not None):
        parser.error('--atlas_labels and --nb_points only with a .trk or .tck atlas')
    if args.nb_points is None:
        args.nb_points = 20
    if not 2 <= args.nb_points <= 256:
        parser.error('--nb_points must be in 2 .. 256')
    for name in ('max_mdf', 'max_ratio'):
        value = getattr(args, name)
        if value is not None and not value > 0:
            parser.error(f'--{name} must be positive')
    args.profile = parse_metrics(parser, args.profile)
    written = OUTPUTS + (PROFILE_OUTPUTS if args.profile else ()) + \
        ((REGISTER_OUTPUT,) if args.register else ())
    held = [args.out_prefix + s for s in written if os.path.exists(args.out_prefix + s)]
    if held and not args.overwrite:
        parser.error(f'{held[0]} exists; use -f to overwrite')
    return args


def bundle_file(prefix, name):
    return f'{prefix}_{name}.trk'


def main(argv=None):
    args = parse_args(argv)
    from tracktolearn_amd.bundle_profile import BundleProfiles, json_ready
    from tracktolearn_amd.bundle_recognize import BundleAtlas, read_names
    from tracktolearn_amd.experiment.oracle_validator import load_tractogram
    from tracktolearn_amd.io import nifti
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.tractogram import Tractogram
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
    device = get_device()
    if args.atlas_labels is None:
        atlas = BundleAtlas.from_centroids(args.reference, args.atlas, args.atlas_names,
                                           device=device)
    else:
        label = np.load(args.atlas_labels)
        if label.ndim != 1 or label.dtype.kind not in 'iu' or (label.size and label.min() < 0):
            raise ValueError(f'{args.atlas_labels}: one bundle number >= 0 per line of the atlas, '
                             f'not {label.dtype} {label.shape}')
        names = [f'bundle_{b}' for b in range(int(label.max()) + 1 if label.size else 1)]
        if args.atlas_names is not None:
            with open(args.atlas_names) as f:
                names = read_names(json.load(f))
        atlas = BundleAtlas.from_tractogram(args.reference, args.atlas, label, names,
                                            args.nb_points, device=device)
    if args.profile and (atlas.one_model_per_label() is None or len(atlas.names) > 64):
        raise ValueError('--profile needs an atlas of one model line per bundle, 64 bundles at '
                         'most')
    folder = os.path.dirname(os.path.abspath(args.out_prefix))
    os.makedirs(folder, exist_ok=True)
    if args.register:
        from tracktolearn_amd.bundle_register import register_atlas
        fit = register_atlas(atlas, tract, in_rasmm=True, kind=args.register,
                             progressive=not args.register_no_progressive,
                             max_fixed=args.register_max_fixed)
        atlas = fit['atlas']
        record = {'kind': fit['kind'], 'matrix': fit['matrix'].tolist(),
                  'params': fit['params'].tolist(), 'centre': fit['centre'].tolist(),
                  'cost_before': fit['cost_before'], 'cost_after': fit['cost_after'],
                  'evaluations': fit['evaluations'], 'n_fixed': fit['n_fixed'],
                  'n_moving': fit['n_moving']}
        with open(args.out_prefix + REGISTER_OUTPUT, 'w') as f:
            json.dump(json_ready(record), f, indent=2, allow_nan=False)
    models = atlas.one_model_per_label()
    got = atlas.recognize(tract, in_rasmm=True, max_mdf=args.max_mdf, max_ratio=args.max_ratio)
    np.save(args.out_prefix + OUTPUTS[0], got['bundle'])
    record = np.zeros(len(got['bundle']), RECORD)
    for key in RECORD.names:
        record[key] = got[key]
    np.save(args.out_prefix + OUTPUTS[1], record)
    summary = json_ready(atlas.summary())
    with open(args.out_prefix + OUTPUTS[2], 'w') as f:
        json.dump(summary, f, indent=2, allow_nan=False)
    if args.save_bundles:
        trk_header = sio.create_tractogram_header(
            atlas.affine, dims, np.sqrt((atlas.lin * atlas.lin).sum(0)))
        for b, name in enumerate(atlas.names):
            rows = np.flatnonzero(got['bundle'] == b)
            if rows.size:
                sio.save(Tractogram([tract.streamlines[i] for i in rows.tolist()],
                                    affine_to_rasmm=np.eye(4)),
                         bundle_file(args.out_prefix, name), trk_header)
    if args.profile:
        profiles = BundleProfiles(dims, ref.affine, atlas.names, nb_points=atlas.K, device=device,
                                  n_iter=1, max_mdf=args.max_mdf, model=models)
        profiles.add_tractogram(tract, got['bundle'], in_rasmm=True)
        for name, path in args.profile.items():
            profiles.add_metric(name, np.asarray(nifti.load(path).get_fdata(), np.float32))
        profiles.save(args.out_prefix)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
