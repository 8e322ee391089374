#!/usr/bin/env python3
"""ttl_track.py -- generate a tractogram from a trained agent on the MI355X.

Same command line as TrackToLearn/runners/ttl_track.py:
    ttl_track.py in_odf in_seed in_mask out_tractogram [--input_wm]
        [--sh_basis B] [--compress T] [-f] [--save_seeds] [--agent DIR]
        [--hyperparameters JSON] [--n_actor N] [--npv N] [--min_length m]
        [--max_length M] [--noise s] [--keyed_noise] [--fa_map F] [--bidirectional]
        [--binary_stopping_threshold t] [--rng_seed S] [--direct_output]
        [--odf_policy {det,prob}] [--theta DEG] [--sf_threshold R] [--step_size MM]
        [--act_include FILE --act_exclude FILE] [--act_mode {act,cmc}]
        [--act_filter {none,exclude,endpoints}] [--act_in_step]
        [--connectome LABELS --connectome_out PREFIX] [--connectome_radius MM]
        [--connectome_only] [--connectome_metric NAME=FILE ...]
        [--density_map PREFIX] [--density_zoom K] [--density_dec] [--density_only]

With ``--odf_policy`` no agent is loaded: the streamlines follow the fODF
itself (classical deterministic / probabilistic tracking as one GPU kernel,
tracking/odf_policy.py).

With ``--act_include`` / ``--act_exclude`` (tissue maps on the grid of in_mask,
e.g. grey matter and CSF) a streamline also ends where it reaches the include
map -- validly -- or the exclude map -- it is then discarded (ACT), or with the
per-step probabilities of CMC (``--act_mode cmc``).  in_mask should then be a
brain mask (white and grey matter): a point that leaves in_mask in the step in
which it reaches the include map is still dropped.  ``--act_in_step`` has the
step's own launches apply the maps (``ttl_env_set_act``): the same tractogram,
byte for byte, with the graphed tracking loop.

With ``--connectome`` (a label image on the grid of in_mask) the node x node
matrices of the streamlines that are written (connectome.py) are
accumulated on the GPU while tracking; ``--connectome_only`` writes no
tractogram at all.  Every ``--connectome_metric NAME=FILE`` (a scalar map on the
same grid: FA, MD, AFD) adds PREFIX_mean_NAME.npy, the map's mean along the
streamlines of every edge.

With ``--density_map PREFIX`` the track density maps of the streamlines that
are written (density.py) are accumulated the same way on the grid
of in_mask, ``--density_zoom K`` times finer: PREFIX_count.nii.gz (streamlines
per voxel), PREFIX_length.nii.gz (mm of streamline per voxel),
PREFIX_ends.nii.gz, with ``--density_dec`` PREFIX_dec.nii.gz (the mm along x, y
and z) and PREFIX.json; ``--density_only`` writes no tractogram.  With
``--compress`` the maps are of the compressed points.

Launch with ``torchrun --nproc-per-node R`` to shard every seed batch over R
GPUs (volumes replicated, RCCL gather-to-root of the finished tracts, rank 0
writes the file).
"""
import argparse
import json
import os
import random
from argparse import RawTextHelpFormatter
from os.path import join

import numpy as np
import torch

from tracktolearn_amd.algorithms.sac_auto import SACAuto
from tracktolearn_amd.environments.noisy_tracking_env import \
    NoisyTrackingEnvironment
from tracktolearn_amd.io import nifti
from tracktolearn_amd.io import streamlines as sio
from tracktolearn_amd.tracking.tracker import Tracker, detect_format
from tracktolearn_amd.utils.torch_utils import get_device

_ROOT = os.sep.join(os.path.normpath(
    os.path.dirname(os.path.abspath(__file__))).split(os.sep)[:-2])
DEFAULT_MODEL = os.path.join(_ROOT, 'models')


def per_rank_noise_rng(rng_seed, rank):
    """Generator of the exploration noise of one rank of a sharded run.  The
    ranks must share ``rng_seed`` for seed generation and shuffling (every
    rank derives the same seed list and takes its slice of each batch), so
    the noise gets its own stream per rank; with one rank the env keeps the
    reference's single stream."""
    return np.random.RandomState((int(rng_seed) + 1 + int(rank)) % (2 ** 32))


def load_on_mask_grid(option, volume_file, in_mask):
    """The volume of ``option`` (float64), which must be on the tracking mask's grid."""
    vol = nifti.load(volume_file)
    mask = nifti.load(in_mask)
    if tuple(vol.shape[:3]) != tuple(mask.shape[:3]) or \
            not np.allclose(vol.affine, mask.affine, atol=1e-3):
        raise ValueError('{} {} is not on the grid of the tracking mask {}'.format(
            option, volume_file, in_mask))
    return np.asarray(vol.get_fdata(dtype=np.float64)).reshape(vol.shape[:3])


def load_fa_map(fa_map_file, in_mask):
    """The FA volume of ``--fa_map`` (float64), on the tracking mask's grid."""
    return load_on_mask_grid('--fa_map', fa_map_file, in_mask)


#: track_dto keys copied onto the experiment as they are (argparse names)
_PASS_THROUGH = ('in_odf', 'in_seed', 'in_mask', 'out_tractogram', 'noise',
                 'binary_stopping_threshold', 'n_actor', 'npv', 'min_length',
                 'max_length', 'sh_basis', 'save_seeds', 'agent', 'hyperparameters')

#: hyperparameters.json key -> attribute (the file a training run writes,
#: trainers/train.py; the shipped one is models/hyperparameters.json)
_HYPER = {'algorithm': 'algorithm', 'max_angle': 'theta', 'hidden_dims': 'hidden_dims',
          'n_dirs': 'n_dirs', 'target_sh_order': 'target_sh_order'}


class TrackToLearnTrack(object):
    """Tracking experiment: the noisy env built from files, a trained SACAuto
    policy, `Tracker.track`, a .trk / .tck file (runners/ttl_track.py:38-186 of
    the reference: same track_dto keys, same order of the side effects on the
    random generators)."""

    def __init__(self, track_dto):
        for key in _PASS_THROUGH:
            setattr(self, key, track_dto[key])
        self.input_wm = track_dto.get('input_wm', False)
        self.direct_output = bool(track_dto.get('direct_output', False))
        self.reference_file = self.in_mask
        self.compress = track_dto['compress'] or 0.0
        # tracking never computes rewards and never consults the oracle
        self.compute_reward, self.alignment_weighting = False, 0.0
        self.oracle_checkpoint, self.oracle_bonus = None, 0.0
        self.oracle_stopping_criterion = False
        # --fa_map implies keyed noise: only the in-kernel draw scales by FA
        self.fa_map_file = track_dto.get('fa_map')
        self.keyed_noise = bool(track_dto.get('keyed_noise')) or bool(self.fa_map_file)
        self.bidirectional = bool(track_dto.get('bidirectional'))
        # tissue maps: ACT / CMC stopping and the filter of the output stage
        self.act_include_file = track_dto.get('act_include')
        self.act_exclude_file = track_dto.get('act_exclude')
        self.act_mode = track_dto.get('act_mode') or 'act'
        self.act_filter = track_dto.get('act_filter') or 'exclude'
        if not self.act_include_file:
            self.act_filter = None
        self.act_in_step = bool(track_dto.get('act_in_step')) and bool(self.act_include_file)
        # the structural connectome of the streamlines that are written
        self.connectome_file = track_dto.get('connectome')
        self.connectome_out = track_dto.get('connectome_out')
        self.connectome_radius = track_dto.get('connectome_radius')
        if self.connectome_radius is None:
            self.connectome_radius = 2.0
        self.connectome_only = bool(track_dto.get('connectome_only'))
        self.connectome_metric = list(track_dto.get('connectome_metric') or ())
        # the track density maps of the streamlines that are written
        self.density_map = track_dto.get('density_map')
        self.density_zoom = track_dto.get('density_zoom') or 1
        self.density_dec = bool(track_dto.get('density_dec'))
        self.density_only = bool(track_dto.get('density_only'))
        self.fa_map = None
        self.device = torch.device('cuda', torch.cuda.current_device()) \
            if torch.cuda.is_available() else get_device()
        self.odf_policy = track_dto.get('odf_policy')
        if self.odf_policy:
            self._odf_settings(track_dto)
        else:
            with open(self.hyperparameters, 'r') as json_file:
                hyper = json.load(json_file)
            for key, attr in _HYPER.items():
                setattr(self, attr, hyper[key])
            self.step_size = float(hyper['step_size'])
            self.voxel_size = hyper.get('voxel_size', 2.0)
        self.random_seed = track_dto['rng_seed']
        torch.manual_seed(self.random_seed)
        np.random.seed(self.random_seed)
        random.seed(self.random_seed)
        self.rng = np.random.RandomState(seed=self.random_seed)

    #: the env's curvature criterion is this much wider than the policy's cone:
    #: the cone decides, not the rounding of the segment rebuilt from two points
    ODF_CURVATURE_MARGIN = 5.0

    def _odf_settings(self, track_dto):
        """What hyperparameters.json supplies for an agent, for ``--odf_policy``:
        the SH order of the file, the step in mm as given, the cone."""
        from tracktolearn_amd.datasets.utils import get_sh_order_and_fullness
        from tracktolearn_amd.tracking.odf_policy import DEFAULT_THETA
        self.algorithm, self.hidden_dims = 'OdfTracking', None
        self.n_dirs = 4
        self.odf_theta = float(track_dto.get('theta') or DEFAULT_THETA[self.odf_policy])
        self.sf_threshold = float(track_dto.get('sf_threshold', 0.1))
        self.theta = min(self.odf_theta + self.ODF_CURVATURE_MARGIN, 180.0)
        self.target_sh_order = get_sh_order_and_fullness(
            nifti.load(self.in_odf).shape[-1])[0]
        self.step_size = float(track_dto.get('step_size') or 0.75)
        self.voxel_size = None

    def get_tracking_env(self):
        """The noisy env over the input files (experiment.py:177-204)."""
        env_dto = {key: getattr(self, key) for key in (
            'fa_map', 'n_dirs', 'theta', 'min_length', 'max_length', 'noise', 'npv',
            'rng', 'alignment_weighting', 'oracle_bonus', 'oracle_stopping_criterion',
            'oracle_checkpoint', 'binary_stopping_threshold', 'compute_reward',
            'device', 'target_sh_order', 'in_odf', 'in_seed', 'in_mask', 'sh_basis',
            'input_wm')}
        env_dto.update(dataset_file=None, scoring_data=None, step_size=self.step_size,
                       reference=self.in_odf)
        if self.keyed_noise:
            env_dto.update(device_noise='keyed', noise_seed=self.random_seed)
        if self.fa_map_file:
            env_dto['fa_map'] = load_fa_map(self.fa_map_file, self.in_mask)
        if self.act_include_file:
            env_dto.update(
                act_include=load_on_mask_grid('--act_include', self.act_include_file,
                                              self.in_mask),
                act_exclude=load_on_mask_grid('--act_exclude', self.act_exclude_file,
                                              self.in_mask),
                act_mode=self.act_mode, act_seed=self.random_seed,
                act_in_step=self.act_in_step)
        return NoisyTrackingEnvironment.from_files(env_dto)

    def _step_for_subject(self, subject_voxel_size):
        """Keep the number of voxels traversed per step of the training: an agent
        trained at another voxel size steps proportionally (ttl_track.py:145-157)."""
        if self.voxel_size is None:         # --odf_policy: the step is given in mm
            return self.step_size
        trained = float(self.voxel_size)
        if abs(float(subject_voxel_size) - trained) < 0.1:
            return self.step_size
        step_size_mm = float(subject_voxel_size) / trained * self.step_size
        print('Agent was trained on a voxel size of {}mm and a step size '
              'of {}mm.'.format(self.voxel_size, self.step_size))
        print('Subject has a voxel size of {}mm, setting step size to '
              '{}mm.'.format(subject_voxel_size, step_size_mm))
        return step_size_mm

    def _load_policy(self, env):
        if self.odf_policy:
            from tracktolearn_amd.tracking.odf_policy import OdfTracking
            print('Tracking with the fODF ({}).'.format(self.odf_policy))
            return OdfTracking(env, self.odf_policy, self.odf_theta, self.sf_threshold,
                               seed=self.random_seed)
        input_size = env.reset(0, 1).shape[1]
        print('Tracking with {} agent.'.format(self.algorithm))
        alg = {'SACAuto': SACAuto}[self.algorithm](
            input_size, env.get_action_size(), self.hidden_dims, n_actors=self.n_actor,
            rng=self.rng, device=self.device, replay_size=1)
        alg.agent.load(self.agent, 'last_model_state')
        return alg

    def run(self):
        ref_img = nifti.load(self.reference_file)
        env = self.get_tracking_env()
        env.step_size_mm = self._step_for_subject(ref_img.get_zooms()[0])
        alg = self._load_policy(env)
        connectome = None
        if self.connectome_file:
            from tracktolearn_amd.connectome import Connectome, load_metric
            labels = load_on_mask_grid('--connectome', self.connectome_file, self.in_mask)
            metrics = {name: load_metric(name, f, labels.shape,
                                         nifti.load(self.connectome_file).affine,
                                         f'the label image {self.connectome_file}')
                       for name, f in self.connectome_metric}
            connectome = Connectome(labels, ref_img.affine, radius_mm=self.connectome_radius,
                                    device=self.device, metrics=metrics)
        density = None
        if self.density_map:
            from tracktolearn_amd.density import DensityMap
            mask_shape = tuple(int(v) for v in nifti.load(self.in_mask).shape[:3])
            density = DensityMap(mask_shape, ref_img.affine, zoom=self.density_zoom,
                                 device=self.device, dec=self.density_dec)
        tracker = Tracker(alg, self.n_actor, compress=self.compress,
                          min_length=self.min_length, max_length=self.max_length,
                          save_seeds=self.save_seeds, bidirectional=self.bidirectional,
                          act_filter=self.act_filter, connectome=connectome, density=density)
        # re-derives the step in voxels, the step counts and the neighbourhood
        # radius from the rescaled step (environments/env.py:196-212)
        env.load_subject()
        if tracker.group_size > 1 and not self.keyed_noise:
            # (keyed noise needs no generator: every shard resets with its global
            # start offset, so the streamline ids are those of the one-GPU run)
            env.noise_rng = per_rank_noise_rng(self.random_seed, tracker.rank)
        header = sio.create_tractogram_header(
            ref_img.affine, ref_img.shape[:3], ref_img.get_zooms()[:3])
        if self.connectome_only or self.density_only:
            # either walks the batches without writing them and feeds both products
            (tracker.track_connectome if connectome is not None else tracker.track_density)(env)
            n = None
        else:
            n = tracker.save(env, self.out_tractogram, header, direct=self.direct_output)
        if connectome is not None:
            connectome.save(self.connectome_out)
            totals = connectome.totals()
            print('Saved the connectome of {} streamlines ({} nodes, {} connected, {} skipped) '
                  'to {}'.format(totals['streamlines'], totals['n_nodes'], totals['connected'],
                                 totals['skipped'], self.connectome_out))
        if density is not None:
            density.save(self.density_map)
            totals = density.totals()
            print('Saved the density maps of {} streamlines ({} skipped, grid {}) to {}'.format(
                totals['added'], totals['skipped'], 'x'.join(str(v) for v in totals['dims']),
                self.density_map))
        if n is None:           # not rank 0, --connectome_only or --density_only
            return
        print('Saved {} streamlines to {}'.format(n, self.out_tractogram))


def add_mandatory_options_tracking(p):
    p.add_argument('in_odf',
                   help='File containing the orientation diffusion function \n'
                        'as spherical harmonics file (.nii.gz). Ex: ODF or '
                        'fODF.')
    p.add_argument('in_seed', help='Seeding mask (.nii.gz).')
    p.add_argument('in_mask', help='Tracking mask (.nii.gz).\nTracking will '
                                   'stop outside this mask.')
    p.add_argument('out_tractogram',
                   help='Tractogram output file (must be .trk or .tck).')
    p.add_argument('--input_wm', action='store_true',
                   help='If set, append the WM mask to the input signal.')


def add_out_options(p):
    out_g = p.add_argument_group('Output options')
    out_g.add_argument('--compress', type=float, metavar='thresh',
                       help='If set, will compress streamlines. The parameter '
                            'value is the \ndistance threshold.')
    out_g.add_argument('-f', dest='overwrite', action='store_true',
                       help='Force overwriting of the output files.')
    out_g.add_argument('--save_seeds', action='store_true',
                       help='If set, save the seeds used for the tracking \n '
                            'in the data_per_streamline property.')
    out_g.add_argument('--direct_output', action='store_true',
                       help='Build the file records on the GPU and write each '
                            'seed batch with one write,\ninstead of one Python '
                            'object per streamline. Points may differ from the\n'
                            'default in the last float32 bit.')
    return out_g


def add_track_args(parser):
    add_mandatory_options_tracking(parser)
    basis_group = parser.add_argument_group('Basis options')
    basis_group.add_argument('--sh_basis', default='descoteaux07',
                             choices=['descoteaux07', 'tournier07'],
                             help='Spherical harmonics basis used for the SH '
                                  'coefficients. [%(default)s]')
    add_out_options(parser)
    agent_group = parser.add_argument_group('Tracking agent options')
    agent_group.add_argument('--agent', type=str,
                             help='Path to the folder containing .pth files.\n'
                                  '[{}]'.format(DEFAULT_MODEL))
    agent_group.add_argument('--hyperparameters', type=str,
                             help='Path to the .json file containing the '
                                  'hyperparameters of your tracking agent.')
    agent_group.add_argument('--n_actor', type=int, default=10000, metavar='N',
                             help='Number of streamlines to track simultaneous'
                                  'ly. [%(default)s]')
    seed_group = parser.add_argument_group('Seeding options')
    seed_group.add_argument('--npv', type=int, default=1,
                            help='Number of seeds per voxel [%(default)s].')
    track_g = parser.add_argument_group('Tracking options')
    track_g.add_argument('--min_length', type=float, default=10., metavar='m',
                         help='Minimum length of a streamline in mm. '
                              '[%(default)s]')
    track_g.add_argument('--max_length', type=float, default=300., metavar='M',
                         help='Maximum length of a streamline in mm. '
                              '[%(default)s]')
    track_g.add_argument('--noise', default=0.0, type=float, metavar='sigma',
                         help='Add noise ~ N (0, `noise`) to the agent\'s\n'
                              'output to make tracking more probabilistic.'
                              '[%(default)s]')
    track_g.add_argument('--keyed_noise', action='store_true',
                         help='Draw the noise on the GPU as a function of '
                              '(--rng_seed, seed index, step):\nthe tractogram '
                              'no longer depends on --n_actor or on the number '
                              'of GPUs.\nNot the NumPy stream of the default.')
    track_g.add_argument('--bidirectional', action='store_true',
                         help='Track both ways from every seed: the streamline '
                              'is turned round at the end of\nits forward half '
                              'and tracked on from the seed, so that it runs '
                              'through its seed.')
    track_g.add_argument('--fa_map', type=str, default=None,
                         help='Scale the added noise according to an FA map '
                              '(.nii.gz on the grid of\nin_mask): std = '
                              '(1 - FA) * `noise`. Implies --keyed_noise.')
    track_g.add_argument('--binary_stopping_threshold', type=float, default=0.1,
                         help='Lower limit for interpolation of tracking mask '
                              'value.\nTracking will stop below this '
                              'threshold.')
    odf_g = parser.add_argument_group(
        'Classical tracking from the fODF',
        'Without a trained agent: follow the fODF itself. Makes --agent and '
        '--hyperparameters\nunnecessary.')
    odf_g.add_argument('--odf_policy', choices=['det', 'prob'], default=None,
                       help='det: at each step the strongest direction of the '
                            'spherical function inside a cone\naround the '
                            'previous direction; prob: one sampled in '
                            'proportion to it, as a function of\n(--rng_seed, '
                            'seed index, step).')
    odf_g.add_argument('--theta', type=float, default=None, metavar='DEG',
                       help='Half angle of the cone in degrees. [45 for det, 20 '
                            'for prob]')
    odf_g.add_argument('--sf_threshold', type=float, default=None, metavar='R',
                       help='Directions below this share of the spherical '
                            'function\'s maximum are not followed. [0.1]')
    odf_g.add_argument('--step_size', type=float, default=None, metavar='MM',
                       help='Step size in mm. [0.75]')
    act_g = parser.add_argument_group(
        'Anatomically constrained tracking',
        'Stop on tissue maps (on the grid of in_mask), as ACT / CMC do. in_mask '
        'should then be\na brain mask (white and grey matter).')
    act_g.add_argument('--act_include', type=str, default=None, metavar='FILE',
                       help='Map (.nii.gz) in which a streamline ends validly, e.g. '
                            'grey matter.')
    act_g.add_argument('--act_exclude', type=str, default=None, metavar='FILE',
                       help='Map (.nii.gz) in which a streamline ends invalidly, '
                            'e.g. CSF.')
    act_g.add_argument('--act_mode', choices=['act', 'cmc'], default=None,
                       help='act: stop where a map exceeds 0.5, include first; cmc: '
                            'stop with the\nper-step probabilities of continuous map '
                            'criterion, as a function of\n(--rng_seed, seed index, '
                            'step). [act]')
    act_g.add_argument('--act_filter', choices=['none', 'exclude', 'endpoints'],
                       default=None,
                       help='exclude: discard streamlines the exclude map ended; '
                            'endpoints: also those\nwith an end outside the include '
                            'map; none: keep all. [exclude]')
    act_g.add_argument('--act_in_step', action='store_true',
                       help='Apply the maps inside the tracking step instead of '
                            'between its two halves:\nthe same streamlines, and the '
                            'graphed tracking loop stays available.')
    con_g = parser.add_argument_group(
        'Structural connectome',
        'The node x node matrices of the streamlines that are written, accumulated on '
        'the GPU\nwhile tracking (one process only).')
    con_g.add_argument('--connectome', type=str, default=None, metavar='LABELS',
                       help='Label image (.nii.gz, integers 1 .. N, on the grid of in_mask).')
    con_g.add_argument('--connectome_out', type=str, default=None, metavar='PREFIX',
                       help='Writes PREFIX_count.npy, PREFIX_mean_length.npy, '
                            'PREFIX_count.csv and PREFIX.json.')
    con_g.add_argument('--connectome_radius', type=float, default=None, metavar='MM',
                       help='An end outside every node takes the nearest labelled voxel '
                            'centre within\nthis distance. [2.0]')
    con_g.add_argument('--connectome_only', action='store_true',
                       help='Write the connectome and no tractogram.')
    con_g.add_argument('--connectome_metric', action='append', default=None,
                       metavar='NAME=FILE',
                       help='Scalar map (.nii.gz, on the grid of the label image): writes '
                            'PREFIX_mean_NAME.npy,\nits mean along the streamlines of every '
                            'edge. May be given several times.')
    den_g = parser.add_argument_group(
        'Track density maps',
        'Streamlines, mm of streamline and ends per voxel of the streamlines that are '
        'written,\naccumulated on the GPU while tracking (one process only). With --compress '
        'the maps are\nof the compressed points.')
    den_g.add_argument('--density_map', type=str, default=None, metavar='PREFIX',
                       help='Writes PREFIX_count.nii.gz, PREFIX_length.nii.gz, '
                            'PREFIX_ends.nii.gz and PREFIX.json.')
    den_g.add_argument('--density_zoom', type=int, default=None, metavar='K',
                       help='Super-resolution: a grid K times finer than in_mask, 1 .. 8. [1]')
    den_g.add_argument('--density_dec', action='store_true',
                       help='Also PREFIX_dec.nii.gz: the mm per voxel along x, y and z.')
    den_g.add_argument('--density_only', action='store_true',
                       help='Write the maps and no tractogram.')
    parser.add_argument('--rng_seed', default=1337, type=int,
                        help='Random number generator seed [%(default)s].')


def verify_agent_option(parser, args):
    if (args.agent is not None and args.hyperparameters is None) or \
       (args.agent is None and args.hyperparameters is not None):
        parser.error('You must specify both --agent and --hyperparameters '
                     'arguments or use the default model.')
    if args.agent is None:
        args.agent = DEFAULT_MODEL
        args.hyperparameters = join(DEFAULT_MODEL, 'hyperparameters.json')


def parse_args(argv=None):
    """ Generate a tractogram from a trained model. """
    parser = argparse.ArgumentParser(description=parse_args.__doc__,
                                     formatter_class=RawTextHelpFormatter)
    add_track_args(parser)
    args = parser.parse_args(argv)
    for f in (args.in_odf, args.in_seed, args.in_mask):
        if not os.path.isfile(f):
            parser.error('Input file {} does not exist.'.format(f))
    if os.path.isfile(args.out_tractogram) and not args.overwrite:
        parser.error('Output file {} exists. Use -f to force overwriting.'
                     .format(args.out_tractogram))
    if detect_format(args.out_tractogram) is None:
        parser.error('Invalid output streamline file format (must be trk or '
                     'tck): {0}'.format(args.out_tractogram))
    if args.min_length < 0 or args.max_length < args.min_length:
        parser.error('min_length must be >= 0 and <= max_length.')
    if args.compress is not None and not 0.001 <= args.compress <= 1:
        parser.error('The compression threshold must be in [0.001, 1] mm.')
    if (args.act_include is None) != (args.act_exclude is None):
        parser.error('--act_include and --act_exclude go together.')
    if args.act_include is None:
        for name in ('act_mode', 'act_filter'):
            if getattr(args, name) is not None:
                parser.error('--{} is used only with --act_include / --act_exclude.'
                             .format(name))
        if args.act_in_step:
            parser.error('--act_in_step is used only with --act_include / --act_exclude.')
    else:
        for f in (args.act_include, args.act_exclude):
            if not os.path.isfile(f):
                parser.error('Input file {} does not exist.'.format(f))
        args.act_mode = args.act_mode or 'act'
        args.act_filter = args.act_filter or 'exclude'
    if args.connectome is None:
        for name in ('connectome_out', 'connectome_radius'):
            if getattr(args, name) is not None:
                parser.error('--{} is used only with --connectome.'.format(name))
        if args.connectome_only:
            parser.error('--connectome_only is used only with --connectome.')
        if args.connectome_metric:
            parser.error('--connectome_metric is used only with --connectome.')
    else:
        from tracktolearn_amd.runners.ttl_connectome import metric_options
        try:
            args.connectome_metric = metric_options(args.connectome_metric)
        except ValueError as e:
            parser.error('--connectome_metric: {}.'.format(e))
        for _, f in args.connectome_metric:
            if not os.path.isfile(f):
                parser.error('Input file {} does not exist.'.format(f))
        if not os.path.isfile(args.connectome):
            parser.error('Input file {} does not exist.'.format(args.connectome))
        if args.connectome_out is None:
            parser.error('--connectome needs --connectome_out PREFIX.')
        if args.direct_output:
            parser.error('--connectome reads the packed points, which --direct_output '
                         'never makes: drop one of them.')
        if args.connectome_radius is not None and not \
                (np.isfinite(args.connectome_radius) and args.connectome_radius >= 0):
            parser.error('--connectome_radius must be >= 0 mm.')
    if args.density_map is None:
        if args.density_zoom is not None:
            parser.error('--density_zoom is used only with --density_map.')
        if args.density_dec:
            parser.error('--density_dec is used only with --density_map.')
        if args.density_only:
            parser.error('--density_only is used only with --density_map.')
    else:
        if args.density_zoom is not None and not 1 <= args.density_zoom <= 8:
            parser.error('--density_zoom must be in 1 .. 8.')
        if args.direct_output:
            parser.error('--density_map reads the packed points, which --direct_output '
                         'never makes: drop one of them.')
    if args.odf_policy:
        if args.agent is not None or args.hyperparameters is not None:
            parser.error('--odf_policy tracks without an agent: drop --agent / '
                         '--hyperparameters.')
        if args.noise:
            parser.error('--noise perturbs an agent\'s output; with --odf_policy use '
                         '--odf_policy prob.')
        if args.theta is not None and not 0 <= args.theta <= 90:
            parser.error('--theta must be in [0, 90] degrees.')
        if args.sf_threshold is not None and not 0 <= args.sf_threshold <= 1:
            parser.error('--sf_threshold must be in [0, 1].')
        if args.step_size is not None and not args.step_size > 0:
            parser.error('--step_size must be positive.')
        if args.sf_threshold is None:
            args.sf_threshold = 0.1
    else:
        for name in ('theta', 'sf_threshold', 'step_size'):
            if getattr(args, name) is not None:
                parser.error('--{} is used only with --odf_policy.'.format(name))
        verify_agent_option(parser, args)
    return args


def main(argv=None):
    """ Main tracking script """
    import torch.distributed as dist
    args = parse_args(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1 and not dist.is_initialized():
        # one process per GPU over RCCL.  Rehearsal on a single-GPU box:
        # TTL_ONE_DEVICE=1 keeps every rank on cuda:0 and TTL_DIST_BACKEND=gloo
        # replaces RCCL, which refuses two ranks on one device.
        local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        if os.environ.get('TTL_ONE_DEVICE') == '1':
            local_rank = 0
        torch.cuda.set_device(local_rank)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(os.environ.get('TTL_DIST_BACKEND', 'nccl'))
    experiment = TrackToLearnTrack(vars(args))
    experiment.run()


if __name__ == '__main__':
    main()
