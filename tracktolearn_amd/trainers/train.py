"""TrackToLearnTraining: the algorithm-agnostic training loop.

Mirror of TrackToLearn/trainers/train.py (``run`` / ``rl_train``, argument
groups) and of the parts of TrackToLearn/experiment/experiment.py it needs
(env factory, stopping stats, validation tractogram saving, monitors, the
validators).  ``--oracle_validator`` scores every validation tractogram with
TractOracle on the GPU (experiment/oracle_validator.py: ``Oracle`` and
``Coverage``, printed and kept in ``plots/oracle.npy`` / ``coverage.npy``).
``--tractometer_validator --scoring_data DIR`` segments it into the bundles of
``DIR/scil_scoring_config.json`` on the GPU (experiment/tractometer_validator.py:
``VC``, ``NC``, ``VB``, ``mean_OL`` ..., kept in ``plots/vc.npy`` etc.;
``--tractometer_compute_ic`` adds the invalid connections, ``IC`` and ``IB``).
Comet.ml is outside the hot-path scope: ``--use_comet`` is
accepted and ignored with a notice.
"""
import json
import os
import random
from argparse import ArgumentParser
from os.path import join as pjoin

import numpy as np
import torch

from tracktolearn_amd.environments.noisy_tracking_env import \
    NoisyTrackingEnvironment
from tracktolearn_amd.environments.stopping_criteria import (StoppingFlags,
                                                             is_flag_set)
from tracktolearn_amd.environments.tracking_env import TrackingEnvironment
from tracktolearn_amd.io import streamlines as sio
from tracktolearn_amd.tracking.tracker import Tracker
from tracktolearn_amd.tractogram import Tractogram
from tracktolearn_amd.utils.torch_utils import assert_accelerator, get_device
from tracktolearn_amd.utils.utils import LossHistory


class TrackToLearnTraining(object):
    """Main RL tracking experiment (train.py:28-391)."""

    def __init__(self, train_dto, comet_experiment=None):
        g = train_dto
        self.experiment_path = g['path']
        self.experiment = g['experiment']
        self.name = g['id']
        self.max_ep = g['max_ep']
        self.log_interval = g['log_interval']
        self.noise = g['noise']
        self.lr = g['lr']
        self.gamma = g['gamma']
        self.step_size = g['step_size']
        self.dataset_file = g['dataset_file']
        self.rng_seed = g['rng_seed']
        self.npv = g['npv']
        self.theta = g['theta']
        self.min_length = g['min_length']
        self.max_length = g['max_length']
        self.binary_stopping_threshold = g['binary_stopping_threshold']
        self.alignment_weighting = g['alignment_weighting']
        self.hidden_dims = g['hidden_dims']
        self.n_actor = g['n_actor']
        self.n_dirs = g['n_dirs']
        self.oracle_checkpoint = g['oracle_checkpoint']
        self.oracle_bonus = g['oracle_bonus']
        self.oracle_validator = g['oracle_validator']
        self.oracle_stopping_criterion = g['oracle_stopping_criterion']
        self.tractometer_validator = g['tractometer_validator']
        self.scoring_data = g['scoring_data']
        self.tractometer_reference = g.get('tractometer_reference')
        self.tractometer_dilate = g.get('tractometer_dilate', 1)
        self.tractometer_compute_ic = g.get('tractometer_compute_ic', False)
        if self.tractometer_validator:
            from tracktolearn_amd.experiment.tractometer_validator import CONFIG_NAME
            if not self.scoring_data:
                raise ValueError('--tractometer_validator needs --scoring_data')
            if not os.path.isfile(pjoin(self.scoring_data, CONFIG_NAME)):
                raise ValueError(f'--scoring_data {self.scoring_data} holds no {CONFIG_NAME}')
        self.compute_reward = True       # always during training
        self.fa_map = None
        self.comet_experiment = comet_experiment
        self.last_episode = 0
        self.device = get_device()
        self.use_comet = g['use_comet']
        self.validators = []
        self.score_monitors = {}
        if g['use_comet']:
            print('NOTE: --use_comet is outside the scope of this build and '
                  'is ignored')

        torch.manual_seed(self.rng_seed)
        np.random.seed(self.rng_seed)
        self.rng = np.random.RandomState(seed=self.rng_seed)
        random.seed(self.rng_seed)

        os.makedirs(pjoin(self.experiment_path, 'model'), exist_ok=True)
        self.hyperparameters = {
            'name': self.name, 'experiment': self.experiment,
            'max_ep': self.max_ep, 'log_interval': self.log_interval,
            'lr': self.lr, 'gamma': self.gamma, 'step_size': self.step_size,
            'random_seed': self.rng_seed, 'dataset_file': self.dataset_file,
            'n_seeds_per_voxel': self.npv, 'max_angle': self.theta,
            'min_length': self.min_length, 'max_length': self.max_length,
            'binary_stopping_threshold': self.binary_stopping_threshold,
            'experiment_path': self.experiment_path,
            'hidden_dims': self.hidden_dims, 'last_episode': self.last_episode,
            'n_actor': self.n_actor, 'n_dirs': self.n_dirs, 'noise': self.noise,
            'alignment_weighting': self.alignment_weighting,
            'oracle_bonus': self.oracle_bonus,
            'oracle_checkpoint': self.oracle_checkpoint,
            'oracle_stopping_criterion': self.oracle_stopping_criterion,
        }

    # -- experiment.py:89-175 ------------------------------------------- #
    def _env_dto(self):
        return {
            'dataset_file': self.dataset_file, 'fa_map': self.fa_map,
            'n_dirs': self.n_dirs, 'step_size': self.step_size,
            'theta': self.theta, 'min_length': self.min_length,
            'max_length': self.max_length, 'noise': self.noise,
            'npv': self.npv, 'rng': self.rng,
            'alignment_weighting': self.alignment_weighting,
            'oracle_bonus': self.oracle_bonus,
            'oracle_stopping_criterion': self.oracle_stopping_criterion,
            'oracle_checkpoint': self.oracle_checkpoint,
            'scoring_data': self.scoring_data,
            'binary_stopping_threshold': self.binary_stopping_threshold,
            'compute_reward': self.compute_reward, 'device': self.device,
            'target_sh_order': getattr(self, 'target_sh_order', None),
        }

    def get_env(self):
        return TrackingEnvironment.from_dataset(self._env_dto(), 'training')

    def get_valid_env(self):
        # the reference validates on the 'training' split too (experiment.py:172)
        return NoisyTrackingEnvironment.from_dataset(self._env_dto(), 'training')

    def stopping_stats(self, tractogram):
        """Fraction of streamlines per stopping flag (experiment.py:206-234)."""
        if tractogram is None:
            return {}
        flags = tractogram.data_per_streamline['flags']
        return {f.name: (np.mean(is_flag_set(flags, f)) if len(flags) > 0 else 0)
                for f in StoppingFlags}

    def save_rasmm_tractogram(self, tractogram, subject_id, affine, reference):
        """Validation tractogram -> .trk in RAS+mm (experiment.py:256-310)."""
        filename = pjoin(self.experiment_path, 'tractogram_{}_{}_{}.trk'.format(
            self.experiment, self.name, subject_id))
        keep = [i for i, s in enumerate(tractogram.streamlines) if len(s) > 1]
        world = Tractogram(
            [tractogram.streamlines[i] for i in keep],
            {k: np.asarray(v)[keep].astype(np.float32)
             for k, v in tractogram.data_per_streamline.items()})
        world.apply_affine(affine)
        header = sio.create_tractogram_header(
            reference['affine'], reference['shape'], reference['zooms'])
        sio.save_trk(world, filename, header)
        return filename

    def score_tractogram(self, filename, env):
        """Scores of a tractogram by every validator (experiment.py:236-254)."""
        all_scores = {}
        for scorer in self.validators:
            all_scores.update(scorer(filename, env))
        return all_scores

    def setup_monitors(self):
        p = self.experiment_path
        self.train_reward_monitor = LossHistory('Train Reward', 'train_reward', p)
        self.train_length_monitor = LossHistory('Train Length', 'length_reward', p)
        self.reward_monitor = LossHistory('Reward - Alignment', 'reward', p)
        self.len_monitor = LossHistory('Length', 'length', p)

    def log(self, valid_tractogram, valid_reward, i_episode):
        """experiment.py:312-380 without the Comet calls."""
        if valid_tractogram:
            lens = [len(s) for s in valid_tractogram.streamlines]
        else:
            lens = [0]
        avg_valid_reward = valid_reward / len(lens)
        avg_length = np.mean(lens)
        print('---------------------------------------------------')
        print(self.experiment_path)
        print('Episode {} \t avg length: {} \t total reward: {}'.format(
            i_episode, avg_length, avg_valid_reward))
        print('---------------------------------------------------')
        self.reward_monitor.update(avg_valid_reward)
        self.reward_monitor.end_epoch(i_episode)
        self.len_monitor.update(avg_length)
        self.len_monitor.end_epoch(i_episode)

    # -- train.py:151-179 ------------------------------------------------ #
    def save_hyperparameters(self):
        self.hyperparameters.update({
            'input_size': self.input_size, 'action_size': self.action_size,
            'voxel_size': str(self.voxel_size),
            'target_sh_order': self.target_sh_order})
        with open(pjoin(self.experiment_path, 'model', 'hyperparameters.json'),
                  'w') as json_file:
            json_file.write(json.dumps(self.hyperparameters, indent=4,
                                       separators=(',', ': ')))

    def save_model(self, alg):
        directory = pjoin(self.experiment_path, 'model')
        os.makedirs(directory, exist_ok=True)
        alg.agent.save(directory, 'last_model_state')

    def _validate(self, valid_tracker, valid_env, alg, i_episode):
        valid_env.load_subject()
        valid_tractogram, valid_reward = valid_tracker.track_and_validate(valid_env)
        print(self.stopping_stats(valid_tractogram))
        if valid_tractogram:
            self.save_rasmm_tractogram(valid_tractogram, valid_env.subject_id,
                                       valid_env.affine_vox2rasmm,
                                       valid_env.reference)
            if self.validators:
                # the streamlines just saved, scored from memory (no file round
                # trip; score_tractogram takes the file)
                scores = self.score_tractogram(valid_tractogram, valid_env)
                print(scores)
                for key, value in scores.items():
                    monitor = self.score_monitors.get(key)
                    if monitor is not None:
                        monitor.update(value)
                        monitor.end_epoch(i_episode)
        self.log(valid_tractogram, valid_reward, i_episode)
        self.save_model(alg)

    def rl_train(self, alg, env, valid_env):
        """train.py:181-350: validate, then ``max_ep`` training episodes with a
        validation run + model save every ``log_interval`` episodes."""
        i_episode = 0
        t = 0
        train_tracker = Tracker(alg, self.n_actor, prob=0.0, compress=0.0)
        valid_tracker = Tracker(alg, self.n_actor, prob=1.0, compress=0.0)
        # validators (train.py:216-226), the Tractometer first as there; Comet
        # is ignored: the scores are kept as plots/<name>.npy
        self.validators = []
        self.score_monitors = {}
        p = self.experiment_path
        if self.tractometer_validator:
            from tracktolearn_amd.experiment.tractometer_validator import \
                TractometerValidator
            self.validators.append(TractometerValidator(
                self.scoring_data, self.tractometer_reference,
                dilate_endpoints=self.tractometer_dilate, device=self.device,
                compute_ic=self.tractometer_compute_ic))
            self.score_monitors.update({
                key: LossHistory(key, key.lower(), p)
                for key in ('VC', 'IC', 'NC', 'VB', 'IB', 'mean_OL')})
        if self.oracle_validator:
            from tracktolearn_amd.experiment.oracle_validator import \
                OracleValidator
            self.validators.append(OracleValidator(self.oracle_checkpoint,
                                                   self.device))
            self.score_monitors.update({
                'Oracle': LossHistory('Oracle', 'oracle', p),
                'Coverage': LossHistory('Coverage', 'coverage', p)})
        self._validate(valid_tracker, valid_env, alg, i_episode)
        while i_episode < self.max_ep:
            self.last_episode = i_episode
            env.load_subject()
            tractogram, losses, reward, reward_factors = \
                train_tracker.track_and_train(env)
            lengths = [len(s) for s in tractogram.streamlines]
            avg_length = np.mean(lengths)
            t += sum(lengths)
            avg_reward = reward / self.n_actor
            print(f'Episode Num: {i_episode+1} Avg len: {avg_length:.3f} '
                  f'Avg. reward: {avg_reward:.3f} sub: {env.subject_id}')
            self.train_reward_monitor.update(avg_reward)
            self.train_reward_monitor.end_epoch(i_episode)
            self.train_length_monitor.update(avg_length)
            self.train_length_monitor.end_epoch(i_episode)
            i_episode += 1
            if i_episode % self.log_interval == 0:
                self._validate(valid_tracker, valid_env, alg, i_episode)
        self._validate(valid_tracker, valid_env, alg, i_episode)

    def run(self):
        """train.py:352-391."""
        assert_accelerator()
        env = self.get_env()
        valid_env = self.get_valid_env()
        self.input_size = env.get_state_size()
        self.action_size = env.get_action_size()
        self.voxel_size = env.get_voxel_size()
        self.target_sh_order = env.target_sh_order
        alg = self.get_alg(env.max_nb_steps)
        self.save_hyperparameters()
        self.setup_monitors()
        self.rl_train(alg, env, valid_env)


# -- argument groups (experiment.py:383-473, train.py:394-421) ------------- #
def add_experiment_args(parser: ArgumentParser):
    parser.add_argument('path', type=str, help='Path to experiment')
    parser.add_argument('experiment', help='Name of experiment.')
    parser.add_argument('id', type=str, help='ID of experiment.')
    parser.add_argument('--workspace', type=str, default='TractOracle',
                        help='Comet.ml workspace')
    parser.add_argument('--rng_seed', default=1337, type=int,
                        help='Seed to fix general randomness')
    parser.add_argument('--use_comet', action='store_true',
                        help='Use comet to display training or not')
    parser.add_argument('--comet_offline_dir', type=str,
                        help='Comet offline directory.')


def add_data_args(parser: ArgumentParser):
    parser.add_argument('dataset_file',
                        help='Path to preprocessed dataset file (.hdf5, or '
                             'the .npz layout of datasets/SubjectDataset.py)')


def add_environment_args(parser: ArgumentParser):
    parser.add_argument('--n_dirs', default=4, type=int, help='Last n steps taken')
    parser.add_argument('--binary_stopping_threshold', type=float, default=0.1,
                        help='Lower limit for interpolation of tracking mask '
                             'value.\nTracking will stop below this threshold.')


def add_reward_args(parser: ArgumentParser):
    parser.add_argument('--alignment_weighting', default=1, type=float,
                        help='Alignment weighting for reward')


def add_model_args(parser: ArgumentParser):
    parser.add_argument('--n_actor', default=4096, type=int,
                        help='Number of learners')
    parser.add_argument('--hidden_dims', default='1024-1024-1024', type=str,
                        help='Hidden layers of the model')


def add_tracking_args(parser: ArgumentParser):
    parser.add_argument('--npv', default=2, type=int,
                        help='Number of random seeds per seeding mask voxel.')
    parser.add_argument('--theta', default=30, type=int,
                        help='Max angle between segments for tracking.')
    parser.add_argument('--min_length', type=float, default=20., metavar='m',
                        help='Minimum length of a streamline in mm. [%(default)s]')
    parser.add_argument('--max_length', type=float, default=200., metavar='M',
                        help='Maximum length of a streamline in mm. [%(default)s]')
    parser.add_argument('--step_size', default=0.75, type=float,
                        help='Step size for tracking')
    parser.add_argument('--noise', default=0.0, type=float, metavar='sigma',
                        help='Add noise ~ N (0, `noise`) to the agent\'s output '
                             '[%(default)s]')


def add_tractometer_args(parser: ArgumentParser):
    tractom = parser.add_argument_group('Tractometer')
    tractom.add_argument('--scoring_data', type=str, default=None,
                         help='Location of the tractometer scoring data.')
    tractom.add_argument('--tractometer_reference', type=str, default=None,
                         help='Reference anatomy for the Tractometer.')
    tractom.add_argument('--tractometer_validator', action='store_true',
                         help='Run tractometer during validation (needs '
                              '--scoring_data).')
    tractom.add_argument('--tractometer_dilate', default=1, type=int,
                         help='Dilation factor for the ROIs of the Tractometer.')
    tractom.add_argument('--tractometer_compute_ic', action='store_true',
                         help='Also segment the invalid connections: IC, IS, IB and '
                              'NC carry real values.')


def add_oracle_args(parser: ArgumentParser):
    oracle = parser.add_argument_group('Oracle')
    oracle.add_argument('--oracle_checkpoint', type=str,
                        default='models/tractoracle.ckpt',
                        help='Checkpoint file (.ckpt) of the Oracle')
    oracle.add_argument('--oracle_validator', action='store_true',
                        help='Run a TractOracle model during validation.')
    oracle.add_argument('--oracle_stopping_criterion', action='store_true',
                        help='Stop streamlines according to the Oracle.')
    oracle.add_argument('--oracle_bonus', default=10, type=float,
                        help='Sparse oracle weighting for reward.')


def add_rl_args(parser):
    parser.add_argument('--max_ep', default=1000, type=int,
                        help='Number of episodes to run the training algorithm')
    parser.add_argument('--log_interval', default=50, type=int,
                        help='Log statistics, save the model and '
                             'hyperparameters at n steps')
    parser.add_argument('--lr', default=0.0005, type=float, help='Learning rate')
    parser.add_argument('--gamma', default=0.95, type=float,
                        help='Gamma param for reward discounting')
    add_reward_args(parser)


def add_training_args(parser):
    add_experiment_args(parser)
    add_data_args(parser)
    add_environment_args(parser)
    add_model_args(parser)
    add_rl_args(parser)
    add_tracking_args(parser)
    add_oracle_args(parser)
    add_tractometer_args(parser)
