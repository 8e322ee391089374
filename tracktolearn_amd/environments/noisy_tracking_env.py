"""NoisyTrackingEnvironment: gaussian noise on the action, float64 direction
arithmetic.

Host-side mirror of TrackToLearn/environments/noisy_tracking_env.py.  The
reference adds ``rng.normal(0, noise, size)`` (float64 -- also when noise is
0) to the float32 action before ``TrackingEnvironment.step``, so normalise /
scale / position update run in float64; the HIP library does the
same in TTL_MODE_F64DIR.

``env_dto['device_noise']`` chooses where the noise comes from:

  False (default)  ``rng.normal`` on the host every step, the reference's stream;
  True             ``torch.randn`` on the device every step;
  'keyed'          drawn inside the step's first kernel as a pure function of
                   (``noise_seed``, global seed index of the streamline, step)
                   (``ttl_env_set_noise``): reproducible across
                   batch sizes, shard counts and loop flavours, free-running
                   loops included; optionally scaled by ``fa_map``.
"""
import ctypes as C

import numpy as np
import torch

from tracktolearn_amd import _lib
from tracktolearn_amd.environments.tracking_env import TrackingEnvironment


class NoisyTrackingEnvironment(TrackingEnvironment):

    _force_f64_directions = True
    #: the backward pass of a batch draws with ``noise_seed ^ BACKWARD_SEED_XOR``
    #: and the same ids: other numbers than the forward pass, as independent of
    #: the batching
    BACKWARD_SEED_XOR = 0x9E3779B97F4A7C15

    def __init__(self, dataset_file, split_id: str, env_dto: dict):
        self.noise = env_dto['noise']
        #: False: env_dto['rng'] on the host (the reference's stream); True:
        #: torch on the device; 'keyed': inside the step's kernel (neither of
        #: the last two is bit-compatible with the reference's RNG stream)
        mode = env_dto.get('device_noise', False)
        self.device_noise = 'keyed' if mode == 'keyed' else bool(mode)
        self.fa_map = None
        fa = env_dto.get('fa_map')
        if fa is not None and not (isinstance(fa, (str, bytes)) and not fa):
            if self.device_noise != 'keyed':
                # noisy_tracking_env.py:65-72 scales the noise by (1 - FA) but its
                # broadcast (N,3)+(N,) only works for N == 3;
                # the branch is unreachable from ttl_track.py ('fa_map_file' key).
                raise NotImplementedError('FA-scaled noise is not supported')
            # keyed noise: sigma of a row = max(0, (1 - FA) * noise), FA sampled
            # like the mask; coefficients once per subject on the host
            self.fa_map = np.asarray(getattr(fa, 'data', fa), dtype=np.float64)
            if self.fa_map.ndim != 3:
                raise ValueError('fa_map must be a 3-D volume')
        #: seed of the keyed noise (default: the seed of env_dto['rng'])
        self.noise_seed = env_dto.get('noise_seed')
        if self.noise_seed is None and self.device_noise == 'keyed':
            # word 0 of a RandomState nothing has drawn from yet is its seed
            self.noise_seed = int(env_dto['rng'].get_state()[1][0])
        #: keyed noise: keep the noise every streamline was given in the step
        #: that advanced it in ``noise_out`` ((n, 3) float64, device)
        self.export_noise = bool(env_dto.get('export_noise', False))
        self.noise_out = None
        self._fa_coef = None
        #: keyed noise: streamline g of ``reset(start, end)`` is seed
        #: ``noise_id_offset + start + g`` of the run (``streamline_id_base``)
        self.noise_id_offset = int(env_dto.get('noise_id_offset', 0))
        self.max_action = 1.
        #: generator of the exploration noise; None = ``self.rng`` (the
        #: reference's single stream, noisy_tracking_env.py:73).  A sharded run
        #: gives every rank its own stream (runners/ttl_track.py) so that row i
        #: of every shard does not receive the same noise sequence.
        self.noise_rng = env_dto.get('noise_rng')
        super().__init__(dataset_file, split_id, env_dto)

    def _has_action_noise(self):
        """Noise the host has to supply per step (keeps the free-running loops
        out); keyed noise is drawn by the step itself."""
        return self.noise > 0. and self.device_noise != 'keyed'

    def load_subject(self):
        super().load_subject()
        if self.device_noise == 'keyed' and self.fa_map is not None and self._fa_coef is None:
            if tuple(self.fa_map.shape) != tuple(self._mask_dim):
                raise ValueError(f'fa_map grid {tuple(self.fa_map.shape)} differs from '
                                 f"the tracking mask's {tuple(self._mask_dim)}")
            from scipy.ndimage import spline_filter
            coef = np.ascontiguousarray(
                spline_filter(self.fa_map, order=3, output=np.float64))
            self._fa_coef = torch.from_numpy(coef).to(self.device)

    def _start(self, initial_points):
        state = super()._start(initial_points)
        if self.device_noise == 'keyed':
            self._install_keyed_noise()
        return state

    def reset_backward(self):
        state = super().reset_backward()
        if self.device_noise == 'keyed':
            self._install_keyed_noise(self.BACKWARD_SEED_XOR)
        return state

    def _install_keyed_noise(self, seed_xor=0):
        """Tell the handle what to draw for this batch: streamline g of the
        batch is seed ``streamline_id_base() + g`` of the run."""
        n = self._n_total
        d = _lib.NoiseDesc()
        d.seed = (int(self.noise_seed) ^ seed_xor) & 0xffffffffffffffff
        d.id_base = self.streamline_id_base()
        d.sigma = float(self.noise)
        if self._fa_coef is not None:
            d.fa_coef = self._fa_coef.data_ptr()
            d.fa_dim[:] = [int(v) for v in self._fa_coef.shape]
        self.noise_out = None
        if self.export_noise:
            self.noise_out = torch.zeros((n, 3), dtype=torch.float64, device=self.device)
            d.noise_out = self.noise_out.data_ptr()
        _lib.check(self._lib.ttl_env_set_noise(self._handle, C.byref(d)), 'ttl_env_set_noise')

    def _noise_for(self, actions):
        """noisy_tracking_env.py:73-77.  sigma == 0 adds +0.0 (done inside the
        kernel) and, unlike the reference, does not advance ``rng``."""
        if not self.noise > 0.:
            return None
        if self.device_noise == 'keyed':
            return None         # drawn inside the step (ttl_env_set_noise)
        if self.device_noise:
            return torch.randn(actions.shape, dtype=torch.float64,
                               device=self.device) * float(self.noise)
        rng = self.noise_rng if self.noise_rng is not None else self.rng
        noise = rng.normal(0., self.noise, size=tuple(actions.shape))
        return torch.from_numpy(np.ascontiguousarray(noise)).to(self.device)
