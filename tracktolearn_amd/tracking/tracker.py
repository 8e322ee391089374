"""Tracker: batches seeds through the environment and the agent.

Mirror of TrackToLearn/tracking/tracker.py (track / track_and_train /
track_and_validate).  The per-streamline Python work of the reference's
generator (length filter, optional compression, voxel->file space) runs on the
GPU over the whole finished batch (``parallel.select_tracts``): only the points
that end up in the file are downloaded.  ``device_output=False`` keeps the
earlier path (torch length filter on the device, compression per streamline on
the host) as the comparison baseline.  ``track_to_file`` goes one step
further: the output stage writes the file's records and no per-streamline
object is made at all.
"""
from collections import defaultdict

import numpy as np
import torch
from tqdm import tqdm

from tracktolearn_amd.algorithms.shared.utils import add_to_means
from tracktolearn_amd.tractogram import (LazyTractogram, TractogramItem,
                                         compress_streamline)


class TrkFile:
    """Format tag for '.trk' (stands in for nibabel.streamlines.TrkFile at
    tracker.py:127)."""
    EXT = '.trk'


class TckFile:
    """Format tag for '.tck'."""
    EXT = '.tck'


def detect_format(filename):
    """nibabel.streamlines.detect_format by extension."""
    lower = str(filename).lower()
    if lower.endswith('.trk'):
        return TrkFile
    if lower.endswith('.tck'):
        return TckFile
    return None


def to_file_space(streamline, tracts_format, affine, vox_size):
    """Voxel space -> the space the file format expects, as the reference
    writes it (tracker.py:127-136; pinned by tests/golden/tracker_*.npz):
    .trk: voxmm with corner origin, ``(s + 0.5) * vox_size`` evaluated IN
    PLACE on the float32 points (the reference edits the env's history view:
    the sum rounds to float32, the product is taken in float64 and rounded to
    float32); .tck: world space as ``s @ A[:3, :3] + A[:3, 3]`` in float64 --
    a row vector times the matrix, i.e. A's transpose applied, as upstream."""
    if tracts_format is TrkFile:
        out = np.array(streamline, dtype=np.float32)       # a copy
        out += 0.5
        out *= vox_size
        return out
    return np.dot(streamline, affine[:3, :3]) + affine[:3, 3]


class Tracker(object):
    """Generates streamlines with an agent, with or without training it
    (tracker.py:19-60)."""

    def __init__(self, alg, n_actor, prob=0., compress=0.0, min_length=20,
                 max_length=200, save_seeds=False, device_output=None,
                 bidirectional=False, act_filter=None, connectome=None, density=None):
        self.alg = alg
        self.n_actor = n_actor
        self.prob = prob
        self.compress = compress
        self.min_length = min_length
        self.max_length = max_length
        self.save_seeds = save_seeds
        #: track both ways from every seed: after the forward episode the batch
        #: is turned round (``env.reset_backward``) and tracked on from the seeds,
        #: so that a streamline runs through its seed instead of starting there
        #: (never while training)
        self.bidirectional = bool(bidirectional)
        #: with tissue maps in the env (ACT / CMC stopping): None keeps every
        #: streamline, 'exclude' drops those the exclude map ended at either end,
        #: 'endpoints' additionally wants every tracked half ended by the include map
        if act_filter == 'none':
            act_filter = None
        if act_filter not in (None, 'exclude', 'endpoints'):
            raise ValueError(f"act_filter must be None, 'exclude' or 'endpoints', "
                             f'not {act_filter!r}')
        self.act_filter = act_filter
        #: filter + compression + pack by the HIP output stage; None: whenever
        #: the env's buffers are on the GPU.  False: the host path
        self.device_output = device_output
        #: one process per GPU: every rank tracks its contiguous shard of each
        #: seed batch and rank 0 yields the collated streamlines
        self.rank, self.group_size = 0, 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.rank, self.group_size = dist.get_rank(), dist.get_world_size()
        #: a ``connectome.Connectome`` on the label image of the env's grid: every
        #: finished batch's ``select_tracts`` result (the streamlines that will be
        #: written) is also added to it on the device, before anything is downloaded
        self.connectome = connectome
        if connectome is not None:
            if device_output is not None and not device_output:
                raise ValueError('a connectome is fed by the device output stage: '
                                 'device_output=False has none')
            if self.group_size > 1:
                raise ValueError('a connectome is not summed across ranks: track it with '
                                 'one process')
        #: a ``density.DensityMap`` whose reference grid is the env's: fed like the
        #: connectome, with the same points.  With ``compress`` the map is of the
        #: compressed points (the streamlines that are written), whose chords cut
        #: corners the tracked steps went round
        self.density = density
        if density is not None:
            if device_output is not None and not device_output:
                raise ValueError('a density map is fed by the device output stage: '
                                 'device_output=False has none')
            if self.group_size > 1:
                raise ValueError('a density map is not summed across ranks: track it with '
                                 'one process')

    # ------------------------------------------------------------------ #
    def _device_output(self, env):
        if self.device_output is None:
            return bool(env._buf_streamlines.is_cuda)
        return bool(self.device_output)

    def _geometry(self, env):
        """The batch geometry of the output stage, stated once: (the voxel size
        of the env's affine in mm, ``min_length`` and ``max_length`` as arc
        lengths in voxels, the compression tolerance in voxels -- 0.0: none)."""
        vox_size = np.mean(np.abs(env.affine_vox2rasmm)[np.diag_indices(4)][:3])
        return (vox_size, self.min_length / vox_size, self.max_length / vox_size,
                self.compress / vox_size if self.compress else 0.0)

    @staticmethod
    def _seeds(env, device):
        """The finished batch's seeds as an (n, 3) float64 tensor on ``device``."""
        n = env._n_total
        if n == 0:              # an empty shard of a sharded batch
            return torch.zeros((0, 3), dtype=torch.float64, device=device)
        return torch.from_numpy(np.ascontiguousarray(
            np.asarray(env.initial_points)[:n], dtype=np.float64).reshape(-1, 3)).to(device)

    def _act_reject(self, env):
        """(n,) bool on the env's device: the rows of the finished batch that
        ``act_filter`` drops, from the flags the batch ended with and, after a
        backward pass, those its forward pass ended with.  None: no filter."""
        n = env._n_total
        if self.act_filter is None or n == 0:
            return None
        from tracktolearn_amd.environments.stopping_criteria import (
            ACT_EXCLUDE_FLAG, StoppingFlags)
        target = StoppingFlags.STOPPING_TARGET.value
        ends = [env._buf_flags[:n]]
        if env.flags_forward is not None:
            ends.append(env.flags_forward[:n])
        reject = torch.zeros(n, dtype=torch.bool, device=ends[0].device)
        for flags in ends:
            reject |= (flags & ACT_EXCLUDE_FLAG) != 0
            if self.act_filter == 'endpoints':
                reject |= (flags & target) == 0
        return reject

    def _batch_arrays(self, env, scaled_min, scaled_max, tol_vox=0.0):
        """Streamlines of the finished batch whose arc length (voxels) is in
        [scaled_min, scaled_max] (the filter of tracker.py:120-121), compressed
        to ``tol_vox`` voxels when that is > 0 (tracker.py:123-125): one
        ``select_tracts`` over the env's buffers.  Returns (packed points
        (M, 3) f32, points per streamline (k,) i64, seeds (k, 3) f64 -- a host
        tensor: ``env.initial_points`` at the downloaded row indices)."""
        points, counts, rows = self._selected_batch(env, scaled_min, scaled_max, tol_vox)
        return points, counts, self._seeds(env, 'cpu')[rows.cpu()]

    def _selected_batch(self, env, scaled_min, scaled_max, tol_vox=0.0):
        """``select_tracts`` over the env's finished batch (packed points, points
        per streamline, source rows: device tensors), which a connectome also
        receives here, still on the device: the env's voxel space has centre
        origin, the label grid corner origin, so the points get + 0.5 in float32."""
        from tracktolearn_amd.parallel import select_tracts
        n = env._n_total
        points, counts, rows = select_tracts(
            env._buf_streamlines[:n], env._buf_lengths[:n], env._buf_flags[:n],
            scaled_min, scaled_max, tol_vox, reject=self._act_reject(env))
        if self.connectome is not None or self.density is not None:
            self._check_products(env)
            offsets = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=counts.device)
            torch.cumsum(counts, 0, out=offsets[1:])
            corner = points + 0.5
            if self.connectome is not None:
                self.connectome.add(corner, offsets)
            if self.density is not None:
                self.density.add(corner, offsets)
        return points, counts, rows

    def _check_products(self, env):
        """What a connectome and a density map both need of ``env``: the device
        output stage, and the grid of the tracking mask."""
        if not self._device_output(env):
            what = 'a connectome' if self.connectome is not None else 'a density map'
            raise ValueError(f'{what} is fed by the device output stage, which this '
                             'env (host buffers) does not have')
        dims = tuple(int(v) for v in tuple(env.tracking_mask.data.shape)[:3])
        if self.connectome is not None and dims != tuple(self.connectome.dims):
            raise ValueError(f'the connectome\'s label image {tuple(self.connectome.dims)} is '
                             f'not on the grid of the tracking mask {dims}')
        if self.density is not None and dims != tuple(self.density.ref_dims):
            raise ValueError(f'the density map\'s reference grid {tuple(self.density.ref_dims)} '
                             f'is not the grid of the tracking mask {dims}')

    def _batch_arrays_host(self, env, scaled_min, scaled_max):
        """``device_output=False``: the length filter as torch expressions on
        the device, no compression.  Returns (packed points (M, 3) f32, kept
        lengths (k,) i64, seeds (k, 3) f64) as device tensors."""
        from tracktolearn_amd.parallel import arc_accept, kept_lengths, pack_points
        n = env._n_total
        hist = env._buf_streamlines[:n]
        keep_len = kept_lengths(env._buf_lengths[:n], env._buf_flags[:n])
        sel = torch.nonzero(arc_accept(hist, keep_len, scaled_min, scaled_max,
                                       self._act_reject(env))).squeeze(1)
        keep_sel = keep_len[sel]
        return pack_points(hist[sel], keep_sel), keep_sel, self._seeds(env, hist.device)[sel]

    def _batch_items(self, env, scaled_min, scaled_max, transform=None, tol_vox=0.0):
        """(streamline, seed) pairs of the finished batch on this process;
        with a process group, every rank's pairs, on rank 0 only.
        ``transform`` (packed (M, 3) points -> packed points) is applied to the
        whole batch before it is cut into streamlines.  With the device output
        stage the streamlines are already compressed to ``tol_vox`` (each rank
        sends only the points it kept)."""
        if self._device_output(env):
            points, keep_sel, seeds = self._batch_arrays(env, scaled_min, scaled_max,
                                                         tol_vox)
        else:
            if self.connectome is not None or self.density is not None:
                self._check_products(env)         # raises: no device output stage
            points, keep_sel, seeds = self._batch_arrays_host(env, scaled_min, scaled_max)
        if self.group_size > 1:
            # gather-to-root of exact sizes: only rank 0 consumes the tracts
            from tracktolearn_amd.parallel import gather_ragged_to_root
            points, _ = gather_ragged_to_root(points)
            keep_sel, _ = gather_ragged_to_root(keep_sel)
            seeds, _ = gather_ragged_to_root(seeds)
            if self.rank != 0:
                return
        points = points.cpu().numpy()
        keep_np = keep_sel.cpu().numpy()
        seeds = seeds.cpu().numpy()
        if transform is not None:
            # the whole batch at once: the same element-wise arithmetic as per
            # streamline, a few numpy calls instead of a few per streamline
            points = transform(points)
        offsets = np.concatenate(([0], np.cumsum(keep_np)))
        for k in range(len(keep_np)):
            yield points[offsets[k]:offsets[k + 1]], seeds[k]

    def batch_output(self, env, tracts_format):
        """The output stage over the env's finished batch: the TractogramItems
        ``track`` yields for it (length filter, compression, file space)."""
        affine = env.affine_vox2rasmm
        vox_size, scaled_min_length, scaled_max_length, compress_th_vox = self._geometry(env)
        # .trk: the file-space conversion is element-wise, so it runs once over
        # the packed batch -- bit for bit what the per-streamline call gives.
        # On the host path only without compression, which there comes after
        on_device = self._device_output(env)
        whole_batch = tracts_format is TrkFile and (on_device or not self.compress)
        for streamline, seed in self._batch_items(
                env, scaled_min_length, scaled_max_length,
                transform=(lambda p: to_file_space(p, TrkFile, affine, vox_size))
                if whole_batch else None, tol_vox=compress_th_vox):
            if self.compress and not on_device:
                streamline = compress_streamline(streamline, compress_th_vox)
            if not whole_batch:
                streamline = to_file_space(streamline, tracts_format,
                                           affine, vox_size)
            seed_dict = {}
            if self.save_seeds:
                seed_dict = {'seeds': seed - 0.5}
            yield TractogramItem(streamline, seed_dict, {})

    def _episode(self, env, start, end):
        """Tracks seeds [start, end) as one batch, and back again from the seeds
        when ``bidirectional``; returns the summed reward."""
        reward = self.alg.validation_episode(env.reset(start, end), env, self.prob)
        if self.bidirectional:
            reward += self.alg.validation_episode(env.reset_backward(), env, self.prob)
        return reward

    def _tracked_batches(self, env):
        """Tracks the seeds a batch (this rank's shard of it) at a time; yields
        once per batch, the finished batch in the env's buffers."""
        batch_size = self.n_actor
        for start in tqdm(range(0, len(env.seeds), batch_size),
                          disable=self.rank != 0):
            end = min(start + batch_size, len(env.seeds))
            if self.group_size > 1:
                from tracktolearn_amd.parallel import shard_bounds
                lo, hi = shard_bounds(end - start, self.rank, self.group_size)
                start, end = start + lo, start + hi
            if end > start:
                self._episode(env, start, end)
            else:           # an empty shard still joins the collectives
                env._n_total = 0
            yield

    def track(self, env, tracts_format):
        """Tracking only; a lazy tractogram whose iteration does the work
        (tracker.py:62-150).  Streamlines come out in the space the format
        expects: voxmm with corner origin for .trk ((s + 0.5) * voxel size),
        world space for .tck (``s @ A[:3,:3] + A[:3,3]`` as the reference
        writes it)."""
        self.alg.agent.eval()
        affine = env.affine_vox2rasmm
        # shuffle so that partial displays of huge tractograms look uniform
        np.random.shuffle(env.seeds)

        def tracking_generator():
            for _ in self._tracked_batches(env):
                yield from self.batch_output(env, tracts_format)

        tractogram = LazyTractogram.from_data_func(tracking_generator)
        tractogram.affine_to_rasmm = affine
        return tractogram

    def _track_products(self, env):
        """``track`` for the products alone: every batch is tracked and its
        ``select_tracts`` result handed to the connectome and the density map on
        the device; nothing is cut into items or downloaded."""
        self.alg.agent.eval()
        np.random.shuffle(env.seeds)
        _, scaled_min, scaled_max, tol_vox = self._geometry(env)
        for _ in self._tracked_batches(env):
            self._selected_batch(env, scaled_min, scaled_max, tol_vox)

    def track_connectome(self, env):
        """``track`` for the connectome alone (``_track_products``; a density map
        that is attached is fed too).  Returns the connectome."""
        if self.connectome is None:
            raise ValueError('track_connectome needs Tracker(..., connectome=...)')
        self._track_products(env)
        return self.connectome

    def track_density(self, env):
        """``track`` for the density map alone (``_track_products``; a connectome
        that is attached is fed too).  Returns the map."""
        if self.density is None:
            raise ValueError('track_density needs Tracker(..., density=...)')
        self._track_products(env)
        return self.density

    def track_to_file(self, env, path, header=None):
        """``track`` and ``io.streamlines.save`` in one: the output stage
        builds each batch's file body on the device (``select_tracts_file``),
        which is downloaded once and appended with one write -- no
        per-streamline Python.  With a process group every rank builds its
        chunk and rank 0 appends them in rank order, the order ``track``
        yields.  Returns the number of streamlines written (None off rank
        0).  Seeds are saved (``save_seeds``) in .trk files only; .tck has no
        properties."""
        from tracktolearn_amd.io import streamlines as sio
        if self.connectome is not None:
            raise ValueError('track_to_file packs file records and never materialises the '
                             'points a connectome reads: use track, or track_connectome')
        if self.density is not None:
            raise ValueError('track_to_file packs file records and never materialises the '
                             'points a density map reads: use track, or track_density')
        fmt = detect_format(path)
        if fmt is None:
            raise ValueError('output must be .trk or .tck')
        self.alg.agent.eval()
        desc = self.file_desc(env, fmt, header)
        np.random.shuffle(env.seeds)
        writer = sio.PackedWriter(path, fmt.EXT, header, desc.n_props) \
            if self.rank == 0 else None
        try:
            for _ in self._tracked_batches(env):
                words, k = self.batch_body(env, desc)
                if writer is not None:
                    writer.append(words, k)
        finally:
            if writer is not None:
                writer.close()
        return writer.count if writer is not None else None

    def save(self, env, path, header, direct=False):
        """This env's tractogram to ``path`` with ``header``: ``track_to_file``
        when ``direct`` (the output stage writes the file's records: no
        per-streamline Python), otherwise ``track`` + ``io.streamlines.save``.
        Returns the number of streamlines written; None off rank 0, whose
        peers take part in the collectives only."""
        from tracktolearn_amd.io import streamlines as sio
        if direct:
            return self.track_to_file(env, path, header)
        tractogram = self.track(env, detect_format(path))
        if self.rank != 0:
            for _ in tractogram:
                pass
            return None
        return sio.save(tractogram, path, header=header)

    def file_desc(self, env, tracts_format, header=None):
        """The ``io.streamlines.BodyDesc`` of the file ``track`` + ``save``
        write for this env: the seeds as properties with ``save_seeds``, in
        .trk only."""
        from tracktolearn_amd.io import streamlines as sio
        n_props = 3 if self.save_seeds and tracts_format is TrkFile else 0
        return sio.body_desc(tracts_format.EXT, env.affine_vox2rasmm, self._geometry(env)[0],
                             header, n_props)

    def batch_body(self, env, desc):
        """The output stage of ``track_to_file`` over the env's finished
        batch: (the body's words as a host array, streamlines in it); with a
        process group every rank's, in rank order, on rank 0 and (None, the
        count) elsewhere.  One download."""
        from tracktolearn_amd.parallel import select_tracts_file
        _, scaled_min, scaled_max, tol_vox = self._geometry(env)
        n = env._n_total
        words, k, _ = select_tracts_file(
            env._buf_streamlines[:n], env._buf_lengths[:n], env._buf_flags[:n],
            scaled_min, scaled_max, desc,
            # the batch's seeds, uploaded once
            self._seeds(env, env._buf_streamlines.device) if desc.n_props else None,
            tol_error=tol_vox, reject=self._act_reject(env))
        if self.group_size > 1:
            from tracktolearn_amd.parallel import (all_gather_counts,
                                                   gather_ragged_to_root)
            words, _ = gather_ragged_to_root(words)
            k = sum(all_gather_counts(k))
            if self.rank != 0:
                return None, k
        return words.cpu().numpy(), k

    def track_and_train(self, env):
        """One training "epoch": n_actor random seeds tracked while learning
        (tracker.py:152-202)."""
        self.alg.agent.train()
        mean_losses = defaultdict(list)
        mean_reward_factors = defaultdict(list)
        state = env.nreset(self.n_actor)
        reward, losses, length, reward_factors = self.alg._episode(state, env)
        train_tractogram = env.get_streamlines()
        if len(losses.keys()) > 0:
            mean_losses = add_to_means(mean_losses, losses)
        if len(reward_factors.keys()) > 0:
            mean_reward_factors = add_to_means(mean_reward_factors,
                                               reward_factors)
        return train_tractogram, mean_losses, reward, mean_reward_factors

    def track_and_validate(self, env):
        """Track every seed without training, still summing the reward
        (tracker.py:204-259)."""
        self.alg.agent.eval()
        tractogram = None
        cummulative_reward = 0
        for start in tqdm(range(0, len(env.seeds), self.n_actor)):
            reward = self._episode(env, start, min(start + self.n_actor, len(env.seeds)))
            batch = env.get_streamlines()
            if tractogram is None and len(batch) > 0:
                tractogram = batch
            elif len(batch) > 0:
                tractogram += batch
            cummulative_reward += reward
        return tractogram, cummulative_reward
