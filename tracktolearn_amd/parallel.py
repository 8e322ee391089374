"""Multi-GPU layout of the environment path: one process per GPU, streamlines
sharded, volumes replicated, no collective on the step path.

The reference is single-process.  Streamlines are independent
given the read-only volumes, so rank r of R tracks the contiguous slice
``shard_bounds(n, r, R)`` of every seed batch and never talks to its peers
while stepping.  The only exchange is collating the finished tracts at
``get_streamlines()`` time.  Only one rank consumes them (rank 0 writes the
file), so the collate is a gather-to-root of exact sizes: one all-gather of
the per-rank row counts (8 bytes each), then every rank sends its kept
lengths / flags / seeds / packed points straight into its slice of the root's
buffers (batched point-to-point over RCCL/xGMI -- xGMI is point to point, each
sender uses its own link to the root; gloo in the CPU tests).  No padding, and
1/R of the bytes an all-gather of the same data would land on every GPU.
``all_gather_ragged`` remains for callers that need the data everywhere.
"""
import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from tracktolearn_amd import _lib
from tracktolearn_amd.environments.stopping_criteria import StoppingFlags
from tracktolearn_amd.tractogram import Tractogram


def shard_bounds(n, rank, world):
    """[start, end) of rank's contiguous shard of n seeds (ceil split; the
    last shards may be short or empty)."""
    per = -(-n // world)
    start = min(rank * per, n)
    return start, min(start + per, n)


def kept_lengths(lengths, flags):
    """Points kept per streamline: the last point is dropped when CURVATURE or
    MASK stopped it (TrackToLearn/environments/tracking_env.py:263-284)."""
    cut = (StoppingFlags.STOPPING_CURVATURE.value |
           StoppingFlags.STOPPING_MASK.value)
    return lengths.to(torch.int64) - ((flags & cut) != 0).to(torch.int64)


def _device_lib(device):
    """What every launch from this file starts with: (the loaded library, the
    raw HIP stream of ``device`` that torch is on)."""
    from tracktolearn_amd.environments.env import _raw_stream
    return _lib.load(), C.c_void_p(_raw_stream(device.index or 0))


def _point_rows(history):
    """The (n, T, 3) history as the kernels read it: a row's points one after
    the other; rows may be further apart than their points (a slice of a
    larger buffer)."""
    return history if history.stride(2) == 1 and history.stride(1) == 3 \
        else history.contiguous()


def pack_points(history, keep_len):
    """Ragged pack: (n, T, 3) history + kept lengths -> (sum(keep_len), 3)
    points, streamline-major.  On the GPU: one wave per streamline
    (``ttl_pack_streamlines``; the boolean-mask indexing it replaces took
    56 ms for the 68 M points of a 1 048 576-streamline tractogram, the kernel
    moves them at memory speed).  Host tensors (the gloo tests) index."""
    if not history.is_cuda:
        steps = torch.arange(history.shape[1], device=history.device)
        return history[steps[None, :] < keep_len[:, None]]
    n = int(history.shape[0])
    keep = keep_len.to(torch.int64).contiguous()
    ends = torch.cumsum(keep, 0)
    total = int(ends[-1].item()) if n else 0
    out = torch.empty((total, 3), dtype=torch.float32, device=history.device)
    if total:
        lib, stream = _device_lib(history.device)
        hist = _point_rows(history)
        offsets = ends - keep
        _lib.check(lib.ttl_pack_streamlines(
            hist.data_ptr(), hist.stride(0), keep.data_ptr(), offsets.data_ptr(), n,
            out.data_ptr(), stream), 'ttl_pack_streamlines')
    return out


def tract_survivors(history, lengths, flags, min_arc, max_arc, tol_error=0.0,
                    max_segment_length=10.0):
    """``ttl_tract_select`` over CUDA tensors: the first half of
    ``select_tracts``.  Returns (the history as the kernel read it, ``sel``
    (2, n) int32: surviving points per row -- 0 for a rejected row -- and the
    0 / 1 accept flags, ``mask`` (n, ceil(T / 64)) int64: bit ``j & 63`` of word
    ``j >> 6`` is set iff point j of the row survives)."""
    n, dev = int(history.shape[0]), history.device
    lib, stream = _device_lib(dev)
    hist = _point_rows(history)
    lengths = lengths.to(torch.int32).contiguous()
    flags = flags.to(torch.int32).contiguous()
    pitch = hist.stride(0)
    sel = torch.empty((2, n), dtype=torch.int32, device=dev)
    mask = torch.empty((n, lib.ttl_tract_mask_words(pitch)), dtype=torch.int64, device=dev)
    _lib.check(lib.ttl_tract_select(
        hist.data_ptr(), pitch, lengths.data_ptr(), flags.data_ptr(), n,
        float(min_arc), float(max_arc), float(tol_error), float(max_segment_length),
        sel[0].data_ptr(), sel[1].data_ptr(), mask.data_ptr(), stream), 'ttl_tract_select')
    return hist, sel, mask


def _check_reject(reject, n):
    if reject is not None and (reject.dtype is not torch.bool or tuple(reject.shape) != (n,)):
        raise ValueError(f'reject must be a bool tensor of shape ({n},)')


def _drop_rejected(sel, reject):
    """Between ``tract_survivors`` and the scans: a rejected row keeps no point
    and is not accepted (the emit kernels skip unaccepted rows)."""
    if reject is not None:
        sel.masked_fill_(reject.to(sel.device)[None, :], 0)


def _selected(history, lengths, flags, min_arc, max_arc, tol_error, max_segment_length,
              reject):
    """The GPU front half of ``select_tracts`` and ``select_tracts_file``:
    ``tract_survivors``, the rejected rows dropped, the scans and the host's
    look at their totals.  Returns (``emit``, points M, accepted rows k, the
    library): ``emit(name, *outputs)`` launches that emit entry point -- the
    two take the same inputs, held here -- into ``outputs`` unless k is 0."""
    n = int(history.shape[0])
    lib, stream = _device_lib(history.device)
    hist, sel, mask = tract_survivors(history, lengths, flags, min_arc, max_arc,
                                      tol_error, max_segment_length)
    _drop_rejected(sel, reject)
    # two 1-D scans: torch's scan along the inner dimension of a (2, n) tensor
    # takes 0.6 ms at n = 262 144, longer than both kernels together
    ends = (torch.cumsum(sel[0], 0, dtype=torch.int64),
            torch.cumsum(sel[1], 0, dtype=torch.int64))
    total, k = torch.stack((ends[0][-1], ends[1][-1])).tolist()   # the one synchronising copy

    def emit(name, *outputs):
        if k:
            _lib.check(getattr(lib, name)(
                hist.data_ptr(), hist.stride(0), n, sel[0].data_ptr(), sel[1].data_ptr(),
                ends[0].data_ptr(), ends[1].data_ptr(), mask.data_ptr(), *outputs, stream), name)
    return emit, total, k, lib


def select_tracts(history, lengths, flags, min_arc, max_arc, tol_error=0.0,
                  max_segment_length=10.0, reject=None):
    """The tracker's output stage over a finished batch: (n, T, 3) float32
    history + the env's int32 lengths / flags -> the streamlines whose arc
    length (voxels, float64) is in [min_arc, max_arc], compressed with
    ``tractogram.compress_streamline(s, tol_error, max_segment_length)`` when
    ``tol_error > 0``.  Returns (packed points (M, 3) f32, points per
    streamline (k,) i64, source rows (k,) i64) on the input's device, accepted
    rows in row order.  ``reject`` (n,) bool or None: rows dropped whatever
    their length (the tissue-map filter of ``Tracker(act_filter=...)``).
    On the GPU: ``ttl_tract_select`` (one wave per row:
    kept length, arc, accept, survivor bitmask), a prefix sum, then
    ``ttl_tract_emit`` (one wave per row: the pack); the largest allocation is
    the packed output.  Host tensors (the gloo tests) take the torch filter
    and ``compress_streamline`` -- the specification the kernels are tested
    against."""
    n = int(history.shape[0])
    dev = history.device
    _check_reject(reject, n)
    if n == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    if not history.is_cuda:
        return _select_tracts_host(history, lengths, flags, min_arc, max_arc,
                                   tol_error, max_segment_length, reject)
    emit, total, k, _ = _selected(history, lengths, flags, min_arc, max_arc, tol_error,
                                  max_segment_length, reject)
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    rows = torch.empty(k, dtype=torch.int32, device=dev)
    emit('ttl_tract_emit', points.data_ptr(), counts.data_ptr(), rows.data_ptr())
    return points, counts, rows.to(torch.int64)


def select_tracts_file(history, lengths, flags, min_arc, max_arc, desc, seeds=None,
                       tol_error=0.0, max_segment_length=10.0, reject=None):
    """``select_tracts`` whose pack writes the batch's file body instead of the
    packed points: ``desc`` is an ``io.streamlines.BodyDesc``, ``seeds`` the
    (n, 3) float64 seeds by input row (needed when ``desc.n_props == 3``),
    ``reject`` as for ``select_tracts``.
    Returns (words int32 -- the 4-byte words of the body, on the input's
    device --, accepted rows k, points M).  On the GPU the same
    ``ttl_tract_select``, scans and synchronising copy, then
    ``ttl_tract_emit_file``; host tensors take ``_select_tracts_host`` and
    ``io.streamlines.packed_body``, the kernel's specification."""
    from tracktolearn_amd.io.streamlines import packed_body
    n = int(history.shape[0])
    dev = history.device
    if desc.n_props == 3 and seeds is None:
        raise ValueError('n_props == 3 needs the seeds')
    _check_reject(reject, n)
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), 0, 0
    if not history.is_cuda:
        points, counts, rows = _select_tracts_host(history, lengths, flags, min_arc, max_arc,
                                                   tol_error, max_segment_length, reject)
        kept = None if seeds is None else \
            np.asarray(seeds, dtype=np.float64).reshape(-1, 3)[rows.numpy()]
        words = packed_body(points.numpy(), counts.numpy(), kept, desc)
        return torch.from_numpy(words.view(np.int32)), len(counts), len(points)
    emit, total, k, lib = _selected(history, lengths, flags, min_arc, max_arc, tol_error,
                                    max_segment_length, reject)
    c_desc = desc.to_c()
    size = lib.ttl_tract_file_words(c_desc.format, c_desc.n_props, k, total)
    if size < 0:
        raise ValueError('format {} with {} properties is not a file body'.format(
            c_desc.format, c_desc.n_props))
    words = torch.empty(size, dtype=torch.int32, device=dev)
    if seeds is not None:
        seeds = torch.as_tensor(seeds, dtype=torch.float64).to(dev).reshape(n, 3).contiguous()
    emit('ttl_tract_emit_file', seeds.data_ptr() if seeds is not None else None,
         C.byref(c_desc), words.data_ptr())
    return words, k, total


def arc_accept(history, keep_len, min_arc, max_arc, reject=None):
    """The arc-length filter as torch expressions (the specification of
    ``ttl_tract_select``'s, and the ``device_output=False`` path): (n,) bool,
    True where the float64 arc length of a row's first ``keep_len`` points is in
    [min_arc, max_arc] and ``reject`` (as for ``select_tracts``) is not set."""
    seg = (history[:, 1:] - history[:, :-1]).double()
    seg_len = torch.sqrt((seg ** 2).sum(dim=2))
    steps = torch.arange(seg_len.shape[1], device=history.device)
    valid = steps[None, :] < (keep_len - 1)[:, None]
    arc = (seg_len * valid).sum(dim=1)
    ok = (arc >= min_arc) & (arc <= max_arc)
    if reject is not None:
        ok &= ~reject
    return ok


def _select_tracts_host(history, lengths, flags, min_arc, max_arc, tol_error,
                        max_segment_length, reject=None):
    from tracktolearn_amd.tractogram import compress_streamline
    keep_len = kept_lengths(lengths, flags)
    rows = torch.nonzero(arc_accept(history, keep_len, min_arc, max_arc, reject)).squeeze(1)
    hist = history.numpy()
    lines = [hist[r, :k] for r, k in zip(rows.tolist(), keep_len[rows].tolist())]
    if tol_error > 0:
        lines = [compress_streamline(s, tol_error, max_segment_length) for s in lines]
    counts = torch.tensor([len(s) for s in lines], dtype=torch.int64)
    points = np.concatenate(lines) if lines else np.zeros((0, 3), np.float32)
    return (torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).reshape(-1, 3),
            counts, rows)


def all_gather_counts(values, group=None):
    """All-gather one int64 per rank."""
    world = dist.get_world_size(group)
    mine = torch.tensor([int(values)], dtype=torch.int64,
                        device=_coll_device(group))
    out = torch.empty(world, dtype=torch.int64, device=mine.device)
    dist.all_gather_into_tensor(out, mine, group=group)
    return out.tolist()


def _coll_device(group):
    backend = dist.get_backend(group)
    if backend == 'nccl':
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device('cpu')


def all_gather_ragged(rows, group=None):
    """All-gather tensors whose first dimension differs per rank: pad to the
    longest shard, one all_gather_into_tensor, cut the padding.  Returns the
    per-rank pieces in rank order."""
    world = dist.get_world_size(group)
    dev = _coll_device(group)
    rows = rows.to(dev).contiguous()
    counts = all_gather_counts(rows.shape[0], group)
    longest = max(max(counts), 1)
    padded = torch.zeros((longest,) + tuple(rows.shape[1:]), dtype=rows.dtype,
                         device=dev)
    padded[:rows.shape[0]] = rows
    out = torch.empty((world * longest,) + tuple(rows.shape[1:]),
                      dtype=rows.dtype, device=dev)
    dist.all_gather_into_tensor(out, padded, group=group)
    return [out[r * longest:r * longest + counts[r]] for r in range(world)]


def gather_ragged_to_root(rows, dst=0, group=None):
    """Gather tensors whose first dimension differs per rank on rank ``dst``
    only, exact sizes, no padding: the root allocates sum(counts) rows and
    every other rank's send lands directly in its slice.  Returns
    ``(all_rows, counts)`` on the root (rank order) and ``(None, counts)``
    elsewhere."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = _coll_device(group)
    rows = rows.to(dev).contiguous()
    counts = all_gather_counts(rows.shape[0], group)
    ops, out = [], None
    if rank == dst:
        out = torch.empty((sum(counts),) + tuple(rows.shape[1:]),
                          dtype=rows.dtype, device=dev)
        offs = np.concatenate(([0], np.cumsum(counts)))
        out[offs[dst]:offs[dst + 1]] = rows
        for r in range(world):
            if r != dst and counts[r] > 0:
                peer = dist.get_global_rank(group, r) if group is not None else r
                ops.append(dist.P2POp(dist.irecv, out[offs[r]:offs[r + 1]],
                                      peer, group))
    elif rows.shape[0] > 0:
        peer = dist.get_global_rank(group, dst) if group is not None else dst
        ops.append(dist.P2POp(dist.isend, rows, peer, group))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    return out, counts


def tract_arrays(env):
    """This rank's finished tracts as device arrays: (kept lengths int64 (n,),
    flags int32 (n,), packed points float32 (sum(kept), 3))."""
    n = env._n_total
    lengths, flags = env._buf_lengths[:n], env._buf_flags[:n]
    keep = kept_lengths(lengths, flags)
    return keep, flags, pack_points(env._buf_streamlines[:n], keep)


def gather_tract_arrays(env, dst=0, group=None):
    """Every rank's ``tract_arrays`` on rank ``dst`` (rank order): (keep,
    flags, points, bytes received) there, None elsewhere.  This is the
    path's one exchange step; bench.py times it as ``collate_ms``."""
    keep, flags, points = tract_arrays(env)
    keep_all, _ = gather_ragged_to_root(keep, dst, group)
    flags_all, _ = gather_ragged_to_root(flags, dst, group)
    pts_all, _ = gather_ragged_to_root(points, dst, group)
    if keep_all is None:
        return None
    moved = sum(int(a.numel() - b.numel()) * a.element_size() for a, b in
                ((keep_all, keep), (flags_all, flags), (pts_all, points)))
    return keep_all, flags_all, pts_all, moved


def _seeds_of(env):
    return torch.from_numpy(np.ascontiguousarray(env.initial_points, dtype=np.float64))


def tractogram_of(keep, flags, points, seeds):
    """``tract_arrays`` (tensors on any device, of one rank or of all) and the
    seeds of the same rows -> the Tractogram ``get_streamlines()`` returns:
    one view of the downloaded points per streamline, seeds and flags as
    ``data_per_streamline``."""
    keep, flags, points = (t.cpu().numpy() for t in (keep, flags, points))
    offsets = np.concatenate(([0], np.cumsum(keep)))
    lines = [points[offsets[i]:offsets[i + 1]] for i in range(len(keep))]
    return Tractogram(streamlines=lines,
                      data_per_streamline={
                          'seeds': seeds.cpu().numpy() if torch.is_tensor(seeds) else seeds,
                          'flags': flags.astype(np.int64)})


def gather_tractogram(env, dst=0, group=None):
    """The sharded ``get_streamlines()``: every rank's finished tracts as one
    Tractogram (rank order, then streamline order) on rank ``dst``; None on
    the other ranks."""
    seeds_all, _ = gather_ragged_to_root(_seeds_of(env), dst, group)
    got = gather_tract_arrays(env, dst, group)
    if got is None:
        return None
    return tractogram_of(*got[:3], seeds_all)


def all_gather_tract_index(env, group=None):
    """(lengths, flags) of every rank's streamlines, concatenated in rank
    order (device tensors)."""
    n = env._n_total
    lengths = torch.cat(all_gather_ragged(env._buf_lengths[:n], group))
    flags = torch.cat(all_gather_ragged(env._buf_flags[:n], group))
    return lengths, flags


def all_gather_tractogram(env, group=None):
    """Every rank's finished tracts as one Tractogram (rank order, then
    streamline order) -- the sharded ``get_streamlines()``."""
    keep, flags, points = tract_arrays(env)
    keep, flags, seeds, points = (torch.cat(all_gather_ragged(t, group))
                                  for t in (keep, flags, _seeds_of(env), points))
    return tractogram_of(keep, flags, points, seeds)


# --------------------------------------------------------------------------
# data-parallel learner (BASELINE config 5: training on 8 GPUs)
# --------------------------------------------------------------------------
def broadcast_parameters(modules, src=0, group=None):
    """Make every rank start from rank ``src``'s weights (and buffers)."""
    for m in modules:
        for t in list(m.parameters()) + list(m.buffers()):
            dist.broadcast(t.data, src=src, group=group)


def all_reduce_gradients(params, group=None):
    """Average the gradients of ``params`` over the ranks with ONE flattened
    all-reduce (RCCL ring over xGMI is per-link bound, so a single ~10-20 MB
    bucket per network beats one collective per tensor).  Parameters without
    a gradient are skipped on every rank alike."""
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat /= dist.get_world_size(group)
    offset = 0
    for g in grads:
        n = g.numel()
        g.copy_(flat[offset:offset + n].view_as(g))
        offset += n
