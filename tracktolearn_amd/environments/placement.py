"""The arithmetic of the placement search (``BaseEnv._tune_placement``)."""


def placement_plan(volume_bytes, buffer_bytes, free_bytes, volume_candidates,
                   buffer_candidates, ring_len, *, cap_bytes, free_fraction,
                   budget_override=None):
    """``(budget, volume candidates, state-buffer candidates)`` of one search.
    The extra volume copies and the candidate state buffers together take at
    most ``cap_bytes`` and at most ``free_fraction`` of the device memory free
    when the search starts (``budget_override``, TTL_PLACEMENT_SEARCH_BYTES,
    replaces both): the copies half of it at most, the buffers what they leave.
    No buffer when not even a ring of them fits or ``ring_len`` < 2."""
    budget = int(min(cap_bytes, free_fraction * free_bytes))
    if budget_override is not None:
        budget = int(budget_override)
    kv = max(1, min(volume_candidates, 1 + budget // max(2 * volume_bytes, 1)))
    left = budget - (kv - 1) * volume_bytes
    kr = buffer_candidates if ring_len >= 2 else 0
    if kr > 0:
        kr = min(kr, left // max(buffer_bytes, 1))
        if kr < ring_len:
            kr = 0
    return budget, kv, kr


def pick_ring(times, n_buffers, ring_len):
    """Indices of the ``ring_len`` state buffers that were fastest with the
    winning volume, whose row of gather times is ``times`` (buffer ``r`` at
    ``times[r]``; the allocator's own blocks behind them are ignored).  Buffers
    never timed (early exit) rank last, in allocation order; ties by index."""
    order = sorted(range(n_buffers),
                   key=lambda r: (times[r] if r < len(times) else float('inf'), r))
    return order[:ring_len]
