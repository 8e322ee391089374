"""StatePool: the placed buffers a large batch's state rows are written into."""
import torch


# TensorImpls + Python storage objects alive on the storage at this address
_storage_users = getattr(torch._C, '_storage_Use_Count', None)


class StatePool:
    """``buffers``: (rows, width) tensors of one shape, an allocation each (plain
    tensors: CPU ones work too); ``memory``: the owners of those allocations.
    A buffer is handed out again only when no tensor refers to it any more (the
    use count of its storage), so a state tensor stays intact for as long as the
    caller holds it, like a fresh allocation.  ``rotate``: a plain ring instead,
    a tensor is overwritten ``len(pool)`` requests after it was handed out,
    referenced or not (``TTL_STATE_RING_ROTATE``, a torch without the use count,
    the placement search)."""

    def __init__(self, buffers=(), memory=None, rotate=False):
        self.buffers, self.memory, self.rotate = list(buffers), memory, bool(rotate)
        self._pos = 0
        # address of every buffer's storage (alive as long as the buffer) and its
        # use count while nothing is handed out, taken at the first request:
        # whoever built the pool may still hold temporaries
        self._storages = self._idle = None

    def __len__(self):
        return len(self.buffers)

    def rows(self, n):
        """A placed view of ``n`` rows, or None when none fits: no buffer, ``n``
        larger than a buffer, or the caller still holds a tensor on every one."""
        ring = self.buffers
        if not ring or n > ring[0].shape[0]:
            return None
        if self.rotate:
            self._pos = (self._pos + 1) % len(ring)
            return ring[self._pos][:n]
        if self._idle is None:
            self._storages = [b.untyped_storage()._cdata for b in ring]
            self._idle = [_storage_users(s) for s in self._storages]
        for k in range(1, len(ring) + 1):
            pos = (self._pos + k) % len(ring)
            if _storage_users(self._storages[pos]) <= self._idle[pos]:
                self._pos = pos
                return ring[pos][:n]
        return None
