"""Records of one step: what ``harvest()`` needs from it, and ``step()``'s info."""
import numpy as np


class _PendingStep:
    """A launched step ``harvest()`` has not taken yet: the row order of its
    state rows, those rows, the rows it advanced, its device ``dones``, the
    tensors its kernels borrow (``keep``), whether dones / reward went to pinned
    memory behind its first kernel (``early``), after ``step()`` the host dones."""
    __slots__ = ('order', 'state', 'n', 'done', 'keep', 'early', 'dones_host')

    def __init__(self, order, state, n, done, keep, early):
        self.order, self.state, self.n, self.done = order, state, n, done
        self.keep, self.early, self.dones_host = keep, early, None


class _StepInfo(dict):
    """``info`` dict of ``step``; 'continue_idx' is downloaded on first use
    (the reference puts the host index array there, tracking_env.py:220)."""

    def __init__(self, env, n_active, reward_info):
        super().__init__(reward_info=reward_info)
        self._idx_dev = env._idx_view(n_active)

    def __missing__(self, key):
        if key == 'continue_idx':
            val = self._idx_dev.to('cpu').numpy().astype(np.int64)
            self[key] = val
            return val
        raise KeyError(key)

    def __contains__(self, key):
        return key == 'continue_idx' or super().__contains__(key)
