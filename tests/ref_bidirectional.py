"""Bidirectional tracking (ttl_env_reset_backward) restated on the
CPU oracle.

The reference has no bidirectional mode, so the yardstick is the project's own
oracle (oracle/env_oracle.py, imported, not edited) plus the replay rule:
``reset_backward()`` reverses the valid points of every finished row and re-arms
the batch; in the step that follows, a row whose length is still below its
``init_len`` *replays* -- its new point is the one already stored, the action is
ignored, only LENGTH can stop it, its reward is 0.  Everything else is the
oracle's own arithmetic (``scale_actions``, ``_stopping``, ``format_state``).

``suppress=False`` evaluates every criterion on replaying rows too.  Either way
``replay_log`` keeps the replayed decisions on which the full set of criteria
and LENGTH alone disagree: (streamline, points after the step, all bits).

Also here: the inputs of tests/test_bidirectional.py -- seeds that include the
border shell of the ball mask, and actions scripted per (streamline id, pass,
step) so that the GPU and the restatement consume the same values.
"""
import numpy as np

from oracle import env_oracle as orc

CUT = orc.FLAG_MASK | orc.FLAG_CURVATURE


class _Bidirectional:
    """``reset_backward`` / replaying ``step`` on top of an oracle env class."""

    suppress = True
    init_len = None

    def _start(self, initial_points):
        self.init_len = self.seed_index = self.flags_forward = None
        self.replay_log = []
        return super()._start(initial_points)

    def reset_backward(self):
        assert len(self.continue_idx) == 0, 'rows are still active'
        n = len(self.streamlines)
        f = (self.lengths - ((self.flags & CUT) != 0)).astype(np.int32)
        assert f.min() >= 1
        for g in range(n):
            self.streamlines[g, :f[g]] = self.streamlines[g, :f[g]][::-1].copy()
        self.flags_forward = self.flags.copy()
        self.init_len, self.seed_index = f, f - 1
        self.replay_log = []
        self.flags = np.zeros(n, dtype=int)
        self.lengths = np.ones(n, dtype=np.int32)
        self.length = 1
        self.dones = np.full(n, False)
        self.continue_idx = np.arange(n)
        self.state = orc.format_state(self.vol, self.neigh, self.streamlines, 1, self.n_dirs)
        return self.state[self.continue_idx]

    def step(self, actions):
        if self.init_len is None:
            return super().step(actions)
        idx, L, hist = self.continue_idx, self.length, self.streamlines
        replay = L < self.init_len[idx]
        live = idx[~replay]
        self.last_replay = replay
        # ordinary rows: tracking_env.py:135-183 through the oracle's own pieces
        if len(live):
            directions = orc.scale_actions(self._perturb(actions[~replay]), self.step_size)
            if L == 1:
                saved = hist[live, L, :].copy()
                hist[live, L, :] = hist[live, L - 1, :] + directions
                flip, _ = self._stopping(live, L + 1)
                hist[live, L, :] = saved
                directions[flip] *= -1
            hist[live, L, :] = hist[live, L - 1, :] + directions
        # replaying rows: the point is the one already stored at hist[g][L]
        self.length = L = L + 1
        stopping = np.zeros(len(idx), dtype=bool)
        new_flags = np.zeros(len(idx), dtype=int)
        stopping[~replay], new_flags[~replay] = self._stopping(live, L)
        _, full = self._stopping(idx[replay], L)
        kept = full & orc.FLAG_LENGTH
        for g, bits in zip(idx[replay][full != kept], full[full != kept]):
            self.replay_log.append((int(g), L, int(bits)))
        if not self.suppress:
            kept = full
        stopping[replay], new_flags[replay] = kept != 0, kept

        self.not_stopping = np.logical_not(stopping)
        self.new_continue_idx = idx[~stopping]
        self.stopping_idx = idx[stopping]
        self.flags[self.stopping_idx] = new_flags[stopping]
        self.dones[self.stopping_idx] = 1

        reward = np.zeros(hist.shape[0])
        if self.compute_reward:
            reward = np.zeros(len(idx))
            if len(live):
                p2 = hist[live, L - 3] if L >= 3 else None
                align = orc.peaks_alignment_reward(self.peaks, hist[live, L - 1],
                                                   hist[live, L - 2], p2)
                reward[~replay], _ = orc.combine_rewards(
                    [('peaks_reward', self.alignment_weighting, align),
                     ('oracle_reward', 0.0, None)], len(live))
        self.state[idx] = orc.format_state(self.vol, self.neigh, hist[idx], L, self.n_dirs)
        return (self.state[idx], reward, self.dones[idx],
                {'continue_idx': idx, 'reward_info': {}})


class BidirectionalOracleEnv(_Bidirectional, orc.OracleTrackingEnv):
    pass


class BidirectionalOracleNoisyEnv(_Bidirectional, orc.OracleNoisyTrackingEnv):
    pass


# --------------------------------------------------------------------------- #
# inputs
def border_seeds(mask, n, seed=7):
    """n seeds in the ball mask: every fourth one in a voxel of its border shell
    (a mask voxel with a neighbour outside), pushed towards the outside, so that
    some first steps leave in both directions and some seeds fail the mask test
    themselves; every eighth one near the centre."""
    rng = np.random.RandomState(seed)
    m = np.asarray(mask).astype(bool)
    pad = np.pad(m, 1)
    inner = np.ones_like(m)
    for ax in range(3):
        for sh in (-1, 1):
            inner &= np.roll(pad, sh, axis=ax)[1:-1, 1:-1, 1:-1]
    shell = np.argwhere(m & ~inner)
    vox = np.argwhere(m)
    centre = (np.asarray(m.shape) - 1) / 2.0
    seeds = vox[rng.randint(0, len(vox), n)] + rng.uniform(-0.5, 0.5, (n, 3))
    pick = shell[rng.randint(0, len(shell), n)]
    out = pick - centre
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    edge = pick + rng.uniform(-0.5, 0.5, (n, 3)) + out * rng.uniform(0.0, 1.2, (n, 1))
    seeds[1::4] = edge[1::4]
    # ... and every eighth one near the centre, where a circle of kind 0 (see
    # scripted_actions) fits into the ball and runs into LENGTH
    seeds[2::8] = (centre + rng.uniform(-1.0, 1.0, (n, 3)))[2::8]
    return seeds


def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _noise(ids, pass_no, step, comp):
    """Centred, unit-variance noise keyed by (id, pass, step, component)."""
    with np.errstate(over='ignore'):
        base = _mix32(np.asarray(ids, dtype=np.uint32) * np.uint32(0x27D4EB2F) +
                      np.uint32((pass_no * 1000003 + step * 7919 + comp * 104729 + 12345)
                                & 0xffffffff))
        acc = np.zeros(len(base))
        for k in range(4):
            acc += (_mix32(base + np.uint32(k * 0x9E3779B9 & 0xffffffff)) >> np.uint32(8)) \
                * 2.0 ** -24
    return (acc - 2.0) * np.sqrt(3.0)


TURN_DEG = 20.0


def scripted_actions(state, n_sh, ids, pass_no, step):
    """float32 (n, 3) actions for the active rows ``ids`` (global streamline ids),
    from the newest segment in their state rows (``state[:, n_sh:n_sh + 3]``;
    zeros at the first step of a pass):

      kind 0 (a third of the (id, pass) pairs)  turn by TURN_DEG in a fixed plane:
             a circle of 2.2 voxels radius, stays inside unless it starts at the
             border, ends by LENGTH;
      kind 1  follow the previous direction with a small wobble: leaves by MASK;
      kind 2  a large wobble: stops by CURVATURE.
    """
    ids = np.asarray(ids)
    n = len(ids)
    z = np.stack([_noise(ids, pass_no, step, c) for c in range(3)], axis=1)
    fixed = np.stack([_noise(ids, pass_no, 9999, c) for c in range(3)], axis=1)
    kind = _mix32(ids.astype(np.uint32) * np.uint32(2654435761) + np.uint32(pass_no)) % 3
    prev = np.asarray(state)[:, n_sh:n_sh + 3].astype(np.float64)
    nrm = np.linalg.norm(prev, axis=1, keepdims=True)
    fresh = nrm[:, 0] == 0
    nrm[fresh] = 1.0
    d = prev / nrm
    d[fresh] = z[fresh]
    a = np.empty((n, 3))
    # kind 0: rotate d by TURN_DEG about normalised (d x fixed)
    w = np.cross(d, fixed)
    w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-12)
    # (the plane's normal with one sign for the whole pass: d x fixed changes sign
    # whenever d passes fixed)
    sense = np.stack([_noise(ids, pass_no, 9998, c) for c in range(3)], axis=1)
    w *= np.where((w * sense).sum(axis=1) < 0, -1.0, 1.0)[:, None]
    t = np.deg2rad(TURN_DEG)
    a[:] = d * np.cos(t) + np.cross(w, d) * np.sin(t)
    wob = np.where(kind == 1, 0.04, 0.5)[:, None]
    a[kind != 0] = (d + wob * z)[kind != 0]
    a[fresh] = z[fresh]
    return np.ascontiguousarray(a, dtype=np.float32)
