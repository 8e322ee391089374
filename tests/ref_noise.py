"""NumPy restatement of the keyed action noise (include/ttl_hip.h,
ttl_env_set_noise): Philox4x32-10 keyed by the seed, counter =
(id low, id high, step, j), two 53-bit uniforms per call, Box-Muller in
float64.  The GPU tests hold the library to this file; the CPU tests hold this
file to the Random123 known answers and to N(0, 1)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox(counter, key, rounds=10):
    """Philox4x32 on arrays: counter (..., 4) and key (..., 2) of uint32 words
    (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape).copy() for j in range(2))
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0          # 32 x 32 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _uniform(lo, hi):
    """((hi:lo >> 11) + 0.5) * 2^-53"""
    w = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, ids, step):
    """Standard normals (len(ids), 3) float64 of streamlines ``ids`` (int64,
    >= 0) at ``step`` under ``seed`` (any int, taken modulo 2^64)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.ndim == 1 and (ids >= 0).all()
    u = ids.astype(np.uint64)
    key = np.array([seed & MASK32, seed >> 32], dtype=np.uint64)
    z = np.empty((len(ids), 4), dtype=np.float64)
    for j in (0, 1):
        ctr = np.stack([u & MASK32, u >> np.uint64(32), np.full_like(u, int(step)),
                        np.full_like(u, j)], axis=-1)
        c = philox(ctr, key)
        u1, u2 = _uniform(c[:, 0], c[:, 1]), _uniform(c[:, 2], c[:, 3])
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * j] = r * np.cos(2.0 * np.pi * u2)
        z[:, 2 * j + 1] = r * np.sin(2.0 * np.pi * u2)
    return np.ascontiguousarray(z[:, :3])
