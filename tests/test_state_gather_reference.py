"""The state gather (csrc/ttl_state.hip: k_state, k_state_dd and the fused step
tails) against the plain float64 definition of tests/ref_state.py: every
record width, row containment, coordinates at and beyond the volume border,
the coordinate shift, every launch path over several steps.

Every comparison covers every element of every row: the signal block within
``16 * 2**-24 * S`` (ref_state's docstring derives the bound), the direction
block bit for bit.  Nothing is masked out except rows the reference itself
makes NaN (a non-finite coordinate), and those must be NaN in the kernel too.

Shapes: a 6 x 7 x 5 volume (not cubic, no dimension a multiple of the 4-voxel
brick) and 203 rows (several workgroups for every lane-group size, a multiple
of none of 16 / 8 / 5 / 4 / 2 rows per wave) for the resets; 14^3 and 700 rows
(as test_other_sh_orders) for the episodes.  Seeds are multiples of 2**-16 and
volume magnitudes lie in [0.1, 1], so that no product can underflow
(``ref_state.check_inputs``).

The CPU tests show that the reference agrees with SciPy, that the oracle's
float32 restatement sits where it is expected, that a float32 emulation of
each kernel's operation order stays inside the bound on every input set the GPU
tests use, and that every mutation of the reference leaves it.
"""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import ref_state as rs
from helpers import synthetic_subject

DIMS = (6, 7, 5)
N_SWEEP = 203
SWEEP_R = 0.375
SWEEP_K = 3
WIDTHS = list(range(1, 69)) + [125, 128, 129, 132]
CONTAINED = [5, 6, 7, 33, 34, 35, 45, 63]
EDGE_C = [45, 34]
EDGE_R_DD = [0.3, 0.5, 0.999]
EDGE_R_56 = [0.0, 1.0, 1.25]
SHIFTS = [0.0, 0.5, -0.5]
STEP_C = [7, 33, 34, 35, 45]
STEP_K = [1, 4, 13, 100]
STEP_D, STEP_N, STEP_R = 14, 700, 0.75
POISON = 0x7fc0abcd            # one fixed NaN bit pattern
EMULATED_C = [4, 5, 8, 28, 33, 45, 64, 65, 129]    # kernel rows == emulate_k_state_dd, bit for bit
EMULATED_EDGE = (34, 0.5)
PINNED_MAX_C = 64               # wider records ran looping kernels of unstated order at the fixture's commit
TRACE_K = 4                     # the K whose episodes the fixture holds
CONFIGS = ['three_launch', 'one_launch', 'sorted_order', 'free_running']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'state_rows_trace.json')


# --------------------------------------------------------------------------- #
# input sets (shared by the CPU and the GPU tests)
@functools.lru_cache(maxsize=None)
def volume(C_, dims=DIMS):
    rng = np.random.RandomState(1000 + C_)
    v = rng.uniform(0.1, 1.0, dims + (C_,)) * rng.choice([-1.0, 1.0], dims + (C_,))
    return v.astype(np.float32)


def _quant(x):
    return (np.round(np.asarray(x, np.float64) * 65536.0) / 65536.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_seeds(C_):
    rng = np.random.RandomState(C_)
    return _quant(rng.uniform(-2.0, np.array(DIMS) + 2.0, (N_SWEEP, 3)))


@functools.lru_cache(maxsize=None)
def edge_heads(radius, nonfinite=True):
    """Per axis (the other two random inside): -1e9, -6, -4 - r, -1 - r, -1, -r,
    -+2**-20, 0, r, 1 - r, 0.5, dim - 1 -+ r, dim - 1, dim -+ r, dim, dim + 5,
    1e9 and every integer k +- r inside the volume; the 3-axis product of six
    of them; with ``nonfinite`` ten rows with NaN / inf at the end."""
    r = np.float32(radius)
    rng = np.random.RandomState(77)
    f = np.float32
    rows = []

    def axis_values(dim):
        d = f(dim)
        vals = [f(-1e9), f(-6), f(-4) - r, f(-1) - r, f(-1), -r, f(-2.0 ** -20), f(0),
                f(2.0 ** -20), r, f(1) - r, f(0.5), d - f(1) - r, d - f(1), d - f(1) + r,
                d - r, d, d + r, d + f(5), f(1e9)]
        for k in range(dim):
            for v in (f(k) + r, f(k) - r):
                if 0 <= v <= dim - 1:
                    vals.append(v)
        return vals

    for a in range(3):
        for v in axis_values(DIMS[a]):
            p = _quant(rng.uniform(0.5, np.array(DIMS) - 1.5))
            p[a] = v
            rows.append(p)
    sub = [[f(-1) - r, f(-2.0 ** -20), r, f(d) - f(1) - r, f(d) - f(1), f(d) + r] for d in DIMS]
    for x in sub[0]:
        for y in sub[1]:
            for z in sub[2]:
                rows.append(np.array([x, y, z], np.float32))
    if nonfinite:
        for a in range(3):
            for v in (np.nan, np.inf, -np.inf):
                p = _quant(rng.uniform(0.5, np.array(DIMS) - 1.5))
                p[a] = v
                rows.append(p)
        rows.append(np.full(3, np.nan, np.float32))
    return np.array(rows, dtype=np.float32)


def edge_cases():
    return [(C_, r) for C_ in EDGE_C for r in EDGE_R_DD + EDGE_R_56]


def _random_walk(n, length, seed=5):
    rng = np.random.RandomState(seed)
    steps = rng.standard_normal((n, length, 3)).astype(np.float32)
    return np.cumsum(steps, axis=1, dtype=np.float32)


def _reset_reference(vol, heads, radius, shift, K, mutate=None):
    heads = np.asarray(heads, np.float32)
    return rs.state_rows_f64(vol, heads, radius, shift, heads[:, None, :], 1, K, mutate)


#: the case each mutation must be caught on: (kind, C, radius, shift)
MUTATION_CASE = {
    'clip_weights': ('edge', 34, 0.5, 0.0),
    'swap_yz_strides': ('sweep', 33, SWEEP_R, 0.0),
    'plus_no_cross': ('edge', 34, 0.5, 0.0),
    'minus_no_cross': ('edge', 34, 0.5, 0.0),
    'offset_sign': ('sweep', 33, SWEEP_R, 0.0),
    'shift_centre_only': ('edge', 34, 0.5, 0.5),
    'tail_columns_zero': ('sweep', 33, SWEEP_R, 0.0),
    'dirs_off_by_one': ('steps', 7, STEP_R, 0.0),
    'dirs_not_padded': ('steps', 7, STEP_R, 0.0),
}


def _case_heads(kind, C_, radius):
    return sweep_seeds(C_) if kind == 'sweep' else edge_heads(radius)


# --------------------------------------------------------------------------- #
# CPU
def test_reference_agrees_with_scipy_map_coordinates():
    """One channel of the float64 volume, order 1, mode 'nearest' (= clipped
    indices), inside and outside the volume.  3.3e-16 measured with the
    shift of 0.5 used here; the bound is nine float64 roundings of values <= 1."""
    from scipy.ndimage import map_coordinates
    vol = volume(33)
    heads = np.concatenate((sweep_seeds(33), edge_heads(0.375, nonfinite=False)))
    heads = heads[np.abs(heads).max(axis=1) < 1e6]      # SciPy's own index arithmetic
    value, _ = _reset_reference(vol, heads, 0.375, 0.5, 1)
    pts = rs.stencil_points(heads, 0.375, 0.5).astype(np.float64).reshape(-1, 3)
    worst = 0.0
    for c in (0, 17, 32):
        want = map_coordinates(vol[..., c].astype(np.float64), pts.T, order=1, mode='nearest')
        got = value[:, :7 * 33].reshape(-1, 7, 33)[:, :, c].reshape(-1)
        worst = max(worst, np.abs(got - want).max())
    print('max |ref_state - map_coordinates| =', worst)
    assert worst <= 1e-15


def test_oracle_format_state_against_the_reference():
    """oracle.env_oracle.format_state forms its weights from the expanded
    polynomial in float32, which cancels, so it is held to an absolute bound,
    not to 16 * 2**-24 * S.  Measured on these inputs (data of size <= 1, sweep
    seeds at C = 33 and 45, edge coordinates at radius 0.5): 1.97e-7, which is
    7.6 * 2**-24 * S at worst here; allowed: 4 x that, 7.9e-7.  The direction
    block is exact."""
    from oracle import env_oracle as orc
    worst = 0.0
    for C_, heads, r in ((33, sweep_seeds(33), SWEEP_R), (45, sweep_seeds(45), SWEEP_R),
                         (34, edge_heads(0.5, nonfinite=False), 0.5)):
        vol = volume(C_)
        hist = np.concatenate((_random_walk(len(heads), 2), heads[:, None, :]), axis=1)
        value, _ = rs.state_rows_f64(vol, heads, r, 0.0, hist, 3, 4)
        got = orc.format_state(vol, orc.neighborhood_offsets(r), hist, 3, 4)
        worst = max(worst, np.abs(got[:, :7 * C_] - value[:, :7 * C_]).max())
        assert np.array_equal(got[:, 7 * C_:], value[:, 7 * C_:].astype(np.float32))
    print('max |format_state - ref_state| =', worst)
    assert worst <= 7.9e-7


def _emulation_excess(vol, heads, radius, shift):
    value, S = _reset_reference(vol, heads, radius, shift, 1)
    n = 7 * vol.shape[3]
    worst = rs.excess(rs.emulate_k_state(vol, heads, radius, shift), value[:, :n], S).max()
    if 0.0 < radius < 1.0:
        worst = max(worst, rs.excess(rs.emulate_k_state_dd(vol, heads, radius, shift),
                                     value[:, :n], S).max())
    return worst


@pytest.mark.parametrize('C_', WIDTHS)
def test_emulations_stay_inside_the_bound_width_sweep(C_):
    """Volume and seeds are drawn per width: every one of the sweep's 72 input
    sets is checked, the no-underflow condition included."""
    rs.check_inputs(volume(C_), sweep_seeds(C_), SWEEP_R, 0.0)
    worst = _emulation_excess(volume(C_), sweep_seeds(C_), SWEEP_R, 0.0)
    print('worst error / bound =', worst)
    assert worst <= 1.0


@pytest.mark.parametrize('C_,radius', edge_cases())
def test_emulations_stay_inside_the_bound_edge_coordinates(C_, radius):
    for shift in SHIFTS:
        rs.check_inputs(volume(C_), edge_heads(radius), radius, shift)
        worst = _emulation_excess(volume(C_), edge_heads(radius), radius, shift)
        print('shift', shift, 'worst error / bound =', worst)
        assert worst <= 1.0


@pytest.mark.parametrize('C_', STEP_C)
def test_emulations_stay_inside_the_bound_episode_like_points(C_):
    """A STAND-IN, not the episodes' own input: their coordinates are whatever
    the step kernels leave (float32 points inside the mask of a 14^3 volume),
    known only on the GPU.  Here: the episodes' volume of this width and 4000
    random float32 points over the same range."""
    vol = volume(C_, (STEP_D,) * 3)
    heads = np.random.RandomState(C_).uniform(0.6, 12.4, (4000, 3)).astype(np.float32)
    rs.check_inputs(vol, heads, STEP_R, 0.0)
    assert _emulation_excess(vol, heads, STEP_R, 0.0) <= 1.0


@pytest.mark.parametrize('mutation', rs.MUTATIONS)
def test_every_mutation_leaves_the_bound_cpu(mutation):
    kind, C_, radius, shift = MUTATION_CASE[mutation]
    if kind == 'steps':
        hist = _random_walk(50, 3)
        good = rs.direction_block(hist, 3, 4)
        assert not np.array_equal(good, rs.direction_block(hist, 3, 4, mutation))
        return
    vol, heads = volume(C_), _case_heads(kind, C_, radius)
    value, S = _reset_reference(vol, heads, radius, shift, 1, mutation)
    n = 7 * C_
    for emu in (rs.emulate_k_state, rs.emulate_k_state_dd):
        assert rs.excess(emu(vol, heads, radius, shift), value[:, :n], S).max() > 1.0


# --------------------------------------------------------------------------- #
# GPU: ttl_env_reset with chosen seeds is the gather alone at L = 1
class _Rig:
    """One packed volume and the per-streamline buffers of a handle."""

    def __init__(self, vol, layout, n_max, K):
        import torch
        from tracktolearn_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        dev = 'cuda:0'
        X, Y, Z, C_ = vol.shape
        self.vol, self.C, self.K, self.n_max, self.layout = vol, C_, K, n_max, layout
        self.coef_pitch = (C_ + 3) // 4 * 4
        self.T = 4                                      # max_nb_steps
        dims = (C.c_int32 * 3)(X, Y, Z)
        n_rec = int(self.lib.ttl_sh_volume_records(dims, layout))
        src = torch.from_numpy(np.ascontiguousarray(vol)).to(dev)
        self.packed = torch.zeros(n_rec * self.coef_pitch, dtype=torch.float32, device=dev)
        _lib.check(self.lib.ttl_pack_sh_volume(src.data_ptr(), self.packed.data_ptr(), dims, C_,
                                               self.coef_pitch, layout, None), 'pack')
        self.mask = torch.ones((X, Y, Z), dtype=torch.float64, device=dev)
        self.hist = torch.zeros((n_max, self.T + 1, 3), dtype=torch.float32, device=dev)
        self.flags = torch.zeros(n_max, dtype=torch.int32, device=dev)
        self.lengths = torch.zeros(n_max, dtype=torch.int32, device=dev)
        self.dones = torch.zeros(n_max, dtype=torch.uint8, device=dev)
        self.idx = torch.zeros((2, n_max), dtype=torch.int32, device=dev)
        self.ws_bytes = int(self.lib.ttl_env_workspace_bytes(n_max))
        self.ws = torch.zeros(self.ws_bytes + 256, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def gather(self, seeds, radius, shift, *, knobs=None, by_position=False, extra_pitch=0):
        """Rows of ttl_env_reset(seeds) as int32 words, (n + 8, state_pitch):
        the buffer is pre-filled with POISON, 8 rows past n included."""
        torch, _lib, lib = self.torch, self._lib, self.lib
        d = _lib.EnvDesc()
        d.abi_version, d.mode = _lib.ABI_VERSION, _lib.MODE_F32
        d.sh_dim[:] = d.mask_dim[:] = self.vol.shape[:3]
        d.n_coef, d.coef_pitch = self.C, self.coef_pitch
        d.sh_packed = self.packed.data_ptr()
        d.sh_coord_shift = float(shift)
        d.sh_layout = self.layout
        d.mask_coef = self.mask.data_ptr()
        d.mask_threshold = 0.1
        d.n_dirs, d.max_nb_steps, d.step_size_vox = self.K, self.T, 0.75
        d.neigh_radius_vox = float(np.float32(radius))
        d.n_max = self.n_max
        d.streamlines, d.flags = self.hist.data_ptr(), self.flags.data_ptr()
        d.lengths, d.dones = self.lengths.data_ptr(), self.dones.data_ptr()
        d.idx_a, d.idx_b = self.idx[0].data_ptr(), self.idx[1].data_ptr()
        d.workspace = (self.ws.data_ptr() + 255) // 256 * 256
        d.workspace_bytes = self.ws_bytes
        n = len(seeds)
        pitch = 7 * self.C + 3 * self.K + extra_pitch
        out = torch.full(((n + 8) * pitch,), POISON, dtype=torch.int32, device='cuda:0')
        dev_seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.float32)).to('cuda:0')
        h = C.c_void_p()
        with pytest.MonkeyPatch.context() as mp:        # the knobs are read at create
            mp.setenv('TTL_ORDER_MIN_ROWS', '1')
            for k, v in (knobs or {}).items():
                mp.setenv(k, str(v))
            _lib.check(lib.ttl_env_create(C.byref(d), C.byref(h)), 'ttl_env_create')
        try:
            _lib.check(lib.ttl_env_reset(h, dev_seeds.data_ptr(), n,
                                         _lib.ORDER_BY_POSITION if by_position else None,
                                         out.data_ptr(), pitch, None), 'ttl_env_reset')
            torch.cuda.synchronize()
        finally:
            lib.ttl_env_destroy(h)
        return out.cpu().numpy().reshape(n + 8, pitch)


def _contained(words, n, width):
    """Nothing outside columns [0, width) of rows 0..n-1 was written, and
    every word inside was."""
    assert (words[n:] == POISON).all(), 'rows past the last one were written'
    assert (words[:n, width:] == POISON).all(), 'words between two rows were written'
    assert not (words[:n, :width] == POISON).any(), 'a word of a row was never written'
    return np.ascontiguousarray(words[:n, :width]).view(np.float32)


def _inside(rows, value, S, C_, what, quiet=False):
    n = 7 * C_
    e = rs.excess(rows[:, :n], value[:, :n], S)
    bad = np.argwhere(e > 1.0)
    if not quiet or len(bad):
        print(what, 'worst error / bound', e.max(), 'elements outside', len(bad))
    assert not len(bad), (what, 'first (row, column) outside the bound', bad[:8].tolist(),
                          'rows', sorted(set(bad[:, 0].tolist()))[:16])
    assert np.array_equal(rows[:, n:], value[:, n:].astype(np.float32)), (what, 'direction block')
    return e.max()


# --------------------------------------------------------------------------- #
# GPU: the bits of the rows, against tests/golden/state_rows_trace.json
# (golden/make_golden_state_rows.py records it with these same functions)
def digest(*arrays):
    """SHA-256 over the bytes of the arrays, the first 128 bits in hex."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def episode_digest(trace):
    """One digest over the per-step digests of an episode."""
    return digest(np.frombuffer(''.join(trace).encode(), np.uint8))


def edge_name(C_, radius, shift):
    return f'C={C_} r={radius} shift={shift}'


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _equals_emulation(rows, C_, heads, radius, shift, what):
    """The signal block of the finite rows equals emulate_k_state_dd bit for bit."""
    n = 7 * C_
    want = rs.emulate_k_state_dd(volume(C_), heads, radius, shift)
    bad = np.argwhere(rows[:, :n].view(np.uint32) != want.view(np.uint32))
    print(what, 'elements that are not the emulation\'s bits:', len(bad))
    assert not len(bad), (what, 'first (row, column)', bad[:8].tolist())


_SWEEP_OUT = {}


def _sweep_variants(C_, extra_pitch=0):
    """{(layout, state_kernel, flavour, by_position): rows} of the width sweep."""
    from tracktolearn_amd import _lib
    out = {}
    for layout in (_lib.SH_LINEAR, _lib.SH_BRICK4):
        rig = _Rig(volume(C_), layout, N_SWEEP, SWEEP_K)
        for kernel in (4, 3, 0):
            for flavour in (0, 8):
                for by_position in (False, True):
                    words = rig.gather(sweep_seeds(C_), SWEEP_R, 0.0, by_position=by_position,
                                       knobs=dict(TTL_STATE_KERNEL=kernel,
                                                  TTL_STORE_FLAVOUR=flavour),
                                       extra_pitch=extra_pitch)
                    out[layout, kernel, flavour, by_position] = _contained(
                        words, N_SWEEP, 7 * C_ + 3 * SWEEP_K)
    return out


def _check_sweep(C_, runs):
    """Every run inside the bound; layout, store flavour and processing order
    change no bit of a kernel's rows.  Returns {TTL_STATE_KERNEL: rows}."""
    value, S = _reset_reference(volume(C_), sweep_seeds(C_), SWEEP_R, 0.0, SWEEP_K)
    out = {}
    for kernel in (4, 3, 0):
        group = {k: v for k, v in runs.items() if k[1] == kernel}
        first_key = next(iter(group))
        for key, rows in group.items():
            assert rows.tobytes() == group[first_key].tobytes(), (key, 'differs from', first_key)
        _inside(group[first_key], value, S, C_, f'C={C_} TTL_STATE_KERNEL={kernel}')
        out[kernel] = group[first_key]
    return out


def _sweep_output(C_):
    if C_ not in _SWEEP_OUT:
        _SWEEP_OUT[C_] = _check_sweep(C_, _sweep_variants(C_))
    return _SWEEP_OUT[C_]


@pytest.mark.gpu
@pytest.mark.parametrize('C_', WIDTHS)
def test_every_record_width(C_):
    """Inside the float64 bound (``_check_sweep``), and the bits: k_state's rows
    and k_state_dd's of records up to 64 floats are the fixture's.  Wider records
    ran looping kernels whose fused operations the compiler chose when the
    fixture was recorded: those rows are held to the emulation of the stated
    order instead, bit for bit, and whether the old digest was kept is printed."""
    out = _SWEEP_OUT[C_] = _check_sweep(C_, _sweep_variants(C_))
    want = golden()['sweep'][str(C_)]
    assert digest(out[0]) == want['0'], 'k_state rows moved'
    for kernel in (4, 3):
        kept = digest(out[kernel]) == want[str(kernel)]
        if C_ <= PINNED_MAX_C:
            assert kept, f'TTL_STATE_KERNEL={kernel} rows moved'
        else:
            print(f'C={C_} TTL_STATE_KERNEL={kernel}: the fixture\'s digest was',
                  'kept' if kept else 'not kept')
    if C_ in EMULATED_C or C_ > PINNED_MAX_C:
        _equals_emulation(out[4], C_, sweep_seeds(C_), SWEEP_R, 0.0, f'C={C_}')


@pytest.mark.gpu
def test_all_k_state_dd_runs_are_bit_identical():
    """TTL_STATE_KERNEL=4 (the last column's floats merged into one 16-byte
    store) and 3 (separate tail stores) are two instantiations of one source
    and must give the same bits at every width.

    They did not while ttl_state.hip left the contraction of its blends to
    the compiler, which fused the fourth float of a column differently in
    the separate-tail kernels (2-4 % of the elements of every C in 4..64 a
    last bit away, at most 2.81 * 2**-24 * S, inside the bound).  The file is
    now compiled without contraction and ``blend<>`` / ``lerp<>`` state every
    fused operation: the order is stated, not found, and every instantiation
    gives the same bits by construction (``test_every_record_width`` holds
    them to ``ref_state.emulate_k_state_dd`` and to the fixture)."""
    differ = {}
    for C_ in WIDTHS:
        out = _sweep_output(C_)
        if out[4].tobytes() != out[3].tobytes():
            value, S = _reset_reference(volume(C_), sweep_seeds(C_), SWEEP_R, 0.0, SWEEP_K)
            n = 7 * C_
            d = np.abs(out[4][:, :n].astype(np.float64) - out[3][:, :n]) / (rs.EPS * S)
            differ[C_] = (int((d > 0).sum()), float(d.max()))
    print('widths whose merged- and separate-tail rows differ: {C: (elements, '
          'max |difference| / (2**-24 S))}', differ)
    assert not differ, sorted(differ)


@pytest.mark.gpu
@pytest.mark.parametrize('C_', CONTAINED)
def test_rows_stay_inside_a_wider_pitch(C_):
    """state_pitch = 7 C + 3 K + 5: the merged-tail 16-byte stores are written
    at ``o - back`` and must not leave columns [0, 7 C + 3 K) of their row
    (``_contained``, on every variant of the sweep)."""
    wide = _check_sweep(C_, _sweep_variants(C_, extra_pitch=5))
    for kernel, rows in _sweep_output(C_).items():      # the pitch changes no bit
        assert rows.tobytes() == wide[kernel].tobytes(), kernel


_EDGE_OUT = {}


def _edge_output(C_, radius, shift):
    key = (C_, radius, shift)
    if key not in _EDGE_OUT:
        from tracktolearn_amd import _lib
        heads = edge_heads(radius)
        rig = _Rig(volume(C_), _lib.SH_BRICK4, len(heads), SWEEP_K)
        _EDGE_OUT[key] = _contained(rig.gather(heads, radius, shift), len(heads),
                                    7 * C_ + 3 * SWEEP_K)
    return _EDGE_OUT[key]


@pytest.mark.gpu
@pytest.mark.parametrize('C_,radius', edge_cases())
def test_edge_coordinates_and_shift(C_, radius):
    """Radii in (0, 1) take k_state_dd, the others k_state.  NULL processing
    order (the rows with NaN / inf coordinates are in)."""
    from tracktolearn_amd import _lib
    heads = edge_heads(radius)
    for shift in SHIFTS:
        rows = _edge_output(C_, radius, shift)
        value, S = _reset_reference(volume(C_), heads, radius, shift, SWEEP_K)
        assert np.isnan(value[:, 0]).sum() == 10 and np.isnan(value[-10:, 0]).all()
        _inside(rows, value, S, C_, f'C={C_} r={radius} shift={shift}')
        # the bits of the finite rows (the NaN payloads of the last 10 are not pinned)
        assert digest(rows[:-10]) == golden()['edge'][edge_name(C_, radius, shift)], shift
        if (C_, radius) == EMULATED_EDGE:
            _equals_emulation(rows[:-10], C_, heads[:-10], radius, shift,
                              edge_name(C_, radius, shift))
        # the finite rows again in the other layout and in the library's sorted
        # processing order: the same bits
        rig = _Rig(volume(C_), _lib.SH_LINEAR, len(heads) - 10, SWEEP_K)
        again = _contained(rig.gather(heads[:-10], radius, shift, by_position=True),
                           len(heads) - 10, 7 * C_ + 3 * SWEEP_K)
        assert again.tobytes() == rows[:-10].tobytes(), shift


# --------------------------------------------------------------------------- #
# GPU: every launch path, several steps
def _step_env(monkeypatch, C_, K, config):
    import torch
    from tracktolearn_amd.datasets.utils import MRIDataVolume as Vol
    from tracktolearn_amd.environments import TrackingEnvironment
    ordered = config == 'sorted_order'
    monkeypatch.setenv('TTL_FUSE_SMALL', '0' if config == 'three_launch' else '1')
    monkeypatch.setenv('TTL_ORDER_INSTEP', '0')
    if ordered:
        monkeypatch.setenv('TTL_ORDER_MIN_ROWS', '1')
        monkeypatch.setenv('TTL_FUSE_MAX_ROWS', '256')
    monkeypatch.setattr(TrackingEnvironment, 'SPATIAL_ORDER_MIN', 1 if ordered else 1 << 30)
    sh = volume(C_, (STEP_D,) * 3)
    _, mask, _ = synthetic_subject(STEP_D, C=1, peaks=False)
    aff = np.eye(4, dtype=np.float32)
    m = Vol(mask.astype(np.float32), aff)
    dto = dict(n_dirs=K, theta=30.0, npv=1, binary_stopping_threshold=0.1, step_size=STEP_R,
               min_length=2.0, max_length=12.0, compute_reward=False, alignment_weighting=1.0,
               oracle_bonus=0.0, oracle_checkpoint=None, oracle_stopping_criterion=False,
               rng=np.random.RandomState(0), device=torch.device('cuda:0'), target_sh_order=8,
               noise=0.0, fa_map=None)
    env = TrackingEnvironment((Vol(sh, aff), m, m, None, None), 'testing', dto)
    rng = np.random.RandomState(C_)
    vox = np.argwhere(mask)
    env.seeds = vox[rng.randint(0, len(vox), STEP_N)] + rng.uniform(-0.5, 0.5, (STEP_N, 3))
    env.spatial_order = ordered
    return env, sh


_STEP_OUT = {}
_STEP_TRACE = {}


def _check_step(env, sh, K, idx, by_streamline, L, what, keep=None, done=None, trace=None):
    """Rows of the streamlines ``idx`` after the step that left them with L
    points, against the reference computed from the handle's own history.
    ``done``: the step's flags of these rows; the handle's own ``lengths`` of
    the rows that stopped must say L as well.  ``trace`` receives the digest of
    the step: the streamlines and their rows, in the order of the streamlines."""
    if trace is not None:
        by_id = np.argsort(idx, kind='stable')
        trace.append(digest(np.asarray(idx, np.int64)[by_id], by_streamline[by_id]))
    hist = env.streamlines[idx]
    if done is not None:
        stopped = done.cpu().numpy()[:len(idx)].astype(bool)
        assert (env.lengths[idx[stopped]] == L).all(), what
    value, S = rs.state_rows_f64(sh, hist[:, L - 1], STEP_R, 0.0, hist, L, K)
    if keep is not None:
        keep.append((by_streamline, hist, L))
    return _inside(by_streamline, value, S, sh.shape[3], what, quiet=True)


def _episode(monkeypatch, C_, K, config):
    import torch
    from tracktolearn_amd import _lib
    env, sh = _step_env(monkeypatch, C_, K, config)
    what = f'C={C_} K={K} {config}'
    keep = _STEP_OUT.setdefault((C_, K), []) if config == 'one_launch' else None
    trace = _STEP_TRACE[C_, K, config] = []
    state = env.reset(0, STEP_N)
    worst = _check_step(env, sh, K, np.arange(STEP_N), state.cpu().numpy(), 1, what + ' reset',
                        trace=trace)
    steps, fills = 0, []
    if config in ('three_launch', 'one_launch'):
        env.profile_begin(64, classes=('prefix', 'state'))      # counts the launches
    if config != 'free_running':
        while env._n_active:
            idx = env.continue_idx
            if config == 'sorted_order' and steps % 2 == 1:
                env._refresh_processing_order(force=True)
            full, _, done, info = env.step_device(env.scripted_actions(state, steps, 9, 0.2))
            dest = info['row_dest'].cpu().numpy()
            worst = max(worst, _check_step(env, sh, K, idx, full.cpu().numpy()[dest], env.length,
                                           f'{what} step {steps}', keep, done, trace))
            state, _ = env.harvest()
            steps += 1
            fills.append((env._library_order()[0], env._n_active))
        if config == 'sorted_order':
            # slot records were read (an order in use) and some of them were holes
            print(what, '(slots, rows) after each harvest', fills)
            assert sum(slots > 0 for slots, _ in fills) >= 2
            assert any(slots > rows > 0 for slots, rows in fills)
        if config in ('three_launch', 'one_launch'):
            # k_prefix / k_tail launches and gather launches the steps made: the
            # one-launch tail is one "gather" per step and nothing else
            launches = {k: v[1] for k, v in env.profile_end().items()}
            assert launches['state'] == steps, launches
            assert launches['prefix'] == (steps if config == 'three_launch' else 0), launches
        print(what, steps, 'steps, worst error / bound', worst)
        return steps
    lib, h, n, idx, L = env._lib, env._handle, STEP_N, np.arange(STEP_N), 1
    buf = env._new_state(STEP_N)
    buf.copy_(state)
    done = torch.empty(STEP_N, dtype=torch.uint8, device=env.device)
    _lib.check(lib.ttl_env_freerun_begin(h, env._host_counts.data_ptr(), env._stream()), 'begin')
    try:
        while n and steps <= env.max_nb_steps + 1:
            a = env.scripted_actions_free(buf[:n], 9, 0.2)
            _lib.check(lib.ttl_env_freerun_step(h, a.data_ptr(), n, buf.data_ptr(),
                                                env._state_pitch, None, done.data_ptr(),
                                                env._stream()), 'ttl_env_freerun_step')
            torch.cuda.synchronize()
            L, steps = L + 1, steps + 1
            n_cont = int(env._host_counts_np[0])
            dest = env._row_dest_view(n).cpu().numpy()
            worst = max(worst, _check_step(env, sh, K, idx, buf[:n].cpu().numpy()[dest], L,
                                           f'{what} step {steps - 1}', None, done, trace))
            nxt = np.empty(n_cont, dtype=idx.dtype)
            nxt[dest[dest < n_cont]] = idx[dest < n_cont]       # survivors first, stable
            idx, n = nxt, n_cont
    finally:
        out = [C.c_int32() for _ in range(3)]
        _lib.check(lib.ttl_env_freerun_end(h, *[C.byref(o) for o in out], env._stream()), 'end')
    assert n == 0 and out[0].value == 0
    print(what, steps, 'steps, worst error / bound', worst)
    return steps


def episode_trace(C_, K, config):
    """The per-step digests of one episode (run now unless it already was)."""
    if (C_, K, config) not in _STEP_TRACE:
        with pytest.MonkeyPatch.context() as mp:
            _episode(mp, C_, K, config)
    return _STEP_TRACE[C_, K, config]


@pytest.mark.gpu
@pytest.mark.parametrize('config', CONFIGS)
@pytest.mark.parametrize('C_', STEP_C)
def test_every_launch_path_over_an_episode(C_, config):
    """To exhaustion (max_nb_steps = 16: every K sees steps with fewer segments
    than K, and K = 1, 4, 13 steps with more).

    The bits, at K = 4: the three-launch and the sorted-order episodes are the
    fixture's.  The one-launch and the free-running tails take the same
    scripted actions (a function of the direction block, the step and the
    streamline), so every step of theirs gives the three-launch episode's rows;
    they are also the fixture's wherever the fixture's commit had them agree
    with its three-launch episode."""
    for K in STEP_K:
        with pytest.MonkeyPatch.context() as mp:
            steps = _episode(mp, C_, K, config)
        assert steps >= 6, steps
    trace = _STEP_TRACE[C_, TRACE_K, config]
    want = golden()['episodes'][str(C_)]
    if config in ('three_launch', 'sorted_order'):
        assert episode_digest(trace) == want[config]
        return
    canonical = episode_trace(C_, TRACE_K, 'three_launch')
    assert trace == canonical, [i for i, (a, b) in enumerate(zip(trace, canonical)) if a != b]
    agreed = golden()['episodes_equal_three_launch'][str(C_)][config]
    kept = episode_digest(trace) == want[config]
    print(f'C={C_} {config}: the fixture\'s commit', 'agreed' if agreed else 'did not agree',
          'with its three-launch episode; its digest was', 'kept' if kept else 'not kept')
    assert kept or not agreed


# --------------------------------------------------------------------------- #
# GPU: the mutated references must reject the kernels' (right) output
@pytest.mark.gpu
@pytest.mark.parametrize('mutation', rs.MUTATIONS)
def test_every_mutation_is_caught_on_the_kernel_output(mutation, monkeypatch):
    kind, C_, radius, shift = MUTATION_CASE[mutation]
    if kind == 'steps':
        K = 4
        if (C_, K) not in _STEP_OUT:
            _episode(monkeypatch, C_, K, 'one_launch')
        caught = 0
        for rows, hist, L in _STEP_OUT[C_, K]:
            want = rs.direction_block(hist, L, K, mutation)
            caught += not np.array_equal(rows[:, 7 * C_:], want)
        # off by one shows from the first step on, the missing padding while L - 1 < K
        assert caught >= 3, caught
        return
    if kind == 'sweep':
        rows, heads = _sweep_output(C_)[4], sweep_seeds(C_)
    else:
        rows, heads = _edge_output(C_, radius, shift), edge_heads(radius)
    value, S = _reset_reference(volume(C_), heads, radius, shift, SWEEP_K, mutation)
    n = 7 * C_
    assert rs.excess(rows[:, :n], value[:, :n], S).max() > 1.0
