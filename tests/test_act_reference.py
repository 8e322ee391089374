"""ACT / CMC stopping as a kernel (ttl_act_flags) against its
NumPy restatement tests/ref_act.py: the restatement against hand cases and its
own named mutants on the CPU, the library against the restatement bit for bit on
the GPU; ``select_tracts(..., reject=...)`` on host tensors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import act_cases
import ref_act

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
MODES = (ref_act.THRESHOLD, ref_act.CMC)


# ------------------------------------------------------------------ CPU part
def test_uniforms_are_multiples_of_2_pow_minus_24():
    u1, u2 = ref_act.uniforms(7, act_cases.IDS_BASE + np.arange(1000), 3)
    for u in (u1, u2):
        assert ((u >= 0) & (u < 1)).all() and np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    assert not np.array_equal(u1, u2)
    assert 0.4 < u1.mean() < 0.6 and 0.4 < u2.mean() < 0.6


@pytest.mark.parametrize('k', range(3))
def test_hand_cases(k):
    case, mode, want = act_cases.hand_cases()[k]
    got = ref_act.act_flags_ordered(
        case['include'], case['exclude'], case['history'], case['n_points'], mode,
        ids=case['ids'], init_len=case['init_len'], coord_shift=case['coord_shift'],
        exponent=case['exponent'], seed=case['seed'], ids_base=case['ids_base'])
    assert got.dtype == np.uint8 and got.tolist() == want.tolist()


def test_hand_values():
    """Trilinear values on a grid whose value is linear in the index are the
    coordinate itself (clamped), exactly, for dyadic coordinates."""
    dims = (5, 4, 3)
    ix, iy, iz = np.meshgrid(*[np.arange(d) for d in dims], indexing='ij')
    inc = (ix + 8 * iy + 64 * iz).astype(np.float32)
    exc = np.zeros(dims, np.float32)
    pts = np.array([[0.25, 1.5, 0.75], [3.75, 2.25, 1.5], [-0.5, -0.25, 2.25], [4.25, 3.25, 0],
                    [4.5, 0, 0]], dtype=np.float32)
    v = ref_act.act_values_ordered(inc, exc, pts[:, None, :], 1)
    clamped = np.clip(pts[:4].astype(np.float64), 0, np.array(dims) - 1.0)
    assert v[:4, 0].tolist() == (clamped @ [1.0, 8.0, 64.0]).tolist()
    assert v[4].tolist() == [0.0, 0.0] and (v[:, 1] == 0).all()      # the far face is outside


def _mutant_modes(mutant):
    if mutant in ('ge_threshold', 'exclude_first'):
        return (ref_act.THRESHOLD,)
    if mutant in ('same_word', 'stop_gt', 'step_off_by_one'):
        return (ref_act.CMC,)
    return MODES


@pytest.mark.parametrize('mutant', ref_act.MUTANTS)
def test_every_mutant_differs_on_a_committed_case(mutant):
    differing = []
    for case in act_cases.cases():
        for mode in _mutant_modes(mutant):
            if not np.array_equal(act_cases.flags_of(case, mode),
                                  act_cases.flags_of(case, mode, mutate=mutant)):
                differing.append((case['name'], mode))
    assert differing, mutant
    if mutant == 'stop_gt':         # decided on the knife rows alone: u1 == P
        assert all(name.startswith('knife') for name, _ in differing)


def test_knife_rows_sit_on_p():
    knives = [c for c in act_cases.cases() if 'knife_row' in c]
    assert len(knives) >= 2
    for case in knives:
        flags, t = act_cases.flags_of(case, ref_act.CMC, return_terms=True)
        r = case['knife_row']
        assert t['u1'][r] == t['P'][r] == t['rho'][r] and 0 < t['P'][r] < 1
        assert flags[r] in (ref_act.TARGET, ref_act.EXCLUDE)             # u1 >= P stops
        assert act_cases.flags_of(case, ref_act.CMC, mutate='stop_gt')[r] == 0


def test_cases_hold_what_they_promise():
    names = [c['name'] for c in act_cases.cases()]
    assert len(set(names)) == len(names)
    assert {c['include'].shape for c in act_cases.cases()} == set(act_cases.GRIDS)
    seen = set()
    for case in act_cases.cases():
        assert case['ids_base'] > 2 ** 32
        v = ref_act.act_values_ordered(case['include'], case['exclude'], case['history'],
                                       case['n_points'], coord_shift=case['coord_shift'])
        inc, exc = v[:, 0], v[:, 1]
        s = inc + exc
        seen |= {k for k, hit in (('s0', (s == 0).any()), ('s1', (s >= 1).any()),
                                  ('inc0', ((inc == 0) & (exc > 0)).any()),
                                  ('exc0', ((exc == 0) & (inc > 0)).any()),
                                  ('half', (inc == 0.5).any()),
                                  ('half_up', (inc == act_cases.HALF_UP).any())) if hit}
        if 'knife_row' in case:
            continue
        x = case['history'][:, case['n_points'] - 1].astype(np.float64) + case['coord_shift']
        dims = np.array(case['include'].shape)
        for c in range(3):
            assert (x[:, c] == -0.5).any() and (x[:, c] == dims[c] - 0.5).any()
            assert ((x[:, c] < -0.5) & (x[:, c] > -0.51)).any()
            assert ((x[:, c] > dims[c] - 0.5) & (x[:, c] < dims[c] - 0.49)).any()
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (x == np.float32(1e30)).any() and (x == np.float32(-1e30)).any()
        assert sorted(case['ids'].tolist()) == list(range(len(case['history'])))
        rel = case['init_len'].astype(int) - case['n_points']
        assert {-1, 0, 1} <= set(rel.tolist())
    assert seen == {'s0', 's1', 'inc0', 'exc0', 'half', 'half_up'}


def test_no_cmc_row_is_undecided():
    """u1 >= P is the one place where two float64 ``pow``s may part: no committed
    row comes within 2^-40 of it (u1 is a multiple of 2^-24)."""
    for case in act_cases.cases():
        for n in (None, 1000):
            for use_init in (True, False):
                _, t = act_cases.flags_of(case, ref_act.CMC, n=n, use_init_len=use_init,
                                          return_terms=True)
                assert not ref_act.undecided(t, case['exponent']).any(), case['name']


def _reject_inputs():
    import torch
    rng = np.random.RandomState(3)
    n, T = 12, 9
    steps = rng.uniform(0.4, 1.0, (n, T, 3)).astype(np.float32)
    hist = torch.from_numpy(np.cumsum(steps, axis=1))
    lengths = torch.from_numpy(rng.randint(2, T + 1, n).astype(np.int32))
    flags = torch.from_numpy(rng.choice([1, 2, 4, 8, 128, 9], n).astype(np.int32))
    return hist, lengths, flags


def test_select_tracts_reject_on_host_tensors():
    import torch
    from tracktolearn_amd.parallel import select_tracts
    hist, lengths, flags = _reject_inputs()
    n = hist.shape[0]
    base = select_tracts(hist, lengths, flags, 2.0, 9.0)
    none = select_tracts(hist, lengths, flags, 2.0, 9.0, reject=None)
    for a, b in zip(base, none):
        assert torch.equal(a, b)
    assert 3 < len(base[2]) < n                 # the length filter itself drops some
    reject = torch.zeros(n, dtype=torch.bool)
    reject[base[2][::2]] = True                 # every other accepted row
    reject[[r for r in range(n) if r not in base[2].tolist()][0]] = True    # and a dropped one
    points, counts, rows = select_tracts(hist, lengths, flags, 2.0, 9.0, reject=reject)
    keep = [k for k, r in enumerate(base[2].tolist()) if not reject[r]]
    assert rows.tolist() == [base[2].tolist()[k] for k in keep]
    assert counts.tolist() == [base[1].tolist()[k] for k in keep]
    offs = np.concatenate(([0], np.cumsum(base[1].numpy())))
    want = np.concatenate([base[0].numpy()[offs[k]:offs[k + 1]] for k in keep])
    assert np.array_equal(points.numpy(), want)
    everything = select_tracts(hist, lengths, flags, 2.0, 9.0, reject=torch.ones(n, dtype=torch.bool))
    assert len(everything[0]) == 0 and len(everything[1]) == 0 and len(everything[2]) == 0
    with pytest.raises(ValueError):
        select_tracts(hist, lengths, flags, 2.0, 9.0, reject=torch.zeros(n - 1, dtype=torch.bool))


def test_select_tracts_file_reject_on_host_tensors():
    import torch
    from tracktolearn_amd.io import streamlines as sio
    from tracktolearn_amd.parallel import select_tracts, select_tracts_file
    hist, lengths, flags = _reject_inputs()
    n = hist.shape[0]
    desc = sio.body_desc('.tck', np.eye(4), 1.0, None, 0)
    reject = torch.zeros(n, dtype=torch.bool)
    reject[::3] = True
    words, k, m = select_tracts_file(hist, lengths, flags, 2.0, 9.0, desc, reject=reject)
    points, counts, _ = select_tracts(hist, lengths, flags, 2.0, 9.0, reject=reject)
    assert (k, m) == (len(counts), len(points))
    base = select_tracts_file(hist, lengths, flags, 2.0, 9.0, desc)
    none = select_tracts_file(hist, lengths, flags, 2.0, 9.0, desc, reject=None)
    assert torch.equal(base[0], none[0]) and base[1:] == none[1:] and base[1] > k


# --------------------------------------------------------------- ABI surface
def test_header_declares_the_entry_point(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'ttl_hip.h')).read()
    assert re.search(r'#define TTL_ABI_VERSION 13\b', text)
    body = text[text.index('#define TTL_HAS_ACT 1'):]
    assert re.search(r'TTL_API int ttl_act_flags\(', body)
    for define in ('TTL_FLAG_TARGET  8', 'TTL_FLAG_EXCLUDE 128', 'TTL_ACT_THRESHOLD 0',
                   'TTL_ACT_CMC       1', 'TTL_ACT_STREAM 0x41435420u'):
        assert '#define ' + define in body
    cc = shutil.which('gcc')
    assert cc is not None
    src = tmp_path / 'act.c'
    src.write_text('#include "ttl_hip.h"\n#ifndef TTL_HAS_ACT\n#error no ACT\n#endif\n'
                   'int main(void) { ttl_act_desc d; d.mode = TTL_ACT_CMC; d.dim[2] = 1;\n'
                   'd.coord_shift = 0.0; d.exponent = 1.0; d.seed = TTL_ACT_STREAM; d.ids_base = 0;\n'
                   'd.include = d.exclude = 0;\n'
                   'return ttl_act_flags(&d, 0, 0, 0, 0, 0, 1, 0, 0, 0) + TTL_FLAG_TARGET + '
                   'TTL_FLAG_EXCLUDE + TTL_ACT_THRESHOLD; }\n')
    out = subprocess.run([cc, '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic',
                          '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_library_binding_names_the_entry_point():
    from tracktolearn_amd import _lib
    from tracktolearn_amd.environments import stopping_criteria as sc
    assert len(_lib.SYMBOLS['ttl_act_flags'][1]) == 10
    assert [f[0] for f in _lib.ActDesc._fields_] == [
        'include', 'exclude', 'dim', 'mode', 'coord_shift', 'exponent', 'seed', 'ids_base']
    assert C.sizeof(_lib.ActDesc) == 64
    assert (_lib.FLAG_TARGET, _lib.FLAG_EXCLUDE) == (ref_act.TARGET, ref_act.EXCLUDE) == (8, 128)
    assert (_lib.ACT_THRESHOLD, _lib.ACT_CMC, _lib.ACT_STREAM) == (0, 1, ref_act.ACT_STREAM)
    assert _lib.ABI_VERSION == 13
    assert sc.ACT_EXCLUDE_FLAG == 128 and sc.StoppingFlags.STOPPING_TARGET.value == 8
    assert 128 not in [f.value for f in sc.StoppingFlags]
    assert hasattr(_lib.load(), 'ttl_act_flags')


# ------------------------------------------------------------------ GPU part
POISON = 0xA5


class _Device:
    """A case's arrays on the GPU and the call."""

    def __init__(self, case, pad=0):
        import torch
        from tracktolearn_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.case = case
        dev = torch.device(DEV)
        self.inc = torch.from_numpy(case['include']).to(dev)
        self.exc = torch.from_numpy(case['exclude']).to(dev)
        hist = case['history'].reshape(len(case['history']), -1)
        if pad:     # rows further apart than their points, NaN in between
            hist = np.concatenate([hist, np.full((len(hist), pad), np.nan, np.float32)], axis=1)
        self.hist = torch.from_numpy(np.ascontiguousarray(hist)).to(dev)
        self.pitch = hist.shape[1]
        self.init_len = torch.from_numpy(case['init_len']).to(dev) \
            if case['init_len'] is not None else None
        self.dev = dev

    def desc(self, mode, **over):
        c = self.case
        d = self._lib.ActDesc()
        d.include, d.exclude = self.inc.data_ptr(), self.exc.data_ptr()
        d.dim[:] = list(c['include'].shape)
        d.mode = mode
        d.coord_shift, d.exponent = c['coord_shift'], c['exponent']
        d.seed = c['seed'] & 0xFFFFFFFFFFFFFFFF
        d.ids_base = c['ids_base']
        for k, v in over.items():
            if k == 'dim':
                d.dim[:] = v
            else:
                setattr(d, k, v)
        return d

    def call(self, mode, ids, use_init_len, n, values=True, **over):
        """(return code, flags (n + 8) uint8 host, values (n, 2) float64 host);
        ``over`` replaces arguments of the call by name."""
        torch = self.torch
        ids_dev = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(self.dev) \
            if ids is not None else None
        flags = torch.full((max(n, 0) + 8,), POISON, dtype=torch.uint8, device=self.dev)
        vals = torch.full((max(n, 0), 2), np.nan, dtype=torch.float64, device=self.dev) \
            if values else None
        a = dict(desc=C.byref(self.desc(mode)),
                 history=self.hist.data_ptr(), row_pitch=self.pitch,
                 ids=ids_dev.data_ptr() if ids_dev is not None else None,
                 init_len=self.init_len.data_ptr() if use_init_len else None, n=n,
                 n_points=self.case['n_points'], flags_out=flags.data_ptr(),
                 values_out=vals.data_ptr() if vals is not None else None)
        a.update(over)
        a['n'] = a.pop('rows', a['n'])          # (``n`` sizes the buffers above)
        rc = self.lib.ttl_act_flags(a['desc'], a['history'], a['row_pitch'], a['ids'],
                                    a['init_len'], a['n'], a['n_points'], a['flags_out'],
                                    a['values_out'], None)
        torch.cuda.synchronize()
        return rc, flags.cpu().numpy(), vals.cpu().numpy() if vals is not None else None


@pytest.fixture(scope='module')
def devices():
    return {c['name']: _Device(c) for c in act_cases.cases()}


def _check(dev, mode, n, use_ids, use_init_len):
    case = dev.case
    rows = len(case['history'])
    if use_ids:
        ids = np.resize(case['ids'], n).astype(np.int32)
    else:
        n = min(n, rows)          # row r judges history row r
        ids = None
    rc, flags, vals = dev.call(mode, ids, use_init_len, n)
    assert rc == 0
    assert (flags[n:] == POISON).all()
    if n == 0:
        return
    want = act_cases.flags_of(case, mode, n=n, use_ids=use_ids, use_init_len=use_init_len)
    want_v = ref_act.act_values_ordered(
        case['include'], case['exclude'], case['history'], case['n_points'],
        ids=ids, n=n, coord_shift=case['coord_shift'])
    assert np.array_equal(vals.view(np.uint64), want_v.view(np.uint64)), case['name']
    assert np.array_equal(flags[:n], want), (case['name'], mode, n,
                                             np.nonzero(flags[:n] != want)[0][:8])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', [c['name'] for c in act_cases.cases()])
def test_kernel_equals_the_restatement(devices, name, mode):
    dev = devices[name]
    for n in act_cases.N_SIZES:
        _check(dev, mode, n, use_ids=True, use_init_len=True)
    rows = len(dev.case['history'])
    _check(dev, mode, rows, use_ids=False, use_init_len=True)
    _check(dev, mode, rows, use_ids=True, use_init_len=False)
    _check(dev, mode, rows, use_ids=False, use_init_len=False)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_wider_row_pitch_and_no_values(mode):
    case = act_cases.cases()[1]
    dev = _Device(case, pad=5)
    assert dev.pitch > 3 * case['n_points'] + 3
    n = 257
    ids = np.resize(case['ids'], n).astype(np.int32)
    rc, flags, _ = dev.call(mode, ids, True, n, values=False)
    assert rc == 0
    assert np.array_equal(flags[:n], act_cases.flags_of(case, mode, n=n))
    assert (flags[n:] == POISON).all()


@pytest.mark.gpu
def test_knife_rows_on_the_device(devices):
    for name, dev in devices.items():
        if 'knife_row' not in dev.case:
            continue
        rc, flags, _ = dev.call(ref_act.CMC, dev.case['ids'], False, len(dev.case['ids']))
        assert rc == 0 and flags[dev.case['knife_row']] in (ref_act.TARGET, ref_act.EXCLUDE)


@pytest.mark.gpu
def test_refusals_leave_flags_untouched(devices):
    from tracktolearn_amd import _lib
    dev = devices['g237']
    case = dev.case
    n = 65
    ids = np.resize(case['ids'], n).astype(np.int32)
    T, CMC = ref_act.THRESHOLD, ref_act.CMC
    refusals = [
        ('null desc', T, dict(desc=None)),
        ('null history', T, dict(history=None)),
        ('null flags', T, dict(flags_out=None)),
        ('null include', T, dict(desc=C.byref(dev.desc(T, include=None)))),
        ('null exclude', T, dict(desc=C.byref(dev.desc(T, exclude=None)))),
        ('dim 0', T, dict(desc=C.byref(dev.desc(T, dim=[2, 0, 7])))),
        ('dim negative', T, dict(desc=C.byref(dev.desc(T, dim=[2, 3, -1])))),
        ('mode 2', T, dict(desc=C.byref(dev.desc(2)))),
        ('mode -1', T, dict(desc=C.byref(dev.desc(-1)))),
        ('n negative', T, dict(rows=-1)),
        ('n_points 0', T, dict(n_points=0)),
        ('row_pitch', T, dict(row_pitch=3 * case['n_points'] - 1)),
        ('ids_base', T, dict(desc=C.byref(dev.desc(T, ids_base=-1)))),
        ('exponent 0', CMC, dict(desc=C.byref(dev.desc(CMC, exponent=0.0)))),
        ('exponent negative', CMC, dict(desc=C.byref(dev.desc(CMC, exponent=-1.0)))),
        ('exponent inf', CMC, dict(desc=C.byref(dev.desc(CMC, exponent=float('inf'))))),
        ('exponent nan', CMC, dict(desc=C.byref(dev.desc(CMC, exponent=float('nan'))))),
    ]
    for what, mode, over in refusals:
        rc, flags, _ = dev.call(mode, ids, True, n, **over)
        assert rc == _lib.ERR_INVALID, what
        if over.get('flags_out', 0) is not None:
            assert (flags == POISON).all(), what
        assert b'ttl_act_flags' in dev.lib.ttl_last_error()
    # the exponent is not read in threshold mode
    rc, flags, _ = dev.call(T, ids, True, n, desc=C.byref(dev.desc(T, exponent=float('nan'))))
    assert rc == 0 and np.array_equal(flags[:n], act_cases.flags_of(case, T, n=n))
