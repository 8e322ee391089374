"""The fODF policy kernel pinned twice (definition at
``ttl_odf_actions`` in include/ttl_hip.h).

``ref_odf_policy.actions_ordered`` restates ``k_odf`` in NumPy float32,
operation for operation in the kernel's order; the library is built without
contraction or fast-math, so both entry points must equal it bit for bit on
every row (GPU tests).  ``ref_odf_policy.actions_float64`` is the definition in
float64 with a per-row ``decided`` flag; where it is decisive the restatement
must choose its vertex and sign (CPU tests).  Hand-built dyadic cases, in which
nothing rounds, pin both to literal vertices, and planted mutations of the
definition show that the inputs the GPU part launches would catch a kernel
carrying any of them.

Undecided shares of the float64 definition on the random inputs (4 000 rows,
hemisphere(3), rel 0.1; printed by the test): det 0.05 - 0.35 %, prob
0.2 - 2.0 % (the cdf edges add to the vertex tests), cap 5 %."""
import ctypes as C

import numpy as np
import pytest

import odf_cases as oc
import ref_odf_policy as ref

F32 = np.float32


def _key_id(k):
    return f'order{k[0]}-theta{int(k[1])}-{"prob" if k[2] else "det"}'


@pytest.fixture(scope='module')
def ordered_cache():
    """actions_ordered of a case, computed once and shared (never written)."""
    cache = {}

    def get(name, c):
        if name not in cache:
            act, vert = ref.actions_ordered(**oc.reference_args(c))
            act.flags.writeable = vert.flags.writeable = False
            cache[name] = (act, vert)
        return cache[name]
    return get


# ------------------------------------------------------------------ CPU part
@pytest.mark.parametrize('key', oc.RANDOM_KEYS, ids=_key_id)
def test_restatement_takes_the_definitions_vertex_where_it_is_decisive(key, ordered_cache):
    c = oc.random_case(*key)
    act32, v32 = ordered_cache(('random',) + key, c)
    act64, v64, decided = ref.actions_float64(**oc.reference_args(c))
    share = 1.0 - decided.mean()
    print(f'{_key_id(key)}: undecided {100 * share:.2f} %, fallback rows '
          f'{int((v64 < 0).sum())}, differing on undecided rows {int((v32 != v64).sum())}')
    assert share <= 0.05                    # a condition on the input, as for the peaks
    assert np.array_equal(v32[decided], v64[decided])
    # +-d_v and p are float32 values: the same sign gives the same action exactly
    assert np.array_equal(act32[decided].astype(np.float64), act64[decided])
    assert (v64 >= 0).mean() > 0.5          # the input exercises the choice, not the fallback


@pytest.mark.parametrize('name', sorted(oc.hand_cases()))
def test_hand_built_cases_give_their_literal_vertices(name):
    c = oc.hand_cases()[name]
    vertex, action = c['expect']
    for fn in (ref.actions_ordered, ref.actions_float64):
        out = fn(**oc.reference_args(c))
        assert out[1].tolist() == [vertex], fn.__name__
        assert np.array_equal(out[0][0], np.asarray(action, out[0].dtype)), fn.__name__


@pytest.mark.parametrize('u,vertex', oc.PROB_U)
def test_prob_pick_at_the_cdf_edges(u, vertex):
    c = oc.prob_hand_case()
    for fn in (ref.actions_ordered, ref.actions_float64):
        out = fn(**oc.reference_args(c, u=F32(u)))
        assert out[1].tolist() == [vertex], fn.__name__
        assert np.array_equal(out[0][0], oc.HAND_DIRS[vertex].astype(out[0].dtype))


def test_uniforms_are_keyed_by_seed_id_and_step():
    ids = np.array([0, 1, 2, (1 << 33) + 1, 1], np.int64)
    u = ref.uniforms(9, ids, 4)
    assert u.dtype == F32 and (u >= 0).all() and (u < 1).all()
    assert u[1] == u[4] and len(set(u[:4].tolist())) == 4
    assert not np.array_equal(u, ref.uniforms(10, ids, 4))
    assert not np.array_equal(u, ref.uniforms(9, ids, 5))
    # not the keyed noise's draw: that one has 0 / 1 in counter word 3
    import ref_noise
    ctr = np.stack([ids & 0xFFFFFFFF, ids >> 32, np.full_like(ids, 4), np.zeros_like(ids)], -1)
    noise_w0 = ref_noise.philox(ctr, np.array([9, 0], np.uint64))[:, 0]
    assert not np.array_equal((noise_w0 >> 8).astype(F32) * F32(2.0 ** -24), u)
    big = ref.uniforms(3, np.arange(200000), 0).astype(np.float64)
    assert abs(big.mean() - 0.5) < 0.005 and abs(big.var() - 1 / 12) < 0.002


def test_edge_ids_draw_a_uniform_on_a_cdf_edge():
    c = oc.uniform_weights_case()
    u = ref.uniforms(c['seed'], c['ids_base'] + c['idx'].astype(np.int64), c['step'])
    k = u[:len(oc.EDGE_IDS)].astype(np.float64) * 64
    assert (k == np.round(k)).all() and (k >= 1).all()
    vert = ref.actions_ordered(**oc.reference_args(c))[1]
    assert vert[:len(oc.EDGE_IDS)].tolist() == k.astype(int).tolist()   # first cdf > k: vertex k


def _gpu_inputs():
    """name -> case of everything the GPU part launches on the explicit entry."""
    cases = {('hand', k): v for k, v in oc.hand_cases().items()}
    cases[('uniform',)] = oc.uniform_weights_case()
    cases[('cone_prob',)] = oc.cone_prob_case()
    for key in oc.RANDOM_KEYS:
        cases[('random',) + key] = oc.random_case(*key)
    return cases


@pytest.mark.parametrize('mutation', ref.MUTATIONS)
def test_every_planted_mutation_changes_an_output_the_gpu_part_checks(mutation, ordered_cache):
    caught = []
    for name, c in _gpu_inputs().items():
        if name[0] == 'random' and (name[1] != 6 or caught):
            continue                        # the small inputs first; one random order suffices
        act, vert = ordered_cache(name, c)
        m_act, m_vert = ref.actions_ordered(**oc.reference_args(c, mutate=mutation))
        if not (np.array_equal(vert, m_vert) and np.array_equal(act, m_act, equal_nan=True)):
            caught.append(name)
    print(mutation, 'caught by', caught)
    assert caught


# ------------------------------------------------------------------ GPU part
DEV = 'cuda:0'


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _launch(lib, c, vertex=True, poison=None):
    """ttl_odf_actions on a case: (actions, vertex) as host arrays."""
    import torch
    state, dir_offset = oc.state_rows(c)
    n, n_coef = c['sh'].shape
    dev = torch.device(DEV)
    st = torch.from_numpy(state).to(dev) if n else torch.zeros((1, state.shape[1]), device=dev)
    Bm, dirs = torch.from_numpy(c['B']).to(dev), torch.from_numpy(c['dirs']).to(dev)
    idx = torch.from_numpy(c['idx']).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    act = torch.full((max(n, 1), 3), 7.0, dtype=torch.float32, device=dev)
    vert = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    rc = lib.ttl_odf_actions(
        st.data_ptr(), state.shape[1], n_coef, dir_offset, Bm.data_ptr(), dirs.data_ptr(),
        c['dirs'].shape[0], c['cos_theta'], c['rel'], c['mode'], c['seed'], c['ids_base'],
        idx.data_ptr(), n, c['step'], act.data_ptr(), vert.data_ptr() if vertex else None,
        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.ttl_last_error()
    torch.cuda.synchronize()
    return act.cpu().numpy(), vert.cpu().numpy()


def _assert_bits(c, got, want):
    n = len(c['sh'])
    act, vert = got
    assert np.array_equal(vert[:n], want[1])
    assert np.array_equal(_bits(act[:n]), _bits(want[0]))
    assert (act[n:] == 7.0).all() and (vert[n:] == -7).all()      # nothing past the rows


@pytest.fixture(scope='module')
def lib():
    from tracktolearn_amd import _lib
    return _lib.load()


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(_gpu_inputs()), ids=lambda n: _key_id(n[1:])
                         if n[0] == 'random' else '-'.join(n))
def test_kernel_equals_the_restatement_bit_for_bit(name, lib, ordered_cache):
    c = _gpu_inputs()[name]
    _assert_bits(c, _launch(lib, c), ordered_cache(name, c))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [oc.DET, oc.PROB], ids=['det', 'prob'])
@pytest.mark.parametrize('shape', oc.SHAPES, ids=lambda s: 'C%d-V%d-n%d' % s)
def test_kernel_at_the_edge_shapes(shape, mode, lib):
    """Every C path (register kernels 6 / 15 / 28 / 45, the generic one), V
    around the vertex blocking, n around the wave, a wide pitch, step-0 rows
    mixed in, a permuted continue_idx over an id base above 2^32."""
    c = oc.shape_case(*shape, mode)
    want = ref.actions_ordered(**oc.reference_args(c))
    _assert_bits(c, _launch(lib, c), want)
    if shape[2]:
        assert (want[1] >= 0).any() or shape[1] < 3


@pytest.mark.gpu
def test_vertex_out_may_be_null(lib):
    c = oc.shape_case(28, 65, 64, oc.DET)
    act, vert = _launch(lib, c, vertex=False)
    assert np.array_equal(_bits(act), _bits(ref.actions_ordered(**oc.reference_args(c))[0]))
    assert (vert == -7).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [oc.DET, oc.PROB], ids=['det', 'prob'])
def test_a_wave_takes_further_row_blocks_over_the_same_lds(mode, lib):
    """More row blocks than the capped grid has waves (4 * cap + 3): some waves
    run their loop twice over the tile they reuse.  Rows repeat with period 7
    (the ids do not)."""
    from tracktolearn_amd import _lib
    n = (4 * _lib.ODF_GRID_CAP + 3) * 64
    base = oc.shape_case(6, 33, 7, mode)
    rep = np.arange(n) % 7
    c = oc.case(base['sh'][rep], base['p'][rep], base['B'], base['dirs'], base['cos_theta'],
                base['rel'], mode, seed=11, ids_base=3, step=9)
    want = ref.actions_ordered(**oc.reference_args(c))
    _assert_bits(c, _launch(lib, c), want)
    if mode == oc.PROB:
        assert len(np.unique(want[1][rep == 1])) > 1       # the picks follow the ids


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [oc.DET, oc.PROB], ids=['det', 'prob'])
def test_the_pick_follows_the_id_not_the_row(mode, lib):
    """The same rows under another row order and another split of id base
    and continue_idx: the same action per streamline id."""
    c = oc.shape_case(28, 65, 1000, mode)
    act, vert = _launch(lib, c)
    perm = np.random.RandomState(4).permutation(1000)
    c2 = oc.case(c['sh'][perm], c['p'][perm], c['B'], c['dirs'], c['cos_theta'], c['rel'], mode,
                 seed=c['seed'], ids_base=c['ids_base'] - 5, idx=c['idx'][perm] + 5,
                 step=c['step'], pitch=c['pitch'])
    act2, vert2 = _launch(lib, c2)
    assert np.array_equal(vert2, vert[perm]) and np.array_equal(_bits(act2), _bits(act[perm]))


def _small_env(n):
    import torch
    from tracktolearn_amd.environments import TrackingEnvironment
    from tracktolearn_amd.utils.synthetic import synthetic_seeds, synthetic_subject
    subject = synthetic_subject(12, 28, seed=5, peaks=False)
    dto = dict(n_dirs=2, theta=60.0, npv=1, binary_stopping_threshold=0.1, step_size=0.75,
               min_length=2.0, max_length=30.0, compute_reward=False, alignment_weighting=0.0,
               oracle_bonus=0.0, rng=np.random.RandomState(0), device=torch.device(DEV),
               target_sh_order=6)
    env = TrackingEnvironment(subject, 'testing', dto)
    env.seeds = synthetic_seeds(subject[1].data, n, seed=2)
    return env


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [oc.DET, oc.PROB], ids=['det', 'prob'])
def test_free_running_entry_point_reads_the_device_words(mode, lib):
    """ttl_env_freerun_odf_actions after a few ordinary steps (length > 1, a
    continue_idx that is no identity any more): row count, step and ids come
    from the device words; the rows past n_rows stay untouched."""
    import torch
    from tracktolearn_amd import _lib
    n_total = 1500
    env = _small_env(n_total)
    state = env.reset(200, 200 + n_total)
    assert env.streamline_id_base() == 200
    for step in range(6):
        env.step_device(env.scripted_actions(state, step, 3, 0.6))
        state, _ = env.harvest()
    n = env._n_active
    idx = env._idx_view(n).cpu().numpy()
    assert 64 < n < n_total and not np.array_equal(idx, np.arange(n))
    tables = {6: oc.tables(6), 'cut': oc.tables(6, 65)}
    dev = torch.device(DEV)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # the env's own state rows for all active rows, then arbitrary rows of the
    # shape tests for fewer
    rows_cases = [(state.cpu().numpy(), tables[6], n), (None, tables['cut'], n - 37)]
    _lib.check(lib.ttl_env_freerun_begin(env._handle, env._host_counts.data_ptr(), stream),
               'ttl_env_freerun_begin')
    try:
        for host_state, (Bm, dirs), n_rows in rows_cases:
            k = min(n, n_rows)
            if host_state is None:
                c0 = oc.shape_case(28, 65, k, mode)
                host_state = np.zeros((k, state.shape[1]), F32)
                host_state[:, :28] = c0['sh']
                host_state[:, 7 * 28:7 * 28 + 3] = c0['p']
            st = torch.zeros((n_total, state.shape[1]), dtype=torch.float32, device=dev)
            st[:len(host_state)] = torch.from_numpy(host_state).to(dev)
            act = torch.full((n_total, 3), 7.0, dtype=torch.float32, device=dev)
            vert = torch.full((n_total,), -7, dtype=torch.int32, device=dev)
            tB, tD = torch.from_numpy(Bm).to(dev), torch.from_numpy(dirs).to(dev)
            _lib.check(lib.ttl_env_freerun_odf_actions(
                env._handle, st.data_ptr(), st.stride(0), 28, 7 * 28, tB.data_ptr(),
                tD.data_ptr(), dirs.shape[0], oc.cos_deg(45.0), 0.1, mode, 99, 200, n_rows,
                act.data_ptr(), vert.data_ptr(), stream), 'ttl_env_freerun_odf_actions')
            torch.cuda.synchronize()
            hs = st[:k].cpu().numpy()
            c = oc.case(hs[:, :28], hs[:, 7 * 28:7 * 28 + 3], Bm, dirs, oc.cos_deg(45.0), 0.1,
                        mode, seed=99, ids_base=200, idx=idx[:k], step=env.length - 1)
            want = ref.actions_ordered(**oc.reference_args(c))
            got_a, got_v = act.cpu().numpy(), vert.cpu().numpy()
            assert np.array_equal(got_v[:k], want[1])
            assert np.array_equal(_bits(got_a[:k]), _bits(want[0]))
            assert (got_a[k:] == 7.0).all() and (got_v[k:] == -7).all()
            assert (want[1] >= 0).mean() > 0.5
    finally:
        out = [C.c_int32() for _ in range(3)]
        _lib.check(lib.ttl_env_freerun_end(env._handle, *(C.byref(o) for o in out), stream),
                   'ttl_env_freerun_end')
    assert out[0].value == n and out[1].value == env.length


@pytest.mark.gpu
def test_refusals_leave_the_output_untouched(lib):
    import torch
    from tracktolearn_amd import _lib
    c = oc.shape_case(28, 65, 64, oc.DET)
    state, dir_offset = oc.state_rows(c)
    dev = torch.device(DEV)
    st, Bm, dirs, idx = (torch.from_numpy(a).to(dev) for a in (state, c['B'], c['dirs'], c['idx']))
    act = torch.full((64, 3), 7.0, dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    good = dict(state=st.data_ptr(), pitch=state.shape[1], n_coef=28, dir_offset=dir_offset,
                B=Bm.data_ptr(), dirs=dirs.data_ptr(), V=65, cos=0.7, rel=0.1, mode=oc.DET,
                seed=1, ids_base=0, idx=idx.data_ptr(), n=64, step=1, act=act.data_ptr(),
                vert=None, stream=stream)
    bad = [dict(n_coef=0), dict(n_coef=_lib.ODF_MAX_COEF + 1, pitch=4096), dict(V=0), dict(V=-3),
           dict(mode=2), dict(mode=-1), dict(state=None), dict(B=None), dict(dirs=None),
           dict(idx=None), dict(act=None), dict(n=-1), dict(pitch=27), dict(pitch=dir_offset + 2),
           dict(dir_offset=-1), dict(ids_base=-1)]
    for change in bad:
        rc = lib.ttl_odf_actions(*{**good, **change}.values())
        assert rc == _lib.ERR_INVALID, change
        assert b'ttl_odf_actions' in lib.ttl_last_error()
    env = _small_env(64)
    env.reset(0, 64)
    fr = dict(env=env._handle, state=st.data_ptr(), pitch=state.shape[1], n_coef=28,
              dir_offset=dir_offset, B=Bm.data_ptr(), dirs=dirs.data_ptr(), V=65, cos=0.7,
              rel=0.1, mode=oc.DET, seed=1, ids_base=0, n_rows=64, act=act.data_ptr(), vert=None,
              stream=stream)
    # not free-running: a call-order error; the argument errors come first
    assert lib.ttl_env_freerun_odf_actions(*fr.values()) == _lib.ERR_STATE
    for change in (dict(env=None), dict(n_coef=0), dict(V=0), dict(mode=5), dict(B=None),
                   dict(act=None), dict(n_rows=0)):
        assert lib.ttl_env_freerun_odf_actions(*{**fr, **change}.values()) == _lib.ERR_INVALID, change
    assert lib.ttl_odf_actions(*{**good, 'n': 0}.values()) == 0      # nothing to do is no error
    torch.cuda.synchronize()
    assert (act.cpu().numpy() == 7.0).all()
