"""Streamline-based linear registration: fit an atlas of model lines to the
subject's streamlines by the bundle-minimum distance, on the GPU.

SLR (Garyfallidis 2015; the first step of RecoBundles): the rigid, similarity or
affine transform that minimises the bundle-minimum distance (BMD) between the
subject's streamlines (the fixed set) and the atlas's model lines (the moving
set), both resampled to K stations.  ``ttl_bundle_register_cost`` computes the
cost of up to 64 candidate transforms in one launch (include/ttl_hip.h states
it); one launch on the 2p + 1 matrices of a central difference is one
function-and-gradient evaluation of SciPy's L-BFGS-B.  With it the chain track ->
register -> recognise -> profile works from a standard atlas:

    atlas = BundleAtlas.from_tractogram('t1.nii.gz', 'atlas.trk', labels, names, 20)
    fit = register_atlas(atlas, 'subject.trk', kind='affine')
    fit['matrix']                       # (4, 4) atlas mm -> subject mm
    got = fit['atlas'].recognize('subject.trk', max_mdf=8.0)

There is no NumPy fallback for the cost: like the rest of the product path it
needs the library.  ``register`` takes another ``evaluate`` so that the driver
can be run against a reference.
"""
import numpy as np
import torch

from tracktolearn_amd import _lib

MAX_POINTS = _lib.PROFILE_MAX_POINTS
MAX_LINES = _lib.REGISTER_MAX_LINES
MAX_TRANSFORMS = _lib.REGISTER_MAX_TRANSFORMS
KINDS = ('translation', 'rigid', 'similarity', 'affine')
N_PARAMS = {'translation': 3, 'rigid': 6, 'similarity': 7, 'affine': 12}
#: the identity in the 12 parameters of ``compose``
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0], np.float64)
#: central-difference steps: mm, degrees, scales and shears
STEPS = np.array([0.01] * 3 + [0.01] * 3 + [1e-4] * 3 + [1e-4] * 3, np.float64)
#: box of L-BFGS-B: mm, degrees, scales, shears
BOUNDS = np.array([(-150.0, 150.0)] * 3 + [(-90.0, 90.0)] * 3 + [(0.5, 2.0)] * 3 +
                  [(-0.5, 0.5)] * 3, np.float64)
FTOL, GTOL, MAX_ITER = 1e-9, 1e-6, 200
#: L-BFGS-B works on params / SCALE: one unit of any variable moves a station 50 mm from the
#: centre by about a millimetre (1 mm, 1 degree, 0.02 of scale or shear)
SCALE = np.array([1.0] * 6 + [0.02] * 6, np.float64)


def bundle_register_cost(fixed, moving, xf, lin):
    """``ttl_bundle_register_cost`` on device tensors: ``fixed`` (A, K, 3) and
    ``moving`` (B, K, 3) float32 stations in one grid's corner-origin voxel
    coordinates, ``xf`` (T, 3, 4) float64 transforms in those coordinates,
    ``lin``: the (3, 3) linear part of voxel -> RAS mm.  Returns (row_min (T, A),
    col_min (T, B), cost (T,)), float64."""
    if not (torch.is_tensor(fixed) and fixed.dtype == torch.float32 and fixed.dim() == 3 and
            fixed.shape[2] == 3 and fixed.is_contiguous()):
        raise ValueError('fixed must be a contiguous (A, K, 3) float32 tensor')
    dev = fixed.device
    A, K = int(fixed.shape[0]), int(fixed.shape[1])
    if not (torch.is_tensor(moving) and moving.dtype == torch.float32 and moving.dim() == 3 and
            tuple(moving.shape[1:]) == (K, 3) and moving.is_contiguous() and moving.device == dev):
        raise ValueError(f'moving must be a contiguous (B, {K}, 3) float32 tensor on the device '
                         f'of fixed')
    B = int(moving.shape[0])
    if not (1 <= A <= MAX_LINES and 1 <= B <= MAX_LINES):
        raise ValueError(f'fixed and moving must have 1 .. {MAX_LINES} lines, not {A} and {B}')
    if not 2 <= K <= MAX_POINTS:
        raise ValueError(f'lines must have 2 .. {MAX_POINTS} stations, not {K}')
    if not (torch.is_tensor(xf) and xf.dtype == torch.float64 and xf.dim() == 3 and
            tuple(xf.shape[1:]) == (3, 4) and xf.is_contiguous() and xf.device == dev):
        raise ValueError('xf must be a contiguous (T, 3, 4) float64 tensor on the device of fixed')
    T = int(xf.shape[0])
    if not 1 <= T <= MAX_TRANSFORMS:
        raise ValueError(f'xf must have 1 .. {MAX_TRANSFORMS} transforms, not {T}')
    lin_c = _lib.lin9(lin)
    row_min = torch.empty((T, A), dtype=torch.float64, device=dev)
    col_min = torch.empty((T, B), dtype=torch.float64, device=dev)
    cost = torch.empty(T, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ttl_bundle_register_cost(
            fixed.data_ptr(), A, moving.data_ptr(), B, K, xf.data_ptr(), T, lin_c,
            row_min.data_ptr(), col_min.data_ptr(), cost.data_ptr(), _lib.stream_of(dev)),
            'ttl_bundle_register_cost')
    return row_min, col_min, cost


# -- transforms -------------------------------------------------------------
def _full(params, kind):
    """The 12 parameters of ``compose`` from the ``N_PARAMS[kind]`` of a kind."""
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {KINDS}, not {kind!r}')
    p = np.asarray(params, np.float64).reshape(-1)
    if p.shape[0] != N_PARAMS[kind]:
        raise ValueError(f'{kind} takes ({N_PARAMS[kind]},) parameters, not {p.shape}')
    full = IDENTITY.copy()
    if kind == 'similarity':
        full[:6], full[6:9] = p[:6], p[6]
    else:
        full[:p.shape[0]] = p
    return full


def _own(full, kind):
    """The parameters of ``kind`` from the 12 (a similarity takes the mean scale)."""
    if kind == 'similarity':
        return np.concatenate([full[:6], [full[6:9].mean()]])
    return full[:N_PARAMS[kind]].copy()


def compose(params, kind, centre):
    """The (4, 4) float64 RAS-mm matrix of ``params`` = (tx, ty, tz [mm], rx, ry,
    rz [degrees], sx, sy, sz, hxy, hxz, hyz), of which ``kind`` takes the first 3
    ('translation'), 6 ('rigid'), 6 and one isotropic scale ('similarity') or all
    12 ('affine'): x' = A (x - c) + c + t with A = Rz Ry Rx H diag(s), H upper
    unit-triangular with (hxy, hxz, hyz), c = ``centre`` (3,) in mm."""
    p = _full(params, kind)
    c = np.asarray(centre, np.float64).reshape(3)
    rx, ry, rz = np.deg2rad(p[3:6])
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    H = np.array([[1, p[9], p[10]], [0, 1, p[11]], [0, 0, 1]])
    A = Rz @ Ry @ Rx @ H @ np.diag(p[6:9])
    out = np.eye(4)
    out[:3, :3] = A
    out[:3, 3] = c + p[:3] - A @ c
    return out


def _corner(affine):
    """corner-origin voxel -> RAS mm of a grid whose ``affine`` maps voxel centres."""
    s = np.asarray(affine, np.float64).reshape(4, 4).copy()
    s[:3, 3] -= 0.5 * s[:3, :3].sum(1)
    return s


def to_voxel(matrix, affine):
    """The (3, 4) float64 form ``ttl_bundle_register_cost`` takes of a (4, 4)
    RAS-mm ``matrix``: the same map in the corner-origin voxel coordinates of the
    grid whose voxel -> RAS mm is ``affine``."""
    s = _corner(affine)
    return np.ascontiguousarray((np.linalg.inv(s) @ np.asarray(matrix, np.float64) @ s)[:3])


def from_voxel(matrix_vox, affine):
    """The (4, 4) RAS-mm matrix of a (3, 4) ``to_voxel`` form."""
    s = _corner(affine)
    v = np.eye(4)
    v[:3] = np.asarray(matrix_vox, np.float64).reshape(3, 4)
    return s @ v @ np.linalg.inv(s)


def to_mm(vox, affine):
    """Corner-origin voxel coordinates (.., 3) in RAS mm, float64."""
    s = _corner(affine)
    return np.asarray(vox, np.float64) @ s[:3, :3].T + s[:3, 3]


def gpu_evaluate(fixed_vox, moving_vox, lin, device='cuda'):
    """``evaluate(mats (T, 3, 4)) -> costs (T,)`` by the launch, the two sets
    uploaded once."""
    dev = torch.device(device)
    fixed = torch.from_numpy(np.ascontiguousarray(fixed_vox, np.float32)).to(dev)
    moving = torch.from_numpy(np.ascontiguousarray(moving_vox, np.float32)).to(dev)

    def evaluate(mats):
        xf = torch.from_numpy(np.ascontiguousarray(mats, np.float64)).to(dev)
        return bundle_register_cost(fixed, moving, xf, lin)[2].cpu().numpy()
    return evaluate


# -- the driver --------------------------------------------------------------
def register(fixed_vox, moving_vox, affine, kind='affine', progressive=True, x0=None, bounds=None,
             steps=None, max_iter=MAX_ITER, evaluate=None, centre=None, device='cuda'):
    """Fit ``moving_vox`` (B, K, 3) to ``fixed_vox`` (A, K, 3), both corner-origin
    voxel coordinates of the grid of ``affine`` (4, 4), by L-BFGS-B on the BMD.
    ``kind``: 'rigid', 'similarity', 'affine' (or 'translation'); ``progressive``:
    translation -> rigid -> similarity -> affine up to ``kind``, each stage from
    the one before.  ``x0``: the (12,) parameters of ``compose`` to start from
    (the identity); ``bounds`` (12, 2) and ``steps`` (12,) per parameter (BOUNDS,
    STEPS); ``max_iter`` per stage.  ``evaluate(mats (T, 3, 4)) -> costs (T,)``:
    the cost of voxel-space transforms (``gpu_evaluate``); every function-and-
    gradient evaluation is one call on the 2p + 1 matrices of a central
    difference, the point first.  ``centre``: (3,) mm (the float64 mean of the
    moving stations that are finite).  Returns a dict: ``matrix`` (4, 4) moving
    mm -> fixed mm, ``params`` (of ``kind``), ``params12``, ``kind``, ``centre``,
    ``cost_before`` (at ``x0``), ``cost_after``, ``evaluations`` (calls of
    ``evaluate``) and ``stages``."""
    from scipy.optimize import minimize
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {KINDS}, not {kind!r}')
    fixed_vox, moving_vox = np.asarray(fixed_vox), np.asarray(moving_vox)
    if fixed_vox.ndim != 3 or moving_vox.ndim != 3 or fixed_vox.shape[2] != 3 or \
            moving_vox.shape[1:] != fixed_vox.shape[1:]:
        raise ValueError(f'fixed_vox and moving_vox must be (A, K, 3) and (B, K, 3), not '
                         f'{fixed_vox.shape} and {moving_vox.shape}')
    affine = np.asarray(affine, np.float64).reshape(4, 4)
    full = IDENTITY.copy() if x0 is None else np.asarray(x0, np.float64).reshape(-1).copy()
    bounds = BOUNDS if bounds is None else np.asarray(bounds, np.float64)
    steps = STEPS if steps is None else np.asarray(steps, np.float64).reshape(-1)
    if full.shape != (12,) or bounds.shape != (12, 2) or steps.shape != (12,):
        raise ValueError('x0 and steps must be (12,) and bounds (12, 2)')
    if centre is None:
        mm = to_mm(moving_vox, affine).reshape(-1, 3)
        mm = mm[np.isfinite(mm).all(1)]
        if not len(mm):
            raise ValueError('moving_vox has no finite station')
        centre = mm.mean(0)
    centre = np.asarray(centre, np.float64).reshape(3)
    if evaluate is None:
        evaluate = gpu_evaluate(fixed_vox, moving_vox, affine[:3, :3], device)
    calls = [0]

    def costs(kind_now, points):
        calls[0] += 1
        mats = np.stack([to_voxel(compose(p, kind_now, centre), affine) for p in points])
        return np.asarray(evaluate(mats), np.float64).reshape(len(points))

    def stage_index(kind_now):              # which of the 12 a stage's parameter is
        return list(range(6)) + [6] if kind_now == 'similarity' else \
            list(range(N_PARAMS[kind_now]))

    cost_before = float(costs('affine', [full])[0])
    chain = KINDS[:KINDS.index(kind) + 1] if progressive else (kind,)
    stages, cost_after = [], cost_before
    for kind_now in chain:
        idx = stage_index(kind_now)
        h, unit = steps[idx], SCALE[idx]

        def fun(q, kind_now=kind_now, h=h, unit=unit):
            p = q * unit
            pts = [p] + [p + s * e for e in np.diag(h) for s in (1.0, -1.0)]
            c = costs(kind_now, pts)
            return c[0], (c[1::2] - c[2::2]) / (2.0 * h) * unit
        if kind_now != 'affine':            # what this stage does not move stays the identity's
            full = _full(_own(full, kind_now), kind_now)
        res = minimize(fun, _own(full, kind_now) / unit, jac=True, method='L-BFGS-B',
                       bounds=[tuple(b / u) for b, u in zip(bounds[idx], unit)],
                       options={'maxiter': int(max_iter), 'ftol': FTOL, 'gtol': GTOL})
        full = _full(res.x * unit, kind_now)
        cost_after = float(res.fun)
        stages.append({'kind': kind_now, 'cost': cost_after, 'iterations': int(res.nit)})
    return {'matrix': compose(_own(full, kind), kind, centre), 'params': _own(full, kind),
            'params12': full, 'kind': kind, 'centre': centre, 'cost_before': cost_before,
            'cost_after': cost_after, 'evaluations': calls[0], 'stages': stages}


def fixed_stations(file_or_tractogram, affine, nb_points, max_fixed=4096, env=None,
                   in_rasmm=False, device='cuda'):
    """The fixed set of ``register_atlas``: the streamlines through the
    validators' one intake, those that take part (2 .. 4096 points, all finite), an
    evenly strided subsample of at most ``max_fixed`` of them, resampled to
    ``nb_points`` stations by the library's resampler.  (n, nb_points, 3) float32,
    corner-origin voxel coordinates."""
    from tracktolearn_amd.bundle_recognize import MODEL_MAX_POINTS
    from tracktolearn_amd.experiment.oracle_validator import (FILENAME, corner_voxels,
                                                              load_tractogram)
    from tracktolearn_amd.oracles.oracle import resample_streamlines
    if int(max_fixed) < 1:
        raise ValueError(f'max_fixed must be 1 or more, not {max_fixed}')
    source = file_or_tractogram
    if isinstance(source, FILENAME):
        source, in_rasmm = load_tractogram(source)[0], True
    points, offsets, _ = corner_voxels(source, affine, getattr(env, 'affine_vox2rasmm', None),
                                       in_rasmm=in_rasmm)
    lens = np.diff(offsets)
    bad = np.add.reduceat(~np.isfinite(points).all(1), offsets[:-1]) if len(lens) else lens
    rows = np.flatnonzero((lens >= 2) & (lens <= MODEL_MAX_POINTS) & (bad == 0))
    if not len(rows):
        raise ValueError('no streamline of 2 .. 4096 finite points to register to')
    rows = rows[::-(-len(rows) // int(max_fixed))]
    dev = torch.device(device)
    pad = np.zeros((len(rows), int(lens[rows].max()), 3), np.float32)
    for i, s in enumerate(rows.tolist()):
        pad[i, :lens[s]] = points[offsets[s]:offsets[s + 1]]
    out = resample_streamlines(torch.from_numpy(pad).to(dev),
                               torch.from_numpy(lens[rows]).to(dev), int(nb_points))
    return out.cpu().numpy()


def register_atlas(atlas, file_or_tractogram, env=None, in_rasmm=False, kind='affine',
                   progressive=True, max_fixed=4096, **options):
    """Fit ``atlas`` (a BundleAtlas) to a .trk / .tck file or the tracker's
    in-memory tractogram: ``register`` with ``fixed_stations`` of the subject as the
    fixed set and ``atlas.models_vox`` (the models with every station finite) as the
    moving set.  Returns ``register``'s dict with ``atlas``, the moved atlas
    (``atlas.transformed(matrix)``), and ``n_fixed`` / ``n_moving``."""
    fixed = fixed_stations(file_or_tractogram, atlas.affine, atlas.K, max_fixed, env, in_rasmm,
                           atlas.device)
    moving = atlas.models_vox[np.isfinite(atlas.models_vox).all((1, 2))]
    if not len(moving):
        raise ValueError('the atlas has no model line with every station finite')
    fit = register(fixed, moving, atlas.affine, kind=kind, progressive=progressive,
                   device=atlas.device, **options)
    return dict(fit, atlas=atlas.transformed(fit['matrix']), n_fixed=len(fixed),
                n_moving=len(moving))


__all__ = ['bundle_register_cost', 'compose', 'to_voxel', 'from_voxel', 'to_mm', 'gpu_evaluate',
           'register', 'fixed_stations', 'register_atlas', 'KINDS', 'N_PARAMS', 'IDENTITY',
           'STEPS', 'BOUNDS', 'MAX_POINTS', 'MAX_LINES', 'MAX_TRANSFORMS']
