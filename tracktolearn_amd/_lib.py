"""ctypes binding of libttl_hip.so (C ABI: include/ttl_hip.h).

There is no CPU fallback: if the shared library is missing or does not load,
``load()`` raises.  Build it with ``python -m tracktolearn_amd.csrc.build``
(or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

import numpy as np

# PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME
# libamdhip64.so.7).  It must be in the process BEFORE libttl_hip.so is
# dlopen-ed so that the dynamic loader binds our NEEDED libamdhip64.so.7 to
# that same copy; loaded the other way round, /opt/rocm's runtime comes in
# first, torch then loads its own as a second runtime, and our kernels run on
# a runtime that has no device ("no ROCm-capable device is detected").
import torch  # noqa: F401  (keep above the CDLL below)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, 'libttl_hip.so')

ABI_VERSION = 13
SH_LINEAR, SH_BRICK4 = 0, 1
MODE_F32 = 0
MODE_F64DIR = 1
MODE_F32NORM = 2
ORDER_ACTIVE = 0
ORDER_PARTITION = 1
ORDER_BY_POSITION = C.c_void_p(1)      # TTL_ORDER_BY_POSITION (ttl_env_reset)
TRACT_FILE_TRK, TRACT_FILE_TCK = 0, 1
TRACTOMETER_LIMITS = 16               # TTL_TRACTOMETER_LIMITS
TRACTOMETER_MAX_ROIS = 128            # TTL_TRACTOMETER_MAX_ROIS
ERR_INVALID, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -3, -4
ODF_DET, ODF_PROB = 0, 1                # TTL_ODF_DET / TTL_ODF_PROB
ODF_MAX_COEF, ODF_GRID_CAP = 64, 1024   # TTL_ODF_MAX_COEF / TTL_ODF_GRID_CAP
FLAG_TARGET, FLAG_EXCLUDE = 8, 128      # TTL_FLAG_TARGET / TTL_FLAG_EXCLUDE
ACT_THRESHOLD, ACT_CMC = 0, 1           # TTL_ACT_THRESHOLD / TTL_ACT_CMC
ACT_STREAM = 0x41435420                 # TTL_ACT_STREAM
HAS_ACT_IN_STEP = 1                     # TTL_HAS_ACT_IN_STEP (ttl_env_set_act)
HAS_CONNECTOME = 1                      # TTL_HAS_CONNECTOME (ttl_connectome_assign / _accumulate)
CONNECTOME_MAX_NODES, CONNECTOME_MAX_REACH = 4096, 8    # TTL_CONNECTOME_MAX_NODES / _MAX_REACH
CONNECTOME_LENGTH_SCALE = 1048576.0     # TTL_CONNECTOME_LENGTH_SCALE: 2^20 units per mm
HAS_TRACT_SAMPLE = 1                    # TTL_HAS_TRACT_SAMPLE (ttl_tract_sample_mean)
HAS_CONNECTOME_METRIC = 1               # TTL_HAS_CONNECTOME_METRIC (.._accumulate_metric)
HAS_TRACT_DENSITY = 1                   # TTL_HAS_TRACT_DENSITY (ttl_tract_density)
DENSITY_MAX_WAVE_SLOTS = 8192           # TTL_DENSITY_MAX_WAVE_SLOTS
DENSITY_WAVE_SLOTS = 2048               # what wave_slots = 0 means
HAS_BUNDLE_PROFILE = 1                  # TTL_HAS_BUNDLE_PROFILE (ttl_bundle_orient / _profile)
PROFILE_MAX_POINTS, PROFILE_MAX_BUNDLES = 256, 64   # TTL_PROFILE_MAX_POINTS / _MAX_BUNDLES
HAS_BUNDLE_RECOGNIZE = 1                # TTL_HAS_BUNDLE_RECOGNIZE (ttl_bundle_recognize)
RECOGNIZE_MAX_MODELS = 4096             # TTL_RECOGNIZE_MAX_MODELS
HAS_BUNDLE_REGISTER = 1                 # TTL_HAS_BUNDLE_REGISTER (ttl_bundle_register_cost)
REGISTER_MAX_TRANSFORMS, REGISTER_MAX_LINES = 64, 1048576   # TTL_REGISTER_MAX_TRANSFORMS / _LINES


class TTLError(RuntimeError):
    pass


class EnvDesc(C.Structure):
    """struct ttl_env_desc (include/ttl_hip.h) -- field order is the ABI."""
    _fields_ = [
        ('abi_version', C.c_uint32),
        ('mode', C.c_int32),
        ('sh_dim', C.c_int32 * 3),
        ('n_coef', C.c_int32),
        ('coef_pitch', C.c_int32),
        ('sh_packed', C.c_void_p),
        ('sh_coord_shift', C.c_float),
        ('sh_layout', C.c_int32),
        ('mask_dim', C.c_int32 * 3),
        ('mask_coef', C.c_void_p),
        ('mask_threshold', C.c_double),
        ('mask_classes', C.c_void_p),
        ('peaks_dim', C.c_int32 * 3),
        ('peaks', C.c_void_p),
        ('compute_reward', C.c_int32),
        ('alignment_weighting', C.c_double),
        ('n_dirs', C.c_int32),
        ('max_nb_steps', C.c_int32),
        ('step_size_vox', C.c_double),
        ('neigh_radius_vox', C.c_float),
        ('curvature_enabled', C.c_int32),
        ('curv_dot_max', C.c_float),
        ('n_max', C.c_int32),
        ('streamlines', C.c_void_p),
        ('flags', C.c_void_p),
        ('lengths', C.c_void_p),
        ('dones', C.c_void_p),
        ('idx_a', C.c_void_p),
        ('idx_b', C.c_void_p),
        ('workspace', C.c_void_p),
        ('workspace_bytes', C.c_size_t),
    ]


class NoiseDesc(C.Structure):
    """struct ttl_noise_desc (include/ttl_hip.h): keyed action noise."""
    _fields_ = [
        ('seed', C.c_uint64),
        ('id_base', C.c_int64),
        ('sigma', C.c_double),
        ('fa_coef', C.c_void_p),
        ('fa_dim', C.c_int32 * 3),
        ('noise_out', C.c_void_p),
    ]


class ColsumSeg(C.Structure):
    """struct ttl_colsum_seg (include/ttl_learner.h)."""
    _fields_ = [
        ('part', C.c_void_p),
        ('ld', C.c_int64),
        ('n_part', C.c_int32),
        ('n', C.c_int32),
        ('out', C.c_void_p),
        ('scale', C.c_float),
        ('accumulate', C.c_int32),
    ]


class TractFileDesc(C.Structure):
    """struct ttl_tract_file_desc (include/ttl_hip.h): a file body's layout
    and point arithmetic."""
    _fields_ = [
        ('format', C.c_int32),
        ('n_props', C.c_int32),
        ('has_pre', C.c_int32),
        ('n_maps', C.c_int32),
        ('has_post', C.c_int32),
        ('reserved', C.c_int32),
        ('pre_scale', C.c_double),
        ('maps', (C.c_double * 12) * 2),
        ('post_scale', C.c_double * 3),
    ]


class ActDesc(C.Structure):
    """struct ttl_act_desc (include/ttl_hip.h): tissue maps and mode of the
    ACT / CMC stopping criterion."""
    _fields_ = [
        ('include', C.c_void_p),
        ('exclude', C.c_void_p),
        ('dim', C.c_int32 * 3),
        ('mode', C.c_int32),
        ('coord_shift', C.c_double),
        ('exponent', C.c_double),
        ('seed', C.c_uint64),
        ('ids_base', C.c_int64),
    ]


class DensityDesc(C.Structure):
    """struct ttl_density_desc (include/ttl_hip.h): the maps of
    ``ttl_tract_density``, its grid and its set sizes."""
    _fields_ = [
        ('dims', C.c_int32 * 3),
        ('lin', C.c_double * 9),
        ('count', C.c_void_p),
        ('length_q', C.c_void_p),
        ('dec_q', C.c_void_p),
        ('ends', C.c_void_p),
        ('wave_slots', C.c_int32),
        ('spill_slots', C.c_int32),
        ('workspace', C.c_void_p),
        ('workspace_bytes', C.c_size_t),
    ]


# name -> (restype, argtypes); every symbol include/ttl_hip.h and
# include/ttl_learner.h declare
SYMBOLS = {
    'ttl_env_workspace_bytes': (C.c_size_t, [C.c_int32]),
    'ttl_sh_volume_records': (C.c_int64, [C.POINTER(C.c_int32), C.c_int32]),
    'ttl_volume_alloc': (C.c_int, [C.c_int32, C.c_size_t, C.c_int32, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int32)]),
    'ttl_volume_free': (C.c_int, [C.c_void_p]),
    'ttl_pack_sh_volume': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                                      C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'ttl_mask_classes': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_double,
                                   C.c_void_p, C.c_void_p]),
    'ttl_env_create': (C.c_int, [C.POINTER(EnvDesc), C.POINTER(C.c_void_p)]),
    'ttl_env_destroy': (None, [C.c_void_p]),
    'ttl_env_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p]),
    'ttl_env_reset_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    'ttl_env_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_env_step_begin': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    'ttl_env_step_end': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p]),
    'ttl_env_wait_counts': (C.c_int, [C.c_void_p]),
    'ttl_env_stopped': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    'ttl_oracle_segments': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_oracle_segments_packed': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p]),
    'ttl_tract_coverage': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float,
                                     C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    'ttl_tractometer_classify': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32,
                                           C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_uint64, C.c_void_p, C.POINTER(C.c_double),
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_tractometer_overlap': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_tractometer_invalid': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_connectome_assign': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double),
                                        C.c_double, C.POINTER(C.c_int32), C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    'ttl_connectome_accumulate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_tract_sample_mean': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    'ttl_connectome_accumulate_metric': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                   C.c_double, C.c_void_p, C.c_void_p,
                                                   C.c_void_p]),
    'ttl_tract_density_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'ttl_tract_density': (C.c_int, [C.POINTER(DensityDesc), C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    'ttl_bundle_orient': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    'ttl_bundle_profile': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                     C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_bundle_recognize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_bundle_register_cost': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_int32,
                                           C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    'ttl_oracle_bonus': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_env_harvest_wait': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.POINTER(C.c_int32)]),
    'ttl_env_harvest': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_void_p]),
    'ttl_env_freerun_begin': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_env_freerun_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_env_freerun_scripted_actions': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_int32, C.c_int32, C.c_uint32,
                                                   C.c_float, C.c_void_p, C.c_void_p]),
    'ttl_env_freerun_end': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.c_void_p]),
    'ttl_env_set_noise': (C.c_int, [C.c_void_p, C.POINTER(NoiseDesc)]),
    'ttl_noise_normals': (C.c_int, [C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p]),
    'ttl_env_stopping_flags': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_env_set_processing_order': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_void_p]),
    'ttl_env_refresh_processing_order': (C.c_int, [C.c_void_p, C.c_void_p]),
    'ttl_env_order_slots': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'ttl_env_tail_riders': (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_void_p)]),
    'ttl_env_view': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p),
                               C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    'ttl_env_profile_begin': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'ttl_env_profile_end': (C.c_int, [C.c_void_p, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int32)]),
    'ttl_scripted_actions': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_uint32,
                                       C.c_uint32, C.c_float, C.c_void_p,
                                       C.c_void_p]),
    'ttl_odf_actions': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                  C.c_uint64, C.c_int64, C.c_void_p, C.c_int32, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_env_freerun_odf_actions': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_float, C.c_float, C.c_int32, C.c_uint64,
                                              C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    'ttl_act_flags': (C.c_int, [C.POINTER(ActDesc), C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    'ttl_env_set_act': (C.c_int, [C.c_void_p, C.POINTER(ActDesc)]),
    'ttl_peaks_from_sh': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_float, C.c_float, C.c_float,
                                    C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_resample_streamlines': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_oracle_net_forward': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    'ttl_pack_streamlines': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_tract_mask_words': (C.c_int32, [C.c_int64]),
    'ttl_tract_stage_points': (C.c_int32, []),
    'ttl_tract_select': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_tract_emit': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    'ttl_tract_file_words': (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    'ttl_tract_emit_file': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(TractFileDesc), C.c_void_p, C.c_void_p]),
    # ---- include/ttl_learner.h
    'ttl_thin_forward': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_sac_losses': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    'ttl_thin_backward': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    'ttl_relu_backward_bias': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    'ttl_colsum_finalize': (C.c_int, [C.POINTER(ColsumSeg), C.c_int32, C.c_void_p]),
    'ttl_sac_actor_head_backward': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                              C.c_void_p]),
    'ttl_td3_losses': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_double,
                                 C.c_double, C.c_double, C.c_void_p]),
    'ttl_polyak_average': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double,
                                     C.c_void_p]),
    'ttl_adam_polyak': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_void_p]),
    'ttl_sac_alpha_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_float, C.c_void_p, C.c_double, C.c_double,
                                     C.c_double, C.c_void_p]),
    'ttl_build_learner_inputs': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    'ttl_replay_add': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_replay_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    'ttl_last_error': (C.c_char_p, []),
    'ttl_abi_version': (C.c_uint32, []),
    'ttl_env_desc_size': (C.c_size_t, []),
}

_lib = None


def load():
    """Load libttl_hip.so once; raise if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TTLError(
            f'{LIB_PATH} not found: the HIP extension is required (build it '
            'with `python -m tracktolearn_amd.csrc.build`); there is no CPU '
            'fallback')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if a symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.ttl_abi_version() != ABI_VERSION:
        raise TTLError('libttl_hip.so ABI version mismatch')
    if lib.ttl_env_desc_size() != C.sizeof(EnvDesc):
        raise TTLError('ttl_env_desc layout mismatch between libttl_hip.so '
                       f'({lib.ttl_env_desc_size()} B) and the ctypes mirror '
                       f'({C.sizeof(EnvDesc)} B)')
    _lib = lib
    return lib


class DeviceVolume:
    """Device memory from ``ttl_volume_alloc`` (on request physically contiguous
    when the driver grants it), exposed through ``__cuda_array_interface__`` so that
    ``torch.as_tensor(vol, device=...)`` wraps it without a copy; the tensor
    keeps this object alive, ``__del__`` returns the memory."""

    def __init__(self, device_index, nbytes, try_contiguous=False):
        lib = load()
        ptr, contiguous = C.c_void_p(), C.c_int32()
        check(lib.ttl_volume_alloc(int(device_index), int(nbytes), int(try_contiguous),
                                   C.byref(ptr), C.byref(contiguous)), 'ttl_volume_alloc')
        self.ptr, self.nbytes, self.contiguous = ptr.value, int(nbytes), int(contiguous.value)
        self.__cuda_array_interface__ = {'shape': (self.nbytes,), 'typestr': '|u1',
                                         'data': (self.ptr, False), 'version': 2}

    def __del__(self):
        ptr, self.ptr = getattr(self, 'ptr', None), None
        if ptr and _lib is not None:
            _lib.ttl_volume_free(ptr)


def check(code, what=''):
    if code != 0:
        msg = load().ttl_last_error().decode('utf-8', 'replace')
        raise TTLError(f'{what} failed ({code}): {msg}')


def ragged_rows(points, offsets):
    """n of the ragged rows an entry takes, or ValueError: ``points`` (P, 3) float32 and
    ``offsets`` (n + 1,) int64, contiguous tensors on one device."""
    if not (torch.is_tensor(points) and points.dtype == torch.float32 and points.dim() == 2 and
            points.shape[1] == 3 and points.is_contiguous()):
        raise ValueError('points must be a contiguous (P, 3) float32 tensor')
    if not (torch.is_tensor(offsets) and offsets.dtype == torch.int64 and offsets.dim() == 1 and
            offsets.is_contiguous() and offsets.device == points.device):
        raise ValueError('offsets must be a contiguous (n + 1,) int64 tensor on the device of '
                         'points')
    return max(int(offsets.shape[0]) - 1, 0)


def lin9(lin):
    """The ``lin[9]`` of an entry from the (3, 3) linear part of voxel -> RAS mm or its 9 values."""
    lin = np.asarray(lin, np.float64)
    if lin.size != 9:
        raise ValueError(f'lin must be (3, 3), not {lin.shape}')
    return (C.c_double * 9)(*lin.reshape(9))


def stream_of(device):
    """The ``hip_stream`` of an entry: torch's current stream of ``device``."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
