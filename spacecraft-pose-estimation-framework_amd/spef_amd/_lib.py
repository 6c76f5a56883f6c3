"""ctypes binding of the C ABI in include/spef.h (libspef_mi355x.so, built in-tree by _build.py).

There is no CPU fallback: if the library is missing or fails to load, importing the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build

OK, ERR_ARG, ERR_HIP, ERR_BLOB, ERR_STATE, ERR_NUMERIC, ERR_COMM = range(7)
IN_U8_NHWC, IN_F32_NCHW = 0, 1
REGRESSION, CLASSIFICATION, KEYPOINTS = 0, 1, 2
ABI_VERSION = 4
COMM_ID_BYTES = 128
METRIC_IDS = {'l2': 0, 'kl': 1, 'js': 2, 'hellinger': 3, 'tv': 4, 'wasserstein': 5}   # spef_video_metric
OPT_FUSE_BLOCKS, OPT_WAVESPEC, OPT_Q8_ROLESPLIT = 1, 6, 7     # public schedule options (include/spef.h)
OPT_FUSE_MIN_HW, OPT_PW_GEMM, OPT_IRB_VARIANT, OPT_TEST_FAIL_BCAST = 2, 3, 4, 5   # internal (csrc/spef_tuning.hpp)
OPT_MX_KERNELS = 8   # internal: fp16mx blocks 2-7 on k_mx.hip (1) or the fp16x2 slab kernels (0)
OPT_TRIM = 9         # internal, one bit per kernel (a cleared bit runs the earlier kernel): bit 0 = the last conv's
#                      128 x 320 tile (0: 64 x 256), bit 1 = mx_irb_kernel's lean tile set-up (0: 64-bit addresses)
OPT_TRIM_DEFAULT = 3
OPT_X2_STAGE = 10    # internal: blocks 8-10 / 14 on x2_irw_st_kernel (1, default: static LDS-DMA staging) or x2_irw_kernel (0)
OPT_X2_STAGE_DEFAULT = 1

# name -> (restype, argtypes); keep in sync with include/spef.h (tests/test_abi.py checks the header)
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
_ip = C.POINTER(C.c_int)
SIGNATURES = {
    'spef_abi_version': (_i, []),
    'spef_last_error': (C.c_char_p, []),
    'spef_init': (_i, [_i, C.POINTER(_vp)]),
    'spef_destroy': (_i, [_vp]),
    'spef_load_weights': (_i, [_vp, _vp, _sz]),
    'spef_load_weights_device': (_i, [_vp, _vp, _sz]),
    'spef_model_info': (_i, [_vp, _ip, _ip, _ip, _ip, _ip]),
    'spef_reserve': (_i, [_vp, _i, _i, _i]),
    'spef_preprocess': (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    'spef_forward': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    'spef_backbone': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'spef_probe': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _ip, _ip, _ip, _vp]),
    'spef_set_decode_tables': (_i, [_vp, _vp, _i, _vp, _i]),
    'spef_decode': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_decode_cov': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'spef_decode_modes': (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_video_create': (_i, [_vp, _i, _i, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(_vp)]),
    'spef_video_reset': (_i, [_vp, _i, _vp]),
    'spef_video_set_state': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    'spef_video_step': (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_video_destroy': (_i, [_vp]),
    'spef_score_create': (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    'spef_score_reset': (_i, [_vp, _i, _vp]),
    'spef_score_step': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    'spef_score_finalize': (_i, [_vp, _vp, _vp]),
    'spef_score_log': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    'spef_score_destroy': (_i, [_vp]),
    'spef_track_create': (_i, [_vp, _i, _vp, C.POINTER(_vp)]),
    'spef_track_reset': (_i, [_vp, _i, _vp]),
    'spef_track_get_state': (_i, [_vp, _i, _i, _vp, _vp]),
    'spef_track_set_state': (_i, [_vp, _i, _i, _vp, _vp]),
    'spef_track_step': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_track_step_modes': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp]),
    'spef_track_destroy': (_i, [_vp]),
    'spef_track_history_create': (_i, [_vp, _i, C.POINTER(_vp)]),
    'spef_track_history_reset': (_i, [_vp]),
    'spef_track_history_count': (_i, [_vp, _vp, _vp]),
    'spef_track_history_push': (_i, [_vp, _vp, _vp, _vp]),
    'spef_track_history_get': (_i, [_vp, _i, _i, _vp, _vp]),
    'spef_track_step_hist': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_track_smooth': (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_track_history_destroy': (_i, [_vp]),
    'spef_observer_create': (_i, [_vp, C.POINTER(_vp)]),
    'spef_observer_info': (_i, [_vp, _ip, _ip]),
    'spef_observer_reset': (_i, [_vp, _vp]),
    'spef_observe': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'spef_observer_update': (_i, [_vp, _i, _vp, C.c_int64, _vp]),
    'spef_observer_read': (_i, [_vp, _i, _i, _vp, _vp]),
    'spef_observer_destroy': (_i, [_vp]),
    'spef_validate_blob': (_i, [_vp, _sz, _ip, _ip, _ip, _ip]),
    'spef_comm_unique_id': (_i, [_vp, _sz]),
    'spef_comm_init': (_i, [_i, _i, _i, _vp, _i, C.POINTER(_vp)]),
    'spef_comm_abort': (_i, [_vp]),
    'spef_comm_destroy': (_i, [_vp]),
    'spef_bcast_weights': (_i, [_vp, _vp, _i]),
    'spef_set_option': (_i, [_vp, _i, _i]),
    'spef_set_keypoints': (_i, [_vp, _vp, _i, _vp, C.c_float, C.c_float]),
    'spef_set_keypoint_distortion': (_i, [_vp, _vp, _i]),
    'spef_decode_keypoints': (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'spef_refine_keypoints': (_i, [_vp, _vp, _vp, _i, _i, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_consensus_keypoints': (_i, [_vp, _vp, _vp, _i, C.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_consensus_keypoints_f64': (_i, [_vp, _vp, _vp, _i, C.c_float, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_track_predict': (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    'spef_roi_boxes': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp]),
    'spef_preprocess_roi': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    'spef_roi_unmap_keypoints': (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    'spef_feature_width': (_i, [_vp, _ip]),
    'spef_features': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'spef_encode_targets': (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_headfit_create': (_i, [_vp, _i, _i, _i, _vp, C.POINTER(_vp)]),
    'spef_headfit_step': (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    'spef_headfit_set_weights': (_i, [_vp, _vp, _vp, _vp]),
    'spef_headfit_get_weights': (_i, [_vp, _vp, _vp, _vp]),
    'spef_headfit_get_state': (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'spef_headfit_get_g': (_i, [_vp, _i, _vp, _vp]),
    'spef_headfit_get_raw': (_i, [_vp, _i, _vp, _vp]),
    'spef_headfit_reset_state': (_i, [_vp, _vp]),
    'spef_headfit_load_model': (_i, [_vp, _vp, _vp]),
    'spef_headfit_commit': (_i, [_vp, _vp, _vp]),
    'spef_headfit_destroy': (_i, [_vp]),
    'spef_profile_begin': (_i, [_vp]),
    'spef_profile_end': (_i, [_vp, C.c_char_p, _sz, C.POINTER(_sz)]),
    'spef_measure_peaks': (_i, [_i, _i, C.POINTER(C.c_double)]),
    'spef_clock_stamp': (_i, [_vp, _i, _vp]),
}


class TrackParams(C.Structure):   # spef_track_params
    _fields_ = [('q', C.c_double * 4), ('p0', C.c_double * 4), ('r', C.c_double * 2), ('cov_scale', C.c_double),
                ('gate_chi2', C.c_double), ('max_coast', C.c_int)]


TRACK_STATE_DOUBLES = 160


class CovParams(C.Structure):     # spef_cov_params
    _fields_ = [('fixed_var', C.c_double * 2), ('floor_var', C.c_double * 2)]


COV_ORI, COV_HINV, COV_POS = 1, 2, 4   # spef_decode_cov's cov_status bits


class ModesParams(C.Structure):   # spef_modes_params
    _fields_ = [('k_max', C.c_int), ('rounds', C.c_int), ('sep_deg', C.c_double), ('seed_rel', C.c_double),
                ('min_mass', C.c_double), ('floor_var', C.c_double)]


class HeadFitParams(C.Structure):   # spef_headfit_params
    _fields_ = [('ori_mode', C.c_int), ('pos_mode', C.c_int), ('optimizer', C.c_int), ('norm_distance', C.c_int),
                ('Bmax', C.c_int), ('seed', C.c_uint32), ('beta', C.c_double), ('momentum', C.c_double),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('weight_decay', C.c_double),
                ('dropout_p', C.c_double)]


class EncodeParams(C.Structure):    # spef_encode_params
    _fields_ = [('ori_var', C.c_double), ('pos_var', C.c_double)]


HEADFIT_RAW = {'W': 0, 'bias': 1, 'W_s1': 2, 'bias_s1': 3, 'W_s2': 4, 'bias_s2': 5, 'Xd': 6}   # spef_headfit_raw
HEADFIT_SGD, HEADFIT_ADAM = 0, 1      # spef_headfit_optimizer
MODES_MAX = 4                          # SPEF_MODES_MAX
ROI_FULL_FRAME, ROI_BAD_BOX = 1, 2     # spef_roi_boxes' / spef_preprocess_roi's status bits


class SpefError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f'[spef error {code}] {msg}')
        self.code = code


_LIB = None


def load(path: str | None = None) -> C.CDLL:
    """Load (once) and return the HIP library; raises if it is absent -- never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch first: its bundled libamdhip64 (SONAME libamdhip64.so.7) then satisfies this library's dependency, so
    # the process holds ONE HIP runtime. Loaded the other way round, torch's libraries pull in their own copy next
    # to /opt/rocm's (they name the unversioned file) and the two runtimes' teardown double-frees at exit.
    import torch  # noqa: F401
    override = path or os.environ.get('SPEF_LIB')    # SPEF_LIB: A/B timing of two builds (tools/ab.py)
    path = override or _build.lib_path()
    if not os.path.exists(path):
        raise ImportError(f'SPEF HIP library not built: {path} (run __graft_entry__.build() or '
                          f'python -m spef_amd._build)')
    if not override:   # the in-tree library must have been linked from exactly the sources beside it
        info = _build.read_info()
        if info.get('source_digest') != _build.source_digest():
            raise ImportError(f'SPEF HIP library {path} is stale or has no BUILD_INFO.json: it was not built from '
                              f'the current csrc/ + include/ (run __graft_entry__.build())')
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if lib.spef_abi_version() != ABI_VERSION:
        raise ImportError('SPEF ABI version mismatch')
    _LIB = lib
    return lib


def check(rc: int) -> None:
    if rc != OK:
        msg = _LIB.spef_last_error().decode(errors='replace') if _LIB else ''
        if rc == ERR_NUMERIC:
            raise ValueError(msg)
        if rc == ERR_ARG:
            raise AssertionError(msg)
        raise SpefError(rc, msg)
