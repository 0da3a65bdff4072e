"""ctypes binding of libwct_hip.so (include/wct_hip.h).

`cffi` is not installable here, so the "thin C-ABI layer" is ctypes.  The
library is loaded lazily; on a box with a GPU and no built library this raises
-- there is no CPU fallback behind these calls.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libwct_hip.so')

# every symbol include/wct_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int)
_U8 = C.POINTER(C.c_uint8)
_D = C.POINTER(C.c_double)
_PP = C.POINTER(C.c_void_p)
SIGNATURES = [
    ('wct_create', C.c_int, [C.c_int, _PP]),
    ('wct_destroy', None, [_P]),
    ('wct_last_error', C.c_char_p, []),
    ('wct_sync', C.c_int, [_P]),
    ('wct_device_count', C.c_int, [_I]),
    ('wct_get_stream', C.c_int, [_P, _PP]),
    ('wct_set_encoder', C.c_int, [_P, _F, _F, C.POINTER(_F), C.POINTER(_F), C.c_int]),
    ('wct_set_decoder', C.c_int, [_P, C.c_int, C.POINTER(_F), C.POINTER(_F), C.c_int]),
    ('wct_transform', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, _F, _I]),
    ('wct_adain', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float, _F]),
    ('wct_transform_mix', C.c_int, [_P, _F, C.c_int, C.POINTER(_F), _I, C.c_int, _F, C.c_int, C.c_float, C.c_int, C.c_float,
                                    _F, _I]),
    ('wct_adain_mix', C.c_int, [_P, _F, C.c_int, C.POINTER(_F), _I, C.c_int, _F, C.c_int, C.c_float, C.c_float, _F]),
    ('wct_transform_masked', C.c_int, [_P, _F, C.c_int, _U8, C.POINTER(_F), _I, C.c_int, C.c_int, C.c_float, C.c_int,
                                       C.c_float, _F, _I]),
    ('wct_adain_masked', C.c_int, [_P, _F, C.c_int, _U8, C.POINTER(_F), _I, C.c_int, C.c_int, C.c_float, C.c_float, _F]),
    ('wct_mask_compact', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I, _I]),
    ('wct_mask_compact_batch', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I, _I]),
    ('wct_style_swap', C.c_int, [_P, _F, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, _F]),
    ('wct_set_style_swap', C.c_int, [_P, C.c_float, C.c_int, C.c_int]),
    ('wct_eigh', C.c_int, [_P, _F, C.c_int, C.c_int, _F, _F, _I]),
    ('wct_conv3x3', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_conv3x3_f16', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_maxpool', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_encode', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_decode', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_coral_stats', C.c_int, [_P, _U8, C.c_int, C.c_int, _D]),
    ('wct_coral_apply', C.c_int, [_P, _U8, C.c_int, C.c_int, _D, _D, _D, _D, _D, _U8, _D]),
    ('wct_content_colors', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, _U8]),
    ('wct_content_colors_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_guided_filter', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_guided_filter_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_set_guided', C.c_int, [_P, C.c_int, C.c_int]),
    ('wct_guided_filter_guide', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_guided_filter_guide_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_set_guided_guide', C.c_int, [_P, C.c_int]),
    ('wct_guided_filter_time', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_guided_filter_time_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.c_int, _P]),
    ('wct_guided_time_max_radius', C.c_int, [C.c_int]),
    ('wct_motion_global', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _I]),
    ('wct_motion_global_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _I]),
    ('wct_guided_filter_motion', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I, _U8]),
    ('wct_guided_filter_motion_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     _I, C.c_int, C.c_int, _P]),
    ('wct_guided_filter_time_guide', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               _I, _U8]),
    ('wct_guided_filter_time_guide_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         C.c_int, _I, C.c_int, C.c_int, _P]),
    ('wct_guided_upsample', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_guided_upsample_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, _P]),
    ('wct_guided_upsample_time', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, _I, _U8]),
    ('wct_guided_upsample_time_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, _I, C.c_int, C.c_int, _P]),
    ('wct_guided_upsample_guide', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, _U8]),
    ('wct_guided_upsample_guide_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.c_int, _P]),
    ('wct_resize', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_resize_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_output_size', C.c_int, [C.c_int, C.c_int, _I, C.c_int, _I, _I]),
    ('wct_stylize', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, C.c_int, _I, C.c_int,
                              C.c_float, C.c_uint, _U8]),
    ('wct_stylize_mix', C.c_int, [_P, _U8, C.c_int, C.c_int, C.POINTER(_U8), _I, _I, C.c_int, _F, _I, C.c_int,
                                  C.c_float, C.c_uint, _U8]),
    ('wct_stylize_masked', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.POINTER(_U8), _I, _I, C.c_int, _I, C.c_int,
                                     C.c_float, C.c_uint, _U8]),
    ('wct_stylize_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _I,
                                        C.c_int, C.c_float, C.c_uint, _P]),
    ('wct_style_prepare', C.c_int, [_P, _U8, C.c_int, C.c_int, _I, C.c_int, C.c_uint, _PP]),
    ('wct_style_free', None, [_P, _P]),
    ('wct_stylize_prepared', C.c_int, [_P, _U8, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _U8]),
    ('wct_stylize_prepared_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _P]),
    ('wct_stylize_prepared_upsampled', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint,
                                                 C.c_int, C.c_int, _U8]),
    ('wct_stylize_prepared_upsampled_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float,
                                                           C.c_uint, C.c_int, C.c_int, _P]),
    ('wct_stylize_prepared_upsampled_guide', C.c_int, [_P, _U8, C.c_int, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint,
                                                       C.c_int, C.c_int, C.c_int, _U8]),
    ('wct_stylize_prepared_upsampled_guide_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int,
                                                                 C.c_float, C.c_uint, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_stylize_prepared_mix', C.c_int, [_P, _U8, C.c_int, C.c_int, _PP, C.c_int, _F, _I, C.c_int, C.c_float, C.c_uint, _U8]),
    ('wct_stylize_prepared_masked', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, _PP, C.c_int, _I, C.c_int, C.c_float, C.c_uint, _U8]),
    ('wct_stylize_prepared_masked_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _U8, _PP, C.c_int, _I, C.c_int, C.c_float,
                                                        C.c_uint, _P]),
    ('wct_style_prepare_region', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, _I, C.c_int, C.c_uint, _PP]),
    ('wct_style_prepare_regions', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, C.c_int, _I, C.c_int, C.c_uint, _PP]),
    ('wct_style_rows', C.c_int, [_P, _P, C.c_int, _I]),
    ('wct_transform_region', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_int, _U8, C.c_int, C.c_float, C.c_int, C.c_float,
                                       _F, _I]),
    ('wct_adain_region', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_int, _U8, C.c_int, C.c_float, C.c_float, _F]),
    ('wct_warm_create', C.c_int, [_P, _I, C.c_int, _PP]),
    ('wct_warm_free', None, [_P, _P]),
    ('wct_warm_reset', C.c_int, [_P, _P]),
    ('wct_warm_basis', C.c_int, [_P, _P, C.c_int, _I, _F]),
    ('wct_stylize_prepared_warm', C.c_int, [_P, _U8, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _P, _U8]),
    ('wct_stylize_prepared_batch_dev_warm', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _P, _P]),
    ('wct_transform_warm', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_uint, _P, C.c_int, _F, _I]),
    ('wct_transform_strength', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_float,
                                         C.c_int, C.c_float, _F, _I]),
    ('wct_adain_strength', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _U8, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_float,
                                     C.c_float, _F]),
    ('wct_stylize_prepared_strength', C.c_int, [_P, _U8, C.c_int, C.c_int, _U8, _P, _I, C.c_int, C.c_float, C.c_uint, _U8]),
    ('wct_stylize_prepared_strength_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _I, C.c_int, C.c_float, C.c_uint, _P]),
    ('wct_stylize_prepared_strength_batch_dev_warm', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _I, C.c_int, C.c_float, C.c_uint,
                                                               _P, _P]),
    ('wct_texture_noise_batch_dev', C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _P]),
    ('wct_texture_noise', C.c_int, [_P, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _U8]),
    ('wct_texture_size', C.c_int, [C.c_int, C.c_int, _I, C.c_int, C.c_int, _I, _I]),
    ('wct_texture_prepared_batch_dev', C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _P, _I, C.c_int, C.c_int,
                                                 C.c_float, C.c_uint, _P]),
    ('wct_texture_prepared', C.c_int, [_P, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _P, _I, C.c_int, C.c_int, C.c_float,
                                       C.c_uint, _U8]),
    ('wct_band_rows', C.c_int, [C.c_int, C.c_int, _I, C.c_int, _I]),
    ('wct_band_plan', C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _I, _I]),
    ('wct_encode_banded', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_decode_banded', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_transform_chunked', C.c_int, [_P, _F, C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, _F, _I]),
    ('wct_stylize_prepared_banded_dev', C.c_int, [_P, _P, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, C.c_int, C.c_int, _P]),
    ('wct_stylize_prepared_banded', C.c_int, [_P, _U8, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, C.c_int, C.c_int, _U8]),
    ('wct_wrap_halo', C.c_int, [C.c_int, _I, _I, _I]),
    ('wct_wrap_check', C.c_int, [C.c_int, C.c_int, _I, C.c_int]),
    ('wct_wrap_pad_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('wct_wrap_pad', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_encode_wrap', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_decode_wrap', C.c_int, [_P, _F, C.c_int, C.c_int, C.c_int, _F]),
    ('wct_stylize_prepared_wrap_batch_dev', C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _P]),
    ('wct_stylize_prepared_wrap', C.c_int, [_P, _U8, C.c_int, C.c_int, _P, _I, C.c_int, C.c_float, C.c_uint, _U8]),
    ('wct_texture_prepared_wrap_batch_dev', C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _P, _I, C.c_int,
                                                      C.c_int, C.c_float, C.c_uint, _P]),
    ('wct_texture_prepared_wrap', C.c_int, [_P, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, _P, _I, C.c_int, C.c_int, C.c_float,
                                            C.c_uint, _U8]),
    ('wct_train_step', C.c_int, [_P, C.c_int, _F, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, _F]),
    ('wct_get_decoder_layer', C.c_int, [_P, C.c_int, C.c_int, _F, _F, _F, _F]),
    ('wct_train_grad_buffer', C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ('wct_train_apply', C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]),
    ('wct_dev_alloc', C.c_int, [_P, C.c_size_t, _PP]),
    ('wct_dev_free', C.c_int, [_P, _P]),
    ('wct_h2d', C.c_int, [_P, _P, _P, C.c_size_t]),
    ('wct_d2h', C.c_int, [_P, _P, _P, C.c_size_t]),
    ('wct_prof_enable', C.c_int, [_P, C.c_int]),
    ('wct_prof_reset', C.c_int, [_P]),
    ('wct_prof_read', C.c_int, [_P, _D, C.POINTER(C.c_longlong), _D, _D]),
    ('wct_eig_stats', C.c_int, [_P, C.POINTER(C.c_longlong)]),
]

WCT_NP, WCT_TF = 0, 1
FLAG_ADAIN, FLAG_MODE_NP, FLAG_SWAP5, FLAG_STYLE_SHARED, FLAG_IMAGES_F32, FLAG_CONTENT_COLORS = 1, 2, 4, 8, 16, 32
FLAG_GUIDED = 64
GUIDED_MAX_RADIUS, GUIDED_MAX_EPS = 64, 65025      # csrc/guided_rule.h
GUIDE_GREY, GUIDE_COLOR = 0, 1                     # WCT_GUIDE_*: the guide of guided smoothing
GUIDES = {'grey': GUIDE_GREY, 'color': GUIDE_COLOR}
# temporal guided smoothing (csrc/guided_time_rule.h): the largest radius at T = 0 .. 3 frames on each side, from
# (2r + 1)^2 (2T + 1) <= 33025; wct_guided_time_max_radius(T) returns the same numbers
GUIDED_TIME_MAX_RADIUS = (64, 51, 40, 33)
# temporal guided smoothing along motion (csrc/guided_motion_rule.h): the largest step between two frames and the largest search
# range of the estimator, and the pixels of a content frame it takes
MOTION_MAX_RANGE, MOTION_MAX_PIXELS = 16, 1 << 28


def guided_eps_q(eps):
    """eps of the usual [0,1]^2 convention of a guided filter in grey levels squared: round(eps * 255^2), at least 1"""
    return max(1, int(round(float(eps) * 65025)))


PROF_CLASSES = ['conv3x3', 'conv_first', 'conv_last', 'pool', 'wct_cov', 'jacobi', 'wct_apply', 'other', 'conv12', 'conv_wino', 'conv_tail']

_lib = None


class WCTHipError(RuntimeError):
    pass


class WCTNotConverged(WCTHipError):
    """WCT_STATUS_NOCONV: an eigendecomposition behind the call ran out of sweeps or met NaN/Inf (the reference's
    np.linalg.svd raises LinAlgError at the same spot, ops.py:110,123).  Outputs were written but are unreliable."""


STATUS_NOCONV = -5
MIX_MAX = 8                  # styles per mix (WCT_MIX_MAX)
BATCH_MAX = 32               # frames per batch call
PASSES_MAX = 16              # passes of one texture call (wct_texture_prepared*)


def load():
    """Load libwct_hip.so and declare every prototype.  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WCTHipError('%s not built: run `python -m wct_tf_amd.build` (hipcc, gfx950). '
                              'There is no CPU fallback for the stylize path.' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        cls = WCTNotConverged if rc == STATUS_NOCONV else WCTHipError
        raise cls('libwct_hip error %d: %s' % (rc, load().wct_last_error().decode()))


def fptr(a):
    return a.ctypes.data_as(_F)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def ptr_array(arrays):
    """float** from a list of contiguous float32 arrays (keeps them alive via the return)."""
    arr = (_F * len(arrays))(*[fptr(a) for a in arrays])
    return arr


def mix_weights(weights, k):
    """Validated style-mix weights as float32 [k] (None: equal weights).  They must be finite, >= 0 and sum to > 0 --
    the rule the library applies (lambda_k = w_k / sum(w), include/wct_hip.h), checked here before any GPU call."""
    if not 1 <= k <= MIX_MAX:
        raise ValueError('a style mix takes 1 .. %d styles, got %d' % (MIX_MAX, k))
    if weights is None:
        return np.ones(k, np.float32)
    w = np.asarray(weights, np.float64).reshape(-1)
    if w.size != k:
        raise ValueError('%d weights for %d styles' % (w.size, k))
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('style weights must be finite and >= 0, got %s' % (list(w),))
    if not w.sum() > 0:
        raise ValueError('style weights sum to 0')
    return np.ascontiguousarray(w, np.float32)


def mask_labels(mask, k, shape=None):
    """A validated label map as contiguous uint8 (spatial control): integer labels 0 .. k - 1 for k = 1 .. MIX_MAX styles, and,
    given `shape`, exactly that shape -- the rules the library applies (include/wct_hip.h), checked here before any GPU call."""
    if not 1 <= k <= MIX_MAX:
        raise ValueError('a mask takes 1 .. %d styles, got %d' % (MIX_MAX, k))
    m = np.asarray(mask)
    if shape is not None and m.shape != tuple(shape):
        raise ValueError('mask of shape %s for content of shape %s' % (m.shape, tuple(shape)))
    if m.size == 0:
        raise ValueError('empty mask')
    if not (np.issubdtype(m.dtype, np.integer) or np.issubdtype(m.dtype, np.bool_)):
        raise ValueError('mask labels must be integers, got %s' % (m.dtype,))
    if m.min() < 0 or m.max() >= k:
        raise ValueError('mask labels must be 0 .. %d for %d styles, got %d .. %d' % (k - 1, k, m.min(), m.max()))
    return np.ascontiguousarray(m, np.uint8)


def style_region_map(label_map, shape, k=None, label=None):
    """The label map of a style image of `shape` (H, W) as contiguous uint8 (style regions, include/wct_hip.h): an integer
    array of exactly that shape with values 0 .. 255 -- and, given k, labels 0 .. k - 1 for k = 1 .. MIX_MAX regions; given
    `label`, a label 0 .. MIX_MAX - 1.  The rules the library applies, checked here before any GPU call."""
    if k is not None and not 1 <= int(k) <= MIX_MAX:
        raise ValueError('style regions: 1 .. %d regions, got %d' % (MIX_MAX, k))
    if label is not None and not 0 <= int(label) < MIX_MAX:
        raise ValueError('a style region takes a label 0 .. %d, got %d' % (MIX_MAX - 1, label))
    m = np.asarray(label_map)
    if not (np.issubdtype(m.dtype, np.integer) or np.issubdtype(m.dtype, np.bool_)):
        raise ValueError('style region labels must be integers, got %s' % (m.dtype,))
    if m.shape != tuple(shape) or m.size == 0:
        raise ValueError('style label map of shape %s for a style of shape %s' % (m.shape, tuple(shape)))
    top = 255 if k is None else int(k) - 1
    if m.min() < 0 or m.max() > top:
        raise ValueError('style region labels must be 0 .. %d, got %d .. %d' % (top, m.min(), m.max()))
    return np.ascontiguousarray(m, np.uint8)


def strength_map(smap, shape):
    """A validated strength map as contiguous uint8: a uint8 array of exactly `shape` (H, W) -- 255 is the call's alpha, 0 keeps the
    content -- checked here before any GPU call."""
    m = np.asarray(smap)
    if m.dtype != np.uint8:
        raise ValueError('a strength map is uint8 (255: the full alpha, 0: keep the content), got %s' % (m.dtype,))
    if m.shape != tuple(shape) or m.size == 0:
        raise ValueError('strength map of shape %s for content of shape %s' % (m.shape, tuple(shape)))
    return np.ascontiguousarray(m)


def strength_maps_frames(smaps, n_frames, shape):
    """The strength maps of `n_frames` frames of `shape` (H, W) as contiguous uint8 [F][H][W]: `smaps` is [F][H][W] (one map per
    frame; the count must equal the frame count), or one [H][W] map used for every frame.  Each map is checked by strength_map."""
    shape = tuple(shape)
    if isinstance(smaps, np.ndarray) and smaps.ndim == 2:
        return np.ascontiguousarray(np.broadcast_to(strength_map(smaps, shape), (n_frames,) + shape))
    if len(smaps) != n_frames:
        raise ValueError('%d strength maps for %d frames' % (len(smaps), n_frames))
    out = np.empty((n_frames,) + shape, np.uint8)
    for f in range(n_frames):
        out[f] = strength_map(smaps[f], shape)
    return out


def mask_labels_frames(masks, k, n_frames, shape):
    """The label maps of `n_frames` frames of `shape` (H, W) as contiguous uint8 [F][H][W]: `masks` is [F][H][W] (one map per
    frame; the count must equal the frame count), or one [H][W] map used for every frame.  Each map is checked by mask_labels."""
    if not 1 <= k <= MIX_MAX:
        raise ValueError('a mask takes 1 .. %d styles, got %d' % (MIX_MAX, k))
    shape = tuple(shape)
    if isinstance(masks, np.ndarray) and masks.ndim == 2:
        return np.ascontiguousarray(np.broadcast_to(mask_labels(masks, k, shape), (n_frames,) + shape))
    if len(masks) != n_frames:
        raise ValueError('%d masks for %d frames' % (len(masks), n_frames))
    out = np.empty((n_frames,) + shape, np.uint8)
    for f in range(n_frames):
        out[f] = mask_labels(masks[f], k, shape)
    return out
