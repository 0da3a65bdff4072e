"""Prepared styles (wct_style), the parts that need no GPU: the ABI declarations, the exported symbols and their ctypes
bindings, the Python-side refusals (raised before any library call) and the unchanged command lines."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ('wct_style_prepare', 'wct_style_free', 'wct_stylize_prepared', 'wct_stylize_prepared_batch_dev',
           'wct_stylize_prepared_mix')
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_prepared_symbols_declared_exported_and_bound(lib):
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    assert re.search(r'typedef\s+struct\s+wct_style\s+wct_style\s*;', header)
    for name in SYMBOLS:
        m = re.search(r'^\s*(int|void)\s+%s\s*\(([^;]*)\)\s*;' % name, header, re.M)
        assert m, name
        assert name in bound and hasattr(lib, name), name
        # one ctypes argument per declared parameter, and the return type of the declaration
        assert len(bound[name][1]) == len(m.group(2).split(',')), name
        assert (bound[name][0] is None) == (m.group(1) == 'void'), name


def test_prepared_calls_refuse_a_null_context(lib):
    import ctypes as C
    h = C.c_void_p()
    lv = (C.c_int * 1)(1)
    img = np.zeros((8, 8, 3), np.uint8)
    p = img.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.wct_style_prepare(None, p, 8, 8, lv, 1, 0, C.byref(h)) == -2 and b'invalid argument' in lib.wct_last_error()
    assert lib.wct_stylize_prepared(None, p, 8, 8, None, lv, 1, C.c_float(1), 0, p) == -2
    assert lib.wct_stylize_prepared_batch_dev(None, None, 8, 8, 1, None, lv, 1, C.c_float(1), 0, None) == -2
    assert lib.wct_stylize_prepared_mix(None, p, 8, 8, None, 1, None, lv, 1, C.c_float(1), 0, p) == -2
    lib.wct_style_free(None, None)                                     # a no-op, not a fault


class _NoLibrary(object):
    """stands in for a Context: any library call through it is an error of the test"""
    h = 1

    def __getattr__(self, name):
        raise AssertionError('the library was reached: %s' % name)


def _model(ctx):
    from wct_tf_amd.wct import WCT
    model = WCT.__new__(WCT)                  # no __init__: no GPU context exists
    model.sess, model.relu_targets, model.wct_mode, model.ss_patch_size, model.ss_stride = ctx, SMALL, 'tf', 3, 1
    return model


def _handle(ctx, levels=(1, 2, 3)):
    from wct_tf_amd.context import PreparedStyle
    return PreparedStyle(ctx, 12345, np.zeros((16, 16, 3), np.uint8), levels)


IMG = np.zeros((16, 16, 3), np.uint8)


def test_swap5_with_a_handle_is_refused_before_the_library():
    ctx = _NoLibrary()
    model, h = _model(ctx), _handle(ctx)
    with pytest.raises(ValueError, match='swap5'):
        model.predict(IMG, h, swap5=True)
    with pytest.raises(ValueError, match='swap5'):
        model.predict_frames(IMG[None], h, swap5=True)
    with pytest.raises(ValueError, match='swap5'):
        model.predict_mix(IMG, [h], swap5=True)
    h.h = None                                 # (nothing to free in this test)


def test_mixed_lists_are_refused_before_the_library():
    ctx = _NoLibrary()
    model, h = _model(ctx), _handle(ctx)
    with pytest.raises(ValueError, match='not a mix of both'):
        model.predict_mix(IMG, [h, IMG])
    with pytest.raises(ValueError, match='not a mix of both'):
        model.predict_mix(IMG, [IMG, h, IMG], [1, 1, 1])
    with pytest.raises(ValueError):            # the weight rules hold for handles as for images
        model.predict_mix(IMG, [h, h], [1, -1])
    with pytest.raises((TypeError, ValueError)):
        model.predict_masked(IMG, [h], np.zeros((16, 16), np.uint8))
    h.h = None


def test_a_handle_of_another_context_is_refused_before_the_library():
    ctx, other = _NoLibrary(), _NoLibrary()
    model, h = _model(ctx), _handle(other)
    for call in (lambda: model.predict(IMG, h), lambda: model.predict_frames(IMG[None], h), lambda: model.predict_mix(IMG, [h])):
        with pytest.raises(ValueError, match='another context'):
            call()
    h.h = None


def test_a_closed_handle_is_refused_before_the_library():
    ctx = _NoLibrary()
    model, h = _model(ctx), _handle(ctx)
    h.h = None                                 # what close() leaves behind
    assert h.closed
    for call in (lambda: model.predict(IMG, h), lambda: model.predict_frames(IMG[None], h), lambda: model.predict_mix(IMG, [h, h])):
        with pytest.raises(ValueError, match='closed'):
            call()
    h.close()                                  # closing twice is harmless
    closed_ctx = _NoLibrary()
    h2 = _handle(closed_ctx)
    closed_ctx.h = None                        # the context was closed: so is the handle
    assert h2.closed


def test_levels_outside_the_handle_are_refused_before_the_library():
    ctx = _NoLibrary()
    model, h = _model(ctx), _handle(ctx, levels=(1, 2))
    with pytest.raises(ValueError, match='relu levels'):
        model.predict(IMG, h)
    h.h = None


def test_command_lines_take_no_new_flag():
    """prepared styles are used inside stylize / stylize_video without a new flag, required or not"""
    from wct_tf_amd import stylize, stylize_video
    args = stylize.build_parser().parse_args(['--relu-targets', 'relu1_1', '--content-path', 'c', '--style-path', 's', '--out-path', 'o'])
    assert stylize.can_prepare(args)
    assert not stylize.can_prepare(stylize.build_parser().parse_args(['--relu-targets', 'relu1_1', '--keep-colors']))
    assert not stylize.can_prepare(stylize.build_parser().parse_args(['--relu-targets', 'relu1_1', '--swap5']))
    for mod in (stylize, stylize_video):
        flags = {a for act in mod.build_parser()._actions for a in act.option_strings}
        assert not any('prepare' in f for f in flags), flags
