"""Masked video, the parts that need no GPU: the ABI declarations and their ctypes bindings, the Python-side refusals (raised
before any library call) and stylize_video's matching of label maps to frames."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ('wct_stylize_prepared_masked', 'wct_stylize_prepared_masked_batch_dev', 'wct_mask_compact_batch')
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in SYMBOLS:
        m = re.search(r'^\s*int\s+%s\s*\(([^;]*)\)\s*;' % name, header, re.M)
        assert m, name
        assert name in bound and hasattr(lib, name), name
        assert len(bound[name][1]) == len(m.group(1).split(',')), name


def test_calls_refuse_a_null_context(lib):
    import ctypes as C
    lv = (C.c_int * 1)(1)
    img = np.zeros((8, 8, 3), np.uint8)
    p = img.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.wct_stylize_prepared_masked(None, p, 8, 8, p, None, 1, lv, 1, C.c_float(1), 0, p) == -2
    assert b'invalid argument' in lib.wct_last_error()
    assert lib.wct_stylize_prepared_masked_batch_dev(None, None, 8, 8, 1, p, None, 1, lv, 1, C.c_float(1), 0, None) == -2
    assert lib.wct_mask_compact_batch(None, p, 1, 8, 8, 8, 8, 1, 1, None, None) == -2


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
    import ctypes as C
    return PreparedStyle(ctx, C.c_void_p(12345), np.zeros((16, 16, 3), np.uint8), levels)


IMG = np.zeros((16, 16, 3), np.uint8)
ZERO = np.zeros((16, 16), np.uint8)


def test_facade_refusals_come_before_the_library():
    ctx = _NoLibrary()
    model, h = _model(ctx), _handle(ctx)
    frames = np.stack([IMG, IMG, IMG])
    for call in (lambda: model.predict_masked(IMG, [h, IMG], ZERO), lambda: model.predict_frames_masked(frames, [IMG, h], ZERO)):
        with pytest.raises(ValueError, match='not a mix of both'):
            call()
    with pytest.raises(ValueError, match='2 masks for 3 frames'):
        model.predict_frames_masked(frames, [h, h], np.stack([ZERO, ZERO]))
    with pytest.raises(ValueError, match='shape'):
        model.predict_frames_masked(frames, [h, h], np.zeros((3, 16, 12), np.uint8))
    with pytest.raises(ValueError, match='shape'):
        model.predict_frames_masked(frames, [h, h], np.zeros((16, 12), np.uint8))
    with pytest.raises(ValueError, match='shape'):
        model.predict_masked(IMG, [h, h], np.zeros((12, 16), np.uint8))
    with pytest.raises(ValueError, match='labels must be 0 .. 1'):
        model.predict_frames_masked(frames, [h, h], np.stack([ZERO, ZERO + 2, ZERO]))
    with pytest.raises(ValueError, match='labels must be 0 .. 1'):
        model.predict_masked(IMG, [h, h], ZERO + 2)
    with pytest.raises(ValueError, match='swap5'):
        model.predict_masked(IMG, [h], ZERO, swap5=True)
    with pytest.raises(ValueError, match='1 .. 8'):
        model.predict_frames_masked(frames, [h] * 9, ZERO)
    other = _handle(_NoLibrary())
    with pytest.raises(ValueError, match='another context'):
        model.predict_frames_masked(frames, [h, other], ZERO)
    with pytest.raises(ValueError, match='relu levels'):
        model.predict_masked(IMG, [h, _handle(ctx, (1, 2))], ZERO)
    h.h = other.h = None                       # (nothing to free in this test)


def test_context_refusals_come_before_the_library():
    from wct_tf_amd.context import Context
    ctx = Context.__new__(Context)             # no __init__: no library, no GPU context
    ctx.h, ctx.lib = 1, _NoLibrary()
    h = _handle(ctx)
    frames = np.stack([IMG] * 4)
    with pytest.raises(ValueError, match='3 masks for 4 frames'):
        ctx.stylize_prepared_masked_batch(frames, [h, h], np.stack([ZERO] * 3), SMALL)
    with pytest.raises(ValueError, match='shape'):
        ctx.stylize_prepared_masked_batch(frames, [h, h], np.zeros((4, 8, 16), np.uint8), SMALL)
    with pytest.raises(ValueError, match='labels must be 0 .. 1'):
        ctx.stylize_prepared_masked_batch(frames, [h, h], np.stack([ZERO] * 3 + [ZERO + 5]), SMALL)
    with pytest.raises(ValueError, match='labels must be 0 .. 1'):
        ctx.stylize_prepared_masked(IMG, [h, h], ZERO + 2, SMALL)
    with pytest.raises(ValueError, match='1 .. 32 frames'):
        ctx.stylize_prepared_masked_batch(np.stack([IMG] * 33), [h], ZERO, SMALL)
    with pytest.raises(ValueError, match='4 masks for 2 frames'):
        ctx.stylize_prepared_masked_batch_dev(None, 16, 16, 2, np.stack([ZERO] * 4), [h], SMALL, 1.0, None)
    with pytest.raises(TypeError):
        ctx.stylize_prepared_masked(IMG, [IMG], ZERO, SMALL)
    h.h = None
    ctx.h = None


def test_a_handle_that_is_not_a_pointer_never_reaches_the_library():
    """check_prepared's last refusal: the library takes addresses, so an object whose `h` is anything but the ctypes pointer
    prepare_style stores is a TypeError in every call that takes handles, after the other refusals"""
    from wct_tf_amd.context import PreparedStyle
    ctx = _NoLibrary()
    model, good = _model(ctx), _handle(ctx)
    fake = PreparedStyle(ctx, 12345, np.zeros((16, 16, 3), np.uint8), (1, 2, 3))
    for call in (lambda: model.predict(IMG, fake), lambda: model.predict_mix(IMG, [good, fake]),
                 lambda: model.predict_masked(IMG, [good, fake], ZERO), lambda: model.predict_frames_masked(IMG[None], [fake], ZERO)):
        with pytest.raises(TypeError, match='not a wct_style pointer'):
            call()
    with pytest.raises(ValueError, match='relu levels'):            # the other refusals come first
        model.predict_masked(IMG, [fake, _handle(ctx, (1, 2))], ZERO)
    good.h = fake.h = None


def test_one_map_serves_every_frame():
    from wct_tf_amd._lib import mask_labels_frames
    m = np.arange(12).reshape(3, 4) % 2
    out = mask_labels_frames(m, 2, 5, (3, 4))
    assert out.shape == (5, 3, 4) and out.dtype == np.uint8 and out.flags['C_CONTIGUOUS'] and all(np.array_equal(o, m) for o in out)
    per_frame = [m, 1 - m]
    assert np.array_equal(mask_labels_frames(per_frame, 2, 2, (3, 4)), np.uint8(np.stack(per_frame)))


def _touch(d, names):
    d.mkdir()
    for n in names:
        (d / n).write_bytes(b'')
    return str(d)


def test_video_maps_are_matched_to_frames_in_sorted_order(tmp_path):
    from wct_tf_amd.stylize_video import list_frames, match_masks
    frames = list_frames(_touch(tmp_path / 'clip', ['frame_10.png', 'frame_2.png', 'frame_1.png']))
    maps = match_masks(_touch(tmp_path / 'maps', ['m_2.png', 'm_10.png', 'm_1.png']), frames)
    assert [os.path.basename(f) for f in frames] == ['frame_1.png', 'frame_2.png', 'frame_10.png']
    assert [os.path.basename(m) for m in maps] == ['m_1.png', 'm_2.png', 'm_10.png']
    one = str(tmp_path / 'maps' / 'm_1.png')
    assert match_masks(one, frames) == [one] * 3
    with pytest.raises(ValueError, match='2 label maps .* for 3 frames'):
        match_masks(_touch(tmp_path / 'few', ['a.png', 'b.png']), frames)


def test_video_count_check_comes_before_the_gpu(tmp_path, monkeypatch):
    from wct_tf_amd import stylize_video

    def no_model(*a, **k):
        raise AssertionError('the model was built before the label maps were counted')
    monkeypatch.setattr(stylize_video, 'WCT', no_model)
    clip = _touch(tmp_path / 'clip', ['frame_1.png', 'frame_2.png'])
    maps = _touch(tmp_path / 'maps', ['m_1.png'])
    with pytest.raises(ValueError, match='1 label maps .* for 2 frames'):
        stylize_video.main(['--relu-targets', 'relu1_1', '--in-path', clip, '--out-path', str(tmp_path / 'o'), '--mask-path', maps,
                            '--mask-styles', 'a.png', 'b.png', '--synthetic-weights', '1'])


BASE = ['--relu-targets', 'relu1_1', '--in-path', 'clip', '--out-path', 'o', '--synthetic-weights', '1']


def test_video_flags():
    from wct_tf_amd.stylize_video import build_parser, check_mask_args
    p = build_parser()
    args = p.parse_args(BASE + ['--mask-path', 'maps', '--mask-styles', 'a.png', 'b.png'])
    check_mask_args(p, args)
    assert args.mask_path == 'maps' and args.mask_styles == ['a.png', 'b.png'] and args.style_path is None
    check_mask_args(p, p.parse_args(BASE + ['--style-path', 's.png']))


@pytest.mark.parametrize('extra', [
    [],                                                                  # neither --style-path nor a mask
    ['--mask-path', 'maps'],
    ['--mask-styles', 'a.png'],
    ['--mask-path', 'maps', '--mask-styles', 'a.png', '--style-path', 's.png'],
    ['--mask-path', 'maps', '--mask-styles', 'a.png', 'b.png', '--keep-colors'],
    ['--mask-path', 'maps', '--mask-styles', 'a.png', 'b.png', '--swap5'],
    ['--mask-path', 'maps', '--mask-styles', 'a.png', 'b.png', '--concat'],
    ['--mask-path', 'maps', '--mask-styles'] + ['s%d.png' % k for k in range(9)],
])
def test_video_flag_errors(extra):
    from wct_tf_amd.stylize_video import build_parser, check_mask_args
    p = build_parser()
    with pytest.raises(SystemExit):
        check_mask_args(p, p.parse_args(BASE + extra))
