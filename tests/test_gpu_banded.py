"""Banded stylization on the GPU (csrc/banded.hip): the banded encoder and decoder give the whole pass's bits, the chunked
transform meets the tolerances of the whole one (and IS the whole one at one chunk), banded frames equal whole-image frames
bit for bit at stat_rows = 0 and do not depend on band_rows at any stat_rows, and a content past the 8.4 MP launch limit
comes back as a frame."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, ROOT, rel_err
from wct_tf_amd import _lib
from wct_tf_amd._lib import WCTHipError
from wct_tf_amd.weights import synthetic_features, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
ALL = ['relu5_1', 'relu4_1', 'relu3_1', 'relu2_1', 'relu1_1']
WCT_TOL = 1e-3                       # the gate of tests/test_gpu_ops.py on the golden files
ALPHA = 0.8


@pytest.fixture(scope='module')
def small_ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.set_weights(synthetic_weights(5, relu_targets=SMALL))
    yield c
    c.close()


@pytest.fixture(scope='module')
def full_ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.set_weights(synthetic_weights(7))
    yield c
    c.close()


# ---- 1. the banded encoder and decoder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('level,H,W,band_rows', [(1, 50, 20, 16), (2, 70, 22, 16), (3, 150, 26, 32), (4, 210, 20, 48), (5, 437, 36, 64)])
def test_banded_encode_and_decode_are_the_whole_pass_bit_for_bit(full_ctx, level, H, W, band_rows):
    """Every output element has the operands of the whole pass in the same order: bit identity, no tolerance."""
    target = 'relu%d_1' % level
    img = np.float32(synthetic_image(60 + level, H, W)) / np.float32(255)
    feat = full_ctx.encode(img, target)
    out = full_ctx.decode(feat, target)
    for rows in (band_rows, (H + 15) // 16 * 16, 0):                  # several bands; band_rows >= H; automatic (one band)
        got = full_ctx.encode_banded(img, target, rows)
        bad = np.argwhere(got != feat)
        assert bad.size == 0, ('encode', target, rows, len(bad), bad[:4].tolist())
        dgot = full_ctx.decode_banded(feat, target, rows)
        bad = np.argwhere(dgot != out)
        assert bad.size == 0, ('decode', target, rows, len(bad), bad[:4].tolist())


# ---- 2. the chunked transform --------------------------------------------------------------------------------------------------
def _golden_cases():
    cases = []
    z = np.load(os.path.join(GOLDEN, 'wct_np_reference.npz'))
    for n in sorted({k.split('/')[0] for k in z.files}):
        alpha = float(z[n + '/alpha'])
        cases.append(('np/' + n, z[n + '/content'], z[n + '/style'], z[n + '/out'], 0.6 if alpha < 0 else alpha, _lib.WCT_NP))
    z = np.load(os.path.join(GOLDEN, 'wct_tf_reference.npz'))
    for n in sorted({k.split('/')[0] for k in z.files}):
        cases.append(('tf/' + n, z[n + '/content'], z[n + '/style'], z[n + '/out'], float(z[n + '/alpha']), _lib.WCT_TF))
    return cases


def _chunked_case(ctx, tag, fc, fs, ref, alpha, mode, log):
    c = fc.shape[-1]
    x, s = fc.reshape(-1, c), fs.reshape(-1, c)
    n = len(x)
    whole = ctx.transform(x, s, alpha, mode)
    for rows in (0, n, n + 5):                                        # one chunk IS wct_transform
        assert np.array_equal(ctx.transform_chunked(x, s, alpha, mode, rows), whole), (tag, rows)
    for chunks in (2, 7, 40):
        rows = -(-n // chunks)
        if rows < 2:
            continue
        got = ctx.transform_chunked(x, s, alpha, mode, rows)
        line = '%-28s N %6d C %3d  %2d chunks of %5d rows: vs reference %.3e (whole: %.3e)  vs whole %.3e' % (
            tag, n, c, -(-n // rows), rows, rel_err(got, ref.reshape(-1, c)), rel_err(whole, ref.reshape(-1, c)), rel_err(got, whole))
        print(line)
        log.append(line)
        assert rel_err(got, ref.reshape(-1, c)) < WCT_TOL, line


def test_chunked_transform_on_the_golden_cases_and_large_maps(full_ctx):
    log = []
    for tag, fc, fs, ref, alpha, mode in _golden_cases():
        _chunked_case(full_ctx, tag, fc, fs, ref, alpha, mode, log)
    for c, h, w in ((64, 512, 512), (512, 32, 32)):                   # (C, N) = (64, 262144), (512, 1024)
        fc, fs = synthetic_features(300 + c, c, h, w, 2.0), synthetic_features(400 + c, c, 24, 40, 2.0)
        _chunked_case(full_ctx, 'np/synthetic', fc, fs, oracle.wct_np(fc, fs, ALPHA), ALPHA, _lib.WCT_NP, log)
        _chunked_case(full_ctx, 'tf/synthetic', fc, fs, oracle.wct_tf(fc, fs, ALPHA), ALPHA, _lib.WCT_TF, log)
    with open(os.path.join(ROOT, 'profiles', 'banded_identity.txt'), 'w') as f:        # recorded, not gated
        f.write('wct_transform_chunked against the reference outputs and against wct_transform (rel_err; tests/test_gpu_banded.py)\n')
        f.write('\n'.join(log) + '\n')
    with pytest.raises(WCTHipError, match='at least 2 rows'):
        full_ctx.transform_chunked(np.zeros((64, 64), np.float32), np.zeros((64, 64), np.float32), 1.0, _lib.WCT_NP, 1)


# ---- 3. frames, stat_rows = 0: the whole-image frame ---------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(100, 84), (150, 70)])
def test_banded_frames_are_the_whole_image_frames_bit_for_bit(small_ctx, size):
    content = synthetic_image(500, *size)
    with small_ctx.prepare_style(synthetic_image(501, 80, 72), SMALL) as h:
        for kw in (dict(), dict(wct_mode='np'), dict(content_colors=True)):
            want = small_ctx.stylize_prepared(content, h, SMALL, alpha=ALPHA, **kw)
            for rows in (16, 32, 48, 0):
                got = small_ctx.stylize_prepared_banded(content, h, SMALL, alpha=ALPHA, band_rows=rows, **kw)
                assert got.shape == want.shape and np.array_equal(got, want), (size, kw, rows, int((got != want).sum()))
        f = np.float32(content) + np.float32(0.25)                     # a float content goes as fp32 in [0,1] (WCT_FLAG_IMAGES_F32)
        want = small_ctx.stylize_prepared(f, h, SMALL, alpha=ALPHA)
        assert np.array_equal(small_ctx.stylize_prepared_banded(f, h, SMALL, alpha=ALPHA, band_rows=32), want)


def test_banded_frames_at_five_levels(full_ctx):
    content = synthetic_image(510, 437, 40)
    with full_ctx.prepare_style(synthetic_image(511, 96, 80), ALL) as h:
        want = full_ctx.stylize_prepared(content, h, ALL, alpha=ALPHA)
        got = full_ctx.stylize_prepared_banded(content, h, ALL, alpha=ALPHA, band_rows=64)
        assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


# ---- 4. frames, stat_rows = 5: pooled statistics -------------------------------------------------------------------------------
def test_pooled_frames_do_not_depend_on_the_bands(small_ctx):
    content = synthetic_image(520, 150, 70)
    with small_ctx.prepare_style(synthetic_image(521, 80, 72), SMALL) as h:
        frames = [small_ctx.stylize_prepared_banded(content, h, SMALL, alpha=ALPHA, band_rows=rows, stat_rows=5) for rows in (16, 32, 48)]
        assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])
        whole = small_ctx.stylize_prepared(content, h, SMALL, alpha=ALPHA)
        d = np.abs(frames[0].astype(int) - whole.astype(int))
        print('stat_rows = 5 against the whole-image frame: max %d LSB, mean %.4f' % (d.max(), d.mean()))


def test_pooled_frames_are_no_further_from_the_oracle_than_whole_ones():
    """the bound of tests/test_gpu_warm.py::assert_no_worse_than_cold, on the contractive net: no further from the oracle frame
    than the whole-image frame, plus 1 LSB in the maximum and 0.05 LSB in the mean"""
    from oracle.contractive import contractive_weights
    from wct_tf_amd.context import Context
    w = contractive_weights(7)
    ctx = Context(0)
    try:
        ctx.set_weights(w)
        content, style = synthetic_image(903, 100, 84), synthetic_image(902, 80, 96)
        want = oracle.stylize(content, style, w, SMALL, alpha=ALPHA)
        with ctx.prepare_style(style, SMALL) as h:
            whole = ctx.stylize_prepared(content, h, SMALL, alpha=ALPHA)
            got = ctx.stylize_prepared_banded(content, h, SMALL, alpha=ALPHA, band_rows=32, stat_rows=5)
        dw, dg = np.abs(whole.astype(int) - want.astype(int)), np.abs(got.astype(int) - want.astype(int))
        print('against the oracle: whole max %d mean %.4f | stat_rows = 5 max %d mean %.4f' % (dw.max(), dw.mean(), dg.max(), dg.mean()))
        assert dg.max() <= dw.max() + 1 and dg.mean() <= dw.mean() + 0.05
    finally:
        ctx.close()


# ---- 5. the limit is lifted ----------------------------------------------------------------------------------------------------
def test_a_content_past_the_launch_limit_comes_back_as_a_frame():
    from wct_tf_amd import WCT
    targets = ['relu1_1']
    model = WCT(None, targets, None, weights=synthetic_weights(5, relu_targets=targets))
    try:
        content = np.ascontiguousarray(np.tile(synthetic_image(530, 290, 290), (10, 10, 1)))          # 2900 x 2900: 8.41 MP
        style = synthetic_image(531, 96, 96)
        assert model.sess.band_rows(2900, 2900, targets) > 0
        with model.prepare_style(style) as h:
            with pytest.raises(WCTHipError):                               # the whole-image call: WCT_STATUS_ARG, as before
                model.sess.stylize_prepared(content, h, targets, alpha=ALPHA)
            auto = model.predict(content, h, alpha=ALPHA)
            assert auto.shape == model.sess.output_size(2900, 2900, targets) + (3,) and auto.dtype == np.uint8
            assert auto.min() != auto.max() and auto.std() > 1             # not a constant frame
            assert np.array_equal(model.predict(content, h, alpha=ALPHA, band_rows=512), auto)
            # just below the limit (8 386 816 pixels) the routing says "whole", the whole-image call agrees, and the bands give its frame
            below = np.ascontiguousarray(content[:2896, :2896])
            assert model.sess.band_rows(2896, 2896, targets) == 0
            assert np.array_equal(model.predict(below, h, alpha=ALPHA, band_rows=512), model.predict(below, h, alpha=ALPHA))
            small = synthetic_image(532, 64, 64)                           # and the context goes on with small images
            assert np.array_equal(model.predict(small, h, alpha=ALPHA), model.predict(small, h, alpha=ALPHA, band_rows=16))
    finally:
        model.sess.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(small_ctx):
    import ctypes as C
    content = synthetic_image(540, 64, 64)
    arr = (C.c_int * 3)(3, 2, 1)
    out = np.empty((64, 64, 3), np.uint8)
    u8p = lambda a: a.ctypes.data_as(_lib._U8)
    with small_ctx.prepare_style(synthetic_image(541, 64, 64), SMALL) as h, small_ctx.prepare_style(synthetic_image(542, 64, 64), SMALL[:2]) as h2:
        want = small_ctx.stylize_prepared(content, h, SMALL, alpha=ALPHA)

        def call(style=h, flags=0, band_rows=16, stat_rows=0):
            return small_ctx.lib.wct_stylize_prepared_banded(small_ctx.h, u8p(content), 64, 64, style.h if hasattr(style, 'h') else style,
                                                             arr, 3, ALPHA, flags, band_rows, stat_rows, u8p(out))
        for kw in (dict(flags=_lib.FLAG_ADAIN), dict(flags=_lib.FLAG_SWAP5), dict(flags=_lib.FLAG_STYLE_SHARED), dict(band_rows=24),
                   dict(band_rows=-16), dict(stat_rows=-1), dict(style=h2)):
            assert call(**kw) == -2, kw                                    # WCT_STATUS_ARG
            assert call() == 0 and np.array_equal(out, want), kw           # and the context stylizes afterwards
        gone = small_ctx.prepare_style(synthetic_image(543, 64, 64), SMALL)
        handle = gone.h
        gone.close()
        assert call(style=handle) == -3                                    # WCT_STATUS_STATE: not a live handle
        assert call() == 0 and np.array_equal(out, want)
