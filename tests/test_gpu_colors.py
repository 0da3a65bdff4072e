"""Luminance-only colour preservation on the GPU (csrc/colors.hip): the stand-alone op against the NumPy oracle
(tests/colors_oracle.py), the flag fused into the stylize chain against the oracle applied to the unflagged frame -- on every
path that ends in stylize_levels -- the refusals of the C ABI, and both command lines.  Everything is np.array_equal: the rule
is integers only.  Synthetic weights as in tests/test_gpu_prepared.py."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle as oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
MODES = [dict(), dict(wct_mode='np'), dict(adain=True)]


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


@pytest.fixture(scope='module')
def model():
    from wct_tf_amd.wct import WCT
    m = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    yield m
    m.sess.close()


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


# ---- the stand-alone op --------------------------------------------------------------------------------------------------
def _op_dev(ctx, s, c, in_place, offset=0):
    """wct_content_colors_batch_dev on device buffers of its own: out a second buffer, or the stylized one; offset: every base
    moved by that many bytes (off the alignment of the wide accesses)"""
    s, c = np.ascontiguousarray(s), np.ascontiguousarray(c)
    if s.ndim == 3:
        s, c = s[None], c[None]
    bufs = [ctx.dev_alloc(s.nbytes + 16), ctx.dev_alloc(c.nbytes + 16), ctx.dev_alloc(s.nbytes + 16)]
    ds, dc, do = [C.c_void_p(b.value + offset) for b in bufs]
    try:
        ctx.h2d(ds, s)
        ctx.h2d(dc, c)
        ctx.content_colors_batch_dev(ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], ds if in_place else do)
        ctx.sync()
        out, kept = np.empty_like(s), np.empty_like(s)
        ctx.d2h(out, ds if in_place else do)
        ctx.d2h(kept, ds)
        if not in_place:
            assert np.array_equal(kept, s)                       # the input is left alone
    finally:
        for b in bufs:
            ctx.dev_free(b)
    return out


# the smallest shapes that take the wide body (W % 4 == 0), rows that are no multiple of four bytes (35 * 3 = 105: sample by
# sample, and a 3-pixel tail group), columns past the content (41 < 48, one group straddling it), rows past it, and both
OP_SIZES = [(48, 48, 48, 48), (48, 48, 37, 41), (33, 35, 33, 35), (16, 20, 9, 20)]


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('ho,wo,hc,wc', OP_SIZES)
def test_op_is_the_oracle(small_ctx, ho, wo, hc, wc, in_place):
    s, c = _noise(1, ho, wo, 3), _noise(2, hc, wc, 3)            # full-range noise: about a third of the pixels clip
    want = oracle.content_colors(s, c)
    assert np.array_equal(_op_dev(small_ctx, s, c, in_place)[0], want)
    if not in_place:
        assert np.array_equal(small_ctx.content_colors(s, c), want)                  # the host call
        from wct_tf_amd import content_colors_np
        assert np.array_equal(content_colors_np(s, c, ctx=small_ctx), want)
        smooth_s, smooth_c = synthetic_image(3, ho, wo), synthetic_image(4, hc, wc)
        assert np.array_equal(small_ctx.content_colors(smooth_s, smooth_c), oracle.content_colors(smooth_s, smooth_c))


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_op_on_bases_off_the_wide_alignment(small_ctx, in_place):
    """W % 4 == 0 but every pointer one byte off: the launch must notice and go sample by sample"""
    s, c = _noise(5, 48, 48, 3), _noise(6, 37, 44, 3)
    assert np.array_equal(_op_dev(small_ctx, s, c, in_place, offset=1)[0], oracle.content_colors(s, c))


def test_op_batched_past_the_grid_cap(small_ctx):
    """32 frames of 256 x 256: twice the groups the capped grid holds at once, and a frame stride on both images"""
    s, c = _noise(7, 32, 256, 256, 3), _noise(8, 32, 200, 256, 3)
    want = oracle.content_colors(s, c)
    assert np.array_equal(small_ctx.content_colors_batch(s, c), want)
    assert np.array_equal(_op_dev(small_ctx, s, c, False), want)


# ---- fused == op(unfused) == oracle ----------------------------------------------------------------------------------------
def _fused_case(ctx, c, s, levels, content_u8=None, **kw):
    plain = ctx.stylize(c, s, levels, alpha=0.8, **kw)
    fused = ctx.stylize(c, s, levels, alpha=0.8, content_colors=True, **kw)
    content_u8 = c if content_u8 is None else content_u8
    assert fused.shape == plain.shape
    assert np.array_equal(fused, oracle.content_colors(plain, content_u8)), (levels, kw)
    assert np.array_equal(fused, ctx.content_colors(plain, content_u8)), (levels, kw)
    assert not np.array_equal(fused, plain)                      # (the flag did something)
    return plain


@pytest.mark.parametrize('kw', MODES, ids=['tf', 'np', 'adain'])
def test_fused_single_level_odd_sizes(small_ctx, kw):
    plain = _fused_case(small_ctx, synthetic_image(11, 33, 35), synthetic_image(12, 40, 36), ['relu1_1'], **kw)
    assert plain.shape == (33, 35, 3)                            # Ho == Hc, rows of 105 bytes


@pytest.mark.parametrize('kw', MODES, ids=['tf', 'np', 'adain'])
def test_fused_three_levels_frame_larger_than_content(small_ctx, kw):
    _fused_case(small_ctx, synthetic_image(13, 100, 84), synthetic_image(14, 90, 70), SMALL, **kw)
    # 98 -> 49 -> 25 rows and 83 -> 42 -> 21 columns at relu3_1, x 4: the frame is larger than its content both ways
    plain = _fused_case(small_ctx, synthetic_image(13, 98, 83), synthetic_image(14, 90, 70), SMALL, **kw)
    assert plain.shape == (100, 84, 3)                           # clamped rows and columns


@pytest.mark.parametrize('kw', MODES, ids=['tf', 'np', 'adain'])
def test_fused_five_levels(full_ctx, kw):
    _fused_case(full_ctx, synthetic_image(15, 96, 96), synthetic_image(16, 112, 80), RELU_TARGETS, **kw)


def test_fused_float_images_are_quantised_by_the_output_rule(small_ctx):
    c = synthetic_image(17, 100, 84).astype(np.float64) * 0.9 + 3.3
    s = synthetic_image(18, 72, 64).astype(np.float64) * 0.8 + 7.7
    c_u8 = oracle.quantise(np.asarray(c / 255., np.float32))     # what Context.stylize hands over, under the output rule
    assert not np.array_equal(c_u8, np.uint8(np.rint(c)))        # (truncation, not rounding: the case pins the rule)
    _fused_case(small_ctx, c, s, SMALL, content_u8=c_u8)


def test_fused_with_swap5(full_ctx):
    full_ctx.set_style_swap(0.6, 3, 1)
    _fused_case(full_ctx, synthetic_image(19, 96, 80), synthetic_image(20, 80, 96), ['relu5_1', 'relu3_1', 'relu1_1'], swap5=True)


# ---- every path honours the flag -------------------------------------------------------------------------------------------
def test_prepared_handle(small_ctx):
    c, s = synthetic_image(21, 100, 84), synthetic_image(22, 90, 70)
    with small_ctx.prepare_style(s, SMALL) as h:
        for kw in MODES:
            plain = small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, **kw)
            got = small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, content_colors=True, **kw)
            assert np.array_equal(got, oracle.content_colors(plain, c)), kw
            assert np.array_equal(got, small_ctx.stylize(c, s, SMALL, alpha=0.8, content_colors=True, **kw)), kw


@pytest.mark.parametrize('batch', [1, 8])
def test_predict_frames(model, batch):
    frames = np.stack([synthetic_image(30 + i, 60, 68) for i in range(batch)])
    s = synthetic_image(29, 80, 64)
    want = oracle.content_colors(model.predict_frames(frames, s, alpha=0.8, batch=batch), frames)
    assert np.array_equal(model.predict_frames(frames, s, alpha=0.8, batch=batch, content_colors=True), want)     # shared style
    with model.prepare_style(s) as h:
        assert np.array_equal(model.predict_frames(frames, h, alpha=0.8, batch=batch, content_colors=True), want)
    # the per-pair batch (a style per frame)
    styles = np.stack([synthetic_image(40 + i, 64, 64) for i in range(batch)])
    plain = model.sess.stylize_batch(frames, styles, SMALL, alpha=0.8)
    assert np.array_equal(model.sess.stylize_batch(frames, styles, SMALL, alpha=0.8, content_colors=True),
                          oracle.content_colors(plain, frames))


def test_predict_and_predict_mix_and_predict_masked(model):
    c = synthetic_image(50, 100, 84)
    styles = [synthetic_image(51, 90, 70), synthetic_image(52, 64, 96)]
    mask = np.zeros((100, 84), np.uint8)
    mask[:, 40:] = 1
    assert np.array_equal(model.predict(c, styles[0], 0.8, content_colors=True), oracle.content_colors(model.predict(c, styles[0], 0.8), c))
    mix = oracle.content_colors(model.predict_mix(c, styles, [1, 3], 0.8), c)
    masked = oracle.content_colors(model.predict_masked(c, styles, mask, 0.8), c)
    assert np.array_equal(model.predict_mix(c, styles, [1, 3], 0.8, content_colors=True), mix)
    assert np.array_equal(model.predict_masked(c, styles, mask, 0.8, content_colors=True), masked)
    handles = [model.prepare_style(s) for s in styles]
    try:
        assert np.array_equal(model.predict_mix(c, handles, [1, 3], 0.8, content_colors=True), mix)
        assert np.array_equal(model.predict_masked(c, handles, mask, 0.8, content_colors=True), masked)
    finally:
        for h in handles:
            h.close()


def test_predict_frames_masked(model):
    frames = np.stack([synthetic_image(60 + i, 60, 68) for i in range(4)])
    styles = [synthetic_image(58, 80, 64), synthetic_image(59, 64, 72)]
    masks = np.zeros((4, 60, 68), np.uint8)
    for f in range(4):
        masks[f, :, 20 + 8 * f:] = 1
    want = oracle.content_colors(model.predict_frames_masked(frames, styles, masks, 0.8, batch=4), frames)
    assert np.array_equal(model.predict_frames_masked(frames, styles, masks, 0.8, batch=4, content_colors=True), want)


def test_predict_frames_warm(model):
    """warm runs are bit-reproducible: the flagged run from a fresh state against the unflagged run from a fresh state"""
    frames = np.stack([synthetic_image(70, 64, 64).astype(np.float32) * (1 - t) + synthetic_image(71, 64, 64) * t
                       for t in np.linspace(0, 0.3, 6)]).astype(np.uint8)
    with model.prepare_style(synthetic_image(72, 80, 80)) as h:
        with model.warm_state() as w:
            plain = model.predict_frames(frames, h, alpha=0.8, batch=2, warm=w)
        with model.warm_state() as w:
            got = model.predict_frames(frames, h, alpha=0.8, batch=2, warm=w, content_colors=True)
            assert all(w.valid(t) for t in SMALL)
    assert np.array_equal(got, oracle.content_colors(plain, frames))


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib, h = small_ctx.lib, small_ctx.h
    s, c = _noise(80, 16, 20, 3), _noise(81, 9, 20, 3)
    out = np.empty_like(s)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    ARG = -2
    assert lib.wct_content_colors(h, p(c), 9, 20, p(s), 16, 20, p(out)) == ARG                    # Ho < Hc
    assert b'content colours' in lib.wct_last_error()
    assert lib.wct_content_colors(h, p(s), 16, 12, p(c), 9, 20, p(out)) == ARG                    # Wo < Wc
    assert lib.wct_content_colors(h, None, 16, 20, p(c), 9, 20, p(out)) == ARG
    assert lib.wct_content_colors(h, p(s), 16, 20, None, 9, 20, p(out)) == ARG
    assert lib.wct_content_colors(h, p(s), 16, 20, p(c), 9, 20, None) == ARG
    assert lib.wct_content_colors(None, p(s), 16, 20, p(c), 9, 20, p(out)) == ARG
    assert lib.wct_content_colors(h, p(s), 16, 20, p(c), 0, 20, p(out)) == ARG
    buf = small_ctx.dev_alloc(s.nbytes)
    try:
        for b in (0, -1, 33):
            assert lib.wct_content_colors_batch_dev(h, buf, 16, 20, buf, 16, 20, b, buf) == ARG
        assert lib.wct_content_colors_batch_dev(h, None, 16, 20, buf, 16, 20, 1, buf) == ARG
        assert lib.wct_content_colors_batch_dev(h, buf, 16, 20, buf, 17, 20, 1, buf) == ARG
    finally:
        small_ctx.dev_free(buf)
    small_ctx.sync()
    assert np.array_equal(small_ctx.content_colors(s, c), oracle.content_colors(s, c))
    img, sty = synthetic_image(82, 48, 48), synthetic_image(83, 48, 48)
    assert np.array_equal(small_ctx.stylize(img, sty, SMALL, content_colors=True),
                          oracle.content_colors(small_ctx.stylize(img, sty, SMALL), img))


# ---- the command lines, end to end ------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def _cli_model():
    from wct_tf_amd.wct import WCT
    return WCT(None, TARGETS, None, weights=synthetic_weights(42, relu_targets=TARGETS))


def test_stylize_cli_folder_and_two_passes(tmp_path):
    from wct_tf_amd.stylize import main
    cdir = tmp_path / 'contents'
    cdir.mkdir()
    contents = {'a': synthetic_image(90, 50, 46), 'b': synthetic_image(91, 48, 64)}
    for name, img in contents.items():
        utils.save_img(str(cdir / (name + '.png')), img)
    style = synthetic_image(92, 56, 48)
    utils.save_img(str(tmp_path / 's.png'), style)
    base = ['--relu-targets'] + TARGETS + ['--content-path', str(cdir), '--style-path', str(tmp_path / 's.png'), '--alpha', '0.8',
                                          '--synthetic-weights', '42', '--content-colors']
    assert main(base + ['--out-path', str(tmp_path / 'one')]) == 2             # a folder: the style is prepared once
    assert main(base + ['--out-path', str(tmp_path / 'two'), '--passes', '2']) == 2
    m = _cli_model()
    try:
        for name, img in contents.items():
            first = m.predict(img, style, 0.8)
            assert first.shape[0] >= img.shape[0] and first.shape[1] >= img.shape[1]
            one = utils.get_img(str(tmp_path / 'one' / ('%s_s.png' % name)))    # the output names are unchanged
            assert np.array_equal(one, oracle.content_colors(first, img)), name
            # two passes: both plain, then the op once, against the ORIGINAL content
            two = utils.get_img(str(tmp_path / 'two' / ('%s_s.png' % name)))
            assert np.array_equal(two, oracle.content_colors(m.predict(first, style, 0.8), img)), name
    finally:
        m.sess.close()


def test_stylize_video_cli_warm_start_and_masks(tmp_path):
    from wct_tf_amd.stylize import mask_labels
    from wct_tf_amd.stylize_video import main
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    a, b = synthetic_image(93, 48, 64).astype(np.float32), synthetic_image(94, 48, 64).astype(np.float32)
    frames = np.stack([a * (1 - t) + b * t for t in np.linspace(0, 0.3, 5)]).astype(np.uint8)
    for i in range(5):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), frames[i])
    styles = [synthetic_image(95, 56, 48), synthetic_image(96, 48, 56)]
    for i, s in enumerate(styles):
        utils.save_img(str(tmp_path / ('s%d.png' % i)), s)
    grey = np.zeros((48, 64), np.uint8)
    grey[:, 30:] = 255
    utils.save_img(str(tmp_path / 'm.png'), np.repeat(grey[..., None], 3, axis=2))
    base = ['--relu-targets'] + TARGETS + ['--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '42', '--batch', '2',
                                          '--content-colors']
    assert main(base + ['--style-path', str(tmp_path / 's0.png'), '--out-path', str(tmp_path / 'warm'), '--warm-start']) == 5
    assert main(base + ['--mask-path', str(tmp_path / 'm.png'), '--mask-styles', str(tmp_path / 's0.png'), str(tmp_path / 's1.png'),
                        '--out-path', str(tmp_path / 'masked')]) == 5
    m = _cli_model()
    try:
        with m.prepare_style(styles[0]) as h, m.warm_state() as w:
            warm = oracle.content_colors(m.predict_frames(frames, h, 0.8, batch=2, warm=w), frames)
        masks = np.stack([mask_labels(grey, 2, (48, 64))] * 5)
        masked = oracle.content_colors(m.predict_frames_masked(frames, styles, masks, 0.8, batch=2), frames)
        for i in range(5):
            got = utils.get_img(str(tmp_path / 'warm' / 'clip_s0' / ('frame_%d.png' % (i + 1))))
            assert np.array_equal(got, warm[i]), i
            got = utils.get_img(str(tmp_path / 'masked' / 'clip_mask_s0+s1' / ('frame_%d.png' % (i + 1))))
            assert np.array_equal(got, masked[i]), i
    finally:
        m.sess.close()
