"""The colour guide of guided smoothing on the GPU (csrc/guided_color.hip): the stand-alone op against the NumPy oracle
(tests/guided_color_oracle.py) on the geometry of tests/test_gpu_guided.py, the grey guide through the new entry points against the
old ones, the flag at the end of the stylize chain against the op applied to the unflagged frame -- on every path that ends in
stylize_levels --, the refusals of the C ABI, and both command lines.  Everything is np.array_equal: the rule is integers only."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle
import guided_color_oracle as oracle
import guided_oracle as grey
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
MODES = [dict(), dict(wct_mode='np'), dict(adain=True)]
G = (3, 650, 'color')              # the flag cases: a 7 x 7 box, eps 0.01, the colour guide
# the kernel's tiling: a block owns SEG rows of a strip of 256 - 2r columns
SEG = 64
strip = lambda r: 256 - 2 * r
# the geometry of tests/test_gpu_guided.py: 9 x 13 under a window that is the whole image; odd and even sizes under the smallest,
# a middle and the largest radius; frames larger than their content both ways; one column past a strip and one row past a segment
OP_CASES = [(9, 13, 9, 13, 16)] + [(h, w, h, w, r) for h, w in ((33, 35), (48, 48)) for r in (1, 4, 64)] + \
    [(16, 20, 9, 13, 4), (48, 48, 37, 41, 4), (SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, 4),
     (SEG + 1, strip(64) + 1, SEG - 3, strip(64) - 2, 64)]


def want(plain, content, g=G):
    return oracle.guided_filter(plain, content, g[0], g[1])


@pytest.fixture(scope='module')
def small_ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.set_weights(synthetic_weights(5, relu_targets=SMALL))
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
def _op_dev(ctx, s, c, r, eps_q, in_place, offset=0, guide='color'):
    """wct_guided_filter_guide_batch_dev on device buffers of its own: out a second buffer, or the stylized one; offset: every
    base moved by that many bytes"""
    s, c = np.ascontiguousarray(s), np.ascontiguousarray(c)
    if s.ndim == 3:
        s, c = s[None], c[None]
    bufs = [ctx.dev_alloc(s.nbytes + 16), ctx.dev_alloc(c.nbytes + 16), ctx.dev_alloc(s.nbytes + 16)]
    ds, dc, do = [C.c_void_p(b.value + offset) for b in bufs]
    try:
        ctx.h2d(ds, s)
        ctx.h2d(dc, c)
        ctx.guided_filter_batch_dev(ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r, eps_q, ds if in_place else do,
                                    guide=guide)
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


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('ho,wo,hc,wc,r', OP_CASES)
def test_op_is_the_oracle(small_ctx, ho, wo, hc, wc, r, in_place):
    s, c = _noise(1, ho, wo, 3), _noise(2, hc, wc, 3)
    ref = oracle.guided_filter(s, c, r, 650)
    assert np.array_equal(_op_dev(small_ctx, s, c, r, 650, in_place)[0], ref)
    if not in_place:
        assert np.array_equal(small_ctx.guided_filter(s, c, r, 650, guide='color'), ref)           # the host call
        from wct_tf_amd import guided_filter_np
        assert np.array_equal(guided_filter_np(s, c, r, 650, guide='color', ctx=small_ctx), ref)
        smooth_s, smooth_c = synthetic_image(3, ho, wo), synthetic_image(4, hc, wc)
        assert np.array_equal(small_ctx.guided_filter(smooth_s, smooth_c, r, 650, guide='color'), oracle.guided_filter(smooth_s, smooth_c, r, 650))


@pytest.mark.parametrize('eps_q', [1, 65025])
def test_op_at_both_ends_of_eps(small_ctx, eps_q):
    s, c = _noise(5, 48, 48, 3), _noise(6, 37, 41, 3)
    for r in (1, 4, 64):
        assert np.array_equal(small_ctx.guided_filter(s, c, r, eps_q, guide='color'), oracle.guided_filter(s, c, r, eps_q)), r
    flat = np.full((40, 44, 3), 200, np.uint8)
    assert np.array_equal(small_ctx.guided_filter(flat, _noise(7, 40, 44, 3), 64, eps_q, guide='color'), flat)      # a constant frame
    # full-range boards in opposite phase between the guide's channels: the largest covariances and det
    yy, xx = np.mgrid[:48, :52]
    board = ((yy + xx) & 1) * 255
    c = np.stack([board, 255 - board, board], -1).astype(np.uint8)
    s = np.repeat(board[..., None], 3, -1).astype(np.uint8)
    assert np.array_equal(small_ctx.guided_filter(s, c, 16, eps_q, guide='color'), oracle.guided_filter(s, c, 16, eps_q))


def test_op_on_the_isoluminant_step_and_the_two_greys_guide(small_ctx):
    s, c, _ = oracle.isoluminant_step()
    got = small_ctx.guided_filter(s, c, 4, 65, guide='color')
    assert np.array_equal(got, oracle.guided_filter(s, c, 4, 65))
    assert not np.array_equal(got, small_ctx.guided_filter(s, c, 4, 65))                 # the grey guide blurs the edge
    xx = np.mgrid[:40, :44][1]
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    for frame in ((xx & 1) * 255, 255 - (xx & 1) * 255):                                 # the largest a_q of either sign
        s, c = rgb(frame), rgb(100 + (xx & 1) * 2)
        assert np.array_equal(small_ctx.guided_filter(s, c, 4, 1, guide='color'), oracle.guided_filter(s, c, 4, 1))


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_op_on_bases_one_byte_off_alignment(small_ctx, in_place):
    s, c = _noise(8, 48, 48, 3), _noise(9, 37, 44, 3)
    assert np.array_equal(_op_dev(small_ctx, s, c, 4, 650, in_place, offset=1)[0], oracle.guided_filter(s, c, 4, 650))


def test_op_on_three_different_frames(small_ctx):
    s, c = _noise(10, 3, 40, 52, 3), _noise(11, 3, 33, 52, 3)
    ref = oracle.guided_filter(s, c, 5, 100)
    assert len({ref[i].tobytes() for i in range(3)}) == 3
    assert np.array_equal(small_ctx.guided_filter_batch(s, c, 5, 100, guide='color'), ref)
    assert np.array_equal(_op_dev(small_ctx, s, c, 5, 100, True), ref)


def test_op_on_a_full_batch(small_ctx):
    s, c = _noise(12, 32, 33, 35, 3), _noise(13, 32, 33, 35, 3)
    assert np.array_equal(small_ctx.guided_filter_batch(s, c, 8, 650, guide='color'), oracle.guided_filter(s, c, 8, 650))


def test_op_on_an_fp32_content(small_ctx):
    """the flag's route for float images: the content is quantised by the output rule inside both kernels"""
    c = synthetic_image(17, 60, 52).astype(np.float64) * 0.9 + 3.3
    s = synthetic_image(18, 72, 64).astype(np.float64) * 0.8 + 7.7
    c_u8 = colors_oracle.quantise(np.asarray(c / 255., np.float32))
    assert not np.array_equal(c_u8, np.uint8(np.rint(c)))
    plain = small_ctx.stylize(c, s, SMALL, alpha=0.8)
    got = small_ctx.stylize(c, s, SMALL, alpha=0.8, guided=G)
    assert np.array_equal(got, want(plain, c_u8))
    assert np.array_equal(got, small_ctx.guided_filter(plain, c_u8, G[0], G[1], guide='color'))


def test_op_clamps(small_ctx):
    s, c = grey.clamp_case()
    raw = oracle.guided_filter_unclamped(s, c, 1, 1)
    assert ((raw < 0) | (raw > 255)).any()
    assert np.array_equal(small_ctx.guided_filter(s, c, 1, 1, guide='color'), np.clip(raw, 0, 255).astype(np.uint8))


def test_the_grey_guide_through_the_new_entry_points_is_the_old_entry_points(small_ctx):
    lib, h = small_ctx.lib, small_ctx.h
    p = lambda a: a.ctypes.data_as(_lib._U8)
    for (ho, wo, hc, wc, r) in (OP_CASES[0], OP_CASES[2], OP_CASES[7], OP_CASES[10]):
        s, c = _noise(20, ho, wo, 3), _noise(21, hc, wc, 3)
        old, new = np.empty_like(s), np.empty_like(s)
        assert lib.wct_guided_filter(h, p(s), ho, wo, p(c), hc, wc, r, 650, p(old)) == 0
        assert lib.wct_guided_filter_guide(h, p(s), ho, wo, p(c), hc, wc, r, 650, _lib.GUIDE_GREY, p(new)) == 0
        assert np.array_equal(new, old) and np.array_equal(old, grey.guided_filter(s, c, r, 650))
        assert np.array_equal(_op_dev(small_ctx, s, c, r, 650, True, guide='grey')[0], old)
        assert np.array_equal(small_ctx.guided_filter(s, c, r, 650), old)                  # the default of the Python call


# ---- flagged == op(unflagged) == oracle ----------------------------------------------------------------------------------------
def _flag_case(ctx, c, s, levels, **kw):
    plain = ctx.stylize(c, s, levels, alpha=0.8, **kw)
    got = ctx.stylize(c, s, levels, alpha=0.8, guided=G, **kw)
    ref = want(plain, c)
    assert got.shape == plain.shape
    assert np.array_equal(got, ref), (levels, kw)
    assert np.array_equal(got, ctx.guided_filter(plain, c, G[0], G[1], guide='color')), (levels, kw)
    assert not np.array_equal(got, plain)                        # (the flag did something)
    assert not np.array_equal(got, grey.guided_filter(plain, c, G[0], G[1]))        # ... and not what the grey guide does
    both = ctx.stylize(c, s, levels, alpha=0.8, guided=G, content_colors=True, **kw)
    assert np.array_equal(both, colors_oracle.content_colors(ref, c)), (levels, kw)      # the colour op runs last
    return plain


@pytest.mark.parametrize('kw', MODES, ids=['tf', 'np', 'adain'])
def test_flag_single_level_odd_sizes(small_ctx, kw):
    plain = _flag_case(small_ctx, synthetic_image(11, 33, 35), synthetic_image(12, 40, 36), ['relu1_1'], **kw)
    assert plain.shape == (33, 35, 3)


def test_flag_three_levels_frame_larger_than_content(small_ctx):
    plain = _flag_case(small_ctx, synthetic_image(13, 98, 83), synthetic_image(14, 90, 70), SMALL)
    assert plain.shape == (100, 84, 3)                           # clamped rows and columns of the guide


def test_flag_settings_follow_the_call(small_ctx):
    """the guide of a call is the call's, not an earlier one's: the two-element form means grey again"""
    c, s = synthetic_image(19, 48, 52), synthetic_image(20, 48, 48)
    plain = small_ctx.stylize(c, s, SMALL, alpha=0.8)
    for g in ((1, 1, 'color'), (5, 100), (64, 65025, 'color'), (5, 100, 'grey'), (5, 100, 'color')):
        ref = want(plain, c, g) if g[2:] == ('color',) else grey.guided_filter(plain, c, g[0], g[1])
        assert np.array_equal(small_ctx.stylize(c, s, SMALL, alpha=0.8, guided=g), ref), g
    assert np.array_equal(small_ctx.stylize(c, s, SMALL, alpha=0.8), plain)
    # the context's own setting, read by the flag of the C call
    lib, h = small_ctx.lib, small_ctx.h
    p = lambda a: a.ctypes.data_as(_lib._U8)
    lv = (C.c_int * 3)(3, 2, 1)
    got = np.empty_like(plain)
    small_ctx.set_guided(5, 100)
    for name, ref in (('color', oracle.guided_filter(plain, c, 5, 100)), ('grey', grey.guided_filter(plain, c, 5, 100))):
        small_ctx.set_guided_guide(name)
        assert lib.wct_stylize(h, p(c), 48, 52, p(s), 48, 48, lv, 3, 0.8, _lib.FLAG_GUIDED, p(got)) == 0
        assert np.array_equal(got, ref), name


def test_prepared_handle(small_ctx):
    c, s = synthetic_image(21, 100, 84), synthetic_image(22, 90, 70)
    with small_ctx.prepare_style(s, SMALL) as h:
        for kw in MODES:
            plain = small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, **kw)
            got = small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, guided=G, **kw)
            assert np.array_equal(got, want(plain, c)), kw
            assert np.array_equal(got, small_ctx.stylize(c, s, SMALL, alpha=0.8, guided=G, **kw)), kw


@pytest.mark.parametrize('batch', [1, 3])
def test_predict_frames(model, batch):
    frames = np.stack([synthetic_image(30 + i, 60, 68) for i in range(batch)])
    s = synthetic_image(29, 80, 64)
    ref = want(model.predict_frames(frames, s, alpha=0.8, batch=batch), frames)
    assert np.array_equal(model.predict_frames(frames, s, alpha=0.8, batch=batch, guided=G), ref)     # shared style
    with model.prepare_style(s) as h:
        assert np.array_equal(model.predict_frames(frames, h, alpha=0.8, batch=batch, guided=G), ref)
        both = model.predict_frames(frames, h, alpha=0.8, batch=batch, guided=G, content_colors=True)
        assert np.array_equal(both, colors_oracle.content_colors(ref, frames))
    styles = np.stack([synthetic_image(40 + i, 64, 64) for i in range(batch)])                           # a style per frame
    plain = model.sess.stylize_batch(frames, styles, SMALL, alpha=0.8)
    assert np.array_equal(model.sess.stylize_batch(frames, styles, SMALL, alpha=0.8, guided=G), want(plain, frames))


def test_predict_and_predict_mix_and_predict_masked(model):
    c = synthetic_image(50, 100, 84)
    styles = [synthetic_image(51, 90, 70), synthetic_image(52, 64, 96)]
    mask = np.zeros((100, 84), np.uint8)
    mask[:, 40:] = 1
    assert np.array_equal(model.predict(c, styles[0], 0.8, guided=G), want(model.predict(c, styles[0], 0.8), c))
    mix = want(model.predict_mix(c, styles, [1, 3], 0.8), c)
    masked = want(model.predict_masked(c, styles, mask, 0.8), c)
    assert np.array_equal(model.predict_mix(c, styles, [1, 3], 0.8, guided=G), mix)
    assert np.array_equal(model.predict_masked(c, styles, mask, 0.8, guided=G), masked)
    handles = [model.prepare_style(s) for s in styles]
    try:
        assert np.array_equal(model.predict_mix(c, handles, [1, 3], 0.8, guided=G), mix)
        assert np.array_equal(model.predict_masked(c, handles, mask, 0.8, guided=G), masked)
    finally:
        for h in handles:
            h.close()


def test_predict_frames_masked(model):
    frames = np.stack([synthetic_image(60 + i, 60, 68) for i in range(3)])
    styles = [synthetic_image(58, 80, 64), synthetic_image(59, 64, 72)]
    masks = np.zeros((3, 60, 68), np.uint8)
    for f in range(3):
        masks[f, :, 20 + 8 * f:] = 1
    ref = want(model.predict_frames_masked(frames, styles, masks, 0.8, batch=3), frames)
    assert np.array_equal(model.predict_frames_masked(frames, styles, masks, 0.8, batch=3, guided=G), ref)


def test_predict_frames_warm_and_strength(model):
    """warm runs are bit-reproducible: the flagged run from a fresh state against the unflagged run from a fresh state"""
    frames = np.stack([synthetic_image(70, 64, 64).astype(np.float32) * (1 - t) + synthetic_image(71, 64, 64) * t
                       for t in np.linspace(0, 0.3, 4)]).astype(np.uint8)
    smap = np.tile(np.linspace(0, 255, 64).astype(np.uint8), (64, 1))
    with model.prepare_style(synthetic_image(72, 80, 80)) as h:
        with model.warm_state() as w:
            plain = model.predict_frames(frames, h, alpha=0.8, batch=2, warm=w)
        with model.warm_state() as w:
            got = model.predict_frames(frames, h, alpha=0.8, batch=2, warm=w, guided=G)
        assert np.array_equal(got, want(plain, frames))
        plain = model.predict(frames[0], h, 0.8, strength=smap)
        assert np.array_equal(model.predict(frames[0], h, 0.8, strength=smap, guided=G), want(plain, frames[0]))
        plain = model.predict_frames(frames, h, alpha=0.8, batch=2, strengths=smap)
        assert np.array_equal(model.predict_frames(frames, h, alpha=0.8, batch=2, strengths=smap, guided=G), want(plain, frames))


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib, h = small_ctx.lib, small_ctx.h
    s, c = _noise(80, 16, 20, 3), _noise(81, 9, 20, 3)
    out = np.empty_like(s)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    ARG = -2
    ref = oracle.guided_filter(s, c, 4, 650)

    def good():
        small_ctx.sync()
        assert np.array_equal(small_ctx.guided_filter(s, c, 4, 650, guide='color'), ref)

    small_ctx.set_guided_guide('color')
    for guide in (2, -1, 64):
        assert lib.wct_guided_filter_guide(h, p(s), 16, 20, p(c), 9, 20, 4, 650, guide, p(out)) == ARG          # a bad guide
        assert b'WCT_GUIDE_COLOR' in lib.wct_last_error()
        assert lib.wct_set_guided_guide(h, guide) == ARG
        good()
    assert lib.wct_set_guided_guide(None, 1) == ARG
    K = _lib.GUIDE_COLOR
    for r, e, word in ((0, 650, b'radius'), (65, 650, b'radius'), (4, 0, b'eps_q'), (4, 65026, b'eps_q')):
        assert lib.wct_guided_filter_guide(h, p(s), 16, 20, p(c), 9, 20, r, e, K, p(out)) == ARG
        assert word in lib.wct_last_error()
    assert lib.wct_guided_filter_guide(h, p(c), 9, 20, p(s), 16, 20, 4, 650, K, p(out)) == ARG            # Ho < Hc
    assert b'guided filter' in lib.wct_last_error()
    assert lib.wct_guided_filter_guide(h, None, 16, 20, p(c), 9, 20, 4, 650, K, p(out)) == ARG
    assert lib.wct_guided_filter_guide(h, p(s), 16, 20, p(c), 9, 20, 4, 650, K, None) == ARG
    assert lib.wct_guided_filter_guide(None, p(s), 16, 20, p(c), 9, 20, 4, 650, K, p(out)) == ARG
    buf = small_ctx.dev_alloc(s.nbytes)
    try:
        for b in (0, -1, 33):
            assert lib.wct_guided_filter_guide_batch_dev(h, buf, 16, 20, buf, 16, 20, b, 4, 650, K, buf) == ARG
        assert lib.wct_guided_filter_guide_batch_dev(h, None, 16, 20, buf, 16, 20, 1, 4, 650, K, buf) == ARG
        assert lib.wct_guided_filter_guide_batch_dev(h, buf, 16, 20, buf, 16, 20, 1, 4, 650, 7, buf) == ARG
        assert lib.wct_guided_filter_guide_batch_dev(h, buf, 1 << 15, 1 << 15, buf, 16, 20, 1, 4, 650, K, buf) == ARG     # 2^31 bytes and more
        assert b'2^31' in lib.wct_last_error()
    finally:
        small_ctx.dev_free(buf)
    good()
    # the refused settings left the flag's guide as it was: colour
    img, sty = synthetic_image(82, 48, 48), synthetic_image(83, 48, 48)
    plain = small_ctx.stylize(img, sty, SMALL)
    small_ctx.set_guided(2, 9)
    small_ctx.set_guided_guide('color')
    assert lib.wct_set_guided_guide(h, 9) == ARG
    lv = (C.c_int * 3)(3, 2, 1)
    got = np.empty_like(plain)
    assert lib.wct_stylize(h, p(img), 48, 48, p(sty), 48, 48, lv, 3, 1.0, _lib.FLAG_GUIDED, p(got)) == 0
    assert np.array_equal(got, oracle.guided_filter(plain, img, 2, 9))
    small_ctx.set_guided_guide('grey')


def test_banded_texture_and_wrap_drivers_refuse_the_flag(small_ctx):
    lib, h = small_ctx.lib, small_ctx.h
    ARG = -2
    img, sty = synthetic_image(84, 48, 48), synthetic_image(85, 48, 48)
    lv = (C.c_int * 3)(3, 2, 1)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    out = np.empty((48, 48, 3), np.uint8)
    F = _lib.FLAG_GUIDED
    with small_ctx.prepare_style(sty, SMALL) as handle:
        plain = small_ctx.stylize_prepared(img, handle, SMALL)
        ref = want(plain, img)
        buf = small_ctx.dev_alloc(out.nbytes)
        try:
            calls = [
                lambda: lib.wct_stylize_prepared_banded(h, p(img), 48, 48, handle.h, lv, 3, 1.0, F, 16, 0, p(out)),
                lambda: lib.wct_stylize_prepared_banded_dev(h, buf, 48, 48, handle.h, lv, 3, 1.0, F, 16, 0, buf),
                lambda: lib.wct_texture_prepared(h, 48, 48, 1, 0, 0, handle.h, lv, 3, 1, 1.0, F, p(out)),
                lambda: lib.wct_texture_prepared_batch_dev(h, 48, 48, 1, 1, 0, 0, handle.h, lv, 3, 1, 1.0, F, buf),
                lambda: lib.wct_stylize_prepared_wrap(h, p(img), 48, 48, handle.h, lv, 3, 1.0, F, p(out)),
                lambda: lib.wct_stylize_prepared_wrap_batch_dev(h, buf, 48, 48, 1, handle.h, lv, 3, 1.0, F, buf),
                lambda: lib.wct_texture_prepared_wrap(h, 48, 48, 1, 0, 0, handle.h, lv, 3, 1, 1.0, F, p(out)),
                lambda: lib.wct_texture_prepared_wrap_batch_dev(h, 48, 48, 1, 1, 0, 0, handle.h, lv, 3, 1, 1.0, F, buf),
            ]
            for call in calls:
                small_ctx.set_guided_guide('color')
                assert call() == ARG
                assert b'WCT_FLAG_GUIDED' in lib.wct_last_error(), lib.wct_last_error()
                small_ctx.sync()
                assert np.array_equal(small_ctx.stylize_prepared(img, handle, SMALL, guided=G), ref)      # a good call on the same context
        finally:
            small_ctx.dev_free(buf)
            small_ctx.set_guided_guide('grey')
        assert np.array_equal(small_ctx.stylize_prepared_banded(img, handle, SMALL, band_rows=16), plain)  # and the drivers still run


# ---- the command lines, end to end ------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def _cli_model():
    from wct_tf_amd.wct import WCT
    return WCT(None, TARGETS, None, weights=synthetic_weights(42, relu_targets=TARGETS))


def test_stylize_cli_one_and_two_passes(tmp_path):
    from wct_tf_amd.stylize import main
    img, style = synthetic_image(90, 50, 46), synthetic_image(92, 56, 48)
    utils.save_img(str(tmp_path / 'c.png'), img)
    utils.save_img(str(tmp_path / 's.png'), style)
    base = ['--relu-targets'] + TARGETS + ['--content-path', str(tmp_path / 'c.png'), '--style-path', str(tmp_path / 's.png'), '--alpha', '0.8',
                                          '--synthetic-weights', '42', '--guided-radius', '4', '--guided-guide', 'color']
    assert main(base + ['--out-path', str(tmp_path / 'one')]) == 1
    assert main(base + ['--out-path', str(tmp_path / 'two'), '--passes', '2', '--guided-eps', '0.001', '--content-colors']) == 1
    m = _cli_model()
    try:
        first = m.predict(img, style, 0.8)
        one = utils.get_img(str(tmp_path / 'one' / 'c_s.png'))
        assert np.array_equal(one, oracle.guided_filter(first, img, 4, 650))
        # two passes: both plain, then the filter and the colour op once each, against the ORIGINAL content
        two = utils.get_img(str(tmp_path / 'two' / 'c_s.png'))
        assert np.array_equal(two, colors_oracle.content_colors(oracle.guided_filter(m.predict(first, style, 0.8), img, 4, 65), img))
    finally:
        m.sess.close()


def test_stylize_video_cli_one_and_two_passes(tmp_path):
    from wct_tf_amd.stylize_video import main
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    a, b = synthetic_image(93, 48, 64).astype(np.float32), synthetic_image(94, 48, 64).astype(np.float32)
    frames = np.stack([a * (1 - t) + b * t for t in np.linspace(0, 0.3, 3)]).astype(np.uint8)
    for i in range(3):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), frames[i])
    style = synthetic_image(95, 56, 48)
    utils.save_img(str(tmp_path / 's0.png'), style)
    base = ['--relu-targets'] + TARGETS + ['--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '42', '--batch', '2',
                                          '--style-path', str(tmp_path / 's0.png'), '--guided-radius', '4', '--guided-guide', 'color']
    assert main(base + ['--out-path', str(tmp_path / 'one')]) == 3
    assert main(base + ['--out-path', str(tmp_path / 'two'), '--passes', '2']) == 3
    m = _cli_model()
    try:
        first = m.predict_frames(frames, style, 0.8, batch=2)
        one = oracle.guided_filter(first, frames, 4, 650)
        two = oracle.guided_filter(m.predict_frames(first, style, 0.8, batch=2), frames, 4, 650)
        for i in range(3):
            assert np.array_equal(utils.get_img(str(tmp_path / 'one' / 'clip_s0' / ('frame_%d.png' % (i + 1)))), one[i]), i
            assert np.array_equal(utils.get_img(str(tmp_path / 'two' / 'clip_s0' / ('frame_%d.png' % (i + 1)))), two[i]), i
    finally:
        m.sess.close()
