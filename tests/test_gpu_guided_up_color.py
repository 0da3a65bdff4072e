"""Guided upsampling under the colour guide on the GPU (csrc/guided_up_color.hip): the stand-alone op against the NumPy oracle
(tests/guided_up_color_oracle.py), the grey guide through the new entry points against the old ones, the fused driver and
WCT.predict / predict_frames against the composition of the stand-alone calls (resize -> stylize_prepared -> guided_upsample ->
content_colors), the refusals of the C ABI, and both command lines.  Everything is np.array_equal: the rule is integers only."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle
import guided_oracle
import guided_up_oracle as grey_oracle
import guided_up_color_oracle as oracle
from guided_up_oracle import CASES
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
MODES = [dict(), dict(wct_mode='np'), dict(adain=True)]
GU = (40, 2, 65, 'color')          # the driver cases: short side 40, a 5 x 5 box, eps 0.001, the colour guide
# the tilings: the full-size kernel's wave owns 128 columns (2 per lane) x 16 rows and its block 64 rows; the means pass's block
# owns SEG rows of a strip of 256 - 2r columns.  The full-size kernel has two load / store paths: whole 16-bit words (W even and
# 2-byte aligned bases) and bytes (any W, any base)
TILE_W, TILE_H, SEG = 128, 64, 64
strip = lambda r: 256 - 2 * r
ARG = -2
GREY, COLOR = 0, 1


@pytest.fixture(scope='module')
def ctx():
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


def _triple(seed, h, w, hc, wc, H, W, batch=None):
    lead = () if batch is None else (batch,)
    return _noise(seed, *lead, h, w, 3), _noise(seed + 100, *lead, hc, wc, 3), _noise(seed + 200, *lead, H, W, 3)


# ---- the stand-alone op ----------------------------------------------------------------------------------------------------------
def _op_dev(ctx, s, c, f, r, eps_q, offset=0, guide='color'):
    """wct_guided_upsample_guide_batch_dev on device buffers of its own; offset: every base moved by that many bytes.  The inputs
    are read back and compared: the call leaves them alone."""
    arrs = [np.ascontiguousarray(a if a.ndim == 4 else a[None]) for a in (s, c, f)]
    s, c, f = arrs
    bufs = [ctx.dev_alloc(a.nbytes + 16) for a in arrs] + [ctx.dev_alloc(f.nbytes + 16)]
    ds, dc, df, do = [C.c_void_p(b.value + offset) for b in bufs]
    try:
        for d, a in zip((ds, dc, df), arrs):
            ctx.h2d(d, a)
        ctx.guided_upsample_batch_dev(ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], df, f.shape[1], f.shape[2], s.shape[0], r, eps_q, do,
                                      guide=guide)
        ctx.sync()
        out = np.empty_like(f)
        ctx.d2h(out, do)
        for d, a in zip((ds, dc, df), arrs):
            kept = np.empty_like(a)
            ctx.d2h(kept, d)
            assert np.array_equal(kept, a)
    finally:
        for b in bufs:
            ctx.dev_free(b)
    return out


@pytest.mark.parametrize('case', CASES, ids=str)
def test_op_is_the_oracle(ctx, case):
    h, w, hc, wc, H, W, r, eps_q = case
    s, c, f = _triple(1, h, w, hc, wc, H, W)
    want = oracle.guided_upsample(s, c, f, r, eps_q)
    assert np.array_equal(_op_dev(ctx, s, c, f, r, eps_q)[0], want)
    assert np.array_equal(ctx.guided_upsample(s, c, f, r, eps_q, guide='color'), want)              # the host call
    from wct_tf_amd.ops import guided_upsample_np
    assert np.array_equal(guided_upsample_np(s, c, f, r, eps_q, ctx=ctx, guide='color'), want)
    s, c, f = grey_oracle.case(2, h, w, hc, wc, H, W)                                               # a smooth content with edges
    assert np.array_equal(ctx.guided_upsample(s, c, f, r, eps_q, guide='color'), oracle.guided_upsample(s, c, f, r, eps_q))


def test_the_grey_guide_through_the_new_entry_points_is_the_old_calls(ctx):
    lib, p = ctx.lib, lambda a: a.ctypes.data_as(_lib._U8)
    for H, W in ((50, 70), (52, 72), (9, 13)):
        s, c, f = _triple(9, 16, 20, 9, 13, H, W)
        want = grey_oracle.guided_upsample(s, c, f, 3, 650)
        old, new = np.empty_like(f), np.empty_like(f)
        assert lib.wct_guided_upsample(ctx.h, p(s), 16, 20, p(c), 9, 13, p(f), H, W, 3, 650, p(old)) == 0
        assert lib.wct_guided_upsample_guide(ctx.h, p(s), 16, 20, p(c), 9, 13, p(f), H, W, 3, 650, GREY, p(new)) == 0
        assert np.array_equal(old, want) and np.array_equal(new, want)
        assert np.array_equal(ctx.guided_upsample(s, c, f, 3, 650), want)                           # guide='grey' is the default
        assert np.array_equal(_op_dev(ctx, s, c, f, 3, 650, guide='grey')[0], want)
        assert not np.array_equal(ctx.guided_upsample(s, c, f, 3, 650, guide='color'), want)


# one column and one row past the full-size kernel's tile -- on the byte path (W odd) and on the word path (W even), at ratio 1 and
# above it --, and one column past the means pass's strip and one row past its segment
PAST = [(33, 35, 33, 35, TILE_H + 1, TILE_W + 1, 2), (33, 35, 33, 35, TILE_H + 2, TILE_W + 2, 2),
        (TILE_H + 1, TILE_W + 1, TILE_H + 1, TILE_W + 1, TILE_H + 1, TILE_W + 1, 3),
        (TILE_H + 1, TILE_W + 2, TILE_H + 1, TILE_W + 2, TILE_H + 1, TILE_W + 2, 3),
        (SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, 4),
        (SEG + 1, strip(4) + 1, SEG - 2, strip(4) - 1, 2 * SEG + 7, 2 * strip(4) + 2, 4)]
assert PAST[4][:6] == (65, 249, 65, 249, 65, 249) and PAST[5][:6] == (65, 249, 62, 247, 135, 498)


@pytest.mark.parametrize('case', PAST, ids=str)
def test_op_past_the_tiles(ctx, case):
    h, w, hc, wc, H, W, r = case
    s, c, f = _triple(3, h, w, hc, wc, H, W)
    assert np.array_equal(_op_dev(ctx, s, c, f, r, 650)[0], oracle.guided_upsample(s, c, f, r, 650))


def test_op_on_three_different_frames(ctx):
    for H, W in ((50, 71), (50, 70)):                                                # the byte path and the word path
        s, c, f = _triple(4, 16, 20, 9, 13, H, W, batch=3)
        want = oracle.guided_upsample(s, c, f, 3, 100)
        assert len({want[i].tobytes() for i in range(3)}) == 3
        assert np.array_equal(ctx.guided_upsample_batch(s, c, f, 3, 100, guide='color'), want)
        assert np.array_equal(_op_dev(ctx, s, c, f, 3, 100), want)


@pytest.mark.parametrize('offset', [4, 2, 1])
def test_op_on_moved_bases(ctx, offset):
    """4 and 2 bytes off: the word path keeps its alignment (W even) and the byte path runs as ever (W odd); 1 byte off: W even
    takes the byte path too"""
    for H, W in ((66, 72), (67, 71)):
        s, c, f = _triple(5, 33, 35, 33, 35, H, W)
        assert np.array_equal(_op_dev(ctx, s, c, f, 2, 650, offset=offset)[0], oracle.guided_upsample(s, c, f, 2, 650)), (H, W)


def test_op_constant_frames_and_the_clamp(ctx):
    _, c, f = _triple(7, 20, 24, 20, 24, 77, 101)
    for value in (0, 77, 255):
        assert (ctx.guided_upsample(np.full((20, 24, 3), value, np.uint8), c, f, 4, 650, guide='color') == value).all()
    s, c = guided_oracle.clamp_case()
    s = s.copy()
    s[..., 1] = 255 - s[..., 1]                                                      # the overshoot of this channel goes below 0
    f = np.repeat(np.repeat(c, 3, 0), 3, 1)
    raw = oracle.guided_upsample_unclamped(s, c, f, 1, 1)
    assert (raw < 0).any() and (raw > 255).any()
    assert np.array_equal(ctx.guided_upsample(s, c, f, 1, 1, guide='color'), np.clip(raw, 0, 255).astype(np.uint8))


def test_op_brings_back_an_isoluminant_step(ctx):
    s, c, f = oracle.isoluminant_step()
    up = ctx.guided_upsample(s, c, f, 2, 65, guide='color')
    assert np.array_equal(up, oracle.guided_upsample(s, c, f, 2, 65))
    assert (up[:, 83].astype(int) - up[:, 82]).min() > 120


# ---- the refusals of the C ABI ---------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    s, c, f = _triple(8, 16, 20, 9, 13, 40, 61)
    out = np.empty_like(f)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    want = oracle.guided_upsample(s, c, f, 4, 650)

    def good():
        ctx.sync()
        assert np.array_equal(ctx.guided_upsample(s, c, f, 4, 650, guide='color'), want)

    def refused(rc, word):
        assert rc == ARG and word in lib.wct_last_error(), lib.wct_last_error()

    up = lambda s_, h_, w_, c_, hc_, wc_, f_, H_, W_, r_, e_, o_, g_=COLOR: \
        lib.wct_guided_upsample_guide(h, s_, h_, w_, c_, hc_, wc_, f_, H_, W_, r_, e_, g_, o_)
    for g in (2, -1, 77):
        refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out), g), b'guide')
    good()
    for r in (0, 65, -1):
        refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, r, 650, p(out)), b'radius')
    for e in (0, 65026, -5):
        refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, e, p(out)), b'eps_q')
    good()
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 8, 61, 4, 650, p(out)), b'H x W')               # H < hc
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 12, 4, 650, p(out)), b'H x W')              # W < wc
    refused(up(p(s), 8, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'h x w')               # h < hc
    refused(up(p(s), 16, 12, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'h x w')              # w < wc
    good()
    refused(up(None, 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'stylized')
    refused(up(p(s), 16, 20, None, 9, 13, p(f), 40, 61, 4, 650, p(out)), b'content_small')
    refused(up(p(s), 16, 20, p(c), 9, 13, None, 40, 61, 4, 650, p(out)), b'content_full')
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, None), b'out')
    assert lib.wct_guided_upsample_guide(None, p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, COLOR, p(out)) == ARG
    good()
    buf = ctx.dev_alloc(f.nbytes * 2)
    other = C.c_void_p(buf.value + f.nbytes)
    try:
        dev = lambda *a: lib.wct_guided_upsample_guide_batch_dev(h, *a)
        for b in (0, -1, 33):
            refused(dev(buf, 16, 20, buf, 9, 13, buf, 40, 61, b, 4, 650, COLOR, other), b'B =')
        refused(dev(buf, 16, 20, buf, 9, 13, buf, 40, 61, 1, 4, 650, 5, other), b'guide')
        refused(dev(None, 16, 20, buf, 9, 13, buf, 40, 61, 1, 4, 650, COLOR, other), b'stylized')
        good()
        refused(dev(buf, 16, 20, buf, 9, 13, buf, 1 << 15, 1 << 15, 1, 4, 650, COLOR, other), b'2^31')
        for k in (0, 1, 2):                                                         # out over each input in turn
            ins = [other, other, other]
            ins[k] = buf
            refused(dev(ins[0], 16, 20, ins[1], 9, 13, ins[2], 40, 61, 1, 4, 650, COLOR, buf), b'overlaps')
    finally:
        ctx.dev_free(buf)
    good()


def test_driver_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    img, sty = synthetic_image(10, 96, 130), synthetic_image(11, 64, 72)
    lv = (C.c_int * 3)(3, 2, 1)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    out = np.empty_like(img)
    with ctx.prepare_style(sty, SMALL) as handle:
        want = ctx.stylize_prepared_upsampled(img, handle, SMALL, (40, 54), 2, 65, guide='color')
        call = lambda H=96, W=130, hc=40, wc=54, flags=0, r=2, e=65, g=COLOR, c=p(img), o=p(out), st=handle.h: \
            lib.wct_stylize_prepared_upsampled_guide(h, c, H, W, hc, wc, st, lv, 3, 1.0, flags, r, e, g, o)
        for kw, word in ((dict(g=2), b'guide'), (dict(g=-1), b'guide'), (dict(hc=97), b'H x W'), (dict(r=0), b'radius'), (dict(e=0), b'eps_q'),
                         (dict(flags=_lib.FLAG_GUIDED), b'WCT_FLAG_GUIDED'), (dict(flags=_lib.FLAG_IMAGES_F32), b'WCT_FLAG_IMAGES_F32'),
                         (dict(c=None), b'null'), (dict(o=None), b'null')):
            assert call(**kw) == ARG, kw
            assert word in lib.wct_last_error(), (kw, lib.wct_last_error())
            ctx.sync()
            assert call() == 0 and np.array_equal(out, want), kw
        buf = ctx.dev_alloc(img.nbytes * 2)
        try:
            dev = lambda B=1, g=COLOR, o=C.c_void_p(buf.value + img.nbytes): \
                lib.wct_stylize_prepared_upsampled_guide_batch_dev(h, buf, 96, 130, B, 40, 54, handle.h, lv, 3, 1.0, 0, 2, 65, g, o)
            for B in (0, 33):
                assert dev(B=B) == ARG and b'B =' in lib.wct_last_error()
            assert dev(g=9) == ARG and b'guide' in lib.wct_last_error()
            assert dev(o=C.c_void_p(buf.value + 12)) == ARG and b'overlaps' in lib.wct_last_error()
        finally:
            ctx.dev_free(buf)
        assert np.array_equal(ctx.stylize_prepared_upsampled(img, handle, SMALL, (40, 54), 2, 65, guide='color'), want)
        grey = ctx.stylize_prepared_upsampled(img, handle, SMALL, (40, 54), 2, 65)
        assert call(g=GREY) == 0 and np.array_equal(out, grey) and not np.array_equal(grey, want)
        old = np.empty_like(img)
        assert lib.wct_stylize_prepared_upsampled(h, p(img), 96, 130, 40, 54, handle.h, lv, 3, 1.0, 0, 2, 65, p(old)) == 0
        assert np.array_equal(old, grey)


# ---- the driver == the composition of the stand-alone calls ------------------------------------------------------------------------
def _composition(ctx, img, handle, work, r, eps_q, colors, **kw):
    small = ctx.resize(img, work) if tuple(work) != img.shape[:2] else img
    plain = ctx.stylize_prepared(small, handle, SMALL, alpha=0.8, **kw)
    up = ctx.guided_upsample(plain, small, img, r, eps_q, guide='color')
    assert np.array_equal(up, oracle.guided_upsample(plain, small, img, r, eps_q))
    return ctx.content_colors(up, img) if colors else up


@pytest.mark.parametrize('kw', MODES, ids=['tf', 'np', 'adain'])
def test_driver_is_the_composition(ctx, kw):
    img, sty = synthetic_image(20, 96, 130), synthetic_image(21, 80, 64)
    work = (40, 54)
    assert utils.resize_shape(96, 130, 40) == work
    with ctx.prepare_style(sty, SMALL, **kw) as handle:
        for colors in (False, True):
            want = _composition(ctx, img, handle, work, 2, 65, colors, **kw)
            got = ctx.stylize_prepared_upsampled(img, handle, SMALL, work, 2, 65, alpha=0.8, content_colors=colors, guide='color', **kw)
            assert got.shape == img.shape and np.array_equal(got, want), (kw, colors)
        assert not np.array_equal(want, img)


def test_driver_on_three_frames_and_at_the_working_size(ctx):
    frames = np.stack([synthetic_image(30 + i, 96, 130) for i in range(3)])
    with ctx.prepare_style(synthetic_image(29, 80, 64), SMALL) as handle:
        for colors in (False, True):
            want = np.stack([_composition(ctx, f, handle, (40, 54), 2, 65, colors) for f in frames])
            got = ctx.stylize_prepared_upsampled_batch(frames, handle, SMALL, (40, 54), 2, 65, alpha=0.8, content_colors=colors, guide='color')
            assert np.array_equal(got, want), colors
        small = synthetic_image(35, 40, 52)                                          # H == hc, W == wc: no resize
        assert np.array_equal(ctx.stylize_prepared_upsampled(small, handle, SMALL, (40, 52), 2, 65, alpha=0.8, guide='color'),
                              _composition(ctx, small, handle, (40, 52), 2, 65, False))


def test_driver_takes_float_contents_at_the_working_size(ctx):
    """WCT_FLAG_IMAGES_F32 without a resize: all three kernels read the fp32 content under the output rule (W even and W odd: the
    word path and the byte path of the full-size kernel)"""
    lv = (C.c_int * 3)(3, 2, 1)
    with ctx.prepare_style(synthetic_image(41, 64, 72), SMALL) as handle:
        for H, W in ((44, 52), (44, 53)):
            c = synthetic_image(40, H, W).astype(np.float64) * 0.9 + 3.3
            c32 = np.ascontiguousarray(c / 255., np.float32)
            c_u8 = colors_oracle.quantise(c32)
            plain = ctx.stylize_prepared(c, handle, SMALL, alpha=0.8)                    # (at W = 53 the frame is 44 x 56: padding)
            up = oracle.guided_upsample(plain, c_u8, c_u8, 2, 65)
            out = np.empty((H, W, 3), np.uint8)
            for flags, want in ((_lib.FLAG_IMAGES_F32, up), (_lib.FLAG_IMAGES_F32 | _lib.FLAG_CONTENT_COLORS, colors_oracle.content_colors(up, c_u8))):
                assert ctx.lib.wct_stylize_prepared_upsampled_guide(ctx.h, c32.ctypes.data_as(_lib._U8), H, W, H, W, handle.h, lv, 3, 0.8,
                                                                    flags, 2, 65, COLOR, out.ctypes.data_as(_lib._U8)) == 0
                assert np.array_equal(out, want), (W, flags)


@pytest.mark.parametrize('batch', [1, 3])
def test_predict_and_predict_frames(model, batch):
    frames = np.stack([synthetic_image(50 + i, 96, 130) for i in range(batch)])
    sty = synthetic_image(49, 80, 64)
    sess = model.sess
    for colors in (False, True):
        with model.prepare_style(sty) as handle:
            want = np.stack([_composition(sess, f, handle, (40, 54), 2, 65, colors) for f in frames])
            assert np.array_equal(model.predict_frames(frames, handle, alpha=0.8, batch=batch, guided_upsample=GU, content_colors=colors), want)
        assert np.array_equal(model.predict_frames(frames, sty, alpha=0.8, batch=2, guided_upsample=GU, content_colors=colors), want)
        assert np.array_equal(model.predict(frames[0], sty, 0.8, guided_upsample=GU, content_colors=colors), want[0])
    assert np.array_equal(model.predict(frames[0], sty, 0.8, guided_upsample=GU[:3] + ('grey',)),
                          model.predict(frames[0], sty, 0.8, guided_upsample=GU[:3]))


# ---- the command lines, end to end -----------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def _cli_model():
    from wct_tf_amd.wct import WCT
    return WCT(None, TARGETS, None, weights=synthetic_weights(42, relu_targets=TARGETS))


def test_stylize_cli(tmp_path):
    from wct_tf_amd.stylize import main
    img, style = synthetic_image(70, 96, 130), synthetic_image(71, 56, 48)
    utils.save_img(str(tmp_path / 'c.png'), img)
    utils.save_img(str(tmp_path / 's.png'), style)
    base = ['--relu-targets'] + TARGETS + ['--content-path', str(tmp_path / 'c.png'), '--style-path', str(tmp_path / 's.png'), '--alpha', '0.8',
                                          '--synthetic-weights', '42', '--guided-radius', '2', '--guided-eps', '0.001', '--content-size', '40',
                                          '--guided-upsample', '--guided-upsample-guide', 'color']
    assert main(base + ['--out-path', str(tmp_path / 'one')]) == 1
    assert main(base + ['--out-path', str(tmp_path / 'two'), '--content-colors']) == 1
    m = _cli_model()
    try:
        one, two = utils.get_img(str(tmp_path / 'one' / 'c_s.png')), utils.get_img(str(tmp_path / 'two' / 'c_s.png'))
        assert one.shape == img.shape == two.shape                                   # the output has the content's size
        small = m.sess.resize(img, (40, 54))
        want = oracle.guided_upsample(m.predict(small, style, 0.8), small, img, 2, 65)
        assert np.array_equal(one, want)
        assert np.array_equal(two, colors_oracle.content_colors(want, img))
    finally:
        m.sess.close()


def test_stylize_video_cli(tmp_path):
    from wct_tf_amd.stylize_video import main
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    a, b = synthetic_image(72, 96, 130).astype(np.float32), synthetic_image(73, 96, 130).astype(np.float32)
    frames = np.stack([a * (1 - t) + b * t for t in np.linspace(0, 0.3, 3)]).astype(np.uint8)
    for i in range(3):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), frames[i])
    style = synthetic_image(74, 56, 48)
    utils.save_img(str(tmp_path / 's0.png'), style)
    assert main(['--relu-targets'] + TARGETS + ['--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '42', '--batch', '2',
                                                '--style-path', str(tmp_path / 's0.png'), '--guided-radius', '2', '--guided-eps', '0.001',
                                                '--content-size', '40', '--guided-upsample', '--guided-upsample-guide', 'color',
                                                '--out-path', str(tmp_path / 'out')]) == 3
    m = _cli_model()
    try:
        for i in range(3):
            small = m.sess.resize(frames[i], (40, 54))
            want = oracle.guided_upsample(m.predict(small, style, 0.8), small, frames[i], 2, 65)
            got = utils.get_img(str(tmp_path / 'out' / 'clip_s0' / ('frame_%d.png' % (i + 1))))
            assert got.shape == frames[i].shape and np.array_equal(got, want), i
    finally:
        m.sess.close()
