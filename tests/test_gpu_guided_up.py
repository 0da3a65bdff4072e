"""Guided upsampling on the GPU (csrc/guided_up.hip): the stand-alone op against the NumPy oracle (tests/guided_up_oracle.py), the
fused driver and WCT.predict / predict_frames against the composition of the stand-alone calls (resize -> stylize_prepared ->
guided_upsample -> content_colors), the refusals of the C ABI, and both command lines.  Everything is np.array_equal: the rule is
integers only."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle
import guided_up_oracle as oracle
from guided_up_oracle import CASES
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
MODES = [dict(), dict(wct_mode='np'), dict(adain=True)]
GU = (40, 2, 65)                   # the driver cases: short side 40, a 5 x 5 box, eps 0.001
# the tilings: the full-size kernel's wave owns 256 columns x 16 rows and its block 64 rows; the means pass's block owns SEG rows
# of a strip of 256 - 2r columns
TILE_W, TILE_H, SEG = 256, 64, 64
strip = lambda r: 256 - 2 * r
ARG = -2


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
def _op_dev(ctx, s, c, f, r, eps_q, offset=0):
    """wct_guided_upsample_batch_dev on device buffers of its own; offset: every base moved by that many bytes.  The inputs are
    read back and compared: the call leaves them alone."""
    arrs = [np.ascontiguousarray(a if a.ndim == 4 else a[None]) for a in (s, c, f)]
    s, c, f = arrs
    bufs = [ctx.dev_alloc(a.nbytes + 16) for a in arrs] + [ctx.dev_alloc(f.nbytes + 16)]
    ds, dc, df, do = [C.c_void_p(b.value + offset) for b in bufs]
    try:
        for d, a in zip((ds, dc, df), arrs):
            ctx.h2d(d, a)
        ctx.guided_upsample_batch_dev(ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], df, f.shape[1], f.shape[2], s.shape[0], r, eps_q, do)
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
    assert np.array_equal(ctx.guided_upsample(s, c, f, r, eps_q), want)              # the host call
    from wct_tf_amd.ops import guided_upsample_np
    assert np.array_equal(guided_upsample_np(s, c, f, r, eps_q, ctx=ctx), want)
    s, c, f = oracle.case(2, h, w, hc, wc, H, W)                                     # a smooth content with edges
    assert np.array_equal(ctx.guided_upsample(s, c, f, r, eps_q), oracle.guided_upsample(s, c, f, r, eps_q))


# one column and one row past the full-size kernel's tile -- on the byte path (W odd) and on the dword path (W % 4 == 0), at ratio 1
# and above it --, and one column past the means pass's strip and one row past its segment
PAST = [(33, 35, 33, 35, TILE_H + 1, TILE_W + 1, 2), (33, 35, 33, 35, TILE_H + 4, TILE_W + 4, 2),
        (TILE_H + 1, TILE_W + 4, TILE_H + 1, TILE_W + 4, TILE_H + 1, TILE_W + 4, 3),
        (SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, 4),
        (SEG + 1, strip(4) + 1, SEG - 2, strip(4) - 1, 2 * SEG + 7, 2 * strip(4) + 2, 4)]


@pytest.mark.parametrize('case', PAST, ids=str)
def test_op_past_the_tiles(ctx, case):
    h, w, hc, wc, H, W, r = case
    s, c, f = _triple(3, h, w, hc, wc, H, W)
    assert np.array_equal(_op_dev(ctx, s, c, f, r, 650)[0], oracle.guided_upsample(s, c, f, r, 650))


def test_op_on_three_different_frames(ctx):
    for H, W in ((50, 70), (52, 72)):                                                # the byte path and the dword path
        s, c, f = _triple(4, 16, 20, 9, 13, H, W, batch=3)
        want = oracle.guided_upsample(s, c, f, 3, 100)
        assert len({want[i].tobytes() for i in range(3)}) == 3
        assert np.array_equal(ctx.guided_upsample_batch(s, c, f, 3, 100), want)
        assert np.array_equal(_op_dev(ctx, s, c, f, 3, 100), want)


def test_op_on_bases_four_bytes_off(ctx):
    s, c, f = _triple(5, 33, 35, 33, 35, 66, 72)
    assert np.array_equal(_op_dev(ctx, s, c, f, 2, 650, offset=4)[0], oracle.guided_upsample(s, c, f, 2, 650))
    s, c, f = _triple(6, 33, 35, 33, 35, 67, 71)
    assert np.array_equal(_op_dev(ctx, s, c, f, 2, 650, offset=4)[0], oracle.guided_upsample(s, c, f, 2, 650))


def test_op_constant_frames_and_the_clamp(ctx):
    _, c, f = _triple(7, 20, 24, 20, 24, 77, 101)
    for value in (0, 77, 255):
        assert (ctx.guided_upsample(np.full((20, 24, 3), value, np.uint8), c, f, 4, 650) == value).all()
    import guided_oracle
    s, c = guided_oracle.clamp_case()
    f = np.repeat(np.repeat(c, 3, 0), 3, 1)
    raw = oracle.guided_upsample_unclamped(s, c, f, 1, 1)
    assert ((raw < 0) | (raw > 255)).any()
    assert np.array_equal(ctx.guided_upsample(s, c, f, 1, 1), np.clip(raw, 0, 255).astype(np.uint8))


# ---- the refusals of the C ABI ---------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    s, c, f = _triple(8, 16, 20, 9, 13, 40, 61)
    out = np.empty_like(f)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    want = oracle.guided_upsample(s, c, f, 4, 650)

    def good():
        ctx.sync()
        assert np.array_equal(ctx.guided_upsample(s, c, f, 4, 650), want)

    def refused(rc, word):
        assert rc == ARG and word in lib.wct_last_error(), lib.wct_last_error()

    up = lambda s_, h_, w_, c_, hc_, wc_, f_, H_, W_, r_, e_, o_: lib.wct_guided_upsample(h, s_, h_, w_, c_, hc_, wc_, f_, H_, W_, r_, e_, o_)
    for r in (0, 65, -1):
        refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, r, 650, p(out)), b'radius')
    for e in (0, 65026, -5):
        refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, e, p(out)), b'eps_q')
    good()
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 8, 61, 4, 650, p(out)), b'H x W')               # H < hc
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 12, 4, 650, p(out)), b'H x W')              # W < wc
    refused(up(p(s), 8, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'h x w')               # h < hc
    refused(up(p(s), 16, 12, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'h x w')              # w < wc
    refused(up(None, 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)), b'stylized')
    refused(up(p(s), 16, 20, None, 9, 13, p(f), 40, 61, 4, 650, p(out)), b'content_small')
    refused(up(p(s), 16, 20, p(c), 9, 13, None, 40, 61, 4, 650, p(out)), b'content_full')
    refused(up(p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, None), b'out')
    assert lib.wct_guided_upsample(None, p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 650, p(out)) == ARG
    good()
    buf = ctx.dev_alloc(f.nbytes * 2)
    other = C.c_void_p(buf.value + f.nbytes)
    try:
        dev = lambda *a: lib.wct_guided_upsample_batch_dev(h, *a)
        for b in (0, -1, 33):
            refused(dev(buf, 16, 20, buf, 9, 13, buf, 40, 61, b, 4, 650, other), b'B =')
        refused(dev(None, 16, 20, buf, 9, 13, buf, 40, 61, 1, 4, 650, other), b'stylized')
        refused(dev(buf, 16, 20, buf, 9, 13, buf, 1 << 15, 1 << 15, 1, 4, 650, other), b'2^31')
        for k in (0, 1, 2):                                                         # out over each input in turn
            ins = [other, other, other]
            ins[k] = buf
            refused(dev(ins[0], 16, 20, ins[1], 9, 13, ins[2], 40, 61, 1, 4, 650, buf), b'overlaps')
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
        want = ctx.stylize_prepared_upsampled(img, handle, SMALL, (40, 54), 2, 65)
        call = lambda H=96, W=130, hc=40, wc=54, flags=0, r=2, e=65, c=p(img), o=p(out), st=handle.h: \
            lib.wct_stylize_prepared_upsampled(h, c, H, W, hc, wc, st, lv, 3, 1.0, flags, r, e, o)
        for kw, word in ((dict(hc=97), b'H x W'), (dict(wc=131), b'H x W'), (dict(r=0), b'radius'), (dict(e=0), b'eps_q'),
                         (dict(flags=_lib.FLAG_GUIDED), b'WCT_FLAG_GUIDED'), (dict(flags=_lib.FLAG_IMAGES_F32), b'WCT_FLAG_IMAGES_F32'),
                         (dict(flags=_lib.FLAG_SWAP5), b'SWAP5'), (dict(c=None), b'null'), (dict(o=None), b'null')):
            assert call(**kw) == ARG, kw
            assert word in lib.wct_last_error(), (kw, lib.wct_last_error())
            ctx.sync()
            assert call() == 0 and np.array_equal(out, want), kw
        tall = _noise(12, 2000, 64, 3)                                               # 2000 rows to 40: what wct_resize refuses
        assert lib.wct_stylize_prepared_upsampled(h, p(tall), 2000, 64, 40, 64, handle.h, lv, 3, 1.0, 0, 2, 65, p(np.empty_like(tall))) == ARG
        assert b'resize' in lib.wct_last_error(), lib.wct_last_error()
        ctx.sync()
        assert call() == 0 and np.array_equal(out, want)
        buf = ctx.dev_alloc(img.nbytes * 2)
        try:
            dev = lambda B=1, o=C.c_void_p(buf.value + img.nbytes): \
                lib.wct_stylize_prepared_upsampled_batch_dev(h, buf, 96, 130, B, 40, 54, handle.h, lv, 3, 1.0, 0, 2, 65, o)
            for B in (0, 33):
                assert dev(B=B) == ARG and b'B =' in lib.wct_last_error()
            assert dev(o=C.c_void_p(buf.value + 12)) == ARG and b'overlaps' in lib.wct_last_error()
        finally:
            ctx.dev_free(buf)
        assert np.array_equal(ctx.stylize_prepared_upsampled(img, handle, SMALL, (40, 54), 2, 65), want)


# ---- the driver == the composition of the stand-alone calls ------------------------------------------------------------------------
def _composition(ctx, img, handle, work, r, eps_q, colors, **kw):
    small = ctx.resize(img, work) if tuple(work) != img.shape[:2] else img
    plain = ctx.stylize_prepared(small, handle, SMALL, alpha=0.8, **kw)
    up = ctx.guided_upsample(plain, small, img, r, eps_q)
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
            got = ctx.stylize_prepared_upsampled(img, handle, SMALL, work, 2, 65, alpha=0.8, content_colors=colors, **kw)
            assert got.shape == img.shape and np.array_equal(got, want), (kw, colors)
        assert not np.array_equal(want, img)


def test_driver_on_three_frames_and_at_the_working_size(ctx):
    frames = np.stack([synthetic_image(30 + i, 96, 130) for i in range(3)])
    with ctx.prepare_style(synthetic_image(29, 80, 64), SMALL) as handle:
        for colors in (False, True):
            want = np.stack([_composition(ctx, f, handle, (40, 54), 2, 65, colors) for f in frames])
            got = ctx.stylize_prepared_upsampled_batch(frames, handle, SMALL, (40, 54), 2, 65, alpha=0.8, content_colors=colors)
            assert np.array_equal(got, want), colors
        small = synthetic_image(35, 40, 52)                                          # H == hc, W == wc: no resize
        assert np.array_equal(ctx.stylize_prepared_upsampled(small, handle, SMALL, (40, 52), 2, 65, alpha=0.8),
                              _composition(ctx, small, handle, (40, 52), 2, 65, False))


def test_driver_takes_float_contents_at_the_working_size(ctx):
    """WCT_FLAG_IMAGES_F32 without a resize: both kernels read the fp32 content under the output rule"""
    c = synthetic_image(40, 44, 52).astype(np.float64) * 0.9 + 3.3
    c32 = np.ascontiguousarray(c / 255., np.float32)
    c_u8 = colors_oracle.quantise(c32)
    lv = (C.c_int * 3)(3, 2, 1)
    with ctx.prepare_style(synthetic_image(41, 64, 72), SMALL) as handle:
        plain = ctx.stylize_prepared(c, handle, SMALL, alpha=0.8)
        out = np.empty((44, 52, 3), np.uint8)
        for flags, want in ((_lib.FLAG_IMAGES_F32, oracle.guided_upsample(plain, c_u8, c_u8, 2, 65)),
                            (_lib.FLAG_IMAGES_F32 | _lib.FLAG_CONTENT_COLORS,
                             colors_oracle.content_colors(oracle.guided_upsample(plain, c_u8, c_u8, 2, 65), c_u8))):
            assert ctx.lib.wct_stylize_prepared_upsampled(ctx.h, c32.ctypes.data_as(_lib._U8), 44, 52, 44, 52, handle.h, lv, 3, 0.8, flags,
                                                          2, 65, out.ctypes.data_as(_lib._U8)) == 0
            assert np.array_equal(out, want), flags


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
    small = synthetic_image(60, 36, 50)                                              # already small enough: worked on as it is
    with model.prepare_style(sty) as handle:
        assert np.array_equal(model.predict(small, handle, 0.8, guided_upsample=GU), _composition(sess, small, handle, (36, 50), 2, 65, False))


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
                                          '--guided-upsample']
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
                                                '--content-size', '40', '--guided-upsample', '--out-path', str(tmp_path / 'out')]) == 3
    m = _cli_model()
    try:
        for i in range(3):
            small = m.sess.resize(frames[i], (40, 54))
            want = oracle.guided_upsample(m.predict(small, style, 0.8), small, frames[i], 2, 65)
            got = utils.get_img(str(tmp_path / 'out' / 'clip_s0' / ('frame_%d.png' % (i + 1))))
            assert got.shape == frames[i].shape and np.array_equal(got, want), i
    finally:
        m.sess.close()
