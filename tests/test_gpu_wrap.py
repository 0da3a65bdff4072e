"""Seamless textures on the GPU (include/wct_hip.h, "seamless textures"): the wrap kernel against np.pad, the wrap passes against
the plain passes on host-padded maps (bit for bit: the same launches on the same input), batch independence, the texture chain,
and -- on the contractive net of the end-to-end tests (oracle/contractive.py) -- the property itself: shift equivariance, parity
with the periodic oracle (tests/wrap_oracle.py) and the seam of a tile."""
import ctypes as C

import numpy as np
import pytest

import oracle
import texture_oracle
import wrap_oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
ARG = -2
GUARD = 256
ALPHA = 0.8


@pytest.fixture(scope='module')
def full():
    from wct_tf_amd.wct import WCT
    m = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(7))
    yield m
    m.sess.close()


@pytest.fixture(scope='module')
def contractive():
    """the contractive net, a context that holds it, a style and its handle, one 64 x 96 content and -- computed ONCE -- the
    periodic and the plain oracle's frames of it"""
    from oracle.contractive import contractive_weights
    from wct_tf_amd.context import Context
    w = contractive_weights(7)
    c = Context(0)
    c.set_weights(w)
    style = synthetic_image(*wrap_oracle.SEAM_CASE['style'])
    x = synthetic_image(910, 64, 96)
    handle = c.prepare_style(style, SMALL)
    want = {'wrap': wrap_oracle.stylize(x, style, w, SMALL, alpha=ALPHA), 'plain': oracle.stylize(x, style, w, SMALL, alpha=ALPHA)}
    yield c, handle, x, want
    c.close()


def lsb(got, want):
    d = np.abs(got.astype(int) - want.astype(int))
    return int(d.max()), float(d.mean())


def no_further(d, ref):
    """tests/test_gpu_warm.py::assert_no_worse_than_cold's bound: no further than the reference distance plus 1 LSB in the maximum
    and 0.05 LSB in the mean (a uint8 tie can flip on any last-bit change)"""
    return d[0] <= ref[0] + 1 and d[1] <= ref[1] + 0.05


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _pad_dev(ctx, x, pads):
    """wct_wrap_pad_batch_dev of x [B][H][W][C] into a buffer of its own, GUARD bytes of 0xA5 in front of the output and behind it,
    which must come back untouched"""
    t, b, l, r = pads
    B, H, W, E = x.shape
    shape = (B, t + H + b, l + W + r, E)
    n = int(np.prod(shape)) * 4
    fill = np.full(GUARD + n + GUARD, 0xA5, np.uint8)
    src, buf = ctx.dev_alloc(x.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(src, x)
        ctx.h2d(buf, fill)
        ctx.wrap_pad_batch_dev(src, B, H, W, E, pads, C.c_void_p(buf.value + GUARD))
        ctx.sync()
        got = np.empty_like(fill)
        ctx.d2h(got, buf)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(buf)
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + n:] == 0xA5), (x.shape, pads)
    return got[GUARD:GUARD + n].view(np.float32).reshape(shape)


# one float per lane (E = 3): a single pixel under a halo of 96 periods, rows of 21 and 144 floats, pads of 0 and of several periods;
# 16-byte groups (E = 64: 16 per pixel, E = 512: 128): halos wider than the map on every side
PAD_CASES = [((1, 1, 3), (96, 96, 96, 96)), ((1, 1, 3), (0, 3, 7, 1)), ((5, 7, 3), (96, 96, 96, 96)), ((5, 7, 3), (0, 3, 7, 1)),
             ((32, 48, 3), (96, 96, 96, 96)), ((32, 48, 3), (0, 3, 7, 1)), ((2, 3, 64), (6, 5, 6, 5)), ((6, 5, 512), (6, 5, 6, 5))]


@pytest.mark.parametrize('shape,pads', PAD_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_wrap_pad_is_np_pad(full, shape, pads):
    ctx = full.sess
    rng = np.random.default_rng(sum(shape) + sum(pads))
    x = rng.standard_normal((3,) + shape).astype(np.float32)
    x.view(np.uint32)[0, 0, 0, 0] = 0x7FC01234                       # bytes are moved, not values: a NaN payload survives
    t, b, l, r = pads
    want = np.pad(x, ((0, 0), (t, b), (l, r), (0, 0)), mode='wrap')
    assert np.array_equal(_pad_dev(ctx, x, pads).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(_pad_dev(ctx, x[:1], pads).view(np.uint32), want[:1].view(np.uint32))
    assert np.array_equal(ctx.wrap_pad(x[1], pads).view(np.uint32), want[1].view(np.uint32))       # the host form


# ---- encode / decode against the host-padded pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize('level', [1, 2, 3, 4, 5])
def test_encode_and_decode_wrap_are_the_plain_passes_on_the_padded_map(full, level):
    ctx = full.sess
    target = 'relu%d_1' % level
    s = 1 << (level - 1)
    H, W = (32, 48) if level >= 4 else (20, 36)
    enc, before, after = ctx.wrap_halo(target)
    img = np.float32(synthetic_image(70 + level, H, W)) / np.float32(255)
    f = ctx.encode_wrap(img, target)
    assert f.shape[:2] == (H // s, W // s)
    padded = ctx.encode(np.pad(img, ((enc, enc), (enc, enc), (0, 0)), mode='wrap'), target)
    assert np.array_equal(f, padded[enc // s:enc // s + H // s, enc // s:enc // s + W // s])
    assert not np.array_equal(f, ctx.encode(img, target))             # (and not the reflect-padded pass)
    d = ctx.decode_wrap(f, target)
    assert d.shape == (H, W, 3)
    dp = ctx.decode(np.pad(f, ((before, after), (before, after), (0, 0)), mode='wrap'), target)
    assert np.array_equal(d, dp[before * s:before * s + H, before * s:before * s + W])


# ---- batch independence, the texture chain ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', [SMALL, RELU_TARGETS], ids=['three-levels', 'five-levels'])
def test_frames_do_not_depend_on_their_batch(full, levels):
    ctx = full.sess
    frames = np.stack([synthetic_image(80 + i, 32, 48) for i in range(3)])
    with ctx.prepare_style(synthetic_image(22, 64, 80), levels) as handle:
        got = ctx.stylize_prepared_wrap_batch(frames, handle, levels, alpha=ALPHA)
        assert got.shape == frames.shape and got.dtype == np.uint8
        for f in range(3):
            assert np.array_equal(ctx.stylize_prepared_wrap_batch(frames[f:f + 1], handle, levels, alpha=ALPHA)[0], got[f]), f
            assert np.array_equal(ctx.stylize_prepared_wrap(frames[f], handle, levels, alpha=ALPHA), got[f]), f
        assert not np.array_equal(got, ctx.stylize_prepared_batch(frames, handle, levels, alpha=ALPHA))
        if levels is RELU_TARGETS:                                       # (the model's own targets) the facade, in batches of 2 and 1
            assert np.array_equal(full.predict_frames(frames, handle, alpha=ALPHA, wrap=True, batch=2), got)


MODES = {'wct': dict(), 'adain': dict(adain=True), 'np': dict(wct_mode='np')}


@pytest.mark.parametrize('passes,mode', [(1, 'wct'), (2, 'wct'), (2, 'adain'), (2, 'np')])
def test_texture_chain_is_the_host_loop(full, passes, mode):
    ctx = full.sess
    kw = MODES[mode]
    h, w = 32, 48
    with ctx.prepare_style(synthetic_image(23, 64, 72), RELU_TARGETS) as handle:
        want = np.stack([ctx.texture_noise(h, w, 11, 2 + b) for b in range(3)])
        assert np.array_equal(want, texture_oracle.noise_batch(h, w, 3, 11, first_sample=2))
        for _ in range(passes):
            want = ctx.stylize_prepared_wrap_batch(want, handle, RELU_TARGETS, alpha=ALPHA, **kw)
        got = ctx.texture_prepared_wrap_batch(h, w, 3, 11, 2, handle, RELU_TARGETS, passes=passes, alpha=ALPHA, **kw)
        assert np.array_equal(got, want)
        assert np.array_equal(ctx.texture_prepared_wrap(h, w, 11, 3, handle, RELU_TARGETS, passes=passes, alpha=ALPHA, **kw), want[1])
        if mode == 'wct':
            assert np.array_equal(full.synthesize(handle, (h, w), seeds=[2, 3, 4], seed=11, passes=passes, alpha=ALPHA, tile=True), want)
            assert not np.array_equal(full.synthesize(handle, (h, w), seeds=[2, 3, 4], seed=11, passes=passes, alpha=ALPHA), want)


# ---- the property: shift equivariance, parity with the periodic oracle, the seam ----------------------------------------------------
@pytest.mark.parametrize('a,b', [(1, 2), (3, 0)])
def test_a_shift_of_the_tile_is_a_shift_of_the_frame(contractive, a, b):
    """wrap(roll(x)) against roll(wrap(x)) for shifts by multiples of 16, the stride of everything in the construction: the two
    differ by summation order alone (the transform sums over the same pixels in another order), so they are no further apart than
    the device frame is from the periodic oracle's.  The plain call fails the same assertion: the test cannot pass vacuously."""
    ctx, handle, x, want = contractive
    shift = (16 * a, 16 * b)
    rolled = np.roll(x, shift, (0, 1))
    dev = ctx.stylize_prepared_wrap_batch(x[None], handle, SMALL, alpha=ALPHA)[0]
    dev_r = ctx.stylize_prepared_wrap_batch(rolled[None], handle, SMALL, alpha=ALPHA)[0]
    d, ref = lsb(dev_r, np.roll(dev, shift, (0, 1))), lsb(dev, want['wrap'])
    plain = ctx.stylize_prepared_batch(x[None], handle, SMALL, alpha=ALPHA)[0]
    plain_r = ctx.stylize_prepared_batch(rolled[None], handle, SMALL, alpha=ALPHA)[0]
    pd, pref = lsb(plain_r, np.roll(plain, shift, (0, 1))), lsb(plain, want['plain'])
    print('shift %s: wrap max %d mean %.4f (device to oracle %d, %.4f) | plain max %d mean %.4f (device to oracle %d, %.4f)'
          % (shift, d[0], d[1], ref[0], ref[1], pd[0], pd[1], pref[0], pref[1]))
    assert no_further(d, ref), (d, ref)
    assert not no_further(pd, pref), (pd, pref)


def test_the_tile_frame_is_the_periodic_oracles(contractive):
    """the device tile against wrap_oracle's frame is no further than the plain device frame is from the plain oracle's on the
    same input (the bound of tests/test_gpu_warm.py::assert_no_worse_than_cold)"""
    ctx, handle, x, want = contractive
    dev = ctx.stylize_prepared_wrap_batch(x[None], handle, SMALL, alpha=ALPHA)[0]
    plain = ctx.stylize_prepared_batch(x[None], handle, SMALL, alpha=ALPHA)[0]
    d, ref = lsb(dev, want['wrap']), lsb(plain, want['plain'])
    print('tile to periodic oracle: max %d mean %.4f | plain to plain oracle: max %d mean %.4f' % (d + ref))
    assert no_further(d, ref), (d, ref)
    assert lsb(dev, want['plain'])[0] > ref[0] + 1                   # (and the two oracles are not the same frame)


def test_a_tile_has_no_seam(contractive):
    """the mean step across the joints of the tile laid beside itself is no larger than the largest mean step between adjacent
    interior rows or columns; tests/test_wrap_cpu.py checks the same case on the oracle"""
    ctx, handle, _, _ = contractive
    case = wrap_oracle.SEAM_CASE
    h, w = case['size']
    tile = ctx.texture_prepared_wrap(h, w, case['seed'], case['sample'], handle, case['targets'], passes=1, alpha=case['alpha'])
    plain = ctx.texture_prepared(h, w, case['seed'], case['sample'], handle, case['targets'], passes=1, alpha=case['alpha'])
    joint, inner = wrap_oracle.seam_steps(tile)
    pj, pi = wrap_oracle.seam_steps(plain)
    print('seam, device: tile joint %.3f interior max %.3f | plain joint %.3f interior max %.3f' % (joint, inner, pj, pi))
    assert tile.shape == (h, w, 3) and joint <= inner


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(full):
    ctx = full.sess
    lib, h = ctx.lib, ctx.h
    H, W, big = 32, 48, 2896
    lv = (C.c_int * 5)(5, 4, 3, 2, 1)
    one = (C.c_int * 1)(1)
    frame = synthetic_image(90, H, W)
    out = np.empty((H, W, 3), np.uint8)
    p = out.ctypes.data_as(_lib._U8)
    large = np.zeros((big, big, 3), np.uint8)                         # (a refusal must come before a byte of it is read)
    buf, big_in, big_out = ctx.dev_alloc(4 * H * W * 3), ctx.dev_alloc(large.nbytes), ctx.dev_alloc(large.nbytes)
    try:
        handle = ctx.prepare_style(synthetic_image(27, 64, 64), RELU_TARGETS)
        earlier = ctx.stylize_prepared_wrap(frame, handle, SMALL, alpha=ALPHA)

        def batch(hh=H, ww=W, b=1, levels=lv, n=5, flags=0, src=buf, o=buf, c=h):
            return lib.wct_stylize_prepared_wrap_batch_dev(c, src, hh, ww, b, handle.h, levels, n, ALPHA, flags, o)

        def host(hh=H, ww=W, levels=lv, n=5, flags=0, src=frame.ctypes.data_as(_lib._U8), o=p, c=h):
            return lib.wct_stylize_prepared_wrap(c, src, hh, ww, handle.h, levels, n, ALPHA, flags, o)

        def tex(hh=H, ww=W, b=1, levels=lv, n=5, flags=0, passes=2, o=buf, c=h):
            return lib.wct_texture_prepared_wrap_batch_dev(c, hh, ww, b, 1, 0, 0, handle.h, levels, n, passes, ALPHA, flags, o)

        def tex_host(hh=H, ww=W, levels=lv, n=5, flags=0, passes=2, o=p, c=h):
            return lib.wct_texture_prepared_wrap(c, hh, ww, 1, 0, 0, handle.h, levels, n, passes, ALPHA, flags, o)

        def refused(rc, word=None):
            assert rc == ARG, (rc, lib.wct_last_error())
            assert word is None or word in lib.wct_last_error(), lib.wct_last_error()
            ctx.sync()
            assert np.array_equal(ctx.stylize_prepared_wrap(frame, handle, SMALL, alpha=ALPHA), earlier)

        for call in (batch, host, tex, tex_host):
            refused(call(hh=40), b'multiples of 16')                     # an odd multiple of 8 under relu5_1
            refused(call(ww=47), b'multiples of 16')
            refused(call(hh=16), b'too small for relu5_1')
            for flag, word in ((_lib.FLAG_CONTENT_COLORS, b'CONTENT_COLORS'), (_lib.FLAG_SWAP5, b'SWAP5'),
                               (_lib.FLAG_STYLE_SHARED, b'STYLE_SHARED')):
                refused(call(flags=flag), word)
            refused(call(levels=(C.c_int * 1)(7), n=1))
            refused(call(n=0))
            refused(call(o=None))
            refused(call(c=None))
        for call in (tex, tex_host):
            refused(call(flags=_lib.FLAG_IMAGES_F32), b'IMAGES_F32')
            refused(call(passes=0))
            refused(call(passes=17))
        for call in (batch, tex):
            refused(call(b=0))
            refused(call(b=33))
        # a tile that a plain call takes, its halo past the limit of one launch
        refused(batch(hh=big, ww=big, levels=one, n=1, src=big_in, o=big_out), b'2^31')
        refused(host(hh=big, ww=big, levels=one, n=1, src=large.ctypes.data_as(_lib._U8), o=large.ctypes.data_as(_lib._U8)), b'2^31')
        refused(tex(hh=big, ww=big, levels=one, n=1, o=big_out), b'2^31')
        # the kernel's own entry point
        x = np.zeros((4, 4, 3), np.float32)
        y = np.empty((6, 6, 3), np.float32)
        fp = lambda a: a.ctypes.data_as(_lib._F)
        refused(lib.wct_wrap_pad(h, fp(x), 4, 4, 3, -1, 1, 1, 1, fp(y)))
        refused(lib.wct_wrap_pad(h, fp(x), 4, 4, 3, 1 << 30, 1, 1 << 30, 1, fp(y)), b'2^31')
        refused(lib.wct_wrap_pad_batch_dev(h, buf, 33, 4, 4, 3, 1, 1, 1, 1, buf), b'1 .. 32')
        refused(lib.wct_wrap_pad_batch_dev(h, buf, 1, 4, 4, 3, 1 << 30, 1, 1 << 30, 1, buf), b'2^31')
        refused(lib.wct_encode_wrap(h, fp(x), 18, 20, 3, fp(y)), b'multiples of 4')
        # and the accepted flags are accepted
        assert batch(flags=_lib.FLAG_ADAIN) == 0 and batch(flags=_lib.FLAG_MODE_NP) == 0 and tex(flags=_lib.FLAG_ADAIN) == 0
        ctx.sync()
        handle.close()
    finally:
        for b in (buf, big_in, big_out):
            ctx.dev_free(b)


# ---- the command line, end to end ---------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def test_texture_cli_tile_and_preview(tmp_path):
    from wct_tf_amd.texture import main
    from wct_tf_amd.wct import WCT
    style = synthetic_image(28, 56, 48)
    utils.save_img(str(tmp_path / 'a.png'), style)
    base = ['--relu-targets'] + TARGETS + ['--synthetic-weights', '42', '--size', '32', '48', '--samples', '2', '--passes', '2',
                                          '--seed', '3', '--alpha', '0.8', '--style-path', str(tmp_path / 'a.png')]
    assert main(base + ['--out-path', str(tmp_path / 'tile'), '--tile', '--tile-preview', '2']) == 4
    assert main(base + ['--out-path', str(tmp_path / 'bare'), '--tile']) == 2
    m = WCT(None, TARGETS, None, weights=synthetic_weights(42, relu_targets=TARGETS))
    try:
        want = m.synthesize(style, (32, 48), seeds=2, seed=3, passes=2, alpha=0.8, tile=True)
        for i in range(2):
            tile = utils.get_img(str(tmp_path / 'tile' / ('a_texture_s3_%d.png' % i)))
            assert np.array_equal(tile, want[i]), i
            assert np.array_equal(utils.get_img(str(tmp_path / 'bare' / ('a_texture_s3_%d.png' % i))), want[i]), i
            preview = utils.get_img(str(tmp_path / 'tile' / ('a_texture_s3_%d_tiled.png' % i)))
            assert preview.shape == (64, 96, 3) and np.array_equal(preview, np.tile(tile, (2, 2, 1))), i
        assert sorted(f.name for f in (tmp_path / 'bare').iterdir()) == ['a_texture_s3_0.png', 'a_texture_s3_1.png']
    finally:
        m.sess.close()
