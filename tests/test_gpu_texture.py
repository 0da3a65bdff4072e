"""Texture synthesis on the GPU (csrc/noise.hip, the texture drivers of csrc/api_stylize.hip): the noise op against the NumPy
oracle (tests/texture_oracle.py) at every edge of its 16-byte groups, the device pass chain against the host loop it replaces,
WCT.synthesize, the refusals of the C ABI, and the command line.  Everything is np.array_equal: the noise rule is integers only,
and the chain runs the launches of the prepared calls.  Synthetic weights as in tests/test_gpu_colors.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import texture_oracle as oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
MODES = {'tf': dict(wct_mode='tf', adain=False), 'np': dict(wct_mode='np', adain=False), 'adain': dict(wct_mode='tf', adain=True)}
ARG, STATE = -2, -3


@pytest.fixture(scope='module')
def small():
    from wct_tf_amd.wct import WCT
    m = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    yield m
    m.sess.close()


@pytest.fixture(scope='module')
def full():
    from wct_tf_amd.wct import WCT
    m = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(7))
    yield m
    m.sess.close()


@functools.lru_cache(maxsize=None)
def _want(h, w, seed, sample, smooth):
    return oracle.noise(h, w, seed, sample, smooth)


def _want_batch(h, w, b, seed, first, smooth):
    return np.stack([_want(h, w, seed, first + i, smooth) for i in range(b)])


# ---- the noise op ------------------------------------------------------------------------------------------------------------
GUARD = 16


def _noise_dev(ctx, h, w, b, seed, first, smooth, offset):
    """wct_texture_noise_batch_dev into a buffer of its own, the output base `offset` bytes off the (at least 16-byte) alignment
    of the allocation; the bytes in front of the output and the GUARD bytes behind it must come back untouched"""
    n = b * h * w * 3
    fill = np.full(offset + n + GUARD, 0xA5, np.uint8)
    buf = ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(buf, fill)
        ctx.texture_noise_batch_dev(h, w, b, seed, first, smooth, C.c_void_p(buf.value + offset))
        ctx.sync()
        got = np.empty_like(fill)
        ctx.d2h(got, buf)
    finally:
        ctx.dev_free(buf)
    assert np.all(got[:offset] == 0xA5) and np.all(got[offset + n:] == 0xA5), (h, w, b, offset)
    return got[offset:offset + n].reshape(b, h, w, 3)


# (1, 1) and (2, 3): less than one group; (5, 7): 105 bytes an image -- six groups and a 9-byte tail on an aligned base, a
# 15-byte (or 8-byte) head first on a shifted one, and images that start in the middle of a group; (17, 33) and (40, 56): rows
# of 99 and 168 bytes, several blocks at B = 32
@pytest.mark.parametrize('smooth', [False, True], ids=['raw', 'smooth'])
@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7), (17, 33), (40, 56)])
def test_noise_op_is_the_oracle(small, h, w, smooth):
    ctx = small.sess
    for b in (1, 3, 32):
        for seed in (0, 7, 0xFFFFFFFF):
            for first in (0, 5):
                want = _want_batch(h, w, b, seed, first, smooth)
                for offset in (0, 1, 8):
                    got = _noise_dev(ctx, h, w, b, seed, first, smooth, offset)
                    assert np.array_equal(got, want), (b, seed, first, offset)
    # image i of a batch is the B = 1 call with sample = first_sample + i, and the host call, and the stand-alone op
    from wct_tf_amd import texture_noise_np
    batch = _noise_dev(ctx, h, w, 32, 7, 5, smooth, 0)
    for i in (0, 1, 31):
        assert np.array_equal(batch[i], _noise_dev(ctx, h, w, 1, 7, 5 + i, smooth, 0)[0]), i
        assert np.array_equal(batch[i], ctx.texture_noise(h, w, 7, 5 + i, smooth)), i
        assert np.array_equal(batch[i], texture_noise_np(h, w, 7, 5 + i, smooth, ctx=ctx)), i


def test_noise_op_refusals_leave_the_context_usable(small):
    ctx = small.sess
    lib, h = ctx.lib, ctx.h
    out = np.empty((4, 4, 3), np.uint8)
    p = out.ctypes.data_as(_lib._U8)
    buf = ctx.dev_alloc(64)
    try:
        for b in (0, -1, 33):
            assert lib.wct_texture_noise_batch_dev(h, 4, 4, b, 1, 0, 0, buf) == ARG
        assert b'texture noise' in lib.wct_last_error()
        assert lib.wct_texture_noise_batch_dev(h, 4, 4, 1, 1, 0, 0, None) == ARG
        assert lib.wct_texture_noise_batch_dev(None, 4, 4, 1, 1, 0, 0, buf) == ARG
        assert lib.wct_texture_noise_batch_dev(h, 0, 4, 1, 1, 0, 0, buf) == ARG
        assert lib.wct_texture_noise_batch_dev(h, 4, -1, 1, 1, 0, 0, buf) == ARG
        # 2^31 bytes and more in one call: refused up front, nothing is launched (the buffer is 64 bytes)
        assert lib.wct_texture_noise_batch_dev(h, 30000, 30000, 1, 1, 0, 0, buf) == ARG
        assert b'2^31' in lib.wct_last_error()
        assert lib.wct_texture_noise_batch_dev(h, 4736, 4736, 32, 1, 0, 0, buf) == ARG          # 32 x 67.3 MB = 2^31 + 5.8 MB
        assert lib.wct_texture_noise_batch_dev(h, 1 << 30, 1 << 30, 1, 1, 0, 0, buf) == ARG
    finally:
        ctx.dev_free(buf)
    assert lib.wct_texture_noise(h, 4, 4, 1, 0, 0, None) == ARG
    assert lib.wct_texture_noise(None, 4, 4, 1, 0, 0, p) == ARG
    assert lib.wct_texture_noise(h, 30000, 30000, 1, 0, 0, p) == ARG
    ctx.sync()
    assert np.array_equal(ctx.texture_noise(4, 4, 1), oracle.noise(4, 4, 1))


# ---- the chain ---------------------------------------------------------------------------------------------------------------
H, W = 40, 56              # five levels grow it to 48 x 64 in pass 1 (40 -> 20 -> 10 -> 5 -> 3 rows at relu5_1, x 16), three keep it


def _host_loop(model, frames, handle, passes, alpha, wct_mode, adain):
    """what the device chain replaces: predict_frames on the same handle, once per pass, the frames through the host"""
    keep, model.wct_mode = model.wct_mode, wct_mode
    try:
        outs = []
        for _ in range(passes):
            frames = model.predict_frames(frames, handle, alpha=alpha, adain=adain, batch=len(frames))
            outs.append(frames)
        return outs
    finally:
        model.wct_mode = keep


def test_texture_size_grows_in_pass_one_only(small, full):
    for passes in (1, 2, 3, 16):
        assert full.sess.texture_size(H, W, RELU_TARGETS, passes) == (48, 64)
        assert small.sess.texture_size(H, W, SMALL, passes) == (40, 56)
        assert full.sess.texture_size(33, 35, SMALL, passes) == (36, 36)
    assert full.sess.output_size(H, W, RELU_TARGETS) == (48, 64) and full.sess.output_size(48, 64, RELU_TARGETS) == (48, 64)
    lv = (C.c_int * 1)(5)
    ho, wo = C.c_int(), C.c_int()
    assert full.sess.lib.wct_texture_size(H, W, lv, 1, 0, C.byref(ho), C.byref(wo)) == ARG
    assert full.sess.lib.wct_texture_size(H, W, lv, 1, 17, C.byref(ho), C.byref(wo)) == ARG
    assert full.sess.lib.wct_texture_size(16, W, lv, 1, 1, C.byref(ho), C.byref(wo)) == ARG


@pytest.mark.parametrize('alpha', [1, 0.6])
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('which', ['three-levels', 'five-levels'])
def test_chain_is_the_host_loop(small, full, which, mode, alpha):
    model, levels, size = (small, SMALL, (40, 56)) if which == 'three-levels' else (full, RELU_TARGETS, (48, 64))
    kw = MODES[mode]
    noise = oracle.noise_batch(H, W, 3, 11, first_sample=2)
    with model.sess.prepare_style(synthetic_image(21, 72, 64), levels, **kw) as handle:
        want = _host_loop(model, noise, handle, 3, alpha, **kw)
        for passes in (1, 2, 3):
            got = model.sess.texture_prepared_batch(H, W, 3, 11, 2, handle, levels, passes=passes, alpha=alpha, **kw)
            assert got.dtype == np.uint8 and got.shape == (3,) + size + (3,)
            assert np.array_equal(got, want[passes - 1]), (which, mode, alpha, passes)
        assert not np.array_equal(want[0], want[2])                      # (the passes did something)


@pytest.mark.parametrize('which', ['three-levels', 'five-levels'])
def test_chain_samples_do_not_depend_on_their_batch(small, full, which):
    model, levels = (small, SMALL) if which == 'three-levels' else (full, RELU_TARGETS)
    ctx = model.sess
    with ctx.prepare_style(synthetic_image(22, 64, 80), levels) as handle:
        four = ctx.texture_prepared_batch(H, W, 4, 3, 0, handle, levels, passes=2, alpha=0.8, smooth=True)
        for f in range(4):
            one = ctx.texture_prepared_batch(H, W, 1, 3, f, handle, levels, passes=2, alpha=0.8, smooth=True)
            assert np.array_equal(four[f], one[0]), f
            assert np.array_equal(four[f], ctx.texture_prepared(H, W, 3, f, handle, levels, passes=2, alpha=0.8, smooth=True)), f
        assert np.array_equal(ctx.texture_prepared_batch(H, W, 4, 3, 0, handle, levels, passes=2, alpha=0.8, smooth=True), four)
        assert not np.array_equal(four[0], four[1])
        # smooth noise is the oracle's smooth noise
        loop = _host_loop(model, oracle.noise_batch(H, W, 4, 3, smooth_on=True), handle, 2, 0.8, 'tf', False)[-1]
        assert np.array_equal(four, loop)


# ---- WCT.synthesize ------------------------------------------------------------------------------------------------------------
def test_synthesize_with_an_image_and_with_its_handle(full):
    style = synthetic_image(23, 64, 72)
    got = full.synthesize(style, (H, W), seeds=2, seed=9, passes=2, alpha=0.8)
    assert got.dtype == np.uint8 and got.shape == (2, 48, 64, 3)
    with full.prepare_style(style) as handle:
        assert np.array_equal(full.synthesize(handle, (H, W), seeds=2, seed=9, passes=2, alpha=0.8), got)
        assert not handle.closed
        want = _host_loop(full, oracle.noise_batch(H, W, 2, 9), handle, 2, 0.8, 'tf', False)[-1]
    assert np.array_equal(got, want)


def test_synthesize_with_a_list_of_samples(small):
    with small.prepare_style(synthetic_image(24, 64, 64)) as handle:
        got = small.synthesize(handle, (H, W), seeds=[0, 1, 5], seed=4, passes=2, batch=16)          # two batches: 0 1 | 5
        assert got.shape == (3, 40, 56, 3)
        for i, v in enumerate((0, 1, 5)):
            assert np.array_equal(got[i], small.synthesize(handle, (H, W), seeds=[v], seed=4, passes=2)[0]), v
        assert np.array_equal(small.synthesize(handle, (H, W), seeds=2, seed=4, passes=2), got[:2])
        assert np.array_equal(small.synthesize(handle, (H, W), seeds=[0, 1, 5], seed=4, passes=2, batch=1), got)


def test_synthesize_interpolates_between_two_styles(small):
    from wct_tf_amd import texture_noise_np
    styles = [synthetic_image(25, 64, 64), synthetic_image(26, 56, 72)]
    handles = [small.prepare_style(s) for s in styles]
    try:
        got = small.synthesize(handles, (H, W), seeds=[0, 3], seed=6, passes=2, alpha=0.8, weights=(1, 3))
        assert got.shape == (2, 40, 56, 3)
        for i, v in enumerate((0, 3)):
            img = texture_noise_np(H, W, 6, v, ctx=small.sess)
            assert np.array_equal(img, oracle.noise(H, W, 6, v))
            for _ in range(2):
                img = small.predict_mix(img, handles, (1, 3), alpha=0.8)
            assert np.array_equal(got[i], img), v
        assert np.array_equal(small.synthesize(styles, (H, W), seeds=[0, 3], seed=6, passes=2, alpha=0.8, weights=(1, 3)), got)
    finally:
        for h in handles:
            h.close()


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(full):
    from wct_tf_amd.context import Context
    ctx = full.sess
    lib, h = ctx.lib, ctx.h
    lv = (C.c_int * 3)(3, 2, 1)
    deep = (C.c_int * 2)(5, 1)
    ho, wo = 40, 56
    out = np.empty((ho, wo, 3), np.uint8)
    p = out.ctypes.data_as(_lib._U8)
    other = Context(0)
    other.set_weights(synthetic_weights(5, relu_targets=SMALL))
    buf = ctx.dev_alloc(4 * 48 * 64 * 3)
    style = synthetic_image(27, 64, 64)
    try:
        handle = ctx.prepare_style(style, SMALL)
        foreign = other.prepare_style(style, SMALL)
        freed = ctx.prepare_style(style, SMALL)
        freed_h = C.c_void_p(freed.h.value)
        freed.close()
        earlier = ctx.texture_prepared(H, W, 1, 0, handle, SMALL, passes=2, alpha=0.8)

        def batch(hh=H, ww=W, b=1, st=None, levels=lv, n=3, passes=2, flags=0, o=buf, c=h):
            return lib.wct_texture_prepared_batch_dev(c, hh, ww, b, 1, 0, 0, handle.h if st is None else st, levels, n, passes, 0.8,
                                                      flags, o)

        def host(hh=H, ww=W, st=None, levels=lv, n=3, passes=2, flags=0, o=p, c=h):
            return lib.wct_texture_prepared(c, hh, ww, 1, 0, 0, handle.h if st is None else st, levels, n, passes, 0.8, flags, o)

        def refused(rc, want):
            assert rc == want, (rc, lib.wct_last_error())
            ctx.sync()
            assert np.array_equal(ctx.texture_prepared(H, W, 1, 0, handle, SMALL, passes=2, alpha=0.8), earlier)

        for call in (batch, host):
            for flag in (_lib.FLAG_SWAP5, _lib.FLAG_STYLE_SHARED, _lib.FLAG_IMAGES_F32, _lib.FLAG_CONTENT_COLORS):
                refused(call(flags=flag), ARG)
            for passes in (0, -1, 17):
                refused(call(passes=passes), ARG)
            refused(call(hh=4), ARG)                                     # relu3_1 needs 5 pixels
            assert b'too small for relu3_1' in lib.wct_last_error()
            refused(call(ww=4), ARG)
            refused(call(levels=deep, n=2), ARG)                         # relu5_1 is not in the handle's set
            assert b'not prepared for relu5_1' in lib.wct_last_error()
            refused(call(levels=(C.c_int * 1)(7), n=1), ARG)
            refused(call(levels=None), ARG)
            refused(call(n=0), ARG)
            refused(call(o=None), ARG)
            refused(call(c=None), ARG)
            refused(call(st=foreign.h), STATE)
            refused(call(st=freed_h), STATE)
        for b in (0, -1, 33):
            refused(batch(b=b), ARG)
        # and the accepted flags are accepted
        assert batch(flags=_lib.FLAG_ADAIN) == 0 and batch(flags=_lib.FLAG_MODE_NP) == 0
        ctx.sync()
        handle.close()
    finally:
        ctx.dev_free(buf)
        other.close()


# ---- the command line, end to end ---------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def test_texture_cli_single_style_and_mix(tmp_path):
    from wct_tf_amd.texture import main
    from wct_tf_amd.wct import WCT
    styles = {'a': synthetic_image(28, 56, 48), 'b': synthetic_image(29, 48, 64)}
    for name, img in styles.items():
        utils.save_img(str(tmp_path / (name + '.png')), img)
    base = ['--relu-targets'] + TARGETS + ['--synthetic-weights', '42', '--size', '32', '48', '--samples', '2', '--passes', '2',
                                          '--seed', '3', '--alpha', '0.8']
    assert main(base + ['--style-path', str(tmp_path / 'a.png'), '--out-path', str(tmp_path / 'one')]) == 2
    assert main(base + ['--interp-styles', str(tmp_path / 'a.png'), str(tmp_path / 'b.png'), '--interp-weights', '1', '3',
                        '--out-path', str(tmp_path / 'mix'), '--noise-smooth']) == 2
    m = WCT(None, TARGETS, None, weights=synthetic_weights(42, relu_targets=TARGETS))
    try:
        one = m.synthesize(styles['a'], (32, 48), seeds=2, seed=3, passes=2, alpha=0.8)
        mix = m.synthesize([styles['a'], styles['b']], (32, 48), seeds=2, seed=3, passes=2, alpha=0.8, weights=[1, 3], smooth=True)
        for i in range(2):
            assert np.array_equal(utils.get_img(str(tmp_path / 'one' / ('a_texture_s3_%d.png' % i))), one[i]), i
            assert np.array_equal(utils.get_img(str(tmp_path / 'mix' / ('a+b_texture_s3_%d.png' % i))), mix[i]), i
        assert not np.array_equal(one[0], one[1])
    finally:
        m.sess.close()
