"""Prepared styles (wct_style) on the GPU: every handle-based call against its image-based twin, np.array_equal on the uint8
frames -- the twins are the calls the oracle tests pin.  Synthetic weights as in tests/test_gpu_mix.py."""
import ctypes as C
import os

import numpy as np
import pytest

from wct_tf_amd import _lib
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


# (content, style) sizes across the branches of the layout: style larger, content larger, equal, and level widths that are
# not multiples of 16 (the statistics then come from the stored features, not from the conv epilogue's unit sums)
SIZES = [((96, 96), (128, 144)), ((144, 128), (80, 96)), ((112, 112), (112, 112)), ((100, 84), (90, 70))]


@pytest.mark.parametrize('kw', MODES)
@pytest.mark.parametrize('csize,ssize', SIZES)
def test_predict_with_a_handle_is_predict_five_levels(full_ctx, kw, csize, ssize):
    c, s = synthetic_image(101, *csize), synthetic_image(102, *ssize)
    mode = {k: v for k, v in kw.items() if k == 'wct_mode'}
    with full_ctx.prepare_style(s, RELU_TARGETS, adain=bool(kw.get('adain')), **mode) as h:
        got = full_ctx.stylize_prepared(c, h, RELU_TARGETS, alpha=0.8, **kw)
    want = full_ctx.stylize(c, s, RELU_TARGETS, alpha=0.8, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (kw, csize, ssize)


@pytest.mark.parametrize('kw', MODES)
@pytest.mark.parametrize('level', ['relu1_1', 'relu4_1'])
def test_predict_with_a_handle_is_predict_single_level(full_ctx, kw, level):
    for csize, ssize in SIZES[:2] + SIZES[3:]:
        c, s = synthetic_image(111, *csize), synthetic_image(112, *ssize)
        with full_ctx.prepare_style(s, [level]) as h:           # prepared for wct_tf: the other modes fill in on first use
            got = full_ctx.stylize_prepared(c, h, [level], alpha=0.7, **kw)
        assert np.array_equal(got, full_ctx.stylize(c, s, [level], alpha=0.7, **kw)), (kw, level, csize)


def test_one_handle_serves_interleaved_content_sizes_and_modes(small_ctx):
    s = synthetic_image(120, 96, 80)
    a, b = synthetic_image(121, 64, 64), synthetic_image(122, 160, 128)       # two different pair_layouts against the style
    with small_ctx.prepare_style(s, SMALL) as h:
        for c in (a, b, a):                                                   # the cache fills, hits, and keeps its keys apart
            assert np.array_equal(small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8), small_ctx.stylize(c, s, SMALL, alpha=0.8))
        for c in (a, b, a):
            for kw in MODES + MODES[::-1]:
                got = small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, **kw)
                assert np.array_equal(got, small_ctx.stylize(c, s, SMALL, alpha=0.8, **kw)), (c.shape, kw)


def test_cache_eviction_keeps_the_frames_right(small_ctx):
    """more keys than a level keeps (4): the oldest go, come back on demand, and every frame stays the image-based one"""
    s = synthetic_image(125, 64, 64)
    contents = [synthetic_image(126 + i, 64 + 32 * i, 64) for i in range(6)]
    with small_ctx.prepare_style(s, SMALL) as h:
        for c in contents + contents[:2]:
            assert np.array_equal(small_ctx.stylize_prepared(c, h, SMALL, alpha=0.9), small_ctx.stylize(c, s, SMALL, alpha=0.9)), c.shape


def test_one_handle_serves_every_alpha(small_ctx):
    c, s = synthetic_image(131, 96, 96), synthetic_image(132, 80, 112)
    with small_ctx.prepare_style(s, SMALL) as h:
        for alpha in (0.6, 1.0):
            for kw in MODES:
                assert np.array_equal(small_ctx.stylize_prepared(c, h, SMALL, alpha=alpha, **kw),
                                      small_ctx.stylize(c, s, SMALL, alpha=alpha, **kw)), (alpha, kw)


def test_float_images_are_handed_over_as_float32(small_ctx):
    c = synthetic_image(133, 64, 64).astype(np.float64) * 0.9 + 3.3
    s = synthetic_image(134, 72, 64).astype(np.float64) * 0.8 + 7.7
    with small_ctx.prepare_style(s, SMALL) as h:
        assert np.array_equal(small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8), small_ctx.stylize(c, s, SMALL, alpha=0.8))


@pytest.mark.parametrize('batch', [1, 8, 32])
def test_prepared_batch_is_the_shared_style_batch(small_ctx, batch):
    frames = np.stack([synthetic_image(140 + i, 64, 80) for i in range(batch)])
    s = synthetic_image(139, 96, 64)
    with small_ctx.prepare_style(s, SMALL) as h:
        for kw in MODES:
            got = small_ctx.stylize_prepared_batch(frames, h, SMALL, alpha=0.8, **kw)
            assert np.array_equal(got, small_ctx.stylize_batch(frames, s, SMALL, alpha=0.8, **kw)), (batch, kw)


def _model(weights_seed=5, targets=SMALL):
    from wct_tf_amd.wct import WCT
    return WCT(None, targets, None, weights=synthetic_weights(weights_seed, relu_targets=targets))


def test_predict_frames_with_a_handle(small_ctx):
    model = _model()
    try:
        frames = np.stack([synthetic_image(150 + i, 64, 64) for i in range(7)])
        s = synthetic_image(149, 80, 80)
        h = model.prepare_style(s)
        got = model.predict_frames(frames, h, alpha=0.8, batch=3)               # 7 frames, batches of 3: 3 + 3 + 1
        assert np.array_equal(got, model.predict_frames(frames, s, alpha=0.8, batch=3))
        for i in (0, 6):
            assert np.array_equal(got[i], model.predict(frames[i], s, alpha=0.8))
            assert np.array_equal(got[i], model.predict(frames[i], h, alpha=0.8))
    finally:
        model.sess.close()


def _matrices(stats):
    return sum(v['matrices'] for v in stats.values())


def test_the_style_side_is_skipped_not_recomputed(small_ctx):
    c = synthetic_image(161, 96, 96)
    styles = [synthetic_image(162, 96, 96), synthetic_image(163, 80, 64), synthetic_image(164, 112, 96)]
    handles = [small_ctx.prepare_style(s, SMALL) for s in styles]
    try:
        small_ctx.stylize_prepared(c, handles[0], SMALL, alpha=0.8)             # warm: every state this content needs exists
        small_ctx.stylize_prepared_mix(c, handles, [1, 2, 3], SMALL, alpha=0.8)
        small_ctx.eig_stats()
        small_ctx.stylize(c, styles[0], SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == 2 * len(SMALL)               # content and style of every level
        small_ctx.stylize_prepared(c, handles[0], SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == len(SMALL)                   # the content alone
        small_ctx.stylize_mix(c, styles, [1, 2, 3], SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == 4 * len(SMALL)
        small_ctx.stylize_prepared_mix(c, handles, [3, 2, 1], SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == len(SMALL)
    finally:
        for h in handles:
            h.close()


@pytest.mark.parametrize('kw', MODES)
def test_predict_mix_with_handles_is_predict_mix(small_ctx, kw):
    c = synthetic_image(171, 96, 96)
    styles = [synthetic_image(172, 128, 96), synthetic_image(173, 64, 80), synthetic_image(174, 96, 96)]
    handles = [small_ctx.prepare_style(s, SMALL) for s in styles]
    try:
        for k in (2, 3):
            # the largest weight moves from style 0 (larger than the content) to style 1 (smaller): the content's layout moves
            for weights in ([3, 1, 0.5][:k], [1, 3, 0.5][:k]):
                got = small_ctx.stylize_prepared_mix(c, handles[:k], weights, SMALL, alpha=0.7, **kw)
                assert np.array_equal(got, small_ctx.stylize_mix(c, styles[:k], weights, SMALL, alpha=0.7, **kw)), (k, weights, kw)
        for one in range(3):
            weights = [1.0 if i == one else 0.0 for i in range(3)]
            got = small_ctx.stylize_prepared_mix(c, handles, weights, SMALL, alpha=0.7, **kw)
            assert np.array_equal(got, small_ctx.stylize(c, styles[one], SMALL, alpha=0.7, **kw)), (one, kw)
        got = small_ctx.stylize_prepared_mix(c, [handles[1], handles[1]], [1, 2], SMALL, alpha=0.7, **kw)     # one handle twice
        assert np.array_equal(got, small_ctx.stylize_mix(c, [styles[1], styles[1]], [1, 2], SMALL, alpha=0.7, **kw))
    finally:
        for h in handles:
            h.close()


def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib = small_ctx.lib
    c = np.ascontiguousarray(synthetic_image(181, 64, 64))
    s = np.ascontiguousarray(synthetic_image(182, 64, 80))
    u8p = lambda a: a.ctypes.data_as(_lib._U8)
    lv = (C.c_int * 3)(3, 2, 1)
    out = np.zeros((64, 64, 3), np.uint8)
    want = small_ctx.stylize(c, s, SMALL, alpha=0.7)

    def prepare(levels, flags=0):
        h = C.c_void_p()
        arr = (C.c_int * len(levels))(*levels)
        return lib.wct_style_prepare(small_ctx.h, u8p(s), 64, 80, arr, len(levels), flags, C.byref(h)), h

    def single(h, levels=lv, n=3, flags=0):
        return lib.wct_stylize_prepared(small_ctx.h, u8p(c), 64, 64, h, levels, n, C.c_float(0.7), flags, u8p(out))

    def mix(hs, weights, flags=0):
        arr = (C.c_void_p * max(len(hs), 1))(*[h.value for h in hs])
        w = np.ascontiguousarray(weights, np.float32) if len(weights) else np.zeros(1, np.float32)
        return lib.wct_stylize_prepared_mix(small_ctx.h, u8p(c), 64, 64, arr, len(hs), _lib.fptr(w), lv, 3, C.c_float(0.7), flags, u8p(out))

    def refused(rc, status):
        assert rc == status, (rc, status, lib.wct_last_error())
        assert lib.wct_last_error()

    for flags in (_lib.FLAG_SWAP5, _lib.FLAG_STYLE_SHARED):
        rc, h = prepare([3, 2, 1], flags)
        refused(rc, -2)
        assert not h.value
    refused(prepare([6])[0], -2)
    rc, h = prepare([3, 2, 1])
    assert rc == 0 and h.value
    rc, h21 = prepare([2, 1])
    assert rc == 0
    refused(single(h, flags=_lib.FLAG_SWAP5), -2)
    refused(single(h, flags=_lib.FLAG_STYLE_SHARED), -2)
    refused(single(h21), -2)                                            # relu3_1 is not in that handle's set
    refused(mix([h, h], [1, 1], _lib.FLAG_SWAP5), -2)
    refused(mix([], []), -2)                                            # K outside 1 .. 8
    refused(mix([h] * 9, [1] * 9), -2)
    refused(mix([h, h], [1, -1]), -2)
    refused(mix([h, h21], [1, 1]), -2)
    refused(lib.wct_stylize_prepared_batch_dev(small_ctx.h, None, 64, 64, 1, h, lv, 3, C.c_float(0.7), 0, None), -2)
    assert single(h) == 0 and np.array_equal(out, want)                # ... and the context still works
    lib.wct_style_free(small_ctx.h, h21)
    refused(single(h21, (C.c_int * 2)(2, 1), 2), -3)                   # a freed handle
    lib.wct_style_free(small_ctx.h, h21)                                # freeing twice is a no-op
    out[:] = 0
    assert mix([h, h], [1, 0]) == 0 and np.array_equal(out, want)
    from wct_tf_amd.context import Context
    other = Context(0)
    try:
        other.set_weights(synthetic_weights(5, relu_targets=SMALL))
        out[:] = 0
        rc = lib.wct_stylize_prepared(other.h, u8p(c), 64, 64, h, lv, 3, C.c_float(0.7), 0, u8p(out))
        refused(rc, -3)                                                 # another context's handle
        assert np.array_equal(other.stylize(c, s, SMALL, alpha=0.7), want)
    finally:
        other.close()
    lib.wct_style_free(small_ctx.h, h)
    assert np.array_equal(small_ctx.stylize(c, s, SMALL, alpha=0.7), want)


def test_python_refusals_with_a_real_context(small_ctx):
    from wct_tf_amd.context import Context
    s = synthetic_image(185, 64, 64)
    h = small_ctx.prepare_style(s, SMALL)
    other = Context(0)
    try:
        with pytest.raises(ValueError, match='another context'):
            other.stylize_prepared(s, h, SMALL)
        with pytest.raises(ValueError, match='relu levels'):
            small_ctx.stylize_prepared(s, small_ctx.prepare_style(s, ['relu1_1']), SMALL)
        h.close()
        with pytest.raises(ValueError, match='closed'):
            small_ctx.stylize_prepared(s, h, SMALL)
    finally:
        other.close()


def test_video_cli_frames_are_predict_frames(tmp_path):
    from wct_tf_amd import utils
    from wct_tf_amd.stylize_video import main
    targets = ['relu3_1', 'relu1_1']
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    frames = [synthetic_image(500 + i, 48, 64) for i in range(7)]
    for i, f in enumerate(frames):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), f)
    style = synthetic_image(600, 56, 48)
    utils.save_img(str(tmp_path / 'style.png'), style)
    out_dir = tmp_path / 'out'
    n = main(['--relu-targets'] + targets + ['--in-path', str(in_dir), '--style-path', str(tmp_path / 'style.png'),
              '--out-path', str(out_dir), '--alpha', '0.8', '--synthetic-weights', '42', '--batch', '3'])
    assert n == 7
    model = _model(42, targets)
    try:
        for i, f in enumerate(frames):
            got = utils.get_img(str(out_dir / 'clip_style' / ('frame_%d.png' % (i + 1))))
            assert np.array_equal(got, model.predict(f, style, 0.8)), i
    finally:
        model.sess.close()


def test_stylize_cli_prepares_each_style_once(tmp_path):
    from wct_tf_amd import stylize, utils
    cdir, sdir = tmp_path / 'c', tmp_path / 's'
    cdir.mkdir()
    sdir.mkdir()
    contents = {'c0': synthetic_image(31, 64, 64), 'c1': synthetic_image(32, 80, 64)}
    styles = {'a': synthetic_image(33, 64, 48), 'b': synthetic_image(34, 48, 72)}
    for d, imgs in ((cdir, contents), (sdir, styles)):
        for name, img in imgs.items():
            utils.save_img(str(d / (name + '.png')), img)
    base = ['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--content-path', str(cdir), '--alpha', '0.8']
    out1, out2 = str(tmp_path / 'o1'), str(tmp_path / 'o2')
    assert stylize.main(base + ['--out-path', out1, '--interp-styles', str(sdir / 'a.png'), str(sdir / 'b.png'),
                                '--interp-weights', '1', '3']) == 2
    assert stylize.main(base + ['--out-path', out2, '--style-path', str(sdir), '--passes', '2']) == 4
    model = _model()
    try:
        for cn, c in contents.items():
            want = model.predict_mix(c, [styles['a'], styles['b']], [1, 3], 0.8)
            assert np.array_equal(utils.get_img(os.path.join(out1, '%s_a+b.png' % cn)), want), cn
            for sn, s in styles.items():
                want = model.predict(model.predict(c, s, 0.8), s, 0.8)
                assert np.array_equal(utils.get_img(os.path.join(out2, '%s_%s.png' % (cn, sn))), want), (cn, sn)
    finally:
        model.sess.close()


def test_a_hundred_handles_and_destroy_with_live_ones():
    from wct_tf_amd.context import Context
    ctx = Context(0)
    try:
        ctx.set_weights(synthetic_weights(5, relu_targets=SMALL))
        c, s = synthetic_image(191, 64, 64), synthetic_image(192, 64, 64)
        want = ctx.stylize(c, s, SMALL, alpha=0.8)
        for i in range(100):
            h = ctx.prepare_style(synthetic_image(200 + i % 3, 64, 64) if i % 10 else s, SMALL)
            if i % 25 == 0:
                assert np.array_equal(ctx.stylize_prepared(c, ctx.prepare_style(s, SMALL), SMALL, alpha=0.8), want)
            h.close()
        live = [ctx.prepare_style(s, SMALL) for _ in range(3)]
        assert np.array_equal(ctx.stylize_prepared(c, live[1], SMALL, alpha=0.8), want)
    finally:
        ctx.close()                                                    # wct_destroy frees the three live handles
    assert all(h.closed for h in live)
    for h in live:
        h.close()                                                      # nothing left to free, nothing touched
