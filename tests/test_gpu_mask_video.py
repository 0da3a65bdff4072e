"""Masked video on the GPU: spatial control with prepared styles (wct_stylize_prepared_masked) and on a batch of frames with one
label map each (wct_stylize_prepared_masked_batch_dev).  Every check is np.array_equal against a call that the oracle tests
already pin -- wct_stylize_masked (tests/test_gpu_mask.py) and the prepared calls (tests/test_gpu_prepared.py); no tolerance.
Synthetic weights as in the neighbouring files."""
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


def blobs(seed, h, w, k):
    """blob-shaped random labels 0 .. k-1: the argmax of k smoothed noise fields (tests/test_gpu_mask.py)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((k, h, w))
    for _ in range(4):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5
    return np.uint8(np.argmax(f, 0))


def _matrices(stats):
    return sum(v['matrices'] for v in stats.values())


class Handles(object):
    def __init__(self, ctx, styles, targets=SMALL):
        self.hs = [ctx.prepare_style(s, targets) for s in styles]

    def __enter__(self):
        return self.hs

    def __exit__(self, *exc):
        for h in self.hs:
            h.close()


# ---- 1. handles = images -------------------------------------------------------------------------------------------------
# content size, style sizes: content larger than / equal to / smaller than the styles, styles of different sizes, and level
# widths that are not multiples of 16 (100 x 84)
CASES = [((128, 144), [(64, 64), (80, 96), (64, 72)]), ((96, 96), [(96, 96), (96, 96), (96, 96)]),
         ((64, 80), [(128, 112), (96, 144), (160, 96)]), ((100, 84), [(90, 70), (120, 100), (64, 64)])]


@pytest.mark.parametrize('kw', MODES)
@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('csize,ssizes', CASES)
def test_handles_are_the_images(small_ctx, kw, k, csize, ssizes):
    c = synthetic_image(301, *csize)
    styles = [synthetic_image(310 + i, *s) for i, s in enumerate(ssizes[:k])]
    mask = blobs(k * 7 + csize[0], csize[0], csize[1], k)
    want = small_ctx.stylize_masked(c, styles, mask, SMALL, alpha=0.8, **kw)
    with Handles(small_ctx, styles) as hs:
        got = small_ctx.stylize_prepared_masked(c, hs, mask, SMALL, alpha=0.8, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (kw, k, csize)


@pytest.mark.parametrize('kw', MODES)
def test_handles_are_the_images_five_levels(full_ctx, kw):
    c = synthetic_image(321, 144, 128)
    styles = [synthetic_image(322, 96, 112), synthetic_image(323, 160, 128)]
    mask = blobs(324, 144, 128, 2)
    want = full_ctx.stylize_masked(c, styles, mask, RELU_TARGETS, alpha=0.8, **kw)
    with Handles(full_ctx, styles, RELU_TARGETS) as hs:
        assert np.array_equal(full_ctx.stylize_prepared_masked(c, hs, mask, RELU_TARGETS, alpha=0.8, **kw), want), kw


def test_float_images_are_handed_over_as_float32(small_ctx):
    c = synthetic_image(331, 80, 64).astype(np.float32) * 0.9 + 3.3
    styles = [synthetic_image(332, 72, 64).astype(np.float64) * 0.8 + 7.7, synthetic_image(333, 64, 96).astype(np.float32) + 0.4]
    mask = blobs(334, 80, 64, 2)
    with Handles(small_ctx, styles) as hs:
        for kw in MODES:
            assert np.array_equal(small_ctx.stylize_prepared_masked(c, hs, mask, SMALL, alpha=0.8, **kw),
                                  small_ctx.stylize_masked(c, styles, mask, SMALL, alpha=0.8, **kw)), kw


# ---- 2. batch = single frames --------------------------------------------------------------------------------------------
def _special_masks(n, h, w, k):
    """n >= 5 label maps for k = 3 styles, all different: blobs, then a map without label 1, one where label 2 has exactly one
    pixel at the deepest of three levels (a 4 x 4 block on the stride-4 grid), one that is all label 0 and one all label 2"""
    masks = [blobs(400 + f, h, w, k) for f in range(n)]
    masks[1] = np.where(masks[1] == 1, 2, masks[1]).astype(np.uint8)
    masks[2] = np.uint8(blobs(450, h, w, 2))
    masks[2][8:12, 12:16] = 2
    masks[3] = np.zeros((h, w), np.uint8)
    masks[4] = np.full((h, w), 2, np.uint8)
    return np.stack(masks)


@pytest.mark.parametrize('kw', MODES)
def test_batch_frames_are_the_single_frames(small_ctx, kw):
    B, k, (h, w) = 14, 3, (64, 80)                                # B k = 42 live pairs at most: two groups per level
    frames = np.stack([synthetic_image(340 + f, h, w) for f in range(B)])
    styles = [synthetic_image(360, 64, 64), synthetic_image(361, 48, 64), synthetic_image(362, 96, 80)]
    masks = _special_masks(B, h, w, k)
    assert not (masks[1] == 1).any() and (masks[2][::4, ::4] == 2).sum() == 1 and (masks[2][::2, ::2] == 2).sum() == 4
    assert sum(len(np.unique(m)) for m in masks) > 32            # the grouping is forced at the shallow levels
    with Handles(small_ctx, styles) as hs:
        got = small_ctx.stylize_prepared_masked_batch(frames, hs, masks, SMALL, alpha=0.8, **kw)
        for f in range(B):
            assert np.array_equal(got[f], small_ctx.stylize_prepared_masked(frames[f], hs, masks[f], SMALL, alpha=0.8, **kw)), (f, kw)
        for f in (0, 1, 2, 3):
            assert np.array_equal(got[f], small_ctx.stylize_masked(frames[f], styles, masks[f], SMALL, alpha=0.8, **kw)), (f, kw)
        back = small_ctx.stylize_prepared_masked_batch(frames[::-1], hs, masks[::-1], SMALL, alpha=0.8, **kw)
        assert np.array_equal(back, got[::-1]), kw


def test_batch_of_32_frames_and_one_mask_for_all(small_ctx):
    B, (h, w) = 32, (48, 64)
    frames = np.stack([synthetic_image(370 + f, h, w) for f in range(B)])
    styles = [synthetic_image(402, 64, 48), synthetic_image(403, 48, 48)]
    mask = blobs(404, h, w, 2)
    with Handles(small_ctx, styles) as hs:
        got = small_ctx.stylize_prepared_masked_batch(frames, hs, mask, SMALL, alpha=0.7)        # 64 pairs: two groups
        for f in (0, 15, 16, 31):
            assert np.array_equal(got[f], small_ctx.stylize_masked(frames[f], styles, mask, SMALL, alpha=0.7)), f


# ---- 3. collapse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', MODES)
def test_k1_all_zero_masks_is_the_prepared_batch(small_ctx, kw):
    frames = np.stack([synthetic_image(410 + f, 64, 80) for f in range(5)])
    s = synthetic_image(409, 96, 64)
    with Handles(small_ctx, [s]) as hs:
        got = small_ctx.stylize_prepared_masked_batch(frames, hs, np.zeros((5, 64, 80), np.uint8), SMALL, alpha=0.8, **kw)
        assert np.array_equal(got, small_ctx.stylize_prepared_batch(frames, hs[0], SMALL, alpha=0.8, **kw)), kw
        assert np.array_equal(got[2], small_ctx.stylize(frames[2], s, SMALL, alpha=0.8, **kw)), kw


# ---- 4. many keys --------------------------------------------------------------------------------------------------------
def test_more_keys_than_the_cache_keeps(small_ctx):
    """a content at twice the style's side, label 1 covering 1/16 .. 15/16 of the frame: region 0 of frames 0 .. 4 is larger than
    the style map at every level and has five different sizes, so handle 0 needs five keys besides the one it was prepared
    with -- more than the four a level's cache keeps between calls"""
    shares = [1, 3, 5, 8, 11, 13, 15]                               # sixteenths of the width under label 1
    B, side = len(shares), 128
    frames = np.stack([synthetic_image(420 + f, side, side) for f in range(B)])
    styles = [synthetic_image(430, 64, 64), synthetic_image(431, 64, 64)]
    masks = np.zeros((B, side, side), np.uint8)
    for f, s in enumerate(shares):
        masks[f, :, side - s * side // 16:] = 1
    # the premise, at relu1_1 (style map 64 x 64 = 4096 rows; a pair's statistics slabs are ceil(max(N, Ns) / 64), at most 256):
    # region 0 has 15360, 13312, 11264, 8192, 5120, 3072 and 1024 rows -> 240, 208, 176, 128, 80 slabs and twice the style's 64
    slabs = {min(256, -(-max(int((m == 0).sum()), 64 * 64) // 64)) for m in masks}
    assert slabs == {240, 208, 176, 128, 80, 64} and len(slabs) > 4
    live = len(SMALL) * B * 2
    with Handles(small_ctx, styles) as hs:
        first = small_ctx.stylize_prepared_masked_batch(frames, hs, masks, SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) > live              # the fills ran style eigensolves
        again = small_ctx.stylize_prepared_masked_batch(frames, hs, masks, SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == live             # no new state: the live regions' matrices alone
        assert np.array_equal(first, again)
        for f in range(B):
            assert np.array_equal(again[f], small_ctx.stylize_prepared_masked(frames[f], hs, masks[f], SMALL, alpha=0.8)), f
        for f in (0, 3, 6):
            assert np.array_equal(again[f], small_ctx.stylize_masked(frames[f], styles, masks[f], SMALL, alpha=0.8)), f


# ---- 5. the style side is really skipped ---------------------------------------------------------------------------------
def test_the_style_side_is_skipped_not_recomputed(small_ctx):
    c = synthetic_image(441, 96, 96)
    styles = [synthetic_image(442, 96, 96), synthetic_image(443, 80, 64)]
    mask = blobs(444, 96, 96, 2)
    with Handles(small_ctx, styles) as hs:
        small_ctx.stylize_prepared_masked(c, hs, mask, SMALL, alpha=0.8)          # warm: every state this call needs exists
        small_ctx.eig_stats()
        small_ctx.stylize_masked(c, styles, mask, SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == 2 * 2 * len(SMALL)             # region and style, two regions a level
        small_ctx.stylize_prepared_masked(c, hs, mask, SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == 2 * len(SMALL)                 # the regions alone
        frames = np.stack([c, c[::-1].copy(), c[:, ::-1].copy()])
        small_ctx.stylize_prepared_masked_batch(frames, hs, mask, SMALL, alpha=0.8)
        assert _matrices(small_ctx.eig_stats()) == 3 * 2 * len(SMALL)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib = small_ctx.lib
    c = np.ascontiguousarray(synthetic_image(451, 64, 64))
    styles = [np.ascontiguousarray(synthetic_image(452 + k, 64, 80)) for k in range(2)]
    u8p = lambda a: a.ctypes.data_as(_lib._U8)
    lv = (C.c_int * 3)(3, 2, 1)
    out = np.zeros((64, 64, 3), np.uint8)
    mask = blobs(455, 64, 64, 2)
    want = small_ctx.stylize_masked(c, styles, mask, SMALL, alpha=0.7)

    def prepare(img, levels):
        h = C.c_void_p()
        arr = (C.c_int * len(levels))(*levels)
        assert lib.wct_style_prepare(small_ctx.h, u8p(img), 64, 80, arr, len(levels), 0, C.byref(h)) == 0
        return h

    def single(hs, m=mask, flags=0, levels=lv, n=3, ctx=small_ctx):
        arr = (C.c_void_p * max(len(hs), 1))(*[h.value for h in hs])
        m = np.ascontiguousarray(m, np.uint8)
        return lib.wct_stylize_prepared_masked(ctx.h, u8p(c), 64, 64, u8p(m), arr, len(hs), levels, n, C.c_float(0.7), flags, u8p(out))

    def refused(rc, status):
        assert rc == status, (rc, status, lib.wct_last_error())
        assert lib.wct_last_error()

    h0, h1 = prepare(styles[0], [3, 2, 1]), prepare(styles[1], [3, 2, 1])
    h21 = prepare(styles[1], [2, 1])
    refused(single([h0, h1], flags=_lib.FLAG_SWAP5), -2)
    refused(single([h0, h1], flags=_lib.FLAG_STYLE_SHARED), -2)
    refused(single([h0, h1], m=mask + 1), -2)                           # a label >= K
    refused(single([]), -2)                                             # K outside 1 .. 8
    refused(single([h0] * 9, m=mask * 0), -2)
    refused(single([h0, h21]), -2)                                      # relu3_1 is not in that handle's set
    refused(lib.wct_stylize_prepared_masked_batch_dev(small_ctx.h, None, 64, 64, 1, u8p(mask), (C.c_void_p * 2)(h0.value, h1.value), 2,
                                                      lv, 3, C.c_float(0.7), 0, None), -2)
    assert single([h0, h1]) == 0 and np.array_equal(out, want)          # ... and the context still works
    lib.wct_style_free(small_ctx.h, h21)
    refused(single([h0, h21], levels=(C.c_int * 2)(2, 1), n=2), -3)     # a freed handle
    from wct_tf_amd.context import Context
    other = Context(0)
    try:
        other.set_weights(synthetic_weights(5, relu_targets=SMALL))
        out[:] = 0
        refused(single([h0, h1], ctx=other), -3)                        # another context's handles
        assert np.array_equal(other.stylize_masked(c, styles, mask, SMALL, alpha=0.7), want)
    finally:
        other.close()
    out[:] = 0
    assert single([h0, h1]) == 0 and np.array_equal(out, want)
    lib.wct_style_free(small_ctx.h, h0)
    lib.wct_style_free(small_ctx.h, h1)
    assert np.array_equal(small_ctx.stylize_masked(c, styles, mask, SMALL, alpha=0.7), want)


# ---- 7. facade and CLI ---------------------------------------------------------------------------------------------------
def _model(weights_seed=5, targets=SMALL):
    from wct_tf_amd.wct import WCT
    return WCT(None, targets, None, weights=synthetic_weights(weights_seed, relu_targets=targets))


def test_predict_frames_masked_and_predict_masked_with_handles():
    model = _model()
    try:
        frames = np.stack([synthetic_image(460 + i, 64, 64) for i in range(7)])
        styles = [synthetic_image(470, 80, 80), synthetic_image(471, 64, 48)]
        masks = np.stack([blobs(480 + i, 64, 64, 2) for i in range(7)])
        want = [model.predict_masked(frames[i], styles, masks[i], alpha=0.8) for i in range(7)]
        got = model.predict_frames_masked(frames, styles, masks, alpha=0.8, batch=3)           # 3 + 3 + 1, prepared inside
        assert got.shape == (7, 64, 64, 3) and all(np.array_equal(got[i], want[i]) for i in range(7))
        handles = [model.prepare_style(s) for s in styles]
        assert np.array_equal(model.predict_frames_masked(frames, handles, masks, alpha=0.8, batch=16), got)
        for i in (0, 6):
            assert np.array_equal(model.predict_masked(frames[i], handles, masks[i], alpha=0.8), want[i])
        shared = model.predict_frames_masked(frames, handles, masks[0], alpha=0.8, adain=True)    # one map for every frame
        for i in (0, 3, 6):
            assert np.array_equal(shared[i], model.predict_masked(frames[i], styles, masks[0], alpha=0.8, adain=True))
    finally:
        model.sess.close()


def test_video_cli_mask_directory_end_to_end(tmp_path):
    from PIL import Image
    from wct_tf_amd import stylize, utils
    from wct_tf_amd.stylize_video import main
    targets = ['relu3_1', 'relu1_1']
    in_dir, mask_dir = tmp_path / 'clip', tmp_path / 'maps'
    in_dir.mkdir()
    mask_dir.mkdir()
    frames = [synthetic_image(500 + i, 48, 64) for i in range(5)]
    greys = [np.uint8(blobs(520 + i, 24, 32, 2) * 255) for i in range(5)]                       # maps at half the frame's size
    for i in range(5):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), frames[i])
        Image.fromarray(greys[i]).save(str(mask_dir / ('map_%d.png' % (i + 1))))
    styles = [synthetic_image(600, 56, 48), synthetic_image(601, 48, 72)]
    for name, s in zip('ab', styles):
        utils.save_img(str(tmp_path / (name + '.png')), s)
    out_dir = tmp_path / 'out'
    n = main(['--relu-targets'] + targets + ['--in-path', str(in_dir), '--mask-path', str(mask_dir), '--mask-styles',
              str(tmp_path / 'a.png'), str(tmp_path / 'b.png'), '--out-path', str(out_dir), '--alpha', '0.8',
              '--synthetic-weights', '42', '--batch', '2', '--passes', '2'])
    assert n == 5
    model = _model(42, targets)
    try:
        for i, f in enumerate(frames):
            got = utils.get_img(str(out_dir / 'clip_mask_a+b' / ('frame_%d.png' % (i + 1))))
            want = f
            for _ in range(2):
                want = model.predict_masked(want, styles, stylize.mask_labels(greys[i], 2, want.shape[:2]), 0.8)
            assert np.array_equal(got, want), i
    finally:
        model.sess.close()


def test_stylize_cli_mask_prepares_each_style_once(tmp_path):
    from PIL import Image
    from wct_tf_amd import stylize, utils
    cdir = tmp_path / 'c'
    cdir.mkdir()
    contents = {'c0': synthetic_image(31, 64, 64), 'c1': synthetic_image(32, 80, 64)}
    styles = {'a': synthetic_image(33, 64, 48), 'b': synthetic_image(34, 48, 72)}
    for name, img in contents.items():
        utils.save_img(str(cdir / (name + '.png')), img)
    for name, img in styles.items():
        utils.save_img(str(tmp_path / (name + '.png')), img)
    grey = np.uint8(blobs(35, 32, 32, 2) * 255)
    Image.fromarray(grey).save(str(tmp_path / 'm.png'))
    out = str(tmp_path / 'o')
    assert stylize.main(['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--content-path', str(cdir), '--alpha', '0.8',
                         '--out-path', out, '--mask-path', str(tmp_path / 'm.png'), '--mask-styles', str(tmp_path / 'a.png'),
                         str(tmp_path / 'b.png')]) == 2
    model = _model()
    try:
        for cn, c in contents.items():
            want = model.predict_masked(c, [styles['a'], styles['b']], stylize.mask_labels(grey, 2, c.shape[:2]), 0.8)
            assert np.array_equal(utils.get_img(os.path.join(out, '%s_mask_a+b.png' % cn)), want), cn
    finally:
        model.sess.close()


# ---- 8. compaction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,stride', [(64, 80, 1), (97, 75, 2), (160, 144, 1)])
def test_batched_partition_is_the_partition_of_every_frame(small_ctx, h, w, stride):
    k, B = 3, 6
    masks = np.stack([blobs(700 + f, h, w, k) for f in range(B)])
    masks[1][masks[1] == 1] = 0                                     # a frame without label 1
    masks[2][:] = 2                                                 # a frame that is all one label
    fh, fw = -(-h // stride), -(-w // stride)
    perm, seg = small_ctx.mask_compact_batch(masks, fh, fw, stride, k)
    assert perm.shape == (B, fh * fw) and seg.shape == (B, k + 1)
    for f in range(B):
        p1, s1 = small_ctx.mask_compact(masks[f], fh, fw, stride, k)
        assert np.array_equal(perm[f], p1) and np.array_equal(seg[f], s1), f
