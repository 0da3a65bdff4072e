"""On-device resize on the GPU (csrc/resize.hip, the resize entry points of csrc/api_ops.hip): the op against Pillow itself at
the smallest sizes where the kernel can go wrong, batches at shifted output bases between guard bytes, the chain -- raw frames
in, resized on the device, stylized -- against the same call on Pillow's frames, the refusals of the C ABI, and the command
line.  Everything is np.array_equal: the rule is integers only, and the chain runs the launches of the prepared calls.
Synthetic weights as in tests/test_gpu_texture.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_oracle as oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
ARG = -2
# the kernel's tiling (csrc/resize.hip): 64 output columns, the first height of the list whose tallest tile fits 16 KB
TILE_W, LDS_BYTES, TILE_HEIGHTS = 64, 16384, (32, 16, 8, 4, 2, 1)


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


def _tile_height(H, h, w):
    """the launcher's choice, restated: None where it refuses"""
    bounds, _ = oracle.taps(H, h)
    lo, hi = bounds[:, 0].astype(int), (bounds[:, 0] + bounds[:, 1]).astype(int)
    for th in TILE_HEIGHTS:
        if max(hi[min(y0 + th, h) - 1] - lo[y0] for y0 in range(0, h, th)) * min(TILE_W, w) * 3 <= LDS_BYTES:
            return th
    return None


@functools.lru_cache(maxsize=None)
def _case(H, W, h, w):
    img = oracle.random_image(H * 31 + W, H, W)
    img.setflags(write=False)
    want = oracle.pillow(img, h, w)
    want.setflags(write=False)
    return img, want


# ---- the op against Pillow ---------------------------------------------------------------------------------------------------
# The last three are the sizes the implementation chose.  (64, 128) -> (32, 64): exactly one tile of 32 rows x 64 columns, no
# ragged edge anywhere.  (70, 130) -> (33, 65): that tile plus one row and one column -- a second tile row of one output row
# and a second tile column of one output column (spans of 3 bytes: head and tail only, never a whole group).  (40, 400) ->
# (20, 200): rows of 600 bytes that are no multiple of 16, four tile columns the last of 8 columns, every output row at another
# alignment.  (1200, 8) -> (4, 8) forces the smallest tile height: one output row taps 600 input rows of 24 bytes, two tap 750.
GEOMETRIES = [(1, 1, 3, 2), (2, 2, 1, 1), (3, 3, 1, 1), (70, 1, 35, 1), (1, 9, 4, 3), (5, 7, 96, 96), (37, 53, 24, 35),
              (300, 200, 77, 51), (64, 64, 64, 31), (64, 64, 31, 64), (513, 511, 512, 512), (64, 48, 64, 48), (1200, 8, 4, 8),
              (64, 128, 32, 64), (70, 130, 33, 65), (40, 400, 20, 200)]


def test_the_geometries_are_what_the_comment_says():
    assert _tile_height(1200, 4, 8) == 1 and _tile_height(64, 32, 64) == 32 and _tile_height(70, 33, 65) == 32
    assert _tile_height(5, 96, 96) == 32 and _tile_height(300, 77, 51) == 16 and _tile_height(2000, 4, 64) is None
    assert oracle.ksize(300, 77) > 3 and oracle.ksize(200, 51) > 3


@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: '%dx%d-%dx%d' % g)
def test_resize_op_is_pillow(small, geom):
    H, W, h, w = geom
    img, want = _case(H, W, h, w)
    got = small.sess.resize(img, (h, w))
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, want)
    assert np.array_equal(want, oracle.resize(img, h, w))           # (and Pillow is the rule)
    for v in (0, 255):
        assert np.all(small.sess.resize(np.full((H, W, 3), v, np.uint8), (h, w)) == v), v
    if (H, W) == (h, w):
        assert np.array_equal(got, img)


def test_resize_op_on_a_checkerboard(small):
    img = oracle.checkerboard(97, 131)
    for h, w in ((40, 60), (200, 300), (97, 60)):
        assert np.array_equal(small.sess.resize(img, (h, w)), oracle.pillow(img, h, w)), (h, w)


def test_geometries_alternate_on_one_context(small):
    """the tables of the last geometry stay in the ctx: a change replaces them, a change back builds them again"""
    ctx = small.sess
    for geom in [(37, 53, 24, 35), (5, 7, 96, 96), (37, 53, 24, 35), (53, 37, 24, 35), (37, 53, 24, 35)]:
        img, want = _case(*geom)
        assert np.array_equal(ctx.resize(img, geom[2:]), want), geom


# ---- batches -----------------------------------------------------------------------------------------------------------------
GUARD = 16


def _resize_dev(ctx, frames, h, w, offset):
    """wct_resize_batch_dev into a buffer of its own, the output base `offset` bytes off the (at least 16-byte) alignment of the
    allocation; the bytes in front of the output and the GUARD bytes behind it must come back untouched"""
    b, hi, wi = frames.shape[:3]
    n = b * h * w * 3
    fill = np.full(offset + n + GUARD, 0xA5, np.uint8)
    src, buf = ctx.dev_alloc(frames.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(src, frames)
        ctx.h2d(buf, fill)
        ctx.resize_batch_dev(src, hi, wi, b, (h, w), C.c_void_p(buf.value + offset))
        ctx.sync()
        got = np.empty_like(fill)
        ctx.d2h(got, buf)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(buf)
    assert np.all(got[:offset] == 0xA5) and np.all(got[offset + n:] == 0xA5), (b, offset)
    return got[offset:offset + n].reshape(b, h, w, 3)


@pytest.mark.parametrize('b', [1, 3, 32])
def test_batches_at_shifted_bases_between_guards(small, b):
    ctx = small.sess
    H, W, h, w = 37, 53, 24, 35
    frames = np.stack([oracle.random_image(100 + f, H, W) for f in range(b)])
    want = np.stack([oracle.pillow(f, h, w) for f in frames])
    for offset in (0, 1, 5):
        got = _resize_dev(ctx, frames, h, w, offset)
        assert np.array_equal(got, want), (b, offset)
    for f in (0, b // 2, b - 1):                                     # frame f is the single-image op
        assert np.array_equal(want[f], ctx.resize(frames[f], (h, w))), f
    assert np.array_equal(ctx.resize_batch(frames, (h, w)), want)


def test_a_copy_and_an_upscale_in_a_batch(small):
    frames = np.stack([oracle.random_image(200 + f, 64, 48) for f in range(3)])
    assert np.array_equal(_resize_dev(small.sess, frames, 64, 48, 5), frames)
    up = np.stack([oracle.random_image(210 + f, 5, 7) for f in range(3)])
    assert np.array_equal(_resize_dev(small.sess, up, 96, 96, 1), np.stack([oracle.pillow(f, 96, 96) for f in up]))


# ---- the chain ---------------------------------------------------------------------------------------------------------------
RAW, SIZE = (96, 128), (48, 64)


@functools.lru_cache(maxsize=None)
def _frames(n=3):
    raw = np.stack([synthetic_image(300 + f, *RAW) for f in range(n)])
    return raw, np.stack([utils._imresize(f, SIZE) for f in raw])


@pytest.mark.parametrize('case', ['plain', 'content-colors', 'warm', 'np', 'adain'])
def test_chain_is_the_call_on_pillows_frames(small, case):
    raw, resized = _frames()
    kw = dict(alpha=0.8, batch=2)                                     # two batches: 2 + 1 frames
    if case == 'content-colors':
        kw['content_colors'] = True
    if case == 'adain':
        kw['adain'] = True
    keep, small.wct_mode = small.wct_mode, 'np' if case == 'np' else small.wct_mode
    try:
        with small.prepare_style(synthetic_image(31, 72, 64), adain=case == 'adain') as handle:
            warm = [small.warm_state(), small.warm_state()] if case == 'warm' else [None, None]
            try:
                want = small.predict_frames(resized, handle, warm=warm[0], **kw)
                got = small.predict_frames(raw, handle, warm=warm[1], resize=SIZE, **kw)
            finally:
                for s in warm:
                    if s is not None:
                        s.close()
        assert got.dtype == np.uint8 and got.shape == want.shape == (3,) + SIZE + (3,)
        assert np.array_equal(got, want), case
        if case == 'plain':                                          # and with the style as an image (stylize_batch)
            style = synthetic_image(31, 72, 64)
            assert np.array_equal(small.predict_frames(raw, style, resize=SIZE, **kw), small.predict_frames(resized, style, **kw))
            assert np.array_equal(small.predict_frames(raw, style, resize=SIZE, **kw), want)
    finally:
        small.wct_mode = keep


@pytest.mark.parametrize('colors', [False, True], ids=['plain', 'content-colors'])
def test_masked_chain_is_the_call_on_pillows_frames(small, colors):
    raw, resized = _frames()
    masks = np.zeros((3,) + SIZE, np.uint8)                           # the label maps: at the resized size
    masks[0, :, 32:] = 1
    masks[1, 24:] = 1
    masks[2, 10:30, 20:50] = 1
    styles = [synthetic_image(32, 64, 64), synthetic_image(33, 56, 72)]
    handles = [small.prepare_style(s) for s in styles]
    try:
        want = small.predict_frames_masked(resized, handles, masks, alpha=0.8, batch=2, content_colors=colors)
        got = small.predict_frames_masked(raw, handles, masks, alpha=0.8, batch=2, content_colors=colors, resize=SIZE)
    finally:
        for h in handles:
            h.close()
    assert got.shape == (3,) + SIZE + (3,)
    assert np.array_equal(got, want)


def test_chain_with_the_full_five_levels(full):
    raw, resized = _frames()
    with full.prepare_style(synthetic_image(34, 64, 72)) as handle:
        want = full.predict_frames(resized, handle, alpha=0.8, batch=3, content_colors=True)
        got = full.predict_frames(raw, handle, alpha=0.8, batch=3, content_colors=True, resize=SIZE)
    assert got.shape == (3,) + SIZE + (3,)
    assert np.array_equal(got, want)


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(small):
    ctx = small.sess
    lib, h = ctx.lib, ctx.h
    img, want = _case(37, 53, 24, 35)
    src = np.ascontiguousarray(img)
    out = np.empty((24, 35, 3), np.uint8)
    pi, po = src.ctypes.data_as(_lib._U8), out.ctypes.data_as(_lib._U8)
    din, dout = ctx.dev_alloc(2000 * 64 * 3), ctx.dev_alloc(1 << 16)

    def refused(rc, word=None):
        assert rc == ARG, (rc, lib.wct_last_error())
        if word:
            assert word in lib.wct_last_error(), lib.wct_last_error()
        ctx.sync()
        assert np.array_equal(ctx.resize(img, (24, 35)), want)      # a good call on the same ctx

    try:
        refused(lib.wct_resize(None, pi, 37, 53, 24, 35, po))
        refused(lib.wct_resize(h, None, 37, 53, 24, 35, po), b'null')
        refused(lib.wct_resize(h, pi, 37, 53, 24, 35, None), b'null')
        for sizes in ((0, 53, 24, 35), (37, 0, 24, 35), (37, 53, 0, 35), (37, 53, 24, 0), (37, -1, 24, 35)):
            refused(lib.wct_resize(h, pi, sizes[0], sizes[1], sizes[2], sizes[3], po), b'empty')
            refused(lib.wct_resize_batch_dev(h, din, sizes[0], sizes[1], 1, sizes[2], sizes[3], dout), b'empty')
        refused(lib.wct_resize_batch_dev(None, din, 37, 53, 1, 24, 35, dout))
        refused(lib.wct_resize_batch_dev(h, None, 37, 53, 1, 24, 35, dout), b'null')
        refused(lib.wct_resize_batch_dev(h, din, 37, 53, 1, 24, 35, None), b'null')
        for b in (0, -1, 33):
            refused(lib.wct_resize_batch_dev(h, din, 37, 53, b, 24, 35, dout), b'1 .. 32')
        # 2^31 bytes and more on either side: refused up front, nothing is launched (the buffers are small)
        refused(lib.wct_resize_batch_dev(h, din, 30000, 30000, 1, 24, 35, dout), b'2^31')
        refused(lib.wct_resize_batch_dev(h, din, 37, 53, 1, 30000, 30000, dout), b'2^31')
        refused(lib.wct_resize_batch_dev(h, din, 4736, 4736, 32, 24, 35, dout), b'2^31')       # 32 x 67.3 MB = 2^31 + 5.8 MB
        refused(lib.wct_resize_batch_dev(h, din, 1 << 30, 1 << 30, 1, 24, 35, dout), b'2^31')
        refused(lib.wct_resize(h, pi, 30000, 30000, 24, 35, po), b'2^31')
        # a vertical reduction past the LDS limit: 2000 rows to 4 at 64 columns, 1000 rows of 192 bytes under one output row
        refused(lib.wct_resize_batch_dev(h, din, 2000, 64, 1, 4, 64, dout), b'LDS')
        tall = np.zeros((2000, 64, 3), np.uint8)
        refused(lib.wct_resize(h, tall.ctypes.data_as(_lib._U8), 2000, 64, 4, 64, po), b'LDS')
        # the output inside the input
        refused(lib.wct_resize_batch_dev(h, din, 37, 53, 1, 24, 35, C.c_void_p(din.value + 16)), b'overlaps')
    finally:
        ctx.dev_free(din)
        ctx.dev_free(dout)
    with pytest.raises(_lib.WCTHipError, match='LDS'):
        ctx.resize(np.zeros((2000, 64, 3), np.uint8), (4, 64))
    with pytest.raises(_lib.WCTHipError, match='LDS'):
        ctx.resize_batch(np.zeros((2, 2000, 64, 3), np.uint8), (4, 64))
    assert np.array_equal(ctx.resize(img, (24, 35)), want)


# ---- the command line, end to end ---------------------------------------------------------------------------------------------
def test_video_cli_writes_the_same_frames_with_and_without_device_resize(tmp_path):
    import os
    from wct_tf_amd.stylize_video import main
    frames = tmp_path / 'clip'
    frames.mkdir()
    for f in range(3):
        utils.save_img(str(frames / ('frame_%d.png' % (f + 1))), synthetic_image(400 + f, *RAW))
    utils.save_img(str(tmp_path / 'style.png'), synthetic_image(35, 56, 48))
    base = ['--relu-targets', 'relu3_1', 'relu1_1', '--synthetic-weights', '42', '--in-path', str(frames), '--style-path',
            str(tmp_path / 'style.png'), '--content-size', '48', '--alpha', '0.8', '--batch', '2', '--content-colors']
    assert main(base + ['--out-path', str(tmp_path / 'host')]) == 3
    assert main(base + ['--out-path', str(tmp_path / 'dev'), '--device-resize']) == 3
    for f in range(3):
        name = os.path.join('clip_style', 'frame_%d.png' % (f + 1))
        a, b = utils.get_img(str(tmp_path / 'host' / name)), utils.get_img(str(tmp_path / 'dev' / name))
        assert a.shape == SIZE + (3,) and np.array_equal(a, b), f
