"""Temporal guided upsampling on the GPU (csrc/guided_up_time.hip): the op against the NumPy oracle (tests/guided_up_time_oracle.py)
across the tilings, under motion, at the parameter limits and on a chunked clip; its identities with guided upsampling;
WCT.predict_frames against the composition resize -> predict_frames -> oracle -> content_colors; the refusals of the C ABI; the
video command line.  Everything is np.array_equal: the rule is integers only."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle
import guided_motion_oracle as gm
import guided_up_time_oracle as oracle
from wct_tf_amd import _lib, ops, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
TWO = ['relu2_1', 'relu1_1']
ARG = -2


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def model():
    from wct_tf_amd.wct import WCT
    m = WCT(None, TWO, None, weights=synthetic_weights(5, relu_targets=TWO))
    yield m
    m.sess.close()


# the tiling case: a frame larger than its content, two strips of 256 - 8 columns and two segments of 64 rows at the small size
TILING = dict(F=5, h=70, w=270, hc=67, wc=268, r=4, t=2)


@pytest.fixture(scope='module')
def tiling_clip():
    """the small clip of the tiling case and its two full contents, W % 4 != 0 (three 256-column tiles, three 64-row block rows)
    and the whole-dword path"""
    k = TILING
    s, c, odd = oracle.noise_clip(1, k['F'], k['h'], k['w'], k['hc'], k['wc'], 150, 601)
    even = np.random.default_rng(2).integers(0, 256, (k['F'], 152, 604, 3)).astype(np.uint8)
    return s, c, {(150, 601): odd, (152, 604): even}


@pytest.fixture(scope='module')
def tiling_want(tiling_clip):
    """the oracle on the tiling case, computed once: {(full size, motion): frames}"""
    s, c, fulls = tiling_clip
    zig = oracle.zigzag(TILING['F'], (2, 6))
    want = {(size, False): oracle.guided_upsample_time(s, c, C_, TILING['r'], 650, TILING['t']) for size, C_ in fulls.items()}
    want[(150, 601), True] = oracle.guided_upsample_time(s, c, fulls[150, 601], TILING['r'], 650, TILING['t'], zig)
    return want, zig


@pytest.mark.parametrize('size', [(150, 601), (152, 604)], ids=str)
def test_op_across_the_tiles(ctx, tiling_clip, tiling_want, size):
    s, c, fulls = tiling_clip
    want, _ = tiling_want
    full = fulls[size]
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, TILING['r'], 650, TILING['t']), want[size, False])
    got = ctx.guided_upsample_time_range(s, c, full[1:4], TILING['r'], 650, TILING['t'], 1, 4)
    assert np.array_equal(got, want[size, False][1:4])


def test_op_across_the_tiles_under_small_zigzag_steps(ctx, tiling_clip, tiling_want):
    s, c, fulls = tiling_clip
    want, zig = tiling_want
    full = fulls[150, 601]
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, TILING['r'], 650, TILING['t'], positions=zig), want[(150, 601), True])
    got = ctx.guided_upsample_time_range(s, c, full[1:4], TILING['r'], 650, TILING['t'], 1, 4, positions=zig)
    assert np.array_equal(got, want[(150, 601), True][1:4])
    assert not np.array_equal(want[(150, 601), True], want[(150, 601), False])


def test_op_at_ratio_one(ctx):
    s, c, _ = oracle.noise_clip(3, 4, 40, 52, 37, 50, 37, 50)
    for pos in (None, oracle.zigzag(4, (1, 3))):
        assert np.array_equal(ctx.guided_upsample_time(s, c, c, 3, 650, 2, positions=pos), oracle.guided_upsample_time(s, c, c, 3, 650, 2, pos))


def test_op_under_steps_that_empty_the_neighbours_windows(ctx):
    """steps of (16, -16) per frame on 20 x 24 frames at r = 2: the windows of the neighbouring frames fall outside the frame over
    most of it"""
    s, c, full = oracle.noise_clip(4, 4, 20, 24, 20, 24, 40, 48)
    pos = gm.positions_of([(16, -16)] * 3)
    assert (gm.count3(4, 20, 24, 2, 3, pos) == gm.count3(4, 20, 24, 2, 0, pos)).any()
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, 2, 650, 3, positions=pos), oracle.guided_upsample_time(s, c, full, 2, 650, 3, pos))


def test_identities_with_guided_upsampling(ctx):
    s, c, full = oracle.clip_case(5, 3, 16, 20, 9, 13, 50, 70)
    plain = ctx.guided_upsample_batch(s, c, full, 3, 650)
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, 3, 650, 0), plain)
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, 3, 650, 0, positions=oracle.zigzag(3, (2, 6))), plain)
    assert np.array_equal(ctx.guided_upsample_time(s[1:2], c[1:2], full[1:2], 3, 650, 2), plain[1:2])
    timed = ctx.guided_upsample_time(s, c, full, 3, 650, 2)
    assert not np.array_equal(timed, plain)
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, 3, 650, 2, positions=np.zeros((3, 2), np.int32)), timed)
    assert np.array_equal(ctx.guided_upsample_time(s, c, full, 3, 650, 2, positions=np.tile(np.array([5, -9], np.int32), (3, 1))), timed)


def test_op_at_the_limits(ctx):
    """r = 33, T = 3, eps_q = 1 on 32 resident frames of 70 x 80 -> 140 x 160; frames 8 .. 15 are the extreme of the bounds (frames
    of 0 / 255 under a guide of two neighbouring greys, a full content that swings over 0 .. 255), frames 20 .. 25 a 0 / 255
    checkerboard guide under frames of 255"""
    s, c, full = oracle.noise_clip(6, 32, 70, 80, 70, 80, 140, 160)
    col = np.mgrid[:70, :80][1]
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    s[8:16], c[8:16], full[8:16] = rgb((col & 1) * 255), rgb(100 + (col & 1) * 2), rgb((np.mgrid[:140, :160][1] & 1) * 255)
    s[20:26], c[20:26] = 255, rgb(((col + np.mgrid[:70, :80][0]) & 1) * 255)
    pos = oracle.zigzag(32, (1, 2))
    for p in (None, pos):
        assert np.array_equal(ctx.guided_upsample_time(s, c, full, 33, 1, 3, positions=p), oracle.guided_upsample_time(s, c, full, 33, 1, 3, p))


def test_a_clip_of_forty_frames(ctx):
    s, c, full = oracle.noise_clip(7, 40, 24, 32, 24, 32, 48, 64)
    for pos in (None, oracle.zigzag(40, (2, 6))):
        assert np.array_equal(ctx.guided_upsample_time_clip(s, c, full, 2, 650, 2, positions=pos), oracle.guided_upsample_time(s, c, full, 2, 650, 2, pos))


# ---- the model -------------------------------------------------------------------------------------------------------------------
GU = (48, 3, 650)


@pytest.fixture(scope='module')
def model_clip(model):
    """7 frames of 96 x 128 that drift, their small contents, the plain small frames, and a style"""
    a, b = synthetic_image(80, 96, 128).astype(np.float32), synthetic_image(81, 96, 128).astype(np.float32)
    frames = np.stack([a * (1 - t) + b * t for t in np.linspace(0, 0.3, 7)]).astype(np.uint8)
    sty = synthetic_image(82, 64, 72)
    small = model.sess.resize_batch(frames, (48, 64))
    plain = model.predict_frames(small, sty, alpha=0.8)
    return frames, sty, small, plain


def test_predict_frames_is_the_composition(model, model_clip):
    frames, sty, small, plain = model_clip
    want = oracle.guided_upsample_time(plain, small, frames, 3, 650, 2)
    got = model.predict_frames(frames, sty, alpha=0.8, batch=2, guided_upsample=GU, guided_upsample_frames=2)
    assert got.shape == frames.shape and np.array_equal(got, want)
    assert np.array_equal(model.predict_frames(frames, sty, alpha=0.8, batch=5, guided_upsample=GU, guided_upsample_frames=2), want)
    colored = np.stack([colors_oracle.content_colors(w, f) for w, f in zip(want, frames)])
    with model.prepare_style(sty) as handle:
        got = model.predict_frames(frames, handle, alpha=0.8, batch=5, guided_upsample=GU, guided_upsample_frames=2, content_colors=True)
    assert np.array_equal(got, colored)
    # one frame at T >= 1, and T = 0, are today's call
    today = model.predict_frames(frames[:1], sty, alpha=0.8, guided_upsample=GU)
    assert np.array_equal(model.predict_frames(frames[:1], sty, alpha=0.8, guided_upsample=GU, guided_upsample_frames=2), today)
    assert np.array_equal(model.predict_frames(frames[:1], sty, alpha=0.8, guided_upsample=GU, guided_upsample_frames=0), today)


def test_predict_frames_along_global_motion(model, model_clip):
    frames, sty, small, plain = model_clip
    pos = ops.motion_global_np(small, 4, ctx=model.sess)
    assert np.array_equal(pos, gm.estimate_positions(small, 4))
    want = oracle.guided_upsample_time(plain, small, frames, 3, 650, 2, pos)
    got = model.predict_frames(frames, sty, alpha=0.8, batch=3, guided_upsample=GU, guided_upsample_frames=2, guided_upsample_motion=('global', 4))
    assert np.array_equal(got, want)
    given = oracle.zigzag(7, (1, 2))
    got = model.predict_frames(frames, sty, alpha=0.8, guided_upsample=GU, guided_upsample_frames=2, guided_upsample_motion=given)
    assert np.array_equal(got, oracle.guided_upsample_time(plain, small, frames, 3, 650, 2, given))


def test_video_cli(tmp_path, model, model_clip):
    """the video tool's sliding buffer end to end: frames do not depend on --batch"""
    from wct_tf_amd.stylize_video import main
    frames, sty, small, plain = model_clip
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    for i in range(7):
        utils.save_img(str(in_dir / ('frame_%d.png' % (i + 1))), frames[i])
    utils.save_img(str(tmp_path / 's0.png'), sty)
    assert main(['--relu-targets'] + TWO + ['--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '5', '--batch', '3',
                                            '--style-path', str(tmp_path / 's0.png'), '--guided-radius', '3', '--guided-eps', '0.01',
                                            '--content-size', '48', '--guided-upsample', '--guided-upsample-frames', '2',
                                            '--guided-upsample-motion', 'global', '--guided-upsample-motion-range', '4', '--content-colors',
                                            '--out-path', str(tmp_path / 'out')]) == 7
    want = oracle.guided_upsample_time(plain, small, frames, 3, 650, 2, gm.estimate_positions(small, 4))
    for i in range(7):
        got = utils.get_img(str(tmp_path / 'out' / 'clip_s0' / ('frame_%d.png' % (i + 1))))
        assert np.array_equal(got, colors_oracle.content_colors(want[i], frames[i])), i


# ---- the refusals of the C ABI ---------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    s, c, f = oracle.noise_clip(8, 4, 16, 20, 9, 13, 40, 61)
    out = np.empty_like(f)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    pos = gm.positions_of([(1, 2), (3, -4), (0, 0)])
    ip = lambda a: a.ctypes.data_as(_lib._I)
    want = oracle.guided_upsample_time(s, c, f, 4, 650, 1, pos)

    def good():
        ctx.sync()
        assert np.array_equal(ctx.guided_upsample_time(s, c, f, 4, 650, 1, positions=pos), want)

    def refused(rc, word):
        assert rc == ARG and word in lib.wct_last_error(), lib.wct_last_error()

    def up(s_=p(s), h_=16, w_=20, c_=p(c), hc_=9, wc_=13, f_=p(f), H_=40, W_=61, F_=4, r_=4, e_=650, t_=1, pos_=ip(pos), o_=p(out)):
        return lib.wct_guided_upsample_time(h, s_, h_, w_, c_, hc_, wc_, f_, H_, W_, F_, r_, e_, t_, pos_, o_)

    good()
    for r in (0, 65, -1, 52):
        refused(up(r_=r), b'radius')
    refused(up(r_=34, t_=3), b'radius')
    for e in (0, 65026):
        refused(up(e_=e), b'eps_q')
    for t in (-1, 4):
        refused(up(t_=t), b'frames on each side')
    for F in (0, 33):
        refused(up(F_=F), b'F =')
    refused(up(H_=8), b'H x W')
    refused(up(W_=12), b'H x W')
    refused(up(h_=8), b'stylized frame')
    refused(up(w_=12), b'stylized frame')
    refused(up(s_=None), b'stylized')
    refused(up(c_=None), b'content_small')
    refused(up(f_=None), b'content_full')
    refused(up(o_=None), b'out')
    far = gm.positions_of([(1, 2), (17, 0), (0, 0)])
    refused(up(pos_=ip(far)), b'the step from frame 1 to 2 is (17, 0)')
    assert up(pos_=None) == 0 and np.array_equal(out, oracle.guided_upsample_time(s, c, f, 4, 650, 1))
    assert lib.wct_guided_upsample_time(None, p(s), 16, 20, p(c), 9, 13, p(f), 40, 61, 4, 4, 650, 1, None, p(out)) == ARG
    good()
    buf = ctx.dev_alloc(f.nbytes * 2)
    other = C.c_void_p(buf.value + f.nbytes)
    try:
        dev = lambda *a: lib.wct_guided_upsample_time_batch_dev(h, *a)
        for f0, f1 in ((-1, 2), (2, 2), (3, 5)):
            refused(dev(buf, 16, 20, buf, 9, 13, buf, 40, 61, 4, 4, 650, 1, None, f0, f1, other), b'frames [')
        refused(dev(None, 16, 20, buf, 9, 13, buf, 40, 61, 4, 4, 650, 1, None, 0, 4, other), b'stylized')
        refused(dev(buf, 16, 20, buf, 9, 13, buf, 1 << 15, 1 << 15, 4, 4, 650, 1, None, 0, 1, other), b'2^31')
        for k in (0, 1, 2):                                                         # out over each input in turn
            ins = [other, other, other]
            ins[k] = buf
            refused(dev(ins[0], 16, 20, ins[1], 9, 13, ins[2], 40, 61, 4, 4, 650, 1, None, 0, 4, buf), b'overlaps')
    finally:
        ctx.dev_free(buf)
    good()
