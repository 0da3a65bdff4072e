"""Temporal guided smoothing with the colour guide on the GPU (csrc/guided_color_time.hip): the op against the NumPy oracle
(tests/guided_color_time_oracle.py) on whole clips and sub-ranges, out of place and in place, with and without positions; the grey
guide through the new entry points against the existing ops; equal positions against null positions; both ends of eps_q; full
windows at the sum limit; the chunked op on a clip longer than one call takes; the refusals of the C ABI;
predict_frames(guided_frames_guide=) against the op on the plain frames; and the video tool at two batch sizes.  Everything is
np.array_equal: the rules are integers only."""
import ctypes as C

import numpy as np
import pytest

import guided_color_oracle as gc
import guided_motion_oracle as gm
import guided_color_time_oracle as oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
G, T = (3, 650), 2                 # the predict_frames and tool cases
GREY, COLOR = _lib.GUIDE_GREY, _lib.GUIDE_COLOR


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
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


def _zigzag(frames, step):
    return gm.positions_of([step if f % 2 == 0 else (-step[0], -step[1]) for f in range(frames - 1)])


def _steady(frames, step):
    return gm.positions_of([step] * (frames - 1))


def _op_dev(ctx, s, c, r, eps_q, t, pos, in_place, f0=0, f1=None, offset=0, guide=COLOR):
    """wct_guided_filter_time_guide_batch_dev on device buffers of its own -> frames f0 .. f1 - 1: out a second buffer, or frame f0
    of the stylized one; offset: the image bases moved by that many bytes; pos None: null positions"""
    s, c = np.ascontiguousarray(s), np.ascontiguousarray(c)
    f1 = len(s) if f1 is None else f1
    frame = s[0].nbytes
    bufs = [ctx.dev_alloc(s.nbytes + 16), ctx.dev_alloc(c.nbytes + 16), ctx.dev_alloc(s.nbytes + 16)]
    ds, dc, do = [C.c_void_p(b.value + offset) for b in bufs]
    dout = C.c_void_p(ds.value + f0 * frame) if in_place else do
    pos = None if pos is None else np.ascontiguousarray(pos, np.int32)
    try:
        ctx.h2d(ds, s)
        ctx.h2d(dc, c)
        rc = ctx.lib.wct_guided_filter_time_guide_batch_dev(ctx.h, ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r,
                                                            eps_q, t, guide, None if pos is None else pos.ctypes.data_as(_lib._I), f0, f1,
                                                            dout)
        assert rc == 0, ctx.lib.wct_last_error()
        ctx.sync()
        out, kept = np.empty_like(s[f0:f1]), np.empty_like(s)
        ctx.d2h(out, dout)
        ctx.d2h(kept, ds)
        if in_place:
            assert np.array_equal(kept[:f0], s[:f0]) and np.array_equal(kept[f1:], s[f1:])      # only the range was written
        else:
            assert np.array_equal(kept, s)                                                      # the input is left alone
    finally:
        for b in bufs:
            ctx.dev_free(b)
    return out


# (F, Ho, Wo, Hc, Wc, r, T, positions): two strips and two segments under a zig-zag; windows wholly outside the frame, the frame
# larger than its content; the largest radius of T = 3 across a strip joint; a one-frame clip; null positions
OP_CASES = [(5, 70, 270, 70, 270, 4, 2, _zigzag(5, (3, -5))), (4, 33, 40, 31, 37, 2, 1, _steady(4, (16, -16))),
            (7, 20, 300, 20, 300, 33, 3, _steady(7, (-7, 11))), (1, 33, 35, 33, 35, 4, 2, np.array([[5, -9]], np.int32)),
            (5, 70, 270, 66, 260, 4, 2, None)]


@pytest.fixture(scope='module')
def op_cases():
    """the inputs and the oracle's bytes of OP_CASES, computed once"""
    out = []
    for i, (f, ho, wo, hc, wc, r, t, pos) in enumerate(OP_CASES):
        s, c = _noise(2 * i + 1, f, ho, wo, 3), _noise(2 * i + 2, f, hc, wc, 3)
        out.append((s, c, r, t, pos, oracle.guided_filter(s, c, r, 650, t, pos)))
    return out


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('case', range(len(OP_CASES)), ids=['zigzag', 'outside', 'r33', 'one-frame', 'no-positions'])
def test_op_is_the_oracle(ctx, op_cases, case, in_place):
    s, c, r, t, pos, want = op_cases[case]
    assert np.array_equal(_op_dev(ctx, s, c, r, 650, t, pos, in_place), want)
    if len(s) == 1:
        assert np.array_equal(want, gc.guided_filter(s, c, r, 650))                    # no neighbours: the 2-D colour rule
        assert np.array_equal(ctx.guided_filter_batch(s, c, r, 650, guide='color'), want)
    if not in_place:
        assert np.array_equal(ctx.guided_filter_time(s, c, r, 650, t, positions=pos, guide='color'), want)       # the host call
        from wct_tf_amd import guided_filter_time_np
        assert np.array_equal(guided_filter_time_np(s, c, r, 650, t, ctx=ctx, positions=pos, guide='color'), want)


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_grey_guide_through_the_new_entry_points_is_the_existing_ops(ctx, in_place):
    s, c, pos = _noise(20, 5, 70, 270, 3), _noise(21, 5, 66, 260, 3), _zigzag(5, (3, -5))
    for p in (None, pos):
        bufs = [ctx.dev_alloc(s.nbytes), ctx.dev_alloc(c.nbytes), ctx.dev_alloc(s[1:4].nbytes)]
        try:
            ctx.h2d(bufs[0], s)
            ctx.h2d(bufs[1], c)
            dout = C.c_void_p(bufs[0].value + s[0].nbytes) if in_place else bufs[2]
            if p is None:
                ctx.guided_filter_time_batch_dev(bufs[0], 70, 270, bufs[1], 66, 260, 5, 4, 650, 2, 1, 4, dout)
            else:
                ctx.guided_filter_motion_batch_dev(bufs[0], 70, 270, bufs[1], 66, 260, 5, 4, 650, 2, p, 1, 4, dout)
            ctx.sync()
            want = np.empty_like(s[1:4])
            ctx.d2h(want, dout)
        finally:
            for b in bufs:
                ctx.dev_free(b)
        assert np.array_equal(_op_dev(ctx, s, c, 4, 650, 2, p, in_place, 1, 4, guide=GREY), want)
        assert not np.array_equal(_op_dev(ctx, s, c, 4, 650, 2, p, in_place, 1, 4, guide=COLOR), want)


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_equal_positions_are_null_positions(ctx, in_place):
    s, c = _noise(22, 5, 70, 270, 3), _noise(23, 5, 66, 260, 3)
    for t, r in ((2, 4), (0, 64), (3, 33)):
        want = _op_dev(ctx, s, c, r, 650, t, None, in_place)
        assert np.array_equal(_op_dev(ctx, s, c, r, 650, t, np.zeros((5, 2), np.int32), in_place), want), (t, r)
        assert np.array_equal(_op_dev(ctx, s, c, r, 650, t, np.tile(np.int32([-4000, 123456]), (5, 1)), in_place), want), (t, r)
        if t == 0:
            assert np.array_equal(want, ctx.guided_filter_batch(s, c, r, 650, guide='color'))    # the 2-D colour op, bit for bit


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('f0,f1', [(0, 9), (4, 5), (2, 7), (8, 9)])
def test_sub_ranges_are_slices_of_the_whole_clip(ctx, f0, f1, in_place):
    s, c, pos = _noise(5, 9, 33, 35, 3), _noise(6, 9, 33, 35, 3), _zigzag(9, (4, 7))
    want = oracle.guided_filter(s, c, 4, 650, 2, pos)
    assert np.array_equal(_op_dev(ctx, s, c, 4, 650, 2, pos, in_place, f0, f1), want[f0:f1])
    if not in_place:
        assert np.array_equal(ctx.guided_filter_time_range(s, c, 4, 650, 2, f0, f1, positions=pos, guide='color'), want[f0:f1])


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_op_on_bases_one_byte_off_alignment(ctx, in_place):
    s, c, pos = _noise(8, 4, 48, 48, 3), _noise(9, 4, 37, 44, 3), _steady(4, (-2, 9))
    assert np.array_equal(_op_dev(ctx, s, c, 4, 650, 1, pos, in_place, 1, 3, offset=1), oracle.guided_filter(s, c, 4, 650, 1, pos)[1:3])


@pytest.mark.parametrize('eps_q', [1, 65025])
def test_op_at_both_ends_of_eps(ctx, eps_q):
    s, c = _noise(10, 4, 48, 48, 3), _noise(11, 4, 37, 41, 3)
    for r, t, step in ((1, 3, (1, 1)), (4, 2, (-5, 3)), (51, 1, (16, 16))):
        pos = _steady(4, step)
        assert np.array_equal(ctx.guided_filter_time(s, c, r, eps_q, t, positions=pos, guide='color'), oracle.guided_filter(s, c, r, eps_q, t, pos)), (r, t)
    flat = np.full((4, 40, 44, 3), 200, np.uint8)
    assert np.array_equal(ctx.guided_filter_time(flat, _noise(12, 4, 40, 44, 3), 33, eps_q, 3, positions=_zigzag(4, (6, -6)), guide='color'), flat)


def test_op_with_full_windows_at_the_sum_limit(ctx):
    """an all-255 clip and a checkerboard that alternates in time, drifting by (1, -1) per frame, on a clip whose central pixels
    have full windows of (2r + 1)^2 (2T + 1) = 32805 pixels: window sums of n * 65025, the largest the mod-2^32 prefixes carry"""
    f, r, t = 5, 40, 2
    side, pos = 2 * r + 2 * t + 2, _steady(5, (1, -1))
    ff, yy, xx = np.mgrid[:f, :side, :side]
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    assert gm.count3(f, side, side, r, t, pos).max() == (2 * r + 1) ** 2 * (2 * t + 1)
    white = rgb(np.full((f, side, side), 255))
    assert np.array_equal(ctx.guided_filter_time(white, white, r, 1, t, positions=pos, guide='color'), white)
    board = rgb(((ff + yy + xx) & 1) * 255)
    assert np.array_equal(ctx.guided_filter_time(board, board, r, 1, t, positions=pos, guide='color'), oracle.guided_filter(board, board, r, 1, t, pos))


def test_a_clip_longer_than_one_call_goes_in_chunks_with_sliced_positions(ctx):
    """70 frames at T = 2: chunks of 24 output frames, halos of 4"""
    from wct_tf_amd import guided_filter_time_np
    s, c = _noise(15, 70, 18, 22, 3), _noise(16, 70, 18, 22, 3)
    rng = np.random.default_rng(17)
    pos = (gm.positions_of(rng.integers(-6, 7, (69, 2))) + np.int32(500)).astype(np.int32)
    want = oracle.guided_filter(s, c, 2, 650, 2, pos)
    assert np.array_equal(ctx.guided_filter_time_clip(s, c, 2, 650, 2, positions=pos, guide='color'), want)
    assert np.array_equal(guided_filter_time_np(s, c, 2, 650, 2, ctx=ctx, positions=pos, guide='color'), want)
    assert np.array_equal(guided_filter_time_np(s, c, 2, 650, 2, ctx=ctx, guide='color'), oracle.guided_filter(s, c, 2, 650, 2))


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    s, c = _noise(80, 3, 16, 20, 3), _noise(81, 3, 9, 20, 3)
    pos = _steady(3, (2, -3))
    out = np.empty_like(s)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    pi = lambda a: a.ctypes.data_as(_lib._I)
    ARG = -2
    want = oracle.guided_filter(s, c, 4, 650, 1, pos)

    def good():
        ctx.sync()
        assert np.array_equal(ctx.guided_filter_time(s, c, 4, 650, 1, positions=pos, guide='color'), want)

    host = lambda r=4, e=650, t=1, f=3, g=COLOR, S=s, Cc=c, O=out, P=pos, ho=16, wo=20, hc=9, wc=20, hh=h: lib.wct_guided_filter_time_guide(
        hh, None if S is None else p(S), ho, wo, None if Cc is None else p(Cc), hc, wc, f, r, e, t, g, None if P is None else pi(P),
        None if O is None else p(O))
    far = np.ascontiguousarray([[0, 0], [0, 17], [0, 17]], np.int32)
    for kw, word in ((dict(g=2), b'guide 2'), (dict(g=-1), b'guide -1'), (dict(g=2, P=None), b'guide 2'), (dict(r=0), b'radius'),
                     (dict(r=52), b'1 .. 51'), (dict(r=52, P=None), b'1 .. 51'), (dict(r=52, g=GREY), b'1 .. 51'),
                     (dict(r=41, t=2), b'1 .. 40'), (dict(e=0), b'eps_q'), (dict(t=4), b'frames on each side'), (dict(f=0), b'1 .. 32'),
                     (dict(f=33), b'1 .. 32'), (dict(ho=8), b'never the smaller'), (dict(S=None), b'null'), (dict(Cc=None), b'null'),
                     (dict(O=None), b'null'), (dict(O=None, P=None), b'null'), (dict(S=None, g=GREY), b'null'),
                     (dict(P=far), b'step from frame 0 to 1 is (0, 17)'), (dict(P=far, g=GREY), b'step from frame 0 to 1 is (0, 17)'),
                     (dict(P=np.ascontiguousarray([[0, 0], [0, 0], [-17, 0]], np.int32)), b'step from frame 1 to 2 is (-17, 0)')):
        assert host(**kw) == ARG, kw
        assert word in lib.wct_last_error(), (kw, lib.wct_last_error())
        good()
    assert host(hh=None) == ARG
    buf = ctx.dev_alloc(s.nbytes)
    try:
        dev = lambda f=3, f0=0, f1=3, ho=16, wo=20, g=COLOR, S=buf, O=buf, P=pos: lib.wct_guided_filter_time_guide_batch_dev(
            h, S, ho, wo, buf, 16, 20, f, 4, 650, 1, g, None if P is None else pi(P), f0, f1, O)
        for kw in (dict(f=0), dict(f=33), dict(f0=-1), dict(f0=2, f1=2), dict(f1=4), dict(S=None), dict(O=None), dict(ho=15), dict(P=far),
                   dict(g=7), dict(f0=2, f1=2, P=None), dict(S=None, P=None)):
            assert dev(**kw) == ARG, kw
            assert lib.wct_last_error(), kw
        assert dev(ho=1 << 14, wo=1 << 14) == ARG and b'2^31' in lib.wct_last_error()
    finally:
        ctx.dev_free(buf)
    good()
    assert np.array_equal(ctx.guided_filter_time(s, c, 4, 650, 1, guide='color'), oracle.guided_filter(s, c, 4, 650, 1))


# ---- predict_frames -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip(model):
    """7 frames of 40 x 48 cut from one image by a camera that pans, one prepared style and the plain frames: computed once"""
    base = synthetic_image(30, 64, 90)
    frames = np.stack([base[4 + f:44 + f, 3 + 3 * f:51 + 3 * f] for f in range(7)])
    handle = model.prepare_style(synthetic_image(29, 80, 64))
    plain = model.predict_frames(frames, handle, alpha=0.8, batch=7)
    pos = gm.estimate_positions(frames, 8)
    assert np.array_equal(np.diff(pos, axis=0), np.tile([-1, -3], (6, 1)))
    yield frames, handle, plain, pos
    handle.close()


@pytest.mark.parametrize('batch', [1, 2, 5])
def test_predict_frames_is_the_op_on_the_plain_frames_whatever_the_batch(model, clip, batch):
    frames, handle, plain, pos = clip
    want, want_motion = oracle.guided_filter(plain, frames, G[0], G[1], T), oracle.guided_filter(plain, frames, G[0], G[1], T, pos)
    assert not np.array_equal(want, want_motion)
    kw = dict(alpha=0.8, batch=batch, guided=G, guided_frames=T)
    assert np.array_equal(model.predict_frames(frames, handle, guided_frames_guide='color', **kw), want)
    assert np.array_equal(model.predict_frames(frames, handle, guided_frames_guide='color', guided_motion='global', **kw), want_motion)
    if batch == 2:
        assert np.array_equal(model.sess.guided_filter_time_clip(plain, frames, G[0], G[1], T, guide='color'), want)
        # without the keyword, or with 'grey', the call is today's
        grey = gm.guided_filter_motion(plain, frames, G[0], G[1], T, np.zeros((7, 2), np.int32))
        assert not np.array_equal(grey, want)
        assert np.array_equal(model.predict_frames(frames, handle, **kw), grey)
        assert np.array_equal(model.predict_frames(frames, handle, guided_frames_guide='grey', **kw), grey)


def test_predict_frames_runs_the_colour_op_after_the_filter(model, clip):
    import colors_oracle
    frames, handle, plain, _ = clip
    got = model.predict_frames(frames, handle, alpha=0.8, batch=3, guided=G, guided_frames=T, guided_frames_guide='color', content_colors=True)
    assert np.array_equal(got, colors_oracle.content_colors(oracle.guided_filter(plain, frames, G[0], G[1], T), frames))


# ---- the video tool, end to end ---------------------------------------------------------------------------------------------
def test_stylize_video_cli_on_a_panning_directory_at_two_batch_sizes(tmp_path):
    """12 frames of 40 x 48 cut from one image by a panning camera: the files do not depend on --batch and equal the oracle's chain
    (estimate on the input frames' grey guide, filter the plain run's files along the motion under the colour guide)"""
    from wct_tf_amd.stylize_video import main
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    base = synthetic_image(90, 70, 110)
    frames = np.stack([base[2 + f:42 + f, 3 + 4 * f:51 + 4 * f] for f in range(12)])
    names = ['frame_%d.png' % (i + 1) for i in range(12)]
    for name, img in zip(names, frames):
        utils.save_img(str(in_dir / name), img)
    utils.save_img(str(tmp_path / 's0.png'), synthetic_image(95, 56, 48))
    base_args = ['--relu-targets', 'relu3_1', 'relu1_1', '--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '42',
                 '--style-path', str(tmp_path / 's0.png')]
    smooth = ['--guided-radius', '3', '--guided-frames', '2', '--guided-motion', 'global', '--guided-frames-guide', 'color']
    read = lambda d: [utils.get_img(str(tmp_path / d / 'clip_s0' / n)) for n in names]
    assert main(base_args + ['--batch', '5', '--out-path', str(tmp_path / 'plain')]) == 12
    assert main(base_args + smooth + ['--batch', '2', '--out-path', str(tmp_path / 'b2')]) == 12
    assert main(base_args + smooth + ['--batch', '5', '--out-path', str(tmp_path / 'b5')]) == 12
    plain, b2, b5 = read('plain'), read('b2'), read('b5')
    pos = gm.estimate_positions(frames, 8)
    want = oracle.guided_filter(np.stack(plain), frames, 3, 650, 2, pos)
    assert not np.array_equal(want, gm.guided_filter_motion(np.stack(plain), frames, 3, 650, 2, pos))
    for i in range(12):
        assert np.array_equal(b2[i], b5[i]) and np.array_equal(b5[i], want[i]), i
