"""Temporal guided smoothing on the GPU (csrc/guided_time.hip): the op against the NumPy oracle (tests/guided_time_oracle.py) on
whole clips and on sub-ranges, out of place and in place, the chunked op on a clip longer than one call takes, the refusals of the
C ABI, predict_frames(guided_frames=T) against the oracle applied to the plain frames, and the video tool on two clips at two
batch sizes.  Everything is np.array_equal: the rule is integers only.  Synthetic weights as in tests/test_gpu_guided.py."""
import ctypes as C

import numpy as np
import pytest

import colors_oracle
import guided_oracle as g2
import guided_time_oracle as oracle
from wct_tf_amd import _lib, utils
from wct_tf_amd.weights import synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
G, T = (3, 650), 1                 # the predict_frames and tool cases: a 7 x 7 x 3 box, eps 0.01
# the kernels' tiling: a block owns SEG rows of a strip of 256 - 2r columns of one frame
SEG = 64
strip = lambda r: 256 - 2 * r


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


def _op_dev(ctx, s, c, r, eps_q, t, in_place, f0=0, f1=None, offset=0):
    """wct_guided_filter_time_batch_dev on device buffers of its own -> frames f0 .. f1 - 1: out a second buffer, or frame f0 of
    the stylized one; offset: every base moved by that many bytes"""
    s, c = np.ascontiguousarray(s), np.ascontiguousarray(c)
    f1 = len(s) if f1 is None else f1
    frame = s[0].nbytes
    bufs = [ctx.dev_alloc(s.nbytes + 16), ctx.dev_alloc(c.nbytes + 16), ctx.dev_alloc(s.nbytes + 16)]
    ds, dc, do = [C.c_void_p(b.value + offset) for b in bufs]
    dout = C.c_void_p(ds.value + f0 * frame) if in_place else do
    try:
        ctx.h2d(ds, s)
        ctx.h2d(dc, c)
        ctx.guided_filter_time_batch_dev(ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r, eps_q, t, f0, f1, dout)
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


# (F, Ho, Wo, Hc, Wc, r, T): a one-frame clip; a clip shorter than its window; odd sizes at a small and a middle radius under every
# T; a window that covers the whole clip on all three axes; a frame larger than its content; one column past a strip and one row
# past a segment at a small radius and at the largest radius of T = 3
OP_CASES = [(1, 33, 35, 33, 35, 4, 1), (2, 33, 35, 33, 35, 4, 3)] + [(5, 33, 35, 33, 35, r, t) for r in (1, 4) for t in (1, 2, 3)] + \
    [(3, 9, 13, 9, 13, 16, 3), (4, 16, 20, 9, 13, 4, 1), (4, SEG + 1, strip(4) + 1, SEG + 1, strip(4) + 1, 4, 1),
     (3, SEG + 1, strip(33) + 1, SEG - 3, strip(33) - 2, 33, 3)]


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('f,ho,wo,hc,wc,r,t', OP_CASES)
def test_op_is_the_oracle(ctx, f, ho, wo, hc, wc, r, t, in_place):
    s, c = _noise(1, f, ho, wo, 3), _noise(2, f, hc, wc, 3)
    want = oracle.guided_filter_time(s, c, r, 650, t)
    assert np.array_equal(_op_dev(ctx, s, c, r, 650, t, in_place), want)
    if f == 1:
        assert np.array_equal(want[0], g2.guided_filter(s[0], c[0], r, 650))         # a one-frame clip is the 2-D op's bytes
    if not in_place:
        assert np.array_equal(ctx.guided_filter_time(s, c, r, 650, t), want)         # the host call
        from wct_tf_amd import guided_filter_time_np
        assert np.array_equal(guided_filter_time_np(s, c, r, 650, t, ctx=ctx), want)


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('f,side,r,t', [(3, 104, 51, 1), (5, 82, 40, 2)])
def test_op_with_full_windows_at_the_sum_limit(ctx, f, side, r, t, in_place):
    """an all-255 clip (window sums of n * 65025, the largest the mod-2^32 prefixes carry) and a checkerboard in space that
    alternates in time, on clips whose central pixels have full windows of (2r + 1)^2 (2T + 1) pixels"""
    ff, yy, xx = np.mgrid[:f, :side, :side]
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    assert oracle.count3(f, side, side, r, t).max() == (2 * r + 1) ** 2 * (2 * t + 1)
    for img in (rgb(np.full((f, side, side), 255)), rgb(((ff + yy + xx) & 1) * 255)):
        for eps_q in (1, 650):
            assert np.array_equal(_op_dev(ctx, img, img, r, eps_q, t, in_place), oracle.guided_filter_time(img, img, r, eps_q, t))


def test_no_frames_on_either_side_is_the_batched_2d_op(ctx):
    s, c = _noise(3, 3, 40, 52, 3), _noise(4, 3, 40, 52, 3)
    want = ctx.guided_filter_batch(s, c, 5, 100)
    assert np.array_equal(want, g2.guided_filter(s, c, 5, 100))
    assert np.array_equal(ctx.guided_filter_time(s, c, 5, 100, 0), want)
    assert np.array_equal(_op_dev(ctx, s, c, 5, 100, 0, True), want)
    assert np.array_equal(_op_dev(ctx, s, c, 64, 100, 0, False), g2.guided_filter(s, c, 64, 100))      # T = 0 keeps radius 64


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
@pytest.mark.parametrize('f0,f1', [(0, 9), (4, 5), (2, 7), (8, 9)])
def test_sub_ranges_are_slices_of_the_whole_clip(ctx, f0, f1, in_place):
    s, c = _noise(5, 9, 33, 35, 3), _noise(6, 9, 33, 35, 3)
    want = oracle.guided_filter_time(s, c, 4, 650, 2)
    assert np.array_equal(_op_dev(ctx, s, c, 4, 650, 2, in_place, f0, f1), want[f0:f1])
    if not in_place:
        assert np.array_equal(ctx.guided_filter_time_range(s, c, 4, 650, 2, f0, f1), want[f0:f1])


@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_op_on_bases_one_byte_off_alignment(ctx, in_place):
    s, c = _noise(8, 4, 48, 48, 3), _noise(9, 4, 37, 44, 3)
    assert np.array_equal(_op_dev(ctx, s, c, 4, 650, 1, in_place, 1, 3, offset=1), oracle.guided_filter_time(s, c, 4, 650, 1)[1:3])


@pytest.mark.parametrize('eps_q', [1, 65025])
def test_op_at_both_ends_of_eps(ctx, eps_q):
    s, c = _noise(10, 4, 48, 48, 3), _noise(11, 4, 37, 41, 3)
    for r, t in ((1, 3), (4, 2), (51, 1)):
        assert np.array_equal(ctx.guided_filter_time(s, c, r, eps_q, t), oracle.guided_filter_time(s, c, r, eps_q, t)), (r, t)
    flat = np.full((4, 40, 44, 3), 200, np.uint8)
    assert np.array_equal(ctx.guided_filter_time(flat, _noise(12, 4, 40, 44, 3), 33, eps_q, 3), flat)           # a constant clip


def test_op_clamps(ctx):
    s1, c1 = g2.clamp_case()
    s, c = np.repeat(s1[None], 3, 0), np.repeat(c1[None], 3, 0)
    raw = oracle.guided_filter_time_unclamped(s, c, 1, 1, 1)
    assert ((raw < 0) | (raw > 255)).any()
    assert np.array_equal(ctx.guided_filter_time(s, c, 1, 1, 1), np.clip(raw, 0, 255).astype(np.uint8))


def test_op_on_a_full_clip(ctx):
    s, c = _noise(13, 32, 64, 64, 3), _noise(14, 32, 64, 64, 3)
    assert np.array_equal(ctx.guided_filter_time(s, c, 8, 650, 1), oracle.guided_filter_time(s, c, 8, 650, 1))


def test_a_clip_longer_than_one_call_goes_in_chunks_with_halos(ctx):
    """40 frames at T = 3: chunks of 20 output frames, halos of 6"""
    from wct_tf_amd import guided_filter_time_np
    s, c = _noise(15, 40, 24, 28, 3), _noise(16, 40, 24, 28, 3)
    assert np.array_equal(guided_filter_time_np(s, c, 2, 650, 3, ctx=ctx), oracle.guided_filter_time(s, c, 2, 650, 3))


def test_max_radius_is_the_table(ctx):
    assert [ctx.guided_time_max_radius(t) for t in range(4)] == list(_lib.GUIDED_TIME_MAX_RADIUS) == [64, 51, 40, 33]
    assert [ctx.guided_time_max_radius(t) for t in (-1, 4, 100)] == [0, 0, 0]


# ---- the refusals of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(ctx):
    lib, h = ctx.lib, ctx.h
    s, c = _noise(80, 3, 16, 20, 3), _noise(81, 3, 9, 20, 3)
    out = np.empty_like(s)
    p = lambda a: a.ctypes.data_as(_lib._U8)
    ARG = -2
    want = oracle.guided_filter_time(s, c, 4, 650, 1)

    def good():
        ctx.sync()
        assert np.array_equal(ctx.guided_filter_time(s, c, 4, 650, 1), want)

    host = lambda r=4, e=650, t=1, f=3, S=s, Cc=c, O=out, ho=16, wo=20, hc=9, wc=20, hh=h: lib.wct_guided_filter_time(
        hh, None if S is None else p(S), ho, wo, None if Cc is None else p(Cc), hc, wc, f, r, e, t, None if O is None else p(O))
    for kw, word in ((dict(r=0), b'radius'), (dict(r=52), b'1 .. 51'), (dict(r=41, t=2), b'1 .. 40'), (dict(r=34, t=3), b'1 .. 33'),
                     (dict(r=65, t=0), b'1 .. 64'), (dict(e=0), b'eps_q'), (dict(e=65026), b'eps_q'), (dict(t=4), b'frames on each side'),
                     (dict(t=-1), b'frames on each side'), (dict(f=0), b'1 .. 32'), (dict(f=33), b'1 .. 32'),
                     (dict(ho=8), b'never the smaller'), (dict(wo=12), b'never the smaller'), (dict(S=None), b'null'),
                     (dict(Cc=None), b'null'), (dict(O=None), b'null')):
        assert host(**kw) == ARG, kw
        assert word in lib.wct_last_error(), (kw, lib.wct_last_error())
        good()
    assert host(r=52) == ARG
    msg = lib.wct_last_error()
    assert b'radius 52' in msg and b'1 frames' in msg and b'1 .. 51' in msg and b'33025' in msg      # both numbers and the limit
    assert host(hh=None) == ARG
    buf = ctx.dev_alloc(s.nbytes)
    try:
        dev = lambda f=3, f0=0, f1=3, ho=16, wo=20, S=buf, O=buf: lib.wct_guided_filter_time_batch_dev(h, S, ho, wo, buf, 16, 20, f, 4, 650, 1,
                                                                                                      f0, f1, O)
        for kw in (dict(f=0), dict(f=33), dict(f0=-1), dict(f0=2, f1=2), dict(f0=2, f1=1), dict(f1=4), dict(S=None), dict(O=None),
                   dict(ho=15)):
            assert dev(**kw) == ARG, kw
        assert dev(f0=3, f1=4) == ARG and b'0 <= f0 < f1 <= F' in lib.wct_last_error()
        assert dev(ho=1 << 14, wo=1 << 14) == ARG and b'2^31' in lib.wct_last_error()         # 3 frames of 2^28 x 3 bytes
    finally:
        ctx.dev_free(buf)
    good()


# ---- predict_frames -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip(model):
    """7 frames of 40 x 48 that drift, one prepared style, the plain frames and the oracle of the whole call: computed once"""
    a, b = synthetic_image(30, 40, 48).astype(np.float32), synthetic_image(31, 40, 48).astype(np.float32)
    frames = np.stack([a * (1 - u) + b * u for u in np.linspace(0, 0.4, 7)]).astype(np.uint8)
    handle = model.prepare_style(synthetic_image(29, 80, 64))
    plain = model.predict_frames(frames, handle, alpha=0.8, batch=7)
    want = oracle.guided_filter_time(plain, frames, G[0], G[1], T)
    assert not np.array_equal(want, g2.guided_filter(plain, frames, *G))       # (time does something on these frames)
    yield frames, handle, plain, want
    handle.close()


@pytest.mark.parametrize('batch', [1, 3, 7])
def test_predict_frames_is_the_oracle_on_the_plain_frames_whatever_the_batch(model, clip, batch):
    frames, handle, plain, want = clip
    got = model.predict_frames(frames, handle, alpha=0.8, batch=batch, guided=G, guided_frames=T)
    assert np.array_equal(got, want)
    if batch == 3:
        both = model.predict_frames(frames, handle, alpha=0.8, batch=batch, guided=G, guided_frames=T, content_colors=True)
        assert np.array_equal(both, colors_oracle.content_colors(want, frames))            # the colour op runs last
        from wct_tf_amd import guided_filter_time_np
        assert np.array_equal(got, guided_filter_time_np(plain, frames, G[0], G[1], T, ctx=model.sess))


def test_predict_frames_without_frames_on_either_side_is_the_flagged_call(model, clip):
    frames, handle, plain, _ = clip
    want = g2.guided_filter(plain, frames, *G)
    assert np.array_equal(model.predict_frames(frames, handle, alpha=0.8, batch=3, guided=G, guided_frames=0), want)
    assert np.array_equal(model.predict_frames(frames, handle, alpha=0.8, batch=3, guided=G), want)


def test_predict_frames_with_a_style_image_warm_strengths_and_resize(model, clip):
    frames, handle, plain, want = clip
    style = synthetic_image(29, 80, 64)
    assert np.array_equal(model.predict_frames(frames, style, alpha=0.8, batch=3, guided=G, guided_frames=T), want)
    with model.warm_state() as w:                                 # warm runs are bit-reproducible from a fresh state
        warm_plain = model.predict_frames(frames, handle, alpha=0.8, batch=3, warm=w)
    with model.warm_state() as w:
        got = model.predict_frames(frames, handle, alpha=0.8, batch=3, warm=w, guided=G, guided_frames=T)
    assert np.array_equal(got, oracle.guided_filter_time(warm_plain, frames, G[0], G[1], T))
    smap = np.tile(np.linspace(0, 255, 48).astype(np.uint8), (40, 1))
    s_plain = model.predict_frames(frames, handle, alpha=0.8, batch=3, strengths=smap)
    got = model.predict_frames(frames, handle, alpha=0.8, batch=3, strengths=smap, guided=G, guided_frames=T)
    assert np.array_equal(got, oracle.guided_filter_time(s_plain, frames, G[0], G[1], T))
    raw = np.stack([synthetic_image(40 + i, 50, 60) for i in range(4)])
    small = np.stack([utils._imresize(f, (40, 48)) for f in raw])
    r_plain = model.predict_frames(raw, handle, alpha=0.8, batch=3, resize=(40, 48))
    got = model.predict_frames(raw, handle, alpha=0.8, batch=3, resize=(40, 48), guided=G, guided_frames=T, content_colors=True)
    assert np.array_equal(got, colors_oracle.content_colors(oracle.guided_filter_time(r_plain, small, G[0], G[1], T), small))


# ---- the video tool, end to end ---------------------------------------------------------------------------------------------
TARGETS = ['relu3_1', 'relu1_1']


def test_stylize_video_cli_two_clips_two_batch_sizes_and_two_passes(tmp_path):
    """6 frames of 32 x 40 and then 3 of 40 x 32: two clips.  The files do not depend on --batch and equal the per-clip op on the
    plain run's files; with --passes 2 the op runs once at the end, against the input frames, before the colour op."""
    from wct_tf_amd.stylize_video import main
    in_dir = tmp_path / 'clip'
    in_dir.mkdir()
    clips = [np.stack([synthetic_image(90 + i, 32, 40) for i in range(6)]), np.stack([synthetic_image(100 + i, 40, 32) for i in range(3)])]
    names = ['frame_%d.png' % (i + 1) for i in range(9)]
    for name, img in zip(names, [f for c in clips for f in c]):
        utils.save_img(str(in_dir / name), img)
    utils.save_img(str(tmp_path / 's0.png'), synthetic_image(95, 56, 48))
    base = ['--relu-targets'] + TARGETS + ['--in-path', str(in_dir), '--alpha', '0.8', '--synthetic-weights', '42',
                                          '--style-path', str(tmp_path / 's0.png')]
    smooth = ['--guided-radius', '3', '--guided-frames', '1']
    read = lambda d: [utils.get_img(str(tmp_path / d / 'clip_s0' / n)) for n in names]
    assert main(base + ['--batch', '5', '--out-path', str(tmp_path / 'plain')]) == 9
    assert main(base + smooth + ['--batch', '2', '--out-path', str(tmp_path / 'b2')]) == 9
    assert main(base + smooth + ['--batch', '5', '--out-path', str(tmp_path / 'b5')]) == 9
    plain, b2, b5 = read('plain'), read('b2'), read('b5')
    want = [f for lo, hi, c in ((0, 6, clips[0]), (6, 9, clips[1])) for f in oracle.guided_filter_time(np.stack(plain[lo:hi]), c, 3, 650, 1)]
    for i in range(9):
        assert np.array_equal(b2[i], b5[i]) and np.array_equal(b5[i], want[i]), i
    assert main(base + ['--batch', '5', '--passes', '2', '--out-path', str(tmp_path / 'plain2')]) == 9
    assert main(base + smooth + ['--batch', '2', '--passes', '2', '--content-colors', '--out-path', str(tmp_path / 'two')]) == 9
    plain2, two = read('plain2'), read('two')
    for lo, hi, c in ((0, 6, clips[0]), (6, 9, clips[1])):
        want = colors_oracle.content_colors(oracle.guided_filter_time(np.stack(plain2[lo:hi]), c, 3, 650, 1), c)
        for i in range(lo, hi):
            assert np.array_equal(two[i], want[i - lo]), i
