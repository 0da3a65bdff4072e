"""Strength maps on the GPU: wct_transform_strength / wct_adain_strength against the plain alpha = 1 call blended by the NumPy
rule (bit for bit) and against the float64 oracle (tests/strength_oracle.py), the prepared-style frames against their anchors,
the per-level sampling, the values end to end, the ABI refusals and the command lines."""
import ctypes as C
import os

import numpy as np
import pytest

import strength_oracle as so
from conftest import rel_err, max_rel
from wct_tf_amd import _lib
from wct_tf_amd.weights import synthetic_features, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
WCT_TOL = 1e-3                       # tests/test_gpu_ops.py, tests/test_gpu_mask.py
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
H, W, STRIDE, HM, WM = 19, 23, 4, 70, 86      # N = 437: four pixel blocks, the last of 53 rows; the last row and column clamp


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def small_ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.set_weights(synthetic_weights(5, relu_targets=SMALL))
    yield c
    c.close()


@pytest.fixture(scope='module')
def frame_case(small_ctx):
    """the 90 x 75 content (every level's size is ragged), the 72 x 88 style and its handle"""
    c, s = synthetic_image(11, 90, 75), synthetic_image(12, 72, 88)
    st = small_ctx.prepare_style(s, SMALL)
    yield c, s, st
    st.close()


def _flat(f):
    return np.ascontiguousarray(f.reshape(-1, f.shape[-1]))


def random_map(seed):
    """random bytes with 0 and 255 forced in, at sampled pixels of the interior and of the clamped last row and column"""
    m = np.random.default_rng(seed).integers(0, 256, (HM, WM)).astype(np.uint8)
    m[0, 0], m[4, 8], m[HM - 1, WM - 1], m[HM - 1, 0], m[8, WM - 1] = 0, 255, 0, 255, 0
    assert (H - 1) * STRIDE > HM - 1 and (W - 1) * STRIDE > WM - 1
    return m


def smooth_map(seed, h, w):
    """a smooth random map over the whole byte range"""
    f = np.random.default_rng(seed).standard_normal((h, w))
    for _ in range(6):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
    f = (f - f.min()) / (f.max() - f.min())
    return np.uint8(np.round(f * 255))


_cases = {}


def level_case(ctx, c, kind):
    """the inputs of a one-level case and what the device gives for them, computed once: the strength call at alpha = 0.8 and at
    1, the plain call at alpha = 1"""
    if (c, kind) not in _cases:
        fc = synthetic_features(100 + c, c, H, W, 2.0).reshape(H, W, c)
        fs = synthetic_features(200 + c, c, 20, 26, 2.0).reshape(20, 26, c)
        smap = random_map(c)
        x, s = _flat(fc), _flat(fs)
        if kind == 'adain':
            got, got1, plain = (ctx.adain_strength(x, s, smap, H, W, STRIDE, 0.8), ctx.adain_strength(x, s, smap, H, W, STRIDE, 1.0),
                                ctx.adain(x, s, 1.0))
            sweeps = psweeps = None
        else:
            mode = _lib.WCT_NP if kind == 'np' else _lib.WCT_TF
            got, sweeps = ctx.transform_strength(x, s, smap, H, W, STRIDE, 0.8, mode, return_sweeps=True)
            got1 = ctx.transform_strength(x, s, smap, H, W, STRIDE, 1.0, mode)
            plain, psweeps = ctx.transform(x, s, 1.0, mode, return_sweeps=True)
        _cases[(c, kind)] = dict(fc=fc, fs=fs, smap=smap, got=got, got1=got1, plain=plain, sweeps=sweeps, psweeps=psweeps)
    return _cases[(c, kind)]


LEVEL_CASES = [(c, k) for c in (64, 256, 512) for k in ('tf', 'np')] + [(64, 'adain'), (512, 'adain')]


@pytest.mark.parametrize('c,kind', LEVEL_CASES)
def test_composition_bit_for_bit(ctx, c, kind):
    """the device's rows are the plain alpha = 1 call's rows blended with the content by the NumPy rule: both tile variants of the
    apply (C = 64; C >= 128 with 2 and 4 channel blocks), a ragged last pixel block, the clamped last row and column"""
    k = level_case(ctx, c, kind)
    x = _flat(k['fc'])
    v = so.level_bytes(k['smap'], H, W, STRIDE).reshape(-1)
    assert (v == 0).sum() >= 3 and (v == 255).sum() >= 2
    a = so.level_strength(k['smap'], H, W, STRIDE, 0.8).reshape(-1)
    want = so.blend(k['plain'], x, a)
    diff = k['got'] != want
    print('C = %d %s: %d of %d elements differ from blend(plain alpha = 1, x, a)' % (c, kind, diff.sum(), diff.size))
    assert np.array_equal(k['got'], want)
    assert k['sweeps'] == k['psweeps']
    assert np.array_equal(k['got'][v == 0], x[v == 0])                          # v = 0: the content, whatever alpha
    assert np.array_equal(k['got1'][v == 0], x[v == 0])
    assert np.array_equal(k['got1'][v == 255], k['plain'][v == 255])            # v = 255 with alpha = 1: the plain row
    assert np.array_equal(k['got1'], so.blend(k['plain'], x, so.level_strength(k['smap'], H, W, STRIDE, 1.0).reshape(-1)))
    assert not np.array_equal(k['got'][v == 255], k['plain'][v == 255])         # (alpha = 0.8 is not alpha = 1)


@pytest.mark.parametrize('c,kind', LEVEL_CASES)
def test_against_the_float64_oracle(ctx, c, kind):
    k = level_case(ctx, c, kind)
    o64 = so.transform(k['fc'], k['fs'], k['smap'], STRIDE, 0.8, kind, f64=True).reshape(-1, c)
    o32 = so.transform(k['fc'], k['fs'], k['smap'], STRIDE, 0.8, kind, f64=False).reshape(-1, c)
    e, ref = rel_err(k['got'], o64), rel_err(o32, o64)
    print('C = %d %s: %.2e from the float64 oracle (float32 oracle %.2e), max %.2e' % (c, kind, e, ref, max_rel(k['got'], o64)))
    assert e < max(WCT_TOL, 4 * ref)


# ---- frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True), dict(content_colors=True), dict(f32=True)], ids=str)
def test_an_all_255_map_at_alpha_1_is_the_plain_frame(small_ctx, frame_case, kw):
    c, _, st = frame_case
    kw = dict(kw)
    if kw.pop('f32', False):
        c = np.float32(c) + 0.25
    ones = np.full(c.shape[:2], 255, np.uint8)
    got = small_ctx.stylize_prepared_strength(c, st, ones, SMALL, alpha=1.0, **kw)
    assert got.shape == (92, 76, 3)
    assert np.array_equal(got, small_ctx.stylize_prepared(c, st, SMALL, alpha=1.0, **kw))
    zero = small_ctx.stylize_prepared_strength(c, st, np.zeros_like(ones), SMALL, alpha=1.0, **kw)
    assert not np.array_equal(zero, got)                                        # (the map is read)


def test_batch_frames_are_the_single_calls(small_ctx, frame_case):
    _, _, st = frame_case
    frames = np.stack([synthetic_image(40 + f, 90, 75) for f in range(3)])
    maps = np.stack([smooth_map(50 + f, 90, 75) for f in range(3)])
    got = small_ctx.stylize_prepared_strength_batch(frames, st, maps, SMALL, alpha=0.8)
    singles = [small_ctx.stylize_prepared_strength(frames[f], st, maps[f], SMALL, alpha=0.8) for f in range(3)]
    for f in range(3):
        assert np.array_equal(got[f], singles[f]), f
    assert not np.array_equal(singles[0], small_ctx.stylize_prepared_strength(frames[0], st, maps[1], SMALL, alpha=0.8))
    # one [H][W] map for all frames is the stacked maps
    one = small_ctx.stylize_prepared_strength_batch(frames, st, maps[1], SMALL, alpha=0.8, adain=True)
    assert np.array_equal(one, small_ctx.stylize_prepared_strength_batch(frames, st, np.stack([maps[1]] * 3), SMALL, alpha=0.8, adain=True))
    assert np.array_equal(one[2], small_ctx.stylize_prepared_strength(frames[2], st, maps[1], SMALL, alpha=0.8, adain=True))


def test_resize_is_the_call_on_pillows_frames(small_ctx, frame_case):
    from wct_tf_amd import utils
    _, _, st = frame_case
    raw = np.stack([synthetic_image(60 + f, 120, 100) for f in range(2)])
    maps = np.stack([smooth_map(70 + f, 90, 75) for f in range(2)])
    got = small_ctx.stylize_prepared_strength_batch(raw, st, maps, SMALL, alpha=0.8, resize=(90, 75), content_colors=True)
    host = np.stack([utils._imresize(f, (90, 75)) for f in raw])
    assert np.array_equal(got, small_ctx.stylize_prepared_strength_batch(host, st, maps, SMALL, alpha=0.8, content_colors=True))


def test_warm_with_an_all_255_map_is_the_plain_warm_call(small_ctx, frame_case):
    _, _, st = frame_case
    frames = np.stack([synthetic_image(80 + f, 90, 75) for f in range(2)])
    ones = np.full((90, 75), 255, np.uint8)
    with small_ctx.warm_state(SMALL) as wa, small_ctx.warm_state(SMALL) as wb:
        for step in range(2):                                                   # cold, then from the state the first call left
            plain = small_ctx.stylize_prepared_batch(frames, st, SMALL, alpha=1.0, warm=wa)
            got = small_ctx.stylize_prepared_strength_batch(frames, st, ones, SMALL, alpha=1.0, warm=wb)
            assert np.array_equal(got, plain), step
            assert all(wb.valid(l) for l in (1, 2, 3))


@pytest.mark.parametrize('target,step', [('relu3_1', 4), ('relu2_1', 2)])
def test_each_level_samples_its_own_stride(small_ctx, frame_case, target, step):
    c, _, st = frame_case
    base = smooth_map(90, 90, 75)
    ref = small_ctx.stylize_prepared_strength(c, st, base, [target], alpha=0.8)
    yy, xx = np.mgrid[:90, :75]
    unsampled = (yy % step != 0) | (xx % step != 0)
    other = base.copy()
    other[unsampled] = 255 - other[unsampled]
    assert np.array_equal(small_ctx.stylize_prepared_strength(c, st, other, [target], alpha=0.8), ref)
    one = base.copy()
    one[10 * step, 7 * step] = 255 - one[10 * step, 7 * step]                   # a sampled pixel: feature pixel (10, 7)
    assert not np.array_equal(small_ctx.stylize_prepared_strength(c, st, one, [target], alpha=0.8), ref)


def _frame_error(got, want):
    d = np.abs(got.astype(int) - want.astype(int))
    return 10 * np.log10(255.0 ** 2 / max(np.mean((got.astype(np.float64) - want) ** 2), 1e-12)), d.mean()


def test_values_end_to_end_against_the_float64_oracle(small_ctx, frame_case):
    """The 90 x 75 content under a smooth ramp, alpha = 0.8, three levels, against strength_oracle.stylize in float64.  The
    yardstick is the plain stylize_prepared frame against its own float64 oracle on the same images: the strength frame runs the
    same stages plus three roundings per element, so it may be at most 1 dB and 0.25 mean LSB worse."""
    c, s, st = frame_case
    ramp = np.uint8(np.round(np.linspace(0, 255, 75)))[None, :].repeat(90, 0)
    w = synthetic_weights(5, relu_targets=SMALL)
    got = small_ctx.stylize_prepared_strength(c, st, ramp, SMALL, alpha=0.8)
    plain = small_ctx.stylize_prepared(c, st, SMALL, alpha=0.8)
    psnr, lsb = _frame_error(got, so.stylize(c, s, ramp, w, SMALL, alpha=0.8))
    ppsnr, plsb = _frame_error(plain, so.stylize(c, s, None, w, SMALL, alpha=0.8))
    print('strength frame: psnr %.2f dB, mean LSB %.4f; plain frame: psnr %.2f dB, mean LSB %.4f' % (psnr, lsb, ppsnr, plsb))
    assert got.shape == (92, 76, 3) and not np.array_equal(got, plain)
    assert psnr >= ppsnr - 1.0 and lsb <= plsb + 0.25


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_context_usable(small_ctx, frame_case):
    lib = small_ctx.lib
    c, _, st = frame_case
    c = np.ascontiguousarray(c)
    smap = smooth_map(91, 90, 75)
    lv = (C.c_int * 3)(3, 2, 1)
    out = np.zeros((92, 76, 3), np.uint8)
    u8p = lambda a: a.ctypes.data_as(_lib._U8)
    before = small_ctx.stylize_prepared_strength(c, st, smap, SMALL, alpha=0.7)

    def host(flags=0, m=smap, handle=None, levels=lv, hc=90, wc=75):
        return lib.wct_stylize_prepared_strength(small_ctx.h, u8p(c), hc, wc, u8p(m) if m is not None else None,
                                                 st.h if handle is None else handle, levels, len(levels), C.c_float(0.7), flags, u8p(out))

    dc, dm, do = small_ctx.dev_alloc(3 * c.nbytes), small_ctx.dev_alloc(3 * smap.nbytes), small_ctx.dev_alloc(3 * out.nbytes)
    try:
        def batch(b=3, flags=0, m=dm, handle=None, levels=lv, hc=90, wc=75):
            return lib.wct_stylize_prepared_strength_batch_dev(small_ctx.h, dc, hc, wc, b, m, st.h if handle is None else handle,
                                                               levels, len(levels), C.c_float(0.7), flags, do)

        fake = C.c_void_p(0x1000)
        calls = [(lambda: host(flags=_lib.FLAG_SWAP5), -2, b'SWAP5'), (lambda: host(flags=_lib.FLAG_STYLE_SHARED), -2, b'STYLE_SHARED'),
                 (lambda: host(m=None), -2, b'no map'), (lambda: host(levels=(C.c_int * 2)(4, 1)), -2, b'relu4_1'),
                 (lambda: host(hc=3000, wc=3000), -2, b'limit of one launch'), (lambda: host(handle=fake), -3, b'not a live handle'),
                 (lambda: batch(flags=_lib.FLAG_SWAP5), -2, b'SWAP5'), (lambda: batch(flags=_lib.FLAG_STYLE_SHARED), -2, b'STYLE_SHARED'),
                 (lambda: batch(m=None), -2, b'no map'), (lambda: batch(b=0), -2, b'1 .. 32'), (lambda: batch(b=33), -2, b'1 .. 32'),
                 (lambda: batch(levels=(C.c_int * 2)(4, 1)), -2, b'relu4_1'),
                 (lambda: batch(hc=3000, wc=3000), -2, b'limit of one launch'), (lambda: batch(handle=fake), -3, b'not a live handle')]
        for i, (call, want, word) in enumerate(calls):
            assert call() == want, i
            assert word in lib.wct_last_error(), (i, lib.wct_last_error())
        # the op level: rows that are not the h x w map's, no map
        f = _lib.f32(np.ones((12, 64)))
        o = np.zeros((12, 64), np.float32)
        m8 = np.zeros((6, 8), np.uint8)
        assert lib.wct_transform_strength(small_ctx.h, _lib.fptr(f), 12, 3, 5, u8p(m8), 6, 8, 2, _lib.fptr(f), 12, 64, C.c_float(1),
                                          _lib.WCT_TF, C.c_float(-1), _lib.fptr(o), None) == -2
        assert lib.wct_adain_strength(small_ctx.h, _lib.fptr(f), 12, 3, 4, None, 6, 8, 2, _lib.fptr(f), 12, 64, C.c_float(1),
                                      C.c_float(1e-5), _lib.fptr(o)) == -2 and b'no map' in lib.wct_last_error()
        # a good call on the same context, both ways
        assert host() == 0 and np.array_equal(out, before)
        small_ctx.h2d(dc, np.stack([c] * 3))
        small_ctx.h2d(dm, np.stack([smap] * 3))
        assert batch() == 0
        small_ctx.sync()
        got = np.zeros((3,) + out.shape, np.uint8)
        small_ctx.d2h(got, do)
        assert all(np.array_equal(got[f], before) for f in range(3))
    finally:
        for p in (dc, dm, do):
            small_ctx.dev_free(p)


# ---- command lines ---------------------------------------------------------------------------------------------------------
def test_cli_alpha_map_end_to_end(tmp_path):
    from PIL import Image
    from wct_tf_amd import stylize, stylize_video, utils
    from wct_tf_amd.wct import WCT
    cpath, spath = str(tmp_path / 'cat.png'), str(tmp_path / 'a.png')
    utils.save_img(cpath, synthetic_image(31, 64, 80))
    utils.save_img(spath, synthetic_image(32, 64, 48))
    greys = [smooth_map(33 + f, 32, 40) for f in range(3)]                      # at half the content's size: resized (bilinear)
    mpath = str(tmp_path / 'm.png')
    Image.fromarray(greys[0]).save(mpath)
    out_dir = str(tmp_path / 'out')
    common = ['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--style-path', spath, '--alpha', '0.8']
    assert stylize.main(common + ['--content-path', cpath, '--out-path', out_dir, '--alpha-map', mpath]) == 1
    assert os.listdir(out_dir) == ['cat_a.png']                                 # the name of the plain run
    # a video: three frames, three maps matched in sorted order
    fdir, mdir, vout = tmp_path / 'clip', tmp_path / 'maps', str(tmp_path / 'vout')
    fdir.mkdir()
    mdir.mkdir()
    frames = [synthetic_image(36 + f, 64, 80) for f in range(3)]
    for f in range(3):
        utils.save_img(str(fdir / ('frame_%d.png' % (f + 1))), frames[f])
        Image.fromarray(greys[f]).save(str(mdir / ('map_%d.png' % (f + 1))))
    assert stylize_video.main(common + ['--in-path', str(fdir), '--out-path', vout, '--alpha-map', str(mdir)]) == 3
    model = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    try:
        style = utils.get_img(spath)
        maps = [np.array(Image.fromarray(g).resize((80, 64), Image.BILINEAR)) for g in greys]
        want = model.predict(utils.get_img(cpath), style, 0.8, strength=maps[0])
        assert np.array_equal(utils.get_img(os.path.join(out_dir, 'cat_a.png')), want)
        assert not np.array_equal(want, model.predict(utils.get_img(cpath), style, 0.8))
        assert sorted(os.listdir(os.path.join(vout, 'clip_a'))) == ['frame_1.png', 'frame_2.png', 'frame_3.png']
        for f in range(3):
            want = model.predict(frames[f], style, 0.8, strength=maps[f])
            assert np.array_equal(utils.get_img(os.path.join(vout, 'clip_a', 'frame_%d.png' % (f + 1))), want), f
        assert np.array_equal(model.predict_frames(np.stack(frames), style, 0.8, strengths=np.stack(maps))[1],
                              model.predict(frames[1], style, 0.8, strength=maps[1]))
    finally:
        model.sess.close()
