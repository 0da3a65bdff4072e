"""Guided smoothing without a GPU: the NumPy oracle of the rule against a naive loop over windows and against the float64 guided
filter, the properties the rule was chosen for, the command lines, the Python refusals, and the shared rule header
(wct_tf_amd/csrc/guided_rule.h, what the kernels compile) built for the host under AddressSanitizer + UBSan as a program of its
own."""
import argparse
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 4, 16])
def test_vectorised_oracle_is_the_scalar_loop(r):
    """9 x 13: at r = 16 every window is the whole image"""
    s, c = _rand(1, (9, 13, 3)), _rand(2, (9, 13, 3))
    got = oracle.guided_filter(s, c, r, 650)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.guided_filter_loop(s, c, r, 650))
    if r == 16:
        assert (oracle.count(9, 13, r) == 9 * 13).all()


def test_frame_larger_than_content_reads_the_clamped_guide():
    s, c = _rand(3, (16, 20, 3)), _rand(4, (9, 13, 3))
    assert np.array_equal(oracle.guided_filter(s, c, 2, 100), oracle.guided_filter_loop(s, c, 2, 100))
    g = oracle.guide(c, 16, 20)
    assert np.array_equal(g[9:, :13], np.broadcast_to(g[8:9, :13], (7, 13))) and (g[9:, 13:] == g[8, 12]).all()
    sb, cb = _rand(5, (3, 16, 20, 3)), _rand(6, (3, 9, 13, 3))            # batched: every frame against its own content
    got = oracle.guided_filter(sb, cb, 3, 650)
    for f in range(3):
        assert np.array_equal(got[f], oracle.guided_filter(sb[f], cb[f], 3, 650))


@pytest.mark.parametrize('shape,r,eps_q', [((33, 35), 1, 1), ((48, 48), 4, 650), ((40, 52), 5, 65025), ((30, 31), 8, 7),
                                           ((64, 64), 16, 650), ((70, 66), 64, 1)], ids=str)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(shape, r, eps_q):
    """before the clamp: 0.5 from the final rounding, 255 * 2^-13 from the rounding of a_q (at most half a unit of 2^-12 each,
    their window mean times a guide of at most 255) and 2^-13 from that of b_q: 0.5 + 256 * 2^-13 < 0.54"""
    s, c = _rand(10, shape + (3,)), _rand(11, shape + (3,))
    err = np.abs(oracle.guided_filter_unclamped(s, c, r, eps_q) - oracle.guided_filter_f64(s, c, r, eps_q)).max()
    assert err <= 0.54, err


def test_a_constant_frame_comes_back_exactly():
    c = _rand(12, (40, 44, 3))
    for v, r, eps_q in ((0, 1, 1), (255, 64, 65025), (77, 5, 650)):
        s = np.full((40, 44, 3), v, np.uint8)
        assert np.array_equal(oracle.guided_filter(s, c, r, eps_q), s)


def test_a_grey_image_guiding_itself_at_the_smallest_eps_comes_back_exactly():
    """a = var / (var + 1 / n^2 ...) rounds to a line through the pixel's own value: the filter of I by I is I"""
    g = np.repeat(_rand(13, (40, 44, 1)), 3, axis=2)
    for r in (1, 4, 16):
        assert np.array_equal(oracle.guided_filter(g, g, r, 1), g)


def test_a_step_edge_survives_and_the_noise_falls_below_a_tenth():
    rng = np.random.default_rng(14)
    h, w = 64, 96
    guide = np.where(np.arange(w) < w // 2, 50, 200)[None, :].repeat(h, 0)
    c = np.repeat(guide[..., None], 3, -1).astype(np.uint8)
    s = (guide + rng.integers(-20, 21, (h, w)))[..., None].repeat(3, -1).astype(np.uint8)
    # eps_q = 65 (0.001): a window across the edge has variance 75^2, so a >= 5625 / 5690 and the step keeps 98.8 % of its
    # height -- at most 0.9 grey levels lost on either side, plus what is left of the noise
    out = oracle.guided_filter(s, c, 8, 65).astype(np.float64)[..., 0]
    left, right = out[:, :w // 2], out[:, w // 2:]
    assert abs(left[:, -1].mean() - 50) < 3 and abs(right[:, 0].mean() - 200) < 3            # the step, at the edge itself
    noise_in = (s[..., 0].astype(np.float64) - guide).std()
    noise_out = np.concatenate([(left - 50).ravel(), (right - 200).ravel()]).std()
    assert noise_out < noise_in / 10, (noise_in, noise_out)


def test_a_flat_guide_gives_the_box_mean_of_the_box_mean():
    s = _rand(15, (40, 44, 3))
    c = np.full((40, 44, 3), 128, np.uint8)
    r = 3
    n = oracle.count(40, 44, r).astype(np.float64)
    for ch in range(3):
        mean = oracle.box(s[..., ch].astype(np.float64), r) / n
        want = oracle.box(mean, r) / n
        got = oracle.guided_filter(s, c, r, 650)[..., ch].astype(np.float64)
        assert np.abs(got - want).max() <= 1


def test_the_clamp_case_leaves_the_range_before_the_clamp():
    s, c = oracle.clamp_case()
    raw = oracle.guided_filter_unclamped(s, c, 1, 1)
    share = ((raw < 0) | (raw > 255)).any(-1).mean()
    assert share > 0, share
    out = oracle.guided_filter(s, c, 1, 1)
    assert np.array_equal(out, np.clip(raw, 0, 255))
    assert np.array_equal(out, oracle.guided_filter_loop(s, c, 1, 1))


def test_eps_of_the_unit_convention():
    from wct_tf_amd import _lib
    assert _lib.guided_eps_q(0.01) == oracle.eps_q_of(0.01) == 650
    assert _lib.guided_eps_q(1e-9) == 1 and _lib.guided_eps_q(1.0) == 65025
    assert (_lib.GUIDED_MAX_RADIUS, _lib.GUIDED_MAX_EPS) == (oracle.MAX_RADIUS, oracle.MAX_EPS)


# ---- command lines ---------------------------------------------------------------------------------------------------------
_IMG = ['--relu-targets', 'relu1_1', '--content-path', 'c', '--out-path', 'o', '--synthetic-weights', '1']
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1']


def _check_image(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_interp_args(parser, args)
    stylize.check_mask_args(parser, args)
    stylize.check_color_args(parser, args)
    stylize.check_guided_args(parser, args)
    stylize.check_band_args(parser, args)
    stylize.check_alpha_map_args(parser, args)
    return args


def _check_video(argv):
    from wct_tf_amd import stylize_video
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_mask_args(parser, args)
    stylize_video.check_warm_args(parser, args)
    stylize_video.check_color_args(parser, args)
    stylize_video.check_guided_args(parser, args)
    stylize_video.check_resize_args(parser, args)
    stylize_video.check_alpha_map_args(parser, args)
    return args


def test_both_command_lines_have_the_filter_off_by_default():
    from wct_tf_amd.stylize import guided_of
    for check, argv in ((_check_image, _IMG), (_check_video, _VID)):
        a = check(argv + ['--style-path', 's'])
        assert a.guided_radius == 0 and a.guided_eps == 0.01 and guided_of(a) is None
        a = check(argv + ['--style-path', 's', '--guided-radius', '8'])
        assert guided_of(a) == (8, 650)
        a = check(argv + ['--style-path', 's', '--guided-radius', '64', '--guided-eps', '1e-9'])
        assert guided_of(a) == (64, 1)
        a = check(argv + ['--style-path', 's', '--guided-radius', '1', '--guided-eps', '4'])
        assert guided_of(a) == (1, 65025)                  # eps_q stops at 255^2
    assert guided_of(argparse.Namespace(passes=1)) is None  # a caller's own Namespace without the options


def test_bad_radius_and_eps_are_refused(capsys):
    for check, argv in ((_check_image, _IMG), (_check_video, _VID)):
        for extra, word in ((['--guided-radius', '65'], '--guided-radius'), (['--guided-radius', '-1'], '--guided-radius'),
                            (['--guided-radius', '4', '--guided-eps', '0'], '--guided-eps'),
                            (['--guided-radius', '4', '--guided-eps', '-0.1'], '--guided-eps'),
                            (['--guided-eps', 'nan'], '--guided-eps')):
            with pytest.raises(SystemExit):
                check(argv + ['--style-path', 's'] + extra)
            assert word in capsys.readouterr().err


def test_filter_is_refused_in_bands(capsys):
    with pytest.raises(SystemExit):
        _check_image(_IMG + ['--style-path', 's', '--guided-radius', '4', '--band-rows', '64'])
    assert '--guided-radius' in capsys.readouterr().err
    assert _check_image(_IMG + ['--style-path', 's', '--band-rows', '64']).band_rows == 64
    # a content past the limit of one launch would run in bands: refused when it is met, with the option named
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = _check_image(_IMG + ['--style-path', 's', '--guided-radius', '4'])
    with pytest.raises(SystemExit):
        stylize.check_content_fits(parser, args, np.zeros((4096, 4096, 0), np.uint8), 'big.png')
    assert '--guided-radius' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _check_video(_VID + ['--style-path', 's', '--guided-radius', '4', '--device-resize', '--content-size', '64', '--passes', '2'])
    assert '--passes 1' in capsys.readouterr().err


def test_filter_combines_with_the_other_options():
    from wct_tf_amd import stylize
    a = _check_image(_IMG + ['--guided-radius', '4', '--mask-path', 'm.png', '--mask-styles', 'a', 'b'])
    assert a.guided_radius == 4 and stylize.can_prepare(a)
    a = _check_image(_IMG + ['--guided-radius', '4', '--interp-styles', 'a', 'b', '--interp-weights', '1', '3'])
    assert a.guided_radius == 4 and stylize.can_prepare(a)
    a = _check_image(_IMG + ['--guided-radius', '4', '--content-colors', '--style-path', 's', '--swap5', '--passes', '2'])
    assert a.content_colors and a.swap5
    a = _check_image(_IMG + ['--guided-radius', '4', '--style-path', 's', '--adain', '--alpha-map', 'm.png'])
    assert a.adain and a.alpha_map == 'm.png'
    assert _check_video(_VID + ['--guided-radius', '4', '--style-path', 's', '--warm-start']).warm_start
    assert _check_video(_VID + ['--guided-radius', '4', '--mask-path', 'm', '--mask-styles', 'a', 'b']).mask_path == 'm'
    assert _check_video(_VID + ['--guided-radius', '4', '--style-path', 's', '--device-resize', '--content-size', '64']).device_resize
    assert _check_video(_VID + ['--guided-radius', '4', '--style-path', 's', '--alpha-map', 'm']).alpha_map == 'm'


def test_run_passes_fuses_one_pass_and_applies_the_ops_once_after_several(monkeypatch):
    """the routing of stylize.run_passes, with a stand-in for the prediction and the oracles for the ops: the filter first, the
    colour op last, both against the original content"""
    import colors_oracle
    from wct_tf_amd import ops, stylize
    monkeypatch.setattr(ops, 'content_colors_np', lambda s, c, ctx=None: colors_oracle.content_colors(s, c))
    monkeypatch.setattr(ops, 'guided_filter_np', lambda s, c, r, e, ctx=None: oracle.guided_filter(s, c, r, e))
    content, model = _rand(20, (12, 16, 3)), argparse.Namespace(sess=None)
    calls = []

    def predict(img, colors, guided=None):
        calls.append((colors, guided))
        out = np.uint8(255 - img)
        if guided:
            out = oracle.guided_filter(out, img, *guided)
        return colors_oracle.content_colors(out, img) if colors else out

    ns = lambda **kw: argparse.Namespace(guided_radius=2, guided_eps=0.01, **kw)
    smooth = oracle.guided_filter(np.uint8(255 - content), content, 2, 650)
    one = stylize.run_passes(model, content, ns(passes=1, content_colors=True), predict)
    assert calls == [(True, (2, 650))] and np.array_equal(one, colors_oracle.content_colors(smooth, content))
    del calls[:]
    one = stylize.run_passes(model, content, ns(passes=1, content_colors=False), predict)
    assert calls == [(False, (2, 650))] and np.array_equal(one, smooth)
    del calls[:]
    two = stylize.run_passes(model, content, ns(passes=2, content_colors=True), predict)           # 255 - (255 - x) = x
    assert calls == [(False, None), (False, None)]
    assert np.array_equal(two, colors_oracle.content_colors(oracle.guided_filter(content, content, 2, 650), content))
    del calls[:]
    # a caller's two-argument predict and a Namespace without the options keep working
    plain = stylize.run_passes(model, content, argparse.Namespace(passes=2, content_colors=False), lambda img, colors: np.uint8(255 - img))
    assert np.array_equal(plain, content)


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context
    from wct_tf_amd.wct import WCT
    import wct_tf_amd
    assert wct_tf_amd.guided_filter_np is wct_tf_amd.ops.guided_filter_np and 'guided_filter_np' in wct_tf_amd.__all__
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (16, 20, 3)), _rand(31, (9, 20, 3))
    with pytest.raises(ValueError, match='smaller'):
        ctx.guided_filter(c, s, 4, 650)                  # Ho < Hc
    with pytest.raises(ValueError, match='smaller'):
        ctx.guided_filter(s[:, :10], c, 4, 650)          # Wo < Wc
    with pytest.raises(ValueError, match='guided_filter takes uint8'):
        ctx.guided_filter(s.astype(np.float32), c, 4, 650)
    with pytest.raises(ValueError, match='HxWx3'):
        ctx.guided_filter(s[..., :2], c, 4, 650)
    for r, e, word in ((0, 650, 'radius'), (65, 650, 'radius'), (4, 0, 'eps_q'), (4, 65026, 'eps_q'), (4.5, 650, 'integers')):
        with pytest.raises(ValueError, match=word):
            ctx.guided_filter(s, c, r, e)
        with pytest.raises(ValueError, match=word):
            ctx.guided_filter_batch(s[None], c[None], r, e)
        with pytest.raises(ValueError, match=word):
            ctx.guided_filter_batch_dev(None, 16, 20, None, 9, 20, 1, r, e, None)
        with pytest.raises(ValueError, match=word):
            ctx.set_guided(r, e)
        with pytest.raises(ValueError, match=word):
            ctx.stylize(c, s, ['relu1_1'], guided=(r, e))
    with pytest.raises(ValueError, match=r'\[B\]\[H\]\[W\]\[3\]'):
        ctx.guided_filter_batch(s, c, 4, 650)
    with pytest.raises(ValueError, match='as many contents'):
        ctx.guided_filter_batch(np.stack([s, s]), c[None], 4, 650)
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.guided_filter_batch(np.zeros((33, 4, 4, 3), np.uint8), np.zeros((33, 4, 4, 3), np.uint8), 4, 650)
    # the model's keyword: checked before anything else of the call, refused in bands and on the torus
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    for call in (lambda g: m.predict(c, s, guided=g), lambda g: m.predict_frames(c[None], s, guided=g),
                 lambda g: m.predict_mix(c, [s], guided=g), lambda g: m.predict_masked(c, [s], np.zeros((9, 20)), guided=g),
                 lambda g: m.predict_frames_masked(c[None], [s], np.zeros((9, 20)), guided=g)):
        with pytest.raises(ValueError, match='radius'):
            call((0, 650))
        with pytest.raises(ValueError, match='two integers'):
            call(4)
    with pytest.raises(ValueError, match='guided is not served in bands'):
        m.predict(c, s, band_rows=16, guided=(4, 650))


def test_flag_value_matches_the_header():
    import re
    from wct_tf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    assert int(re.search(r'WCT_FLAG_GUIDED\s*=\s*(\d+)', hdr).group(1)) == _lib.FLAG_GUIDED == 64
    assert 'guided.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_rule.h')).read()
    assert int(re.search(r'WCT_GUIDED_MAX_RADIUS\s+(\d+)', rule).group(1)) == _lib.GUIDED_MAX_RADIUS
    assert int(re.search(r'WCT_GUIDED_MAX_EPS\s+(\d+)', rule).group(1)) == _lib.GUIDED_MAX_EPS
    assert int(re.search(r'WCT_GUIDED_SHIFT\s+(\d+)', rule).group(1)) == oracle.SHIFT


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
def _extremes():
    """inputs that approach the bounds the header states: all-0 / all-255 checkerboards and stripes with full 129 x 129 windows
    (the largest window sums, covariance and variance), and a guide of two neighbouring greys under a 0 / 255 frame (the largest
    a_q: sigma_p / (2 sqrt(eps_q)) = 63.75 at eps_q = 1)"""
    n = 129
    yy, xx = np.mgrid[:n, :n]
    board, stripes = ((yy + xx) & 1) * 255, (xx & 1) * 255
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    cases = []
    for pattern in (board, stripes):
        for eps_q in (1, 65025):
            cases.append((rgb(pattern), rgb(pattern), 64, eps_q))
    cases.append((rgb(stripes), rgb(100 + (xx & 1) * 2), 64, 1))                   # a_q towards +63.75 * 2^12
    cases.append((rgb(255 - stripes), rgb(100 + (xx & 1) * 2), 64, 1))             # ... and towards -63.75 * 2^12
    return cases


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_rule_check.cpp includes csrc/guided_rule.h -- the functions the kernels call --, forms the window sums
    naively and compares the bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into this process.  The
    signed-overflow check of UBSan on the extremes is the proof of the header's bounds."""
    cases = []
    for seed, (h, w, hc, wc, r, eps_q) in enumerate([(9, 13, 9, 13, 16, 650), (33, 35, 33, 35, 1, 1), (33, 35, 33, 35, 4, 65025),
                                                     (16, 20, 9, 13, 3, 650), (48, 48, 37, 41, 5, 7), (40, 36, 40, 36, 64, 1)]):
        cases.append((_rand(50 + seed, (h, w, 3)), _rand(70 + seed, (hc, wc, 3)), r, eps_q))
    s, c = oracle.clamp_case()
    cases.append((s, c, 1, 1))
    cases += _extremes()
    blob = struct.pack('<i', len(cases))
    for s, c, r, eps_q in cases:
        blob += struct.pack('<6i', s.shape[0], s.shape[1], c.shape[0], c.shape[1], r, eps_q)
        blob += s.tobytes() + c.tobytes() + oracle.guided_filter(s, c, r, eps_q).tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    # the adversarial guide reached the neighbourhood of the a_q bound, and stayed under it
    max_a = int(out.stdout.split('max |a_q| ')[1].split(',')[0])
    assert 200000 < max_a < 2 ** 18, out.stdout
