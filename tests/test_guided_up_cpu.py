"""Guided upsampling without a GPU: the oracle against its own naive loop and against the float64 fast guided filter, the rule's
properties, the refusals of the Python layer and of both command lines, and the shared rule header on the host under sanitizers
(tests/emul/guided_up_rule_check.cpp, a stand-alone program)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_oracle
import guided_up_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'

CASES = oracle.CASES


def _rand(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _noise_case(seed, h, w, hc, wc, H, W):
    return _rand(seed, (h, w, 3)), _rand(seed + 100, (hc, wc, 3)), _rand(seed + 200, (H, W, 3))


@pytest.mark.parametrize('case', [(5, 6, 5, 6, 5, 6, 1, 650), (6, 7, 4, 5, 11, 13, 2, 1), (7, 5, 7, 5, 23, 9, 1, 65025)], ids=str)
def test_vectorised_oracle_is_the_scalar_loop(case):
    h, w, hc, wc, H, W, r, eps_q = case
    for s, c, C in (_noise_case(1, h, w, hc, wc, H, W), oracle.case(2, h, w, hc, wc, H, W)):
        assert np.array_equal(oracle.guided_upsample(s, c, C, r, eps_q), oracle.guided_upsample_loop(s, c, C, r, eps_q))


@pytest.mark.parametrize('case', CASES, ids=str)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(case):
    """per pixel and channel, before the clamp: 0.5 + 256 2^-12 + D 2^-8 (guided_up_rule.h), on noise and on a smooth content"""
    h, w, hc, wc, H, W, r, eps_q = case
    for s, c, C in (_noise_case(10, h, w, hc, wc, H, W), oracle.case(11, h, w, hc, wc, H, W)):
        got = oracle.guided_upsample_unclamped(s, c, C, r, eps_q).astype(np.float64)
        want = oracle.guided_upsample_f64(s, c, C, r, eps_q)
        dist, lim = np.abs(got - want), oracle.bound(s, c, C, r, eps_q)
        print('case %s: worst distance %.4f, its bound %.4f, largest bound %.3f' % (case, dist.max(), lim.flat[dist.argmax()], lim.max()))
        assert (dist <= lim + 1e-6).all(), (dist - lim).max()


@pytest.mark.parametrize('value', [0, 77, 255])
def test_a_constant_frame_comes_back_exactly(value):
    _, c, C = _noise_case(20, 20, 24, 20, 24, 77, 101)
    s = np.full((20, 24, 3), value, np.uint8)
    for r, eps_q in ((1, 1), (4, 650), (16, 65025)):
        assert (oracle.guided_upsample(s, c, C, r, eps_q) == value).all()


@pytest.mark.parametrize('case', [(9, 13, 9, 13, 2, 650), (33, 35, 33, 35, 1, 1), (16, 20, 9, 13, 3, 650), (48, 48, 48, 48, 8, 65025)], ids=str)
def test_equal_sizes_stay_within_one_level_of_the_guided_filter(case):
    """H = hc, W = wc: every fraction is 0, and the result is the guided filter with the window means rounded once more"""
    h, w, hc, wc, r, eps_q = case
    s, c = _rand(30, (h, w, 3)), _rand(31, (hc, wc, 3))
    y0, y1, fy = oracle.axis(hc, hc)
    assert (fy == 0).all() and (y0 == np.arange(hc)).all()
    got = oracle.guided_upsample(s, c, c, r, eps_q).astype(int)
    want = guided_oracle.guided_filter(s, c, r, eps_q)[:hc, :wc].astype(int)
    diff = np.abs(got - want)
    print('equal sizes %s: %.3f %% of the bytes differ' % (case, 100.0 * (diff != 0).mean()))
    assert diff.max() <= 1


def test_a_step_edge_comes_back_at_full_sharpness():
    """a 50 | 200 content step at column 83 of 96 x 160, off the small grid, at ratio 8; +-20 noise on the small frame; r 2, eps_q 65.
    The upsampled frame crosses the step between columns 82 and 83; a bilinear upscale of the filtered small frame smears it."""
    H, W, ratio, r, eps_q = 96, 160, 8, 2, 65
    C = np.full((H, W, 3), 50, np.uint8)
    C[:, 83:] = 200
    c = np.round(C.reshape(H // ratio, ratio, W // ratio, ratio, 3).mean((1, 3))).astype(np.uint8)
    noise = np.random.default_rng(40).integers(-20, 21, c.shape)
    s = np.clip(c.astype(int) + noise, 0, 255).astype(np.uint8)
    up = oracle.guided_upsample(s, c, C, r, eps_q).astype(np.float64)
    left, right = up[:, 82].mean(), up[:, 83].mean()
    small = guided_oracle.guided_filter(s, c, r, eps_q)
    smear = np.abs(np.diff(oracle.bilinear_f64(small, H, W).mean((0, 2)))).max()
    print('step edge: %.1f -> %.1f across columns 82 | 83; the bilinear upscale moves at most %.1f per column' % (left, right, smear))
    assert right - left > 120
    assert (up[:, 83] - up[:, 82]).min() > 120
    assert smear < 40


def test_axis_weights_sum_and_taps_stay_inside_the_content():
    for N, m in [(9, 9), (40, 9), (61, 13), (264, 33), (67, 33), (250, 31), (100, 48), (7, 1), (1000, 999), (4000, 512)]:
        p0, p1, f = oracle.axis(N, m)
        assert (f >= 0).all() and (f <= 256).all() and ((256 - f) + f == 256).all()
        assert (p0 >= 0).all() and (p1 <= m - 1).all() and (p0 <= p1).all() and (p1 - p0 <= 1).all()
        assert (np.diff(p0) >= 0).all() and (np.diff(p0) <= 1).all()          # the ratio is at least 1: a step of at most one
        src = np.clip((np.arange(N) + 0.5) * m / N - 0.5, 0, m - 1)          # the weights against the exact map, within 2^-9
        assert np.abs((p0 + f / 256.0) - src).max() <= 2.0 ** -9 + 1e-12
    wy, wx = np.array([256 - 37, 37]), np.array([256 - 255, 255])
    assert (wy[:, None] * wx[None, :]).sum() == 65536


# ---- the command lines ---------------------------------------------------------------------------------------------------------
def _stylize_args(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_interp_args(parser, args)
    stylize.check_mask_args(parser, args)
    stylize.check_color_args(parser, args)
    stylize.check_guided_args(parser, args)
    stylize.check_band_args(parser, args)
    stylize.check_alpha_map_args(parser, args)
    stylize.check_upsample_args(parser, args)
    return args


def _video_args(argv):
    from wct_tf_amd import stylize_video, stylize
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_mask_args(parser, args)
    stylize_video.check_warm_args(parser, args)
    stylize_video.check_color_args(parser, args)
    stylize_video.check_guided_args(parser, args)
    stylize_video.check_resize_args(parser, args)
    stylize_video.check_alpha_map_args(parser, args)
    stylize.check_upsample_args(parser, args, extra=[('--guided-frames', args.guided_frames > 0), ('--warm-start', args.warm_start)])
    return args


BASE = ['--relu-targets', 'relu2_1', 'relu1_1', '--synthetic-weights', '1', '--content-path', 'c', '--style-path', 's', '--out-path', 'o']
VBASE = ['--relu-targets', 'relu2_1', 'relu1_1', '--synthetic-weights', '1', '--in-path', 'i', '--style-path', 's', '--out-path', 'o']
UP = ['--guided-upsample', '--guided-radius', '4', '--content-size', '64']


def test_both_command_lines_take_the_option_and_have_it_off_by_default():
    from wct_tf_amd import stylize
    for parse, base in ((_stylize_args, BASE), (_video_args, VBASE)):
        assert parse(base).guided_upsample is False and stylize.upsample_of(parse(base)) is None
        args = parse(base + UP + ['--guided-eps', '0.001', '--content-colors'])
        assert stylize.upsample_of(args) == (64, 4, 65)


def test_parser_errors_name_the_option(capsys):
    def refused(parse, argv, word):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, (argv, word)

    for parse, base in ((_stylize_args, BASE), (_video_args, VBASE)):
        refused(parse, base + ['--guided-upsample', '--content-size', '64'], '--guided-radius > 0')
        refused(parse, base + ['--guided-upsample', '--guided-radius', '4'], '--content-size > 0')
        for extra, word in ((['--guided-guide', 'color'], '--guided-guide color'), (['--swap5'], '--swap5'),
                            (['--keep-colors'], '--keep-colors'), (['--passes', '2'], '--passes > 1')):
            refused(parse, base + UP + extra, 'does not combine with ' + word)
    no_style = [a for a in BASE if a not in ('--style-path', 's')]
    refused(_stylize_args, no_style + UP + ['--interp-styles', 'a', 'b'], '--interp-styles')
    refused(_stylize_args, no_style + UP + ['--mask-path', 'm', '--mask-styles', 'a', 'b'], '--mask-path')
    refused(_stylize_args, BASE + UP + ['--alpha-map', 'm'], '--alpha-map')
    refused(_stylize_args, BASE + UP + ['--band-rows', '16'], 'guided')          # (the filter is refused in bands already)
    vno_style = [a for a in VBASE if a not in ('--style-path', 's')]
    refused(_video_args, vno_style + UP + ['--mask-path', 'm', '--mask-styles', 'a', 'b'], '--mask-path')
    refused(_video_args, VBASE + UP + ['--alpha-map', 'm'], '--alpha-map')
    refused(_video_args, VBASE + UP + ['--guided-frames', '1'], '--guided-frames')


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_guided_upsample, upsample_work_size
    from wct_tf_amd.wct import WCT
    from wct_tf_amd.utils import resize_shape
    import wct_tf_amd
    assert wct_tf_amd.ops.guided_upsample_np is not None
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c, C = _rand(50, (16, 20, 3)), _rand(51, (9, 13, 3)), _rand(52, (40, 61, 3))
    with pytest.raises(ValueError, match='stylized 9x13 is smaller than content_small'):
        ctx.guided_upsample(c, s, C, 4, 650)
    with pytest.raises(ValueError, match='does not scale down'):
        ctx.guided_upsample(s, c, C[:8], 4, 650)
    with pytest.raises(ValueError, match='does not scale down'):
        ctx.guided_upsample(s, c, C[:, :12], 4, 650)
    with pytest.raises(ValueError, match='takes uint8 images, content_full'):
        ctx.guided_upsample(s, c, C.astype(np.float32), 4, 650)
    with pytest.raises(ValueError, match='HxWx3'):
        ctx.guided_upsample(s[..., :2], c, C, 4, 650)
    for r, e, word in ((0, 650, 'radius'), (65, 650, 'radius'), (4, 0, 'eps_q'), (4, 65026, 'eps_q'), (4.5, 650, 'integers')):
        with pytest.raises(ValueError, match=word):
            ctx.guided_upsample(s, c, C, r, e)
        with pytest.raises(ValueError, match=word):
            ctx.guided_upsample_batch(s[None], c[None], C[None], r, e)
        with pytest.raises(ValueError, match=word):
            ctx.guided_upsample_batch_dev(None, 16, 20, None, 9, 13, None, 40, 61, 1, r, e, None)
    with pytest.raises(ValueError, match=r'\[B\]\[H\]\[W\]\[3\]'):
        ctx.guided_upsample_batch(s, c, C, 4, 650)
    with pytest.raises(ValueError, match='as many contents'):
        ctx.guided_upsample_batch(np.stack([s, s]), c[None], C[None], 4, 650)
    # the working size
    assert upsample_work_size(3000, 4000, 512) == tuple(resize_shape(3000, 4000, 512)) == (512, 683)
    assert upsample_work_size(96, 130, 40) == (40, 54) and upsample_work_size(40, 130, 40) == (40, 130) and upsample_work_size(30, 20, 40) == (30, 20)
    assert check_guided_upsample((40, 2, 65)) == (40, 2, 65)
    for g, word in (((40, 2), 'three integers'), (40, 'three integers'), ((0, 2, 65), 'short side'), ((40, 0, 65), 'radius'),
                    ((40, 2, 0), 'eps_q'), ((40.5, 2, 65), 'three integers')):
        with pytest.raises(ValueError, match=word):
            check_guided_upsample(g)
    # the model's keyword: checked before anything else of the call
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    for call in (lambda **kw: m.predict(C, s, **kw), lambda **kw: m.predict_frames(C[None], s, **kw)):
        with pytest.raises(ValueError, match='radius'):
            call(guided_upsample=(40, 0, 65))
        with pytest.raises(ValueError, match='three integers'):
            call(guided_upsample=(40, 2))
        with pytest.raises(ValueError, match='swap5 is not served with guided_upsample'):
            call(guided_upsample=(40, 2, 65), swap5=True)
        with pytest.raises(ValueError, match='guided is not served with guided_upsample'):
            call(guided_upsample=(40, 2, 65), guided=(2, 65))
    with pytest.raises(ValueError, match='uint8 contents'):
        m.predict(C.astype(np.float32), s, guided_upsample=(40, 2, 65))
    with pytest.raises(ValueError, match='strength is not served'):
        m.predict(C, s, guided_upsample=(40, 2, 65), strength=np.zeros((40, 61), np.uint8))
    with pytest.raises(ValueError, match='resize is not served'):
        m.predict_frames(C[None], s, guided_upsample=(40, 2, 65), resize=(20, 30))


def test_symbols_and_sources_are_in_place():
    from wct_tf_amd import _lib
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {'wct_guided_upsample', 'wct_guided_upsample_batch_dev', 'wct_stylize_prepared_upsampled',
            'wct_stylize_prepared_upsampled_batch_dev'} <= bound
    assert 'guided_up.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_up_rule.h')).read()
    import re
    assert int(re.search(r'WCT_GUIDED_UP_WBITS\s+(\d+)', rule).group(1)) == oracle.WBITS


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_up_rule_check.cpp includes csrc/guided_up_rule.h -- the functions the kernels call -- and compares the
    bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into this process.  The last case is the extreme of
    guided_rule_check.cpp (a 0 / 255 frame under a guide of two neighbouring greys, full 129 x 129 windows: |a_q| = 261120) at
    H = 8 hc; the signed-overflow check of UBSan there, and the program's own comparison with the stated bounds, are their proof."""
    cases = []
    for seed, (h, w, hc, wc, H, W, r, eps_q) in enumerate(CASES[:4] + [CASES[5]]):
        cases.append(_noise_case(60 + seed, h, w, hc, wc, H, W) + (r, eps_q))
    cases.append(oracle.case(70, 20, 24, 17, 21, 77, 101) + (3, 65))
    n = 129
    yy, xx = np.mgrid[:n, :n]
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    small = rgb(100 + (xx & 1) * 2)
    full = rgb((np.mgrid[:8 * n, :8 * n][1] & 1) * 255)                            # the full guide swings over 0 .. 255
    cases.append((rgb((xx & 1) * 255), small, full, 64, 1))
    blob = struct.pack('<i', len(cases))
    for s, c, C, r, eps_q in cases:
        blob += struct.pack('<8i', s.shape[0], s.shape[1], c.shape[0], c.shape[1], C.shape[0], C.shape[1], r, eps_q)
        blob += s.tobytes() + c.tobytes() + C.tobytes() + oracle.guided_upsample(s, c, C, r, eps_q).tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_up_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_up_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    assert int(out.stdout.split('max |a_q| ')[1].split(',')[0]) == 261120, out.stdout
    assert 200000 < int(out.stdout.split('max |am| ')[1].split(',')[0]) < 2 ** 18, out.stdout
