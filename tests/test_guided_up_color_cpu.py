"""Guided upsampling under the colour guide without a GPU: the oracle against its own naive loop and against the float64 fast guided
filter with the colour guide, the rule's properties, the reason for it (an isoluminant step at ratio 8), the refusals of the Python
layer and of both command lines, and the shared rule header on the host under sanitizers
(tests/emul/guided_up_color_rule_check.cpp, a stand-alone program)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_color_oracle
import guided_oracle
import guided_up_oracle
import guided_up_color_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'

CASES = guided_up_oracle.CASES


def _rand(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _noise_case(seed, h, w, hc, wc, H, W):
    return _rand(seed, (h, w, 3)), _rand(seed + 100, (hc, wc, 3)), _rand(seed + 200, (H, W, 3))


@pytest.mark.parametrize('case', [(5, 6, 5, 6, 5, 6, 1, 650), (6, 7, 4, 5, 11, 13, 2, 1), (7, 5, 7, 5, 23, 9, 1, 65025)], ids=str)
def test_vectorised_oracle_is_the_scalar_loop(case):
    h, w, hc, wc, H, W, r, eps_q = case
    for s, c, C in (_noise_case(1, h, w, hc, wc, H, W), guided_up_oracle.case(2, h, w, hc, wc, H, W)):
        assert np.array_equal(oracle.guided_upsample(s, c, C, r, eps_q), oracle.guided_upsample_loop(s, c, C, r, eps_q))


@pytest.mark.parametrize('case', CASES, ids=str)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(case):
    """per pixel and channel, before the clamp: 0.5 + 766 2^-12 + 765 2^-35 + D 2^-8 + E(eps_q) (guided_up_color_rule.h), on noise
    and on a smooth content.  E is the worst case of the colour rule's covariance quantisation and from eps_q of a few hundred
    downwards no useful bound, so the pixels above the other terms are counted and printed too (none but one pixel of
    the smooth case at eps_q = 1, r = 1)."""
    h, w, hc, wc, H, W, r, eps_q = case
    for name, (s, c, C) in (('noise', _noise_case(10, h, w, hc, wc, H, W)), ('smooth', guided_up_oracle.case(11, h, w, hc, wc, H, W))):
        got = oracle.guided_upsample_unclamped(s, c, C, r, eps_q).astype(np.float64)
        want = oracle.guided_upsample_f64(s, c, C, r, eps_q)
        dist, lim = np.abs(got - want), oracle.bound(s, c, C, r, eps_q)
        parts = oracle.bound_parts(s, c, C, r, eps_q)
        print('case %s, %s: worst distance %.4f, its bound %.4f (E = %.4g), %d pixels above the terms without E'
              % (case, name, dist.max(), lim.flat[dist.argmax()], oracle.eps_term(eps_q), (dist > parts + 1e-6).sum()))
        assert (dist <= lim + 1e-6).all(), (dist - lim).max()


def test_the_eps_term_is_the_parent_rules():
    """E(eps_q) is the last term of guided_color_oracle.distance, the bound guided_color_rule.h derives"""
    for eps_q in (1, 7, 65, 650, 65025):
        rest = 0.5 + 2.0 ** -13 + 765 * (2.0 ** -13 + 2.0 ** -35)
        assert abs(guided_color_oracle.distance(eps_q) - rest - oracle.eps_term(eps_q)) < 1e-9 * max(1.0, oracle.eps_term(eps_q))


@pytest.mark.parametrize('value', [0, 77, 255])
def test_a_constant_frame_comes_back_exactly(value):
    _, c, C = _noise_case(20, 20, 24, 20, 24, 77, 101)
    s = np.full((20, 24, 3), value, np.uint8)
    for r, eps_q in ((1, 1), (4, 650), (16, 65025)):
        assert (oracle.guided_upsample(s, c, C, r, eps_q) == value).all()


@pytest.mark.parametrize('case', [(9, 13, 9, 13, 2, 650), (33, 35, 33, 35, 1, 1), (16, 20, 9, 13, 3, 650), (48, 48, 48, 48, 8, 65025)], ids=str)
def test_equal_sizes_stay_within_one_level_of_the_colour_guided_filter(case):
    """H = hc, W = wc: every fraction is 0, and the result is the colour-guide filter with the window means rounded once more"""
    h, w, hc, wc, r, eps_q = case
    s, c = _rand(30, (h, w, 3)), _rand(31, (hc, wc, 3))
    got = oracle.guided_upsample(s, c, c, r, eps_q).astype(int)
    want = guided_color_oracle.guided_filter(s, c, r, eps_q)[:hc, :wc].astype(int)
    diff = np.abs(got - want)
    print('equal sizes %s: %.3f %% of the bytes differ' % (case, 100.0 * (diff != 0).mean()))
    assert diff.max() <= 1


def test_an_isoluminant_step_comes_back_at_full_sharpness():
    """content colours (200,60,60) | (20,141,100), greys 102 | 100, the step at column 83 of 96 x 160, off the small grid, at ratio 8;
    the small frame a 50 | 200 step under +-20 noise; r 2, eps_q 65.  The colour guide crosses the step between columns 82 and 83;
    the grey guide, which cannot see it, never moves more than a few levels per column."""
    s, c, C = oracle.isoluminant_step()
    assert C.shape == (96, 160, 3) and c.shape == (12, 20, 3)
    assert set(np.unique(guided_oracle.guide(C, 96, 160))) == {100, 102}
    up = oracle.guided_upsample(s, c, C, 2, 65).astype(np.float64)
    grey = guided_up_oracle.guided_upsample(s, c, C, 2, 65).astype(np.float64)
    jump = (up[:, 83] - up[:, 82]).min()
    move = np.abs(np.diff(grey, axis=1)).max()
    print('isoluminant step: %.1f -> %.1f across columns 82 | 83 (smallest jump %.0f); the grey guide: %.1f -> %.1f, at most %.1f per '
          'column' % (up[:, 82].mean(), up[:, 83].mean(), jump, grey[:, 82].mean(), grey[:, 83].mean(), move))
    assert jump > 120
    assert move < 40


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


def test_both_command_lines_take_the_option(capsys):
    from wct_tf_amd import stylize

    def refused(parse, argv, word):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, (argv, word)

    for parse, base in ((_stylize_args, BASE), (_video_args, VBASE)):
        assert parse(base).guided_upsample_guide is None and parse(base + UP).guided_upsample_guide is None      # off by default
        assert stylize.upsample_of(parse(base)) is None
        assert stylize.upsample_of(parse(base + UP + ['--guided-eps', '0.001'])) == (64, 4, 65)
        assert stylize.upsample_of(parse(base + UP + ['--guided-eps', '0.001', '--guided-upsample-guide', 'grey'])) == (64, 4, 65)
        assert stylize.upsample_of(parse(base + UP + ['--guided-eps', '0.001', '--guided-upsample-guide', 'color', '--content-colors'])) \
            == (64, 4, 65, 'color')
        refused(parse, base + ['--guided-upsample-guide', 'color'], '--guided-upsample-guide needs --guided-upsample')
        refused(parse, base + ['--guided-radius', '4', '--guided-upsample-guide', 'grey'], '--guided-upsample-guide needs --guided-upsample')
        refused(parse, base + UP + ['--guided-upsample-guide', 'colour'], 'invalid choice')
        refused(parse, base + UP + ['--guided-guide', 'color'], 'does not combine with --guided-guide color')
        refused(parse, base + UP + ['--guided-guide', 'color'], '--guided-upsample-guide color')
        refused(parse, base + UP + ['--guided-upsample-guide', 'color', '--guided-guide', 'color'], 'does not combine with --guided-guide color')
        for extra, word in ((['--swap5'], '--swap5'), (['--keep-colors'], '--keep-colors'), (['--passes', '2'], '--passes > 1')):
            refused(parse, base + UP + ['--guided-upsample-guide', 'color'] + extra, 'does not combine with ' + word)
    refused(_video_args, VBASE + UP + ['--guided-upsample-guide', 'color', '--guided-frames', '1'], '--guided-frames')
    refused(_stylize_args, BASE + UP + ['--guided-upsample-guide', 'color', '--alpha-map', 'm'], '--alpha-map')


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_guided_upsample
    from wct_tf_amd.wct import WCT
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c, C = _rand(50, (16, 20, 3)), _rand(51, (9, 13, 3)), _rand(52, (40, 61, 3))
    for guide in ('colour', 'COLOR', 1, None):
        with pytest.raises(ValueError, match="'grey' or 'color'"):
            ctx.guided_upsample(s, c, C, 4, 650, guide=guide)
        with pytest.raises(ValueError, match="'grey' or 'color'"):
            ctx.guided_upsample_batch(s[None], c[None], C[None], 4, 650, guide=guide)
        with pytest.raises(ValueError, match="'grey' or 'color'"):
            ctx.guided_upsample_batch_dev(None, 16, 20, None, 9, 13, None, 40, 61, 1, 4, 650, None, guide=guide)
    with pytest.raises(ValueError, match='does not scale down'):     # the refusals of the grey call come first, with their words
        ctx.guided_upsample(s, c, C[:8], 4, 650, guide='color')
    with pytest.raises(ValueError, match='radius'):
        ctx.guided_upsample(s, c, C, 0, 650, guide='color')
    assert check_guided_upsample((40, 2, 65)) == (40, 2, 65)
    assert check_guided_upsample((40, 2, 65, 'color')) == (40, 2, 65, 'color')
    assert check_guided_upsample([40, 2, 65, 'grey']) == (40, 2, 65, 'grey')
    for g, word in (((40, 2, 65, 1), "'grey' or 'color'"), ((40, 2, 65, None), "'grey' or 'color'"), ((40, 2, 65, 'colour'), "'grey' or 'color'"),
                    ((40, 2, 65, 'color', 1), 'three integers'), ((40, 2), 'three integers'), ((40, 0, 65, 'color'), 'radius'),
                    ((0, 2, 65, 'color'), 'short side'), ((40, 2, 0, 'color'), 'eps_q')):
        with pytest.raises(ValueError, match=word):
            check_guided_upsample(g)
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    for call in (lambda **kw: m.predict(C, s, **kw), lambda **kw: m.predict_frames(C[None], s, **kw)):
        with pytest.raises(ValueError, match="'grey' or 'color'"):
            call(guided_upsample=(40, 2, 65, 3))
        with pytest.raises(ValueError, match='swap5 is not served with guided_upsample'):
            call(guided_upsample=(40, 2, 65, 'color'), swap5=True)
        with pytest.raises(ValueError, match='guided is not served with guided_upsample'):
            call(guided_upsample=(40, 2, 65, 'color'), guided=(2, 65))


def test_symbols_and_sources_are_in_place():
    from wct_tf_amd import _lib
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {'wct_guided_upsample_guide', 'wct_guided_upsample_guide_batch_dev', 'wct_stylize_prepared_upsampled_guide',
            'wct_stylize_prepared_upsampled_guide_batch_dev'} <= bound
    assert 'guided_up_color.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    csrc = os.path.join(ROOT, 'wct_tf_amd', 'csrc')
    rule = open(os.path.join(csrc, 'guided_up_color_rule.h')).read()
    assert int(re.search(r'WCT_GUIDED_UP_COLOR_MAX_V\s+(\d+)LL', rule).group(1)) == oracle.MAX_V
    assert 65536 * (3 * oracle.MAX_A * 255 + oracle.MAX_B) < oracle.MAX_V < 2 ** 45
    parent = open(os.path.join(csrc, 'guided_color_rule.h')).read()
    assert int(re.search(r'WCT_GUIDED_COLOR_MAX_A\s+(\d+)', parent).group(1)) == oracle.MAX_A
    assert int(re.search(r'WCT_GUIDED_COLOR_MAX_B\s+(\d+)', parent).group(1)) == oracle.MAX_B
    assert int(re.search(r'WCT_GUIDED_UP_WBITS\s+(\d+)', open(os.path.join(csrc, 'guided_up_rule.h')).read()).group(1)) == oracle.WBITS
    assert '#include "guided_color_rule.h"' in rule and '#include "guided_up_rule.h"' in rule


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_up_color_rule_check.cpp includes csrc/guided_up_color_rule.h -- the functions the kernels call -- and compares
    the bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into this process.  The last case is the
    extreme of guided_color_rule_check.cpp (a 0 / 255 frame under a guide of two neighbouring greys, full 129 x 129 windows,
    eps_q = 1) at H = 8 hc with a full guide that swings 0 <-> 255 in every channel; the signed-overflow check of UBSan there, and
    the program's own comparison of its observed maxima with the stated bounds, are their proof."""
    cases = []
    for seed, (h, w, hc, wc, H, W, r, eps_q) in enumerate(CASES[:4] + [CASES[5]]):
        cases.append(_noise_case(60 + seed, h, w, hc, wc, H, W) + (r, eps_q))
    cases.append(guided_up_oracle.case(70, 20, 24, 17, 21, 77, 101) + (3, 65))
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
    exe = str(tmp_path / 'guided_up_color_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_up_color_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    print(out.stdout.strip())
    field = lambda name: int(out.stdout.split('max %s ' % name)[1].split(',')[0].split()[0])
    assert 0 < field('|am|') <= oracle.MAX_A and 0 < field('|bm|') <= oracle.MAX_B and 0 < field('|v|') < oracle.MAX_V
