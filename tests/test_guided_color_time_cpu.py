"""Temporal guided smoothing with the colour guide without a GPU: the NumPy oracle of the rule (the 3 x 3 solve of
guided_color_oracle over the 3-D shifted window of guided_motion_oracle) against a naive loop over windows, against the 2-D colour
rule at T = 0 and on one frame, under equal positions, in chunks, on a constant clip, against the float64 filter within the
header's distance; the effect the feature was built for; the Python and parser refusals; and the shared rule header
(wct_tf_amd/csrc/guided_color_time_rule.h, what the kernels compile) built for the host under AddressSanitizer + UBSan as a
program of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_color_oracle as gc
import guided_motion_oracle as gm
import guided_time_oracle as gt
import guided_color_time_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def _walk(seed, frames, step=16):
    rng = np.random.default_rng(seed)
    return (gm.positions_of(rng.integers(-step, step + 1, (frames - 1, 2))) + rng.integers(-1000, 1000, (1, 2))).astype(np.int32)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r,t,steps', [(1, 1, [(1, -2)] * 2), (2, 2, [(2, 1), (-3, 0)]), (1, 2, None), (2, 1, [(16, -16)] * 2)], ids=str)
def test_vectorised_oracle_is_the_scalar_loop(r, t, steps):
    s, c = _rand(5, (3, 7, 8, 3)), _rand(6, (3, 6, 8, 3))
    pos = None if steps is None else gm.positions_of(steps)
    got = oracle.guided_filter(s, c, r, 650, t, pos)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.guided_filter_loop(s, c, r, 650, t, pos))
    if steps and steps[0] == (16, -16):                  # every neighbour's window is empty: the 2-D bytes
        assert np.array_equal(got, gc.guided_filter(s, c, r, 650))


def test_no_frames_on_each_side_and_a_one_frame_clip_are_the_2d_colour_rule():
    s, c = _rand(1, (4, 19, 23, 3)), _rand(2, (4, 15, 23, 3))
    want = gc.guided_filter(s, c, 3, 650)
    assert np.array_equal(oracle.guided_filter(s, c, 3, 650, 0), want)
    assert np.array_equal(oracle.guided_filter(s, c, 3, 650, 0, _walk(1, 4)), want)
    for t in (1, 3):
        assert np.array_equal(oracle.guided_filter(s[:1], c[:1], 3, 650, t, np.array([[5, -7]], np.int32)), want[:1])


@pytest.mark.parametrize('t', [1, 3])
def test_equal_positions_are_no_positions(t):
    s, c = _rand(3, (5, 13, 17, 3)), _rand(4, (5, 13, 15, 3))
    want = oracle.guided_filter(s, c, 2, 650, t)
    assert not np.array_equal(want, gc.guided_filter(s, c, 2, 650))
    for p in ((0, 0), (7, -3), (-4000, 123456)):
        assert np.array_equal(oracle.guided_filter(s, c, 2, 650, t, np.tile(np.array(p, np.int32), (5, 1))), want), p
    pos = _walk(2, 5, step=3)
    assert np.array_equal(oracle.guided_filter(s, c, 2, 650, t, pos), oracle.guided_filter(s, c, 2, 650, t, pos + np.int32(12345)))


def test_a_chunked_clip_needs_a_halo_of_exactly_two_t_frames():
    s, c, pos = _rand(15, (12, 10, 12, 3)), _rand(16, (12, 10, 12, 3)), _walk(3, 12, step=3)
    for p in (None, pos):
        whole = oracle.guided_filter(s, c, 2, 650, 2, p)
        assert np.array_equal(oracle.guided_filter_chunked(s, c, 2, 650, 2, p, chunk=5, halo=4), whole)
        assert not np.array_equal(oracle.guided_filter_chunked(s, c, 2, 650, 2, p, chunk=5, halo=2), whole)


def test_a_constant_clip_is_exact():
    c = _rand(20, (5, 20, 24, 3))
    for v in (0, 200, 255):
        s = np.full((5, 20, 24, 3), v, np.uint8)
        for eps_q in (1, 650, 65025):
            assert np.array_equal(oracle.guided_filter(s, c, 3, eps_q, 2, _walk(5, 5, step=4)), s), (v, eps_q)


def test_n_stays_within_the_limit_at_each_radius_limit():
    from wct_tf_amd import _lib
    assert _lib.GUIDED_TIME_MAX_RADIUS == (64, 51, 40, 33)
    for t, r in enumerate(_lib.GUIDED_TIME_MAX_RADIUS):
        assert (2 * r + 1) ** 2 * (2 * t + 1) <= gt.MAX_WINDOW == 33025
        assert t == 0 or 33025 < (2 * r + 3) ** 2 * (2 * t + 1)              # (at T = 0 the radius stops at 64, not at the window)
        f, side = 2 * t + 1, 2 * r + 2 * t + 2
        n = gm.count3(f, side, side, r, t, gm.positions_of([(1, -1)] * (f - 1)))
        assert n.min() >= 1 and n.max() == (2 * r + 1) ** 2 * (2 * t + 1)
        assert n.max() * 65025 < 2 ** 31


@pytest.mark.parametrize('eps_q', [650, 65025])
@pytest.mark.parametrize('motion', [False, True])
def test_distance_from_the_float64_filter_is_within_the_headers_bound(eps_q, motion):
    """the bound is distance(eps_q) of guided_color_rule.h (0.79 at 650, 0.594 at 65025): no n in it, so it holds along time"""
    s, c = _rand(30, (5, 24, 28, 3)), _rand(31, (5, 24, 28, 3))
    pos = _walk(7, 5, step=5) if motion else None
    d = np.abs(oracle.guided_filter_unclamped(s, c, 3, eps_q, 2, pos) - oracle.guided_filter_f64(s, c, 3, eps_q, 2, pos)).max()
    print('eps_q', eps_q, 'motion', motion, 'distance', d, 'bound', gc.distance(eps_q))
    assert d <= gc.distance(eps_q)


# ---- what the feature is for -----------------------------------------------------------------------------------------------
def test_the_colour_guide_along_time_keeps_the_edge_and_removes_the_flicker():
    """isoluminant_clip(0): a static content (200, 60, 60) | (20, 141, 100) (greys 102 | 100), 12 frames of 48 x 64 of a 50 | 200 step
    plus N(0, 20) noise per frame, r = 4, eps_q = 650.  Flicker = mean |out_f - out_{f+1}| on the flat left side, jump = the mean
    step across the edge (flicker_flat, edge_jump of the oracle).  Measured with this oracle:
        colour  T = 0 .. 3: flicker 1.723, 0.359, 0.157, 0.110; mean jump 137.65, 137.65, 137.53, 137.49 (smallest 129, 135, 135, 136);
                            error against the clean step 1.488, 0.912, 0.788, 0.738
        grey    T = 0 .. 3: flicker 1.723, 0.359, 0.157, 0.110; mean jump 16.89, 16.78, 16.80, 16.71; error 7.72, 7.26, 7.14, 7.10
    The thresholds sit halfway between the values they separate: jumps 137 | 17 -> 77, flicker at T = 0 | T = 1, 1.72 | 0.36 -> 1.04."""
    s, c, clean = oracle.isoluminant_clip(0)
    w = s.shape[2]
    zero = np.zeros((len(s), 2), np.int32)
    fl, jc, jg = [], [], []
    for t in range(4):
        col, grey = oracle.guided_filter(s, c, 4, 650, t), gm.guided_filter_motion(s, c, 4, 650, t, zero)
        fl.append(oracle.flicker_flat(col, w))
        jc.append(oracle.edge_jump(col, w)[0])
        jg.append(oracle.edge_jump(grey, w)[0])
        print('T', t, 'flicker', fl[-1], 'jump colour', jc[-1], 'grey', jg[-1], 'error', oracle.error_against(col, clean),
              oracle.error_against(grey, clean))
    assert fl[0] > fl[1] > fl[2] > fl[3]
    assert fl[0] > 1.04 > fl[1]
    for t in range(4):
        assert jc[t] > 77 > jg[t], t


# ---- command line ----------------------------------------------------------------------------------------------------------
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1', '--style-path', 's']


def _check_video(argv):
    from wct_tf_amd import stylize, stylize_video
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_mask_args(parser, args)
    stylize_video.check_warm_args(parser, args)
    stylize_video.check_color_args(parser, args)
    stylize_video.check_guided_args(parser, args)
    stylize_video.check_resize_args(parser, args)
    stylize_video.check_alpha_map_args(parser, args)
    stylize.check_upsample_args(parser, args, extra=[('--guided-frames', args.guided_frames > 0), ('--warm-start', args.warm_start)])
    stylize_video.check_upsample_time_args(parser, args)
    return args


def test_the_flag_is_off_by_default_and_goes_with_guided_frames_and_motion():
    from wct_tf_amd import stylize, stylize_video
    ok = ['--guided-radius', '4', '--guided-frames', '2']
    assert _check_video(_VID + ok).guided_frames_guide is None
    assert _check_video(_VID + ok + ['--guided-frames-guide', 'grey']).guided_frames_guide == 'grey'
    a = _check_video(_VID + ok + ['--guided-frames-guide', 'color', '--guided-motion', 'global', '--content-colors', '--warm-start'])
    assert a.guided_frames_guide == 'color' and a.guided_motion == 'global' and a.guided_guide is None
    assert '--guided-frames-guide' in stylize_video.build_parser().format_help()
    assert '--guided-frames-guide' not in stylize.build_parser().format_help()


def test_parser_refusals_name_the_option(capsys):
    r4 = ['--guided-radius', '4']
    up = ['--content-size', '64', '--guided-upsample']
    for extra, words in ((r4 + ['--guided-frames-guide', 'color'], ('--guided-frames-guide', '--guided-frames >= 1')),
                         (['--guided-frames-guide', 'grey'], ('--guided-frames-guide', '--guided-frames >= 1')),
                         (r4 + ['--guided-frames', '0', '--guided-frames-guide', 'color'], ('--guided-frames-guide', '--guided-frames >= 1')),
                         (r4 + ['--guided-frames', '1', '--guided-frames-guide', 'colour'], ('--guided-frames-guide', 'invalid choice')),
                         (r4 + up + ['--guided-frames-guide', 'color'], ('--guided-frames-guide', '--guided-upsample')),
                         (r4 + up + ['--guided-frames', '1', '--guided-frames-guide', 'color'], ('--guided-frames-guide', '--guided-upsample')),
                         # the earlier refusal stays, and now points to the new flag
                         (r4 + ['--guided-frames', '1', '--guided-guide', 'color'], ('--guided-frames', '--guided-guide', '--guided-frames-guide color')),
                         (r4 + ['--guided-frames', '1', '--guided-guide', 'color', '--guided-frames-guide', 'color'], ('--guided-frames', '--guided-guide')),
                         (r4 + ['--guided-frames', '1', '--guided-frames-guide', 'color', '--swap5'], ('--swap5',))):
        with pytest.raises(SystemExit):
            _check_video(_VID + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (extra, err)


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context
    from wct_tf_amd.wct import WCT
    import wct_tf_amd
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (3, 16, 20, 3)), _rand(31, (3, 9, 20, 3))
    zero = np.zeros((3, 2), np.int32)
    calls = (lambda g, p=None: ctx.guided_filter_time(s, c, 4, 650, 1, positions=p, guide=g),
             lambda g, p=None: ctx.guided_filter_time_clip(s, c, 4, 650, 1, positions=p, guide=g),
             lambda g, p=None: ctx.guided_filter_time_range(s, c, 4, 650, 1, 0, 1, positions=p, guide=g),
             lambda g, p=None: ctx.guided_filter_time_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, 0, 3, None, guide=g),
             lambda g, p=None: ctx.guided_filter_motion_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, zero if p is None else p, 0, 3, None, guide=g),
             lambda g, p=None: wct_tf_amd.guided_filter_time_np(s, c, 4, 650, 1, ctx=ctx, positions=p, guide=g))
    for call in calls:
        for bad in ('colour', 'rgb', None, 1, ('color',)):
            with pytest.raises(ValueError, match="guided guide is 'grey' or 'color'"):
                call(bad)
    # the filter's own refusals stay in front of, or behind, the guide's -- all before any library call
    for call in (calls[0], calls[1], calls[2], calls[4], calls[5]):
        with pytest.raises(ValueError, match='step from frame 0 to 1'):
            call('color', [[0, 0], [17, 0], [17, 0]])
    with pytest.raises(ValueError, match='1 .. 51'):
        ctx.guided_filter_time(s, c, 52, 650, 1, guide='color')
    with pytest.raises(ValueError, match='f0 < f1'):
        ctx.guided_filter_time_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, 2, 2, None, guide='color')
    with pytest.raises(ValueError, match='1 .. 32 frames in one call'):
        ctx.guided_filter_time(np.zeros((33, 4, 4, 3), np.uint8), np.zeros((33, 4, 4, 3), np.uint8), 1, 650, 1, guide='color')
    # the model's keyword: checked before anything else of the call
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    big = _rand(32, (3, 32, 40, 3))
    with pytest.raises(ValueError, match='guided_frames_guide needs'):
        m.predict_frames(big, s[0], guided_frames_guide='color')
    with pytest.raises(ValueError, match='guided_frames_guide needs guided_frames >= 1'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames_guide='color')
    with pytest.raises(ValueError, match='guided_frames_guide needs guided_frames >= 1'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=0, guided_frames_guide='grey')
    with pytest.raises(ValueError, match="guided guide is 'grey' or 'color'"):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_frames_guide='colour')
    with pytest.raises(ValueError, match="'color' guide.*guided_frames_guide='color'"):     # the earlier refusal stays and points on
        m.predict_frames(big, s[0], guided=(4, 650, 'color'), guided_frames=1)
    with pytest.raises(ValueError, match="'color' guide"):
        m.predict_frames(big, s[0], guided=(4, 650, 'color'), guided_frames=1, guided_frames_guide='color')
    with pytest.raises(ValueError, match='guided_frames is not served with swap5'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_frames_guide='color', swap5=True)
    with pytest.raises(ValueError, match='step from frame 0 to 1'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_frames_guide='color', guided_motion=[[0, 0], [0, 17], [0, 0]])
    with pytest.raises(ValueError, match='guided_frames_guide is not served with guided_upsample'):
        m.predict_frames(big, s[0], guided_upsample=(16, 2, 650), guided_frames_guide='color')


def test_the_unit_the_symbols_and_the_limits_are_where_the_issue_puts_them():
    from wct_tf_amd import _lib
    assert 'guided_color_time.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    names = [s[0] for s in _lib.SIGNATURES]
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    for name in ('wct_guided_filter_time_guide', 'wct_guided_filter_time_guide_batch_dev'):
        assert name in names and name + '(' in hdr
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_color_time_rule.h')).read()
    assert '#include "guided_color_rule.h"' in rule and '#include "guided_motion_rule.h"' in rule and '33025' in rule
    common = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'common.h')).read()
    assert 'launch_guided_color_time(' in common and 'launch_guided_color_time_ab(' in common and 'guided_color_time_check(' in common
    limits = tuple(max(r for r in range(1, 65) if (2 * r + 1) ** 2 * (2 * t + 1) <= gt.MAX_WINDOW) for t in range(4))
    assert limits == _lib.GUIDED_TIME_MAX_RADIUS == (64, 51, 40, 33)
    for word in ('guided_time_rule.h', 'guided_motion_rule.h'):
        text = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', word)).read()
        assert 'guided_color_time_rule.h' in text


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_color_time_rule_check.cpp includes csrc/guided_color_time_rule.h -- the functions the kernels call --,
    forms the pass-1 window sums over the frames in int32, filters the clips of a file and writes the bytes, which must be the
    oracle's; then it forms the extremes itself (full windows of 31827, 32805 and 31423 pixels of all-255 and of a checkerboard
    that alternates in time, at eps_q = 1 and 65025) and holds |a_q| and |b_q| against the header's bounds.  A stand-alone
    program: nothing sanitized is loaded into this process."""
    cases = []
    for seed, (f, h, w, hc, wc, r, eps_q, t, step) in enumerate([(4, 9, 13, 9, 13, 16, 650, 3, 16), (5, 23, 25, 23, 25, 1, 1, 1, 2),
                                                                 (5, 23, 25, 23, 25, 4, 65025, 2, 7), (4, 16, 20, 9, 13, 3, 650, 1, 16),
                                                                 (2, 20, 24, 20, 24, 5, 7, 3, 5), (3, 20, 24, 20, 24, 2, 650, 0, 16),
                                                                 (4, 14, 18, 12, 18, 2, 65, 2, 0)]):
        cases.append((_rand(50 + seed, (f, h, w, 3)), _rand(70 + seed, (f, hc, wc, 3)), r, eps_q, t, _walk(seed, f, step)))
    s, c, _ = oracle.isoluminant_clip(1, frames=4, h=16, w=20)
    cases.append((s, c, 3, 1, 1, np.zeros((4, 2), np.int32)))
    blob, want = struct.pack('<i', len(cases)), b''
    for s, c, r, eps_q, t, pos in cases:
        blob += struct.pack('<8i', s.shape[0], s.shape[1], s.shape[2], c.shape[1], c.shape[2], r, eps_q, t)
        blob += np.ascontiguousarray(pos, '<i4').tobytes() + s.tobytes() + c.tobytes()
        want += oracle.guided_filter(s, c, r, eps_q, t, pos).tobytes()
    data, res = tmp_path / 'cases.bin', tmp_path / 'out.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_color_time_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_color_time_rule_check.cpp')])
    out = subprocess.run([exe, str(data), str(res)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    got = res.read_bytes()
    assert len(got) == len(want)
    assert got == want, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:10]
    field = lambda name: int(out.stdout.split(name + ' ')[1].split(',')[0].split()[0])
    assert field('full n') == 5 * 81 ** 2 == 32805, out.stdout               # the largest of 31827, 32805, 31423
    assert field('max sum') == 32805 * 65025 < 2 ** 31, out.stdout
    assert field('min n') >= 1 and field('max |a_q|') <= gc.MAX_A and field('max |b_q|') <= gc.MAX_B, out.stdout
