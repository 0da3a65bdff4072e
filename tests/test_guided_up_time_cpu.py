"""Temporal guided upsampling without a GPU: the oracle against its own naive loop and against the float64 filter, the rule's
identities and properties, the flicker it was built against, the refusals of the Python layer and of the video command line, and
the shared rule header on the host under sanitizers (tests/emul/guided_up_time_rule_check.cpp, a stand-alone program)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_motion_oracle as gm
import guided_up_oracle as gu
import guided_up_time_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'
# the positions of the distance test: steps of (1, -2), (3, 0), (-16, 16), (0, 5) between the five frames
STEPS = [(1, -2), (3, 0), (-16, 16), (0, 5)]


@pytest.mark.parametrize('case', [(3, 5, 6, 5, 6, 5, 6, 1, 650, 1), (3, 6, 7, 4, 5, 11, 13, 2, 1, 1), (4, 5, 5, 5, 5, 9, 7, 1, 65025, 2)], ids=str)
def test_vectorised_oracle_is_the_scalar_loop(case):
    """without positions, under small steps, and under steps of 16 on 5 .. 7 pixel frames, which leave the windows of the
    neighbouring frames empty"""
    F, h, w, hc, wc, H, W, r, eps_q, t = case
    s, c, C = oracle.noise_clip(1, F, h, w, hc, wc, H, W)
    for pos in (None, gm.positions_of([(1, -2), (0, 3), (2, 1)][:F - 1]), gm.positions_of([(16, -16), (-16, 16), (16, 16)][:F - 1])):
        assert np.array_equal(oracle.guided_upsample_time(s, c, C, r, eps_q, t, pos), oracle.guided_upsample_time_loop(s, c, C, r, eps_q, t, pos))
    far = gm.positions_of([(16, -16)] * (F - 1))
    assert (gm.count3(F, h, w, r, t, far) == gm.count3(F, h, w, r, 0, far)).all()      # every neighbour's window is empty there


@pytest.mark.parametrize('case', gu.CASES, ids=str)
def test_no_frames_or_one_frame_is_guided_upsampling(case):
    h, w, hc, wc, H, W, r, eps_q = case
    s, c, C = oracle.clip_case(3, 3, h, w, hc, wc, H, W)
    want = gu.guided_upsample(s, c, C, r, eps_q)
    assert np.array_equal(oracle.guided_upsample_time(s, c, C, r, eps_q, 0), want)
    assert np.array_equal(oracle.guided_upsample_time(s, c, C, r, eps_q, 0, oracle.zigzag(3, (2, 6))), want)
    for t in (1, 2):
        assert np.array_equal(oracle.guided_upsample_time(s[1:2], c[1:2], C[1:2], r, eps_q, t), want[1:2])


def test_equal_positions_are_no_positions():
    s, c, C = oracle.clip_case(4, 5, 16, 20, 9, 13, 50, 70)
    want = oracle.guided_upsample_time(s, c, C, 3, 650, 2)
    assert not np.array_equal(want, gu.guided_upsample(s, c, C, 3, 650))
    for p in ((0, 0), (7, -300)):
        assert np.array_equal(oracle.guided_upsample_time(s, c, C, 3, 650, 2, np.tile(np.array(p, np.int32), (5, 1))), want)


def test_a_chunked_clip_needs_a_halo_of_two_t_small_frames():
    """chunks of 3 frames of a 11-frame clip: a halo of 2T small frames gives the whole clip's bytes, with and without positions; a
    halo of T does not -- on this noisy clip (T = 2, r = 2) the first chunk's last frame already differs, because its coefficients
    T frames ahead were formed without the frames T further"""
    s, c, C = oracle.noise_clip(5, 11, 12, 14, 10, 13, 23, 31)
    for pos in (None, oracle.zigzag(11, (2, 5))):
        whole = oracle.guided_upsample_time(s, c, C, 2, 650, 2, pos)
        assert np.array_equal(oracle.guided_upsample_time_chunked(s, c, C, 2, 650, 2, 3, 4, pos), whole)
        assert np.array_equal(oracle.guided_upsample_time_chunked(s, c, C, 2, 650, 2, 4, 5, pos), whole)
        short = oracle.guided_upsample_time_chunked(s, c, C, 2, 650, 2, 3, 2, pos)
        assert not np.array_equal(short, whole) and not np.array_equal(short[2], whole[2])


@pytest.mark.parametrize('value', [0, 77, 255])
def test_a_constant_clip_comes_back_exactly(value):
    _, c, C = oracle.noise_clip(20, 5, 20, 24, 20, 24, 77, 101)
    s = np.full((5, 20, 24, 3), value, np.uint8)
    for r, eps_q, t, pos in ((1, 1, 1, None), (4, 650, 3, oracle.zigzag(5, (2, 6))), (16, 65025, 2, gm.positions_of([(16, -16)] * 4))):
        assert (oracle.guided_upsample_time(s, c, C, r, eps_q, t, pos) == value).all()


@pytest.mark.parametrize('case', [(9, 13, 9, 13, 2, 650), (16, 20, 9, 13, 3, 650)], ids=str)
def test_equal_sizes_stay_within_one_level_of_the_temporal_filter(case):
    import guided_time_oracle as gt
    h, w, hc, wc, r, eps_q = case
    s, c, _ = oracle.noise_clip(30, 5, h, w, hc, wc, hc, wc)
    for pos in (None, oracle.zigzag(5, (1, 3))):
        got = oracle.guided_upsample_time(s, c, c, r, eps_q, 2, pos).astype(int)
        want = (gt.guided_filter_time(s, c, r, eps_q, 2) if pos is None else gm.guided_filter_motion(s, c, r, eps_q, 2, pos))[:, :hc, :wc].astype(int)
        assert np.abs(got - want).max() <= 1


@pytest.mark.parametrize('case', gu.CASES, ids=str)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(case):
    """per pixel and channel, before the clamp: 0.5 + 256 2^-12 + D 2^-8 (guided_up_time_rule.h), on 5-frame clips of noise and of a
    smooth content, at T = 1 and 2 without motion and at T = 2 under positions"""
    h, w, hc, wc, H, W, r, eps_q = case
    worst = 0.0
    for s, c, C in (oracle.noise_clip(10, 5, h, w, hc, wc, H, W), oracle.clip_case(11, 5, h, w, hc, wc, H, W)):
        for t, pos in ((1, None), (2, None), (2, gm.positions_of(STEPS))):
            got = oracle.guided_upsample_time_unclamped(s, c, C, r, eps_q, t, pos).astype(np.float64)
            want = oracle.guided_upsample_time_f64(s, c, C, r, eps_q, t, pos)
            dist, lim = np.abs(got - want), oracle.bound(s, c, C, r, eps_q, t, pos)
            worst = max(worst, float((dist / lim).max()))
            print('case %s T %d %s: worst distance %.4f, its bound %.4f, worst ratio %.3f'
                  % (case, t, 'motion' if pos is not None else 'still', dist.max(), lim.flat[dist.argmax()], (dist / lim).max()))
            assert (dist <= lim + 1e-6).all(), (dist - lim).max()
    print('case %s: worst error / bound %.3f' % (case, worst))


def test_flicker_falls_with_the_frames_and_the_edge_stays():
    """a static 50 | 200 step at full column 66 of 96 x 128, ratio 4, 12 frames, N(0, 20) noise on the small frames, r 4, eps_q 650:
    the flicker of the delivered frames over the flat columns < 42 falls strictly with T (measured 2.17 -> 0.42 / 0.16 / 0.09 grey
    levels), at T = 1 to below half, and the jump between columns 65 and 66 does not shrink (smallest 105 -> 112 / 113 / 113)"""
    s, c, C = oracle.flicker_case()
    fl, jump = [], []
    for t in range(4):
        out = oracle.guided_upsample_time(s, c, C, 4, 650, t)
        fl.append(oracle.flicker(out))
        jump.append(oracle.edge_jump(out))
        print('T %d: flicker %.3f grey levels, edge jump mean %.1f, smallest %.0f' % (t, fl[-1], jump[-1][0], jump[-1][1]))
    assert fl[0] > fl[1] > fl[2] > fl[3]
    assert fl[1] < 0.5 * fl[0]
    for t in (1, 2, 3):
        assert jump[t][1] >= jump[0][1]


def test_the_numpy_rule_of_the_package_is_the_oracle():
    from wct_tf_amd import ops
    s, c, C = oracle.clip_case(6, 5, 16, 20, 9, 13, 50, 70)
    for t, pos in ((0, None), (2, None), (3, oracle.zigzag(5, (2, 6))), (1, gm.positions_of([(16, -16)] * 4))):
        assert np.array_equal(ops.guided_upsample_time_np(s, c, C, 3, 650, t, positions=pos), oracle.guided_upsample_time(s, c, C, 3, 650, t, pos))
    with pytest.raises(ValueError, match='radius'):
        ops.guided_upsample_time_np(s, c, C, 34, 650, 3)
    with pytest.raises(ValueError, match='does not scale down'):
        ops.guided_upsample_time_np(s, c, C[:, :8], 3, 650, 1)


# ---- the command line ------------------------------------------------------------------------------------------------------------
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
    stylize_video.check_upsample_time_args(parser, args)
    return args


VBASE = ['--relu-targets', 'relu2_1', 'relu1_1', '--synthetic-weights', '1', '--in-path', 'i', '--style-path', 's', '--out-path', 'o']
UP = ['--guided-upsample', '--guided-radius', '4', '--content-size', '64']


def test_the_video_command_line_takes_the_options_and_has_them_off_by_default():
    args = _video_args(VBASE + UP)
    assert (args.guided_upsample_frames, args.guided_upsample_motion, args.guided_upsample_motion_range) == (0, None, None)
    args = _video_args(VBASE + UP + ['--guided-upsample-frames', '2', '--guided-upsample-motion', 'global',
                                     '--guided-upsample-motion-range', '5', '--content-colors'])
    assert (args.guided_upsample_frames, args.guided_upsample_motion, args.guided_upsample_motion_range) == (2, 'global', 5)
    assert _video_args(VBASE + ['--guided-upsample', '--guided-radius', '33', '--content-size', '64', '--guided-upsample-frames', '3'])
    from wct_tf_amd import stylize
    assert not any('--guided-upsample-frames' in a.option_strings for a in stylize.build_parser()._actions)     # single images: nothing


def test_parser_errors_name_the_option(capsys):
    def refused(argv, word):
        with pytest.raises(SystemExit):
            _video_args(argv)
        assert word in capsys.readouterr().err, (argv, word)

    plain = VBASE + ['--guided-radius', '4', '--content-size', '64']
    refused(plain + ['--guided-upsample-frames', '1'], '--guided-upsample-frames needs --guided-upsample')
    refused(plain + ['--guided-upsample-motion', 'global'], '--guided-upsample-motion needs --guided-upsample')
    refused(plain + ['--guided-upsample-motion-range', '4'], '--guided-upsample-motion-range needs --guided-upsample')
    refused(VBASE + UP + ['--guided-upsample-frames', '4'], '--guided-upsample-frames must be 0')
    refused(VBASE + UP + ['--guided-upsample-frames', '-1'], '--guided-upsample-frames must be 0')
    refused(VBASE + UP + ['--guided-upsample-motion', 'global'], '--guided-upsample-motion needs --guided-upsample-frames >= 1')
    refused(VBASE + UP + ['--guided-upsample-frames', '1', '--guided-upsample-motion-range', '4'],
            '--guided-upsample-motion-range needs --guided-upsample-motion')
    for r in ('0', '17'):
        refused(VBASE + UP + ['--guided-upsample-frames', '1', '--guided-upsample-motion', 'global', '--guided-upsample-motion-range', r],
                '--guided-upsample-motion-range must be 1 .. 16')
    refused(VBASE + UP + ['--guided-upsample-motion', 'block'], '--guided-upsample-motion')
    for t, r in ((1, 52), (2, 41), (3, 34)):
        refused(VBASE + ['--guided-upsample', '--guided-radius', str(r), '--content-size', '64', '--guided-upsample-frames', str(t)],
                '--guided-radius must be at most %d with --guided-upsample-frames %d' % (r - 1, t))
    refused(VBASE + UP + ['--guided-upsample-frames', '1', '--guided-upsample-guide', 'color'],
            '--guided-upsample-frames goes with the grey guide')
    for extra, word in ((['--swap5'], '--swap5'), (['--keep-colors'], '--keep-colors'), (['--passes', '2'], '--passes > 1'),
                        (['--warm-start'], '--warm-start'), (['--alpha-map', 'm'], '--alpha-map'), (['--guided-frames', '1'], '--guided-frames')):
        refused(VBASE + UP + ['--guided-upsample-frames', '1'] + extra, word)


def test_the_video_tools_buffer_gives_the_whole_clips_frames_wherever_the_batches_are_cut():
    """stylize_video.upsample_clips with the oracle as its op and a window of 10 small frames (chunks of 2 at T = 2, of 6 at T = 1):
    two clips of different sizes in one stream, batches of 1, 3 and 5 frames -- every delivered frame is the whole-clip oracle's,
    and the op never sees the full content of a frame it does not deliver"""
    from wct_tf_amd.stylize_video import upsample_clips
    clips = [oracle.noise_clip(80, 11, 8, 9, 7, 9, 15, 19), oracle.noise_clip(81, 4, 6, 7, 6, 7, 12, 14)]
    for t in (1, 2):
        want = [oracle.guided_upsample_time(s, c, C, 1, 650, t) for s, c, C in clips]
        for batch in (1, 3, 5):
            def batches():
                for k, (s, c, C) in enumerate(clips):
                    for i in range(0, len(s), batch):
                        n = len(s[i:i + batch])
                        yield [(k, i + j) for j in range(n)], s[i:i + batch], c[i:i + batch], C[i:i + batch], ['x'] * n

            def op(plain, small, full, f0, f1):
                assert len(plain) <= 10 and len(full) == f1 - f0
                return oracle.deliver(*[m[f0:f1] for m in oracle.means(plain, small, 1, 650, t)], small.shape[1], small.shape[2], full)

            seen = []
            for files, outs, extras in upsample_clips(batches(), t, op, window=10):
                assert len(files) == len(outs) == len(extras)
                for (k, i), o in zip(files, outs):
                    assert np.array_equal(o, want[k][i]), (t, batch, k, i)
                    seen.append((k, i))
            assert seen == [(0, i) for i in range(11)] + [(1, i) for i in range(4)]


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, upsample_time_chunk
    from wct_tf_amd.wct import WCT
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c, C = oracle.noise_clip(50, 4, 16, 20, 9, 13, 40, 61)
    calls = (lambda *a, **k: ctx.guided_upsample_time(*a, **k), lambda *a, **k: ctx.guided_upsample_time_clip(*a, **k))
    for call in calls:
        with pytest.raises(ValueError, match='smaller than its content'):
            call(c, s, C, 4, 650, 1)
        with pytest.raises(ValueError, match='does not scale down'):
            call(s, c, C[:, :8], 4, 650, 1)
        with pytest.raises(ValueError, match='uint8 images, contents_full'):
            call(s, c, C.astype(np.float32), 4, 650, 1)
        with pytest.raises(ValueError, match='one full content per delivered frame'):
            call(s, c, C[:3], 4, 650, 1)
        with pytest.raises(ValueError, match='as many contents as frames'):
            call(s, c[:3], C, 4, 650, 1)
        for r, e, t, word in ((0, 650, 1, 'radius'), (52, 650, 1, 'radius'), (34, 650, 3, 'radius'), (4, 0, 1, 'eps_q'), (4, 650, 4, 'guided_frames'),
                              (4, 650, 1.5, 'guided_frames')):
            with pytest.raises(ValueError, match=word):
                call(s, c, C, r, e, t)
        with pytest.raises(ValueError, match=r'expected \(4, 2\)'):
            call(s, c, C, 4, 650, 1, positions=np.zeros((3, 2), np.int32))
        with pytest.raises(ValueError, match='must be within 16'):
            call(s, c, C, 4, 650, 1, positions=gm.positions_of([(17, 0)] * 3))
    with pytest.raises(ValueError, match='1 .. 32 frames in one call'):
        ctx.guided_upsample_time(np.repeat(s, 9, 0), np.repeat(c, 9, 0), np.repeat(C, 9, 0), 4, 650, 1)
    with pytest.raises(ValueError, match='range 0 <= f0 < f1 <= frames'):
        ctx.guided_upsample_time_range(s, c, C[:2], 4, 650, 1, 3, 5)
    with pytest.raises(ValueError, match='one full content per delivered frame'):
        ctx.guided_upsample_time_range(s, c, C, 4, 650, 1, 1, 3)
    with pytest.raises(ValueError, match='range 0 <= f0 < f1 <= frames'):
        ctx.guided_upsample_time_batch_dev(None, 16, 20, None, 9, 13, None, 40, 61, 4, 4, 650, 1, 2, 2, None)
    with pytest.raises(ValueError, match='radius'):
        ctx.guided_upsample_time_batch_dev(None, 16, 20, None, 9, 13, None, 40, 61, 4, 41, 650, 2, 0, 4, None)
    # the chunk of a clip: 32 - 4T, lowered where that many full frames would reach 2^31 bytes
    assert [upsample_time_chunk(1080, 1920, t) for t in range(4)] == [32, 28, 24, 20]
    assert upsample_time_chunk(4320, 7680, 1) == 21 and 22 * 4320 * 7680 * 3 >= 2 ** 31 > 21 * 4320 * 7680 * 3
    # the model's keywords: checked before anything else of the call
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    up = dict(guided_upsample=(40, 2, 65))
    with pytest.raises(ValueError, match='need guided_upsample='):
        m.predict_frames(C, s[0], guided_upsample_frames=1)
    with pytest.raises(ValueError, match='need guided_upsample='):
        m.predict_frames(C, s[0], guided_upsample_motion='global')
    with pytest.raises(ValueError, match='guided_upsample_motion needs guided_upsample_frames >= 1'):
        m.predict_frames(C, s[0], guided_upsample_motion='global', **up)
    with pytest.raises(ValueError, match="'color' guide has no form along time"):
        m.predict_frames(C, s[0], guided_upsample=(40, 2, 65, 'color'), guided_upsample_frames=1)
    with pytest.raises(ValueError, match='guided_frames must be 0 .. 3'):
        m.predict_frames(C, s[0], guided_upsample_frames=4, **up)
    with pytest.raises(ValueError, match='radius must be 1 .. 33 with guided_frames 3'):
        m.predict_frames(C, s[0], guided_upsample=(40, 34, 65), guided_upsample_frames=3)
    for kw, name in ((dict(swap5=True), 'swap5'), (dict(guided=(2, 65)), 'guided'), (dict(guided=(2, 65), guided_frames=1), 'guided'),
                     (dict(resize=(20, 30)), 'resize'), (dict(wrap=True), 'wrap')):
        with pytest.raises(ValueError, match='%s is not served with guided_upsample' % name):
            m.predict_frames(C, s[0], guided_upsample_frames=1, **dict(up, **kw))
    with pytest.raises(ValueError, match="None, 'global'"):
        m.predict_frames(C, s[0], guided_upsample_frames=1, guided_upsample_motion='block', **up)
    with pytest.raises(ValueError, match='search range must be 1 .. 16'):
        m.predict_frames(C, s[0], guided_upsample_frames=1, guided_upsample_motion=('global', 17), **up)
    with pytest.raises(ValueError, match='needs contents of at least 48 x 48'):
        m.predict_frames(C, s[0], guided_upsample_frames=1, guided_upsample_motion=('global', 12), **up)      # the working size is 40 x 61
    with pytest.raises(ValueError, match=r'expected \(4, 2\)'):
        m.predict_frames(C, s[0], guided_upsample_frames=1, guided_upsample_motion=np.zeros((5, 2), np.int32), **up)
    with pytest.raises(ValueError, match='uint8 contents'):
        m.predict_frames(C.astype(np.float32), s[0], guided_upsample_frames=1, **up)
    with pytest.raises(ValueError, match=r'\[F\]\[H\]\[W\]\[3\] contents'):
        m.predict_frames(C[0], s[0], guided_upsample_frames=1, **up)
    # what was refused stays refused
    with pytest.raises(ValueError, match='guided_frames is not served with guided_upsample'):
        m.predict_frames(C, s[0], guided_frames=1, **up)


def test_symbols_and_sources_are_in_place():
    from wct_tf_amd import _lib, ops
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {'wct_guided_upsample_time', 'wct_guided_upsample_time_batch_dev'} <= bound
    assert 'guided_up_time.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    assert ops.guided_upsample_time_np is not None
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_up_time_rule.h')).read()
    assert '#include "guided_up_rule.h"' in rule and '#include "guided_motion_rule.h"' in rule


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_up_time_rule_check.cpp includes csrc/guided_up_time_rule.h -- the functions the kernels call -- and compares
    the bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into this process.  The last cases are the
    extreme of the bounds, r = 33, T = 3, eps_q = 1 on 7 frames of 70 x 70 (full windows of 31423 pixels): a 0 / 255 checkerboard
    guide under frames of 255, the same guide under frames that follow it, and frames of 0 / 255 under a guide of two neighbouring
    greys (|a_q| = 261120).  The signed-overflow check of UBSan there, and the program's own comparison with the stated bounds,
    are their proof."""
    cases = []
    for seed, ((h, w, hc, wc, H, W, r, eps_q), F, t, pos) in enumerate([
            (gu.CASES[0], 3, 1, None), (gu.CASES[1], 4, 2, gm.positions_of([(1, -2), (-16, 16), (0, 5)])), (gu.CASES[3], 5, 3, oracle.zigzag(5, (2, 6))),
            (gu.CASES[3], 1, 2, None), (gu.CASES[5], 3, 0, None)]):
        cases.append(oracle.noise_clip(60 + seed, F, h, w, hc, wc, H, W) + (r, eps_q, t, pos))
    cases.append(oracle.clip_case(70, 4, 20, 24, 17, 21, 77, 101) + (3, 65, 2, gm.positions_of([(3, 0), (16, 16), (-5, 1)])))
    n, F = 70, 7
    xx = np.mgrid[:n, :n][1] + np.mgrid[:n, :n][0]
    clip = lambda a: np.repeat(np.repeat(a[None, ..., None], 3, -1), F, 0).astype(np.uint8)
    board = clip((xx & 1) * 255)
    full = clip((np.mgrid[:2 * n, :2 * n][1] & 1) * 255)                               # the full guide swings over 0 .. 255
    cases.append((clip(np.full((n, n), 255)), board, full, 33, 1, 3, None))
    cases.append((board, board, full, 33, 1, 3, oracle.zigzag(F, (1, 1))))
    cases.append((clip((np.mgrid[:n, :n][1] & 1) * 255), clip(100 + (np.mgrid[:n, :n][1] & 1) * 2), full, 33, 1, 3, None))
    blob = struct.pack('<i', len(cases))
    for s, c, C, r, eps_q, t, pos in cases:
        blob += struct.pack('<11i', s.shape[0], s.shape[1], s.shape[2], c.shape[1], c.shape[2], C.shape[1], C.shape[2], r, eps_q, t, pos is not None)
        if pos is not None:
            blob += np.ascontiguousarray(pos, '<i4').tobytes()
        blob += s.tobytes() + c.tobytes() + C.tobytes() + oracle.guided_upsample_time(s, c, C, r, eps_q, t, pos).tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_up_time_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_up_time_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    print(out.stdout)
    assert int(out.stdout.split('max n ')[1].split(',')[0]) == 7 * 67 * 67, out.stdout
    assert int(out.stdout.split('max |a_q| ')[1].split(',')[0]) == 261120, out.stdout
    assert 200000 < int(out.stdout.split('max |am| ')[1].split(',')[0]) < 2 ** 18, out.stdout
