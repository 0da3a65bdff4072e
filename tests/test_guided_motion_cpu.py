"""Temporal guided smoothing along camera motion without a GPU: the NumPy oracle of the shifted-window rule against
guided_time_oracle at equal positions and against a naive loop over windows, the bounds of n, the halo of a chunked clip, the
estimator on panning clips, the effect the feature was built for (flicker along the motion and error against the noise-free
frames), the Python and parser refusals, and the shared rule header (wct_tf_amd/csrc/guided_motion_rule.h, what the kernels
compile) built for the host under AddressSanitizer + UBSan as a program of its own."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_oracle as g2
import guided_time_oracle as gt
import guided_motion_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def _walk(seed, frames, step=16):
    """random positions: steps uniform in [-step, step] on both axes, from an arbitrary start"""
    rng = np.random.default_rng(seed)
    return (oracle.positions_of(rng.integers(-step, step + 1, (frames - 1, 2))) + rng.integers(-1000, 1000, (1, 2))).astype(np.int32)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [0, 1, 3])
def test_equal_positions_are_the_rule_without_motion(t):
    s, c = _rand(1, (5, 19, 23, 3)), _rand(2, (5, 15, 23, 3))
    want = gt.guided_filter_time(s, c, 3, 650, t)
    for p in ((0, 0), (7, -3), (-100000, 99999)):
        pos = np.tile(np.array(p, np.int32), (5, 1))
        assert np.array_equal(oracle.guided_filter_motion(s, c, 3, 650, t, pos), want), p
        assert np.array_equal(oracle.count3(5, 19, 23, 3, t, pos), gt.count3(5, 19, 23, 3, t))


@pytest.mark.parametrize('r,t,steps', [(1, 1, [(1, -2)] * 3), (3, 2, [(2, 1), (-3, 0), (0, 4)]), (2, 3, [(-1, 1)] * 3),
                                       (2, 1, [(16, -16)] * 3), (2, 2, [(16, 16), (-16, 16), (16, 16)])], ids=str)
def test_vectorised_oracle_is_the_scalar_loop(r, t, steps):
    """the step-16 cases at r = 2: a neighbour's window lies wholly outside the 9 x 11 frame (n counts the own frame alone)"""
    s, c = _rand(5, (4, 9, 11, 3)), _rand(6, (4, 9, 11, 3))
    pos = oracle.positions_of(steps)
    got = oracle.guided_filter_motion(s, c, r, 650, t, pos)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.guided_filter_motion_loop(s, c, r, 650, t, pos))
    if steps[0] == (16, -16):
        assert np.array_equal(oracle.count3(4, 9, 11, r, t, pos), np.broadcast_to(g2.count(9, 11, r), (4, 9, 11)))
        assert np.array_equal(got, g2.guided_filter(s, c, r, 650))          # every neighbour's window is empty: the 2-D bytes


def test_frame_larger_than_content_reads_the_clamped_guide():
    s, c = _rand(7, (3, 8, 10, 3)), _rand(8, (3, 5, 7, 3))
    pos = oracle.positions_of([(2, -3), (-1, 1)])
    assert np.array_equal(oracle.guided_filter_motion(s, c, 2, 100, 1, pos), oracle.guided_filter_motion_loop(s, c, 2, 100, 1, pos))


@pytest.mark.parametrize('seed', range(4))
def test_n_stays_within_the_bounds_of_the_rule_without_motion(seed):
    """the own frame gives n >= 1 (in fact its own 2-D count), every frame gives at most (2r + 1)^2"""
    rng = np.random.default_rng(seed)
    f, h, w = 8, int(rng.integers(5, 40)), int(rng.integers(5, 40))
    for r, t in ((1, 3), (4, 2), (9, 1), (33, 3)):
        n = oracle.count3(f, h, w, r, t, _walk(seed, f))
        assert n.min() >= 1 and (n >= g2.count(h, w, r)[None]).all() and n.max() <= (2 * r + 1) ** 2 * (2 * t + 1)
        assert n.max() <= gt.MAX_WINDOW


def test_a_chunked_clip_with_sliced_positions_needs_the_same_halo_of_two_t_frames():
    s, c, pos = _rand(15, (12, 10, 12, 3)), _rand(16, (12, 10, 12, 3)), _walk(3, 12, step=3)
    whole = oracle.guided_filter_motion(s, c, 2, 650, 2, pos)
    assert np.array_equal(oracle.guided_filter_motion_chunked(s, c, 2, 650, 2, pos, chunk=5, halo=4), whole)
    assert not np.array_equal(oracle.guided_filter_motion_chunked(s, c, 2, 650, 2, pos, chunk=5, halo=2), whole)


def test_only_differences_of_positions_count():
    s, c, pos = _rand(17, (5, 12, 14, 3)), _rand(18, (5, 12, 14, 3)), _walk(4, 5, step=4)
    assert np.array_equal(oracle.guided_filter_motion(s, c, 2, 650, 2, pos), oracle.guided_filter_motion(s, c, 2, 650, 2, pos + np.int32(12345)))


# ---- the estimator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [(1, 3), (2, 6)], ids=str)
def test_estimator_finds_the_true_step_of_every_pair_of_a_pan(step):
    _, contents, _, pos = oracle.pan_case(step)
    got = oracle.estimate_positions(contents, 8)
    assert got.dtype == np.int32 and np.array_equal(got, pos)
    assert np.array_equal(np.diff(got, axis=0), np.tile([-step[0], -step[1]], (11, 1)))


def test_estimator_gives_no_motion_on_flat_and_on_unchanged_pairs():
    flat = np.full((3, 32, 40, 3), 117, np.uint8)
    assert not oracle.estimate_positions(flat, 8).any()
    flat[1] = 30                                                 # every candidate has the same mean difference: the smallest wins
    assert not oracle.estimate_positions(flat, 8).any()
    same = np.repeat(_rand(20, (1, 33, 47, 3)), 3, 0)
    assert not oracle.estimate_positions(same, 8).any()
    z = np.zeros((2, 16, 16, 3), np.uint8)
    z[1] = 255                                                   # the 0 / 255 pair
    assert not oracle.estimate_positions(z, 4).any()


def test_estimator_counts_and_ties():
    i0 = np.arange(12 * 16, dtype=np.int64).reshape(12, 16) % 251
    assert oracle.sad_count(i0, i0, 0, 0) == (0, 6 * 8)
    # dy = -3: the even rows 4 .. 10; dx = 2: the even columns 0 .. 12; dy = 3: rows 0 .. 8; dx = -1: columns 2 .. 14
    assert oracle.sad_count(i0, i0, -3, 2)[1] == 4 * 7 and oracle.sad_count(i0, i0, 3, -1)[1] == 5 * 7
    assert oracle.search_ok(4, 16, 16) and not oracle.search_ok(4, 15, 16) and not oracle.search_ok(17, 400, 400) and not oracle.search_ok(0, 9, 9)
    assert oracle.search_ok(16, 64, 1 << 22) and not oracle.search_ok(16, 64, (1 << 22) + 1)


# ---- what the feature is for -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [(1, 3), (2, 6)], ids=str)
def test_a_pan_is_smoothed_along_its_motion(step):
    """checkerboard of 23 x 17 cells (60 | 190) panning by `step` px per frame, sigma = 20 noise per stylized frame, 12 frames of
    48 x 64, r = 4, eps_q = 650, T = 2, seed 0; flicker = mean |out_f(p) - out_{f+1}(p + d)| along the motion, error = mean
    |out - noise-free frame|, over rows 10 .. h - 10, columns 20 .. w - 20, frames 2 .. F - 4.  Measured with this oracle:
        pan (1, 3): flicker 2.453 (T = 0), 1.806 (T = 2, no motion), 1.316 (T = 2 along the estimated motion): ratios 0.729, 0.537;
                    error 6.073, 7.899, 5.867: gap 2.032
        pan (2, 6): flicker 2.464, 2.030, 1.250: ratios 0.616, 0.507; error 5.686, 8.484, 5.362: gap 3.122
    The bounds are the issue's: 0.8 x the uncompensated T = 2 flicker, 0.6 x the T = 0 flicker, and an error at least 1 below."""
    s, c, clean, true_pos = oracle.pan_case(step)
    h, w = s.shape[1:3]
    pos = oracle.estimate_positions(c, 8)
    assert np.array_equal(pos, true_pos)
    d = (-step[0], -step[1])
    outs = {'T=0': gt.guided_filter_time(s, c, 4, 650, 0), 'T=2': gt.guided_filter_time(s, c, 4, 650, 2),
            'T=2 along motion': oracle.guided_filter_motion(s, c, 4, 650, 2, pos)}
    fl = {k: oracle.flicker_along(o, d, h, w) for k, o in outs.items()}
    er = {k: oracle.error_against(o, clean, h, w) for k, o in outs.items()}
    print('pan', step, 'flicker', fl, 'error', er)
    assert fl['T=2 along motion'] < 0.8 * fl['T=2']
    assert fl['T=2 along motion'] < 0.6 * fl['T=0']
    assert er['T=2 along motion'] < er['T=2'] - 1


# ---- command line ----------------------------------------------------------------------------------------------------------
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1', '--style-path', 's']


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


def test_the_options_are_off_by_default_and_go_with_guided_frames():
    from wct_tf_amd import stylize, stylize_video
    a = _check_video(_VID + ['--guided-radius', '4', '--guided-frames', '2'])
    assert a.guided_motion is None and a.guided_motion_range is None
    a = _check_video(_VID + ['--guided-radius', '4', '--guided-frames', '2', '--guided-motion', 'global'])
    assert a.guided_motion == 'global' and a.guided_motion_range is None
    a = _check_video(_VID + ['--guided-radius', '4', '--guided-frames', '1', '--guided-motion', 'global', '--guided-motion-range', '16',
                             '--content-colors', '--warm-start'])
    assert a.guided_motion_range == 16
    text = stylize_video.build_parser().format_help()
    assert '--guided-motion' in text and 'scene cut' in ' '.join(text.split()) and '--guided-motion' not in stylize.build_parser().format_help()


def test_parser_refusals_name_the_option(capsys):
    ok = ['--guided-radius', '4']
    for extra, words in ((ok + ['--guided-motion', 'global'], ('--guided-motion', '--guided-frames')),
                         (['--guided-motion', 'global'], ('--guided-motion', '--guided-frames')),
                         (ok + ['--guided-frames', '0', '--guided-motion', 'global'], ('--guided-motion', '--guided-frames')),
                         (ok + ['--guided-frames', '1', '--guided-motion-range', '4'], ('--guided-motion-range', '--guided-motion')),
                         (ok + ['--guided-motion-range', '4'], ('--guided-motion-range',)),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'global', '--guided-motion-range', '0'], ('--guided-motion-range', '1 .. 16')),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'global', '--guided-motion-range', '17'], ('--guided-motion-range', '1 .. 16')),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'dense'], ('--guided-motion',)),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'global', '--swap5'], ('--swap5',)),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'global', '--keep-colors'], ('--keep-colors',)),
                         (ok + ['--guided-frames', '1', '--guided-motion', 'global', '--guided-guide', 'color'], ('--guided-guide',))):
        with pytest.raises(SystemExit):
            _check_video(_VID + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (extra, err)
    with pytest.raises(SystemExit):
        _check_video(['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1', '--guided-radius', '4',
                      '--guided-frames', '1', '--guided-motion', 'global', '--mask-path', 'm', '--mask-styles', 'a', 'b'])
    assert '--mask-path' in capsys.readouterr().err


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_guided_motion, check_motion_search
    from wct_tf_amd.wct import WCT
    import wct_tf_amd
    assert wct_tf_amd.motion_global_np is wct_tf_amd.ops.motion_global_np and 'motion_global_np' in wct_tf_amd.__all__
    got = check_guided_motion([[0, 0], [16, -16], [0, 0]], 3)
    assert got.dtype == np.int32 and got.flags['C_CONTIGUOUS'] and got.tolist() == [[0, 0], [16, -16], [0, 0]]
    assert check_guided_motion(np.zeros((1, 2), np.int64), 1).dtype == np.int32 and check_motion_search(16, 64, 64) == 16
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (3, 16, 20, 3)), _rand(31, (3, 9, 20, 3))
    calls = (lambda p: ctx.guided_filter_time(s, c, 4, 650, 1, positions=p), lambda p: ctx.guided_filter_time_clip(s, c, 4, 650, 1, positions=p),
             lambda p: ctx.guided_filter_time_range(s, c, 4, 650, 1, 0, 1, positions=p),
             lambda p: ctx.guided_filter_motion_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, p, 0, 3, None),
             lambda p: wct_tf_amd.guided_filter_time_np(s, c, 4, 650, 1, ctx=ctx, positions=p))
    for p, word in (([[0, 0], [17, 0], [17, 0]], 'step from frame 0 to 1'), ([[0, 0], [0, 0], [0, -17]], 'step from frame 1 to 2'),
                    ([[0, 0], [1, 1]], r'expected \(3, 2\)'), ([0, 1, 2], r'expected \(3, 2\)'), ([[0.5, 0], [0, 0], [0, 0]], 'integer'),
                    ('global', 'integer'), ([[0, 0], [0, 0], [1 << 31, 0]], 'step|2\\^30')):
        for call in calls:
            with pytest.raises(ValueError, match=word):
                call(p)
    # the filter's own refusals stay in front
    with pytest.raises(ValueError, match='1 .. 51'):
        ctx.guided_filter_time(s, c, 52, 650, 1, positions=np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError, match='f0 < f1'):
        ctx.guided_filter_motion_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, np.zeros((3, 2), np.int32), 2, 2, None)
    # the estimator
    big = _rand(32, (3, 32, 40, 3))
    for call in (lambda r, a=big: ctx.motion_global(a, r), lambda r, a=big: wct_tf_amd.motion_global_np(a, r, ctx=ctx),
                 lambda r, a=big: ctx.motion_global_batch_dev(None, a.shape[1], a.shape[2], 3, r)):
        for r, word in ((0, '1 .. 16'), (17, '1 .. 16'), (2.5, 'integer'), (None, 'integer'), (9, 'at least 36 x 36')):
            with pytest.raises(ValueError, match=word):
                call(r)
    with pytest.raises(ValueError, match='uint8 contents'):
        ctx.motion_global(big.astype(np.float32), 8)
    with pytest.raises(ValueError, match='uint8 contents'):
        ctx.motion_global(big[0], 8)
    with pytest.raises(ValueError, match='1 .. 32 frames'):
        ctx.motion_global_batch_dev(None, 32, 40, 33, 8)
    # the model's keyword: checked before anything else of the call
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    with pytest.raises(ValueError, match='guided_motion needs guided_frames'):
        m.predict_frames(big, s[0], guided_motion='global')
    with pytest.raises(ValueError, match='guided_motion needs guided_frames'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_motion='global')
    with pytest.raises(ValueError, match='guided_motion needs guided_frames'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=0, guided_motion=np.zeros((3, 2), np.int32))
    for bad, word in (('dense', 'dense motion'), (('block', 8), 'per-block'), (('global', 17), '1 .. 16'), (('global', 9), 'at least 36 x 36'),
                      (np.zeros((2, 2), np.int32), r'expected \(3, 2\)'), ([[0, 0], [0, 17], [0, 0]], 'step from frame 0 to 1')):
        with pytest.raises(ValueError, match=word):
            m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_motion=bad)
    with pytest.raises(ValueError, match='at least 32 x 32'):          # the search runs on the resized contents
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_motion='global', resize=(20, 24))
    with pytest.raises(ValueError, match='guided_frames is not served with swap5'):
        m.predict_frames(big, s[0], guided=(4, 650), guided_frames=1, guided_motion='global', swap5=True)


def test_the_unit_the_symbols_and_the_limits_are_where_the_issue_puts_them():
    from wct_tf_amd import _lib
    assert 'guided_motion.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    names = [s[0] for s in _lib.SIGNATURES]
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    for name in ('wct_motion_global', 'wct_motion_global_batch_dev', 'wct_guided_filter_motion', 'wct_guided_filter_motion_batch_dev'):
        assert name in names and name + '(' in hdr
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_motion_rule.h')).read()
    assert int(re.search(r'WCT_MOTION_MAX_RANGE\s+(\d+)', rule).group(1)) == oracle.MAX_STEP == oracle.MAX_SEARCH == _lib.MOTION_MAX_RANGE
    assert '#include "guided_time_rule.h"' in rule and _lib.MOTION_MAX_PIXELS == 1 << 28
    common = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'common.h')).read()
    assert 'launch_guided_motion(' in common and 'launch_motion_global(' in common


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
def _extremes():
    """at (r, T) = (51, 1), (40, 2), (33, 3), clips of 2T + 1 frames of (2r + 2T + 2)^2 that drift by (1, -1) per frame, so that the
    central pixels have full windows of (2r + 1)^2 (2T + 1) pixels under non-zero shifts: an all-255 clip (the largest SII and SIp:
    n * 65025), a 0 / 255 checkerboard in space that alternates in time (the largest covariance and variance), and a guide of two
    neighbouring greys under a 0 / 255 frame (the largest a_q: 63.75 at eps_q = 1)"""
    cases = []
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    for t, r in ((1, 51), (2, 40), (3, 33)):
        f, side = 2 * t + 1, 2 * r + 2 * t + 2
        pos = oracle.positions_of([(1, -1)] * (f - 1))
        assert oracle.count3(f, side, side, r, t, pos).max() == (2 * r + 1) ** 2 * (2 * t + 1)
        ff, yy, xx = np.mgrid[:f, :side, :side]
        board = ((ff + yy + xx) & 1) * 255
        greys = 100 + ((ff + xx) & 1) * 2
        cases.append((rgb(np.full_like(board, 255)), rgb(np.full_like(board, 255)), r, 1, t, pos))
        cases.append((rgb(board), rgb(board), r, 1, t, pos))
        cases.append((rgb(board), rgb(board), r, 65025, t, pos))
        cases.append((rgb(((ff + xx) & 1) * 255), rgb(greys), r, 1, t, pos))             # a_q towards +63.75 * 2^12 (in the own frame)
    return cases


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_motion_rule_check.cpp includes csrc/guided_motion_rule.h -- the functions the kernels call --, forms the
    pass-1 window sums over the frames in int32 and compares the bytes with the oracle's; it runs the header's estimator against
    the oracle's positions and its comparisons at the SAD cnt extreme of a 0 / 255 pair of 2^28 pixels.  A stand-alone program:
    nothing sanitized is loaded into this process."""
    cases = []
    for seed, (f, h, w, hc, wc, r, eps_q, t, step) in enumerate([(4, 9, 13, 9, 13, 16, 650, 3, 16), (5, 33, 35, 33, 35, 1, 1, 1, 2),
                                                                 (5, 33, 35, 33, 35, 4, 65025, 2, 7), (4, 16, 20, 9, 13, 3, 650, 1, 16),
                                                                 (2, 20, 24, 20, 24, 5, 7, 3, 5), (3, 20, 24, 20, 24, 2, 650, 0, 16)]):
        cases.append((_rand(50 + seed, (f, h, w, 3)), _rand(70 + seed, (f, hc, wc, 3)), r, eps_q, t, _walk(seed, f, step)))
    s, c = g2.clamp_case()
    cases.append((np.repeat(s[None], 3, 0), np.repeat(c[None], 3, 0), 1, 1, 1, oracle.positions_of([(0, 0), (0, 0)])))
    cases += _extremes()
    blob = struct.pack('<i', len(cases))
    for s, c, r, eps_q, t, pos in cases:
        blob += struct.pack('<8i', s.shape[0], s.shape[1], s.shape[2], c.shape[1], c.shape[2], r, eps_q, t)
        blob += np.ascontiguousarray(pos, '<i4').tobytes() + s.tobytes() + c.tobytes() + oracle.guided_filter_motion(s, c, r, eps_q, t, pos).tobytes()
    z = np.zeros((2, 64, 64, 3), np.uint8)
    z[1] = 255
    est = [(oracle.pan_case((1, 3))[1], 8), (oracle.pan_case((2, 6))[1][:4], 8), (_rand(90, (3, 37, 53, 3)), 8), (_rand(91, (2, 64, 70, 3)), 16),
           (z, 16), (np.repeat(_rand(92, (1, 17, 16, 3)), 2, 0), 4)]
    blob += struct.pack('<i', len(est))
    for c, search in est:
        blob += struct.pack('<4i', c.shape[0], c.shape[1], c.shape[2], search) + c.tobytes()
        blob += np.ascontiguousarray(oracle.estimate_positions(c, search), '<i4').tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_motion_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_motion_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases, %d estimator cases' % (len(cases), len(est)) in out.stdout
    field = lambda name: int(out.stdout.split(name + ' ')[1].split(',')[0].split()[0])
    assert field('max n') == 5 * 81 ** 2 == 32805, out.stdout               # the largest of 31827, 32805, 31423
    assert field('max sum') == 32805 * 65025 < 2 ** 31, out.stdout
    assert field('min n') >= 1 and 200000 < field('max |a_q|') < 2 ** 18, out.stdout
    # ceil(16383 / 2) ceil(16385 / 2) = 8192 * 8193 samples at d = (0, 0), each 255: the largest product the comparison forms
    assert field('max product') == 255 * (8192 * 8193) ** 2 < 2 ** 61, out.stdout
