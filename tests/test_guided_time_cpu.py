"""Temporal guided smoothing without a GPU: the NumPy oracle of the 3-D rule against guided_oracle at T = 0, against a naive loop
over 3-D windows and against the float64 filter, the properties the feature was built for (flicker falls, a step stays, a moving
edge costs no cliff), the width of the halo a chunked clip needs, the sliding buffer of the video tool, the command line, the
Python refusals, and the shared rule header (wct_tf_amd/csrc/guided_time_rule.h, what the kernels compile) built for the host
under AddressSanitizer + UBSan as a program of its own."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_oracle as g2
import guided_time_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 4])
def test_no_frames_on_either_side_is_the_2d_rule(r):
    s, c = _rand(1, (1, 33, 35, 3)), _rand(2, (1, 33, 35, 3))
    assert np.array_equal(oracle.guided_filter_time(s, c, r, 650, 0)[0], g2.guided_filter(s[0], c[0], r, 650))
    sb, cb = _rand(3, (3, 33, 35, 3)), _rand(4, (3, 33, 35, 3))
    assert np.array_equal(oracle.guided_filter_time(sb, cb, r, 650, 0), g2.guided_filter(sb, cb, r, 650))
    # a one-frame clip has no neighbours, whatever T
    assert np.array_equal(oracle.guided_filter_time(s, c, r, 650, 2), g2.guided_filter(s, c, r, 650))


@pytest.mark.parametrize('t', [1, 2, 3])
@pytest.mark.parametrize('r', [1, 3])
def test_vectorised_oracle_is_the_scalar_loop(r, t):
    s, c = _rand(5, (4, 9, 11, 3)), _rand(6, (4, 9, 11, 3))
    got = oracle.guided_filter_time(s, c, r, 650, t)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.guided_filter_time_loop(s, c, r, 650, t))
    # F = 2 < 2T + 1: the time window is the whole clip for every frame
    assert np.array_equal(oracle.guided_filter_time(s[:2], c[:2], r, 650, t), oracle.guided_filter_time_loop(s[:2], c[:2], r, 650, t))
    assert (oracle.count3(2, 9, 11, 16, t) == 2 * 9 * 11).all()


def test_frame_larger_than_content_reads_the_clamped_guide():
    s, c = _rand(7, (3, 8, 10, 3)), _rand(8, (3, 5, 7, 3))
    assert np.array_equal(oracle.guided_filter_time(s, c, 2, 100, 1), oracle.guided_filter_time_loop(s, c, 2, 100, 1))


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('eps_q', [1, 650, 65025])
@pytest.mark.parametrize('r', [1, 5])
@pytest.mark.parametrize('shape', [(30, 31), (24, 40)], ids=str)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(shape, r, eps_q, t):
    """before the clamp, as in 2-D: 0.5 from the final rounding, 255 * 2^-13 from the rounding of a_q (at most half a unit of
    2^-12 each, their window mean times a guide of at most 255) and 2^-13 from that of b_q.  None of the three depends on n, so
    the third axis changes nothing.  Largest met on these cases: 0.5041."""
    s, c = _rand(10, (5,) + shape + (3,)), _rand(11, (5,) + shape + (3,))
    err = np.abs(oracle.guided_filter_time_unclamped(s, c, r, eps_q, t) - oracle.guided_filter_time_f64(s, c, r, eps_q, t)).max()
    assert err <= 0.5 + 255 * 2.0 ** -13 + 2.0 ** -13, err


def test_a_constant_clip_comes_back_exactly():
    c = _rand(12, (5, 20, 24, 3))
    for v, r, eps_q, t in ((0, 1, 1, 1), (255, 33, 65025, 3), (77, 5, 650, 2)):
        s = np.full((5, 20, 24, 3), v, np.uint8)
        assert np.array_equal(oracle.guided_filter_time(s, c, r, eps_q, t), s)


@pytest.mark.parametrize('t', [1, 2, 3])
def test_a_clip_of_identical_frames_gives_every_frame_the_2d_bytes(t):
    """n3d = k n and every window sum is k times the 2-D one (k the frames of the window): cov and var scale by k^2 and so does
    eps_q n^2, so a_q is the 2-D a_q, and b_q = rdiv(k (..), k n) likewise; pass 2 scales the same way"""
    s1, c1 = _rand(13, (20, 24, 3)), _rand(14, (20, 24, 3))
    s, c = np.repeat(s1[None], 5, 0), np.repeat(c1[None], 5, 0)
    a3, b3, _, n3 = oracle.coefficients(s, c, 3, 650, t)
    a2, b2, _, n2 = g2.coefficients(s1, c1, 3, 650)
    k = np.array([min(4, f + t) - max(0, f - t) + 1 for f in range(5)])
    assert np.array_equal(n3, k[:, None, None] * n2[None]) and np.array_equal(a3, np.repeat(a2[None], 5, 0)) and \
        np.array_equal(b3, np.repeat(b2[None], 5, 0))
    want = g2.guided_filter(s1, c1, 3, 650)
    got = oracle.guided_filter_time(s, c, 3, 650, t)
    for f in range(5):
        assert np.array_equal(got[f], want), f


def test_a_chunked_clip_needs_a_halo_of_two_t_frames():
    """pass 2 of frame f reads coefficients up to T frames away, each made from frames T further: a frame depends on frames up to
    2T away.  The halo of the header, of ops.guided_filter_time_np and of the video tool is 2T; T is not enough."""
    s, c = _rand(15, (12, 10, 12, 3)), _rand(16, (12, 10, 12, 3))
    whole = oracle.guided_filter_time(s, c, 2, 650, 2)
    assert np.array_equal(oracle.guided_filter_time_chunked(s, c, 2, 650, 2, chunk=5, halo=4), whole)
    assert not np.array_equal(oracle.guided_filter_time_chunked(s, c, 2, 650, 2, chunk=5, halo=2), whole)


def _flat_flicker(out, w=64):
    """mean |frame-to-frame difference| on the flat side, 6 columns away from the step"""
    return np.abs(np.diff(out[..., 0].astype(np.float64)[:, :, :w // 2 - 6], axis=0)).mean()


def test_flicker_on_a_static_step_falls_and_the_step_stays():
    """static step 50 | 200, independent sigma = 20 noise per frame, F = 12, 48 x 64, r = 4, eps_q = 650, seed 0.  Measured with
    this oracle and this seed: flicker 1.882 grey levels at T = 0, 0.368 at T = 1 (ratio 0.196), 0.104 at T = 3 (ratio 0.055);
    step 150.10 / 150.11 / 150.17 of 150 at T = 0 / 1 / 3.  The bounds are 1.5 x the two ratios, the margin for nothing but the
    seed."""
    s, c, _ = oracle.flicker_case(0)
    out = {t: oracle.guided_filter_time(s, c, 4, 650, t) for t in (0, 1, 3)}
    assert np.array_equal(out[0], g2.guided_filter(s, c, 4, 650))
    base = _flat_flicker(out[0])
    print('flicker', {t: _flat_flicker(o) for t, o in out.items()})
    assert _flat_flicker(out[1]) <= 1.5 * 0.196 * base
    assert _flat_flicker(out[3]) <= 1.5 * 0.055 * base
    for t, o in out.items():
        v = o[..., 0].astype(np.float64)
        step = v[:, :, 64 // 2 + 8:].mean() - v[:, :, :64 // 2 - 8].mean()
        print('step', t, step)
        assert abs(step - 150) <= 0.02 * 150, (t, step)


def test_a_moving_edge_costs_no_cliff():
    """the same step moving 3 px per frame: mean |error| against the noise-free frames 2.04 / 1.94 / 2.31 / 2.71 at T = 0 .. 3 with
    this seed, at most 1.33 x that of T = 0; the bound is 1.5 x"""
    s, c, clean = oracle.flicker_case(0, move=3)
    err = [np.abs(oracle.guided_filter_time(s, c, 4, 650, t)[..., 0].astype(np.float64) - clean).mean() for t in range(4)]
    print('moving edge', err)
    for t in (1, 2, 3):
        assert err[t] <= 1.5 * err[0], err


# ---- the sliding buffer of the video tool ----------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', [1, 2, 5, 32])
@pytest.mark.parametrize('t,window', [(1, 8), (2, 12), (1, 32)])
def test_sliding_buffer_gives_the_whole_clip_op_per_clip_wherever_the_batches_are_cut(batch, t, window):
    """two clips (13 frames of 6 x 8, then 4 of 8 x 6) through stylize_video.smooth_clips with the oracle as the resident-clip
    op: every frame equals the whole-clip oracle of its clip, in order, and no call sees more than `window` frames"""
    from wct_tf_amd.stylize_video import smooth_clips
    clips = [(_rand(20, (13, 6, 8, 3)), _rand(21, (13, 6, 8, 3))), (_rand(22, (4, 8, 6, 3)), _rand(23, (4, 8, 6, 3)))]
    names = iter(range(100))
    seen = []

    def batches():
        for s, c in clips:
            for i in range(0, len(s), batch):
                n = len(s[i:i + batch])
                yield [next(names) for _ in range(n)], s[i:i + batch], c[i:i + batch], ['x'] * n

    def op(s, c, f0, f1):
        seen.append(len(s))
        return oracle.guided_filter_time(s, c, 1, 650, t)[f0:f1]

    got = list(smooth_clips(batches(), t, op, window=window))
    files = [f for item in got for f in item[0]]
    assert files == list(range(17))
    frames = [o for item in got for o in item[1]]
    want = [o for s, c in clips for o in oracle.guided_filter_time(s, c, 1, 650, t)]
    assert all(np.array_equal(a, b) for a, b in zip(frames, want)) and len(frames) == 17
    contents = [o for item in got for o in item[2]]
    assert all(np.array_equal(a, b) for a, b in zip(contents, [f for _, c in clips for f in c]))
    assert all(e == 'x' for item in got for e in item[3]) and max(seen) <= window


# ---- command line ----------------------------------------------------------------------------------------------------------
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1']


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


def test_the_option_is_off_by_default_and_the_image_tool_has_none():
    from wct_tf_amd import stylize
    a = _check_video(_VID + ['--style-path', 's'])
    assert a.guided_frames == 0
    a = _check_video(_VID + ['--style-path', 's', '--guided-radius', '8'])
    assert a.guided_frames == 0
    a = _check_video(_VID + ['--style-path', 's', '--guided-radius', '8', '--guided-frames', '2', '--warm-start', '--content-colors',
                             '--passes', '2'])
    assert a.guided_frames == 2
    assert '--guided-frames' not in stylize.build_parser().format_help()


def test_radius_limits_per_frame_count(capsys):
    from wct_tf_amd import _lib
    assert _lib.GUIDED_TIME_MAX_RADIUS == oracle.MAX_RADIUS == (64, 51, 40, 33)
    for t, rmax in enumerate(oracle.MAX_RADIUS):
        assert oracle.params_ok(rmax, 650, t) and not oracle.params_ok(rmax + 1, 650, t)
        assert (2 * rmax + 1) ** 2 * (2 * t + 1) * 65025 < 2 ** 31
        if rmax < 64:
            assert (2 * rmax + 3) ** 2 * (2 * t + 1) > oracle.MAX_WINDOW
        extra = ['--guided-frames', str(t)] if t else []
        assert _check_video(_VID + ['--style-path', 's', '--guided-radius', str(rmax)] + extra).guided_radius == rmax
        with pytest.raises(SystemExit):
            _check_video(_VID + ['--style-path', 's', '--guided-radius', str(rmax + 1)] + extra)
        err = capsys.readouterr().err
        assert '--guided-radius' in err and str(rmax) in err
    assert oracle.MAX_WINDOW == 2 ** 31 // 65025


def test_parser_refusals_name_the_option(capsys):
    ok = ['--style-path', 's', '--guided-radius', '4']
    for extra, word in ((['--style-path', 's', '--guided-frames', '1'], '--guided-radius'),
                        (ok + ['--guided-frames', '4'], '--guided-frames'),
                        (ok + ['--guided-frames', '-1'], '--guided-frames'),
                        (ok + ['--guided-frames', '1', '--guided-guide', 'color'], '--guided-guide'),
                        (ok + ['--guided-frames', '1', '--swap5'], '--swap5'),
                        (ok + ['--guided-frames', '1', '--keep-colors'], '--keep-colors'),
                        (['--guided-radius', '4', '--guided-frames', '1', '--mask-path', 'm', '--mask-styles', 'a', 'b'], '--mask-path')):
        with pytest.raises(SystemExit):
            _check_video(_VID + extra)
        err = capsys.readouterr().err
        assert word in err and '--guided-frames' in err, err
    # the same options without --guided-frames stay allowed
    assert _check_video(_VID + ok + ['--guided-guide', 'color']).guided_guide == 'color'
    assert _check_video(_VID + ok + ['--swap5']).swap5 and _check_video(_VID + ok + ['--keep-colors']).keep_colors


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_guided_time
    from wct_tf_amd.wct import WCT
    import wct_tf_amd
    assert wct_tf_amd.guided_filter_time_np is wct_tf_amd.ops.guided_filter_time_np and 'guided_filter_time_np' in wct_tf_amd.__all__
    assert check_guided_time(51, 650, 1) == (51, 650, 1) and check_guided_time(64, 1, 0) == (64, 1, 0)
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (3, 16, 20, 3)), _rand(31, (3, 9, 20, 3))
    calls = (lambda r, e, t: ctx.guided_filter_time(s, c, r, e, t), lambda r, e, t: ctx.guided_filter_time_clip(s, c, r, e, t),
             lambda r, e, t: ctx.guided_filter_time_range(s, c, r, e, t, 0, 1),
             lambda r, e, t: ctx.guided_filter_time_batch_dev(None, 16, 20, None, 9, 20, 3, r, e, t, 0, 3, None),
             lambda r, e, t: wct_tf_amd.guided_filter_time_np(s, c, r, e, t, ctx=ctx))
    for r, e, t, word in ((0, 650, 1, 'radius'), (52, 650, 1, '1 .. 51'), (41, 650, 2, '1 .. 40'), (34, 650, 3, '1 .. 33'), (65, 650, 0, 'radius'),
                          (4, 0, 1, 'eps_q'), (4, 65026, 1, 'eps_q'), (4, 650, 4, 'guided_frames'), (4, 650, -1, 'guided_frames'),
                          (4, 650, 1.5, 'guided_frames'), (4, 650, None, 'guided_frames'), (4.5, 650, 1, 'integers')):
        for call in calls:
            with pytest.raises(ValueError, match=word):
                call(r, e, t)
    with pytest.raises(ValueError, match='smaller'):
        ctx.guided_filter_time(c, s, 4, 650, 1)           # Ho < Hc
    with pytest.raises(ValueError, match='guided_filter_time takes uint8'):
        ctx.guided_filter_time(s.astype(np.float32), c, 4, 650, 1)
    with pytest.raises(ValueError, match=r'\[B\]\[H\]\[W\]\[3\]'):
        ctx.guided_filter_time(s[0], c[0], 4, 650, 1)
    with pytest.raises(ValueError, match='as many contents'):
        ctx.guided_filter_time_clip(s, c[:2], 4, 650, 1)
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.guided_filter_time(np.zeros((33, 4, 4, 3), np.uint8), np.zeros((33, 4, 4, 3), np.uint8), 4, 650, 1)
    for f0, f1 in ((-1, 2), (2, 2), (0, 4), (3, 1)):
        with pytest.raises(ValueError, match='f0 < f1'):
            ctx.guided_filter_time_range(s, c, 4, 650, 1, f0, f1)
        with pytest.raises(ValueError, match='f0 < f1'):
            ctx.guided_filter_time_batch_dev(None, 16, 20, None, 9, 20, 3, 4, 650, 1, f0, f1, None)
    # the model's keyword: checked before anything else of the call
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    frames, style = c, s[0]
    with pytest.raises(ValueError, match='guided_frames needs guided'):
        m.predict_frames(frames, style, guided_frames=1)
    with pytest.raises(ValueError, match="'color' guide"):
        m.predict_frames(frames, style, guided=(4, 650, 'color'), guided_frames=1)
    with pytest.raises(ValueError, match='guided_frames is not served with swap5'):
        m.predict_frames(frames, style, guided=(4, 650), guided_frames=1, swap5=True)
    with pytest.raises(ValueError, match='guided_frames is not served with wrap'):
        m.predict_frames(frames, style, guided=(4, 650), guided_frames=1, wrap=True)
    with pytest.raises(ValueError, match='guided_frames must be 0 .. 3'):
        m.predict_frames(frames, style, guided=(4, 650), guided_frames=4)
    with pytest.raises(ValueError, match='1 .. 51'):
        m.predict_frames(frames, style, guided=(52, 650), guided_frames=1)


def test_the_unit_the_symbols_and_the_limits_are_where_the_issue_puts_them():
    from wct_tf_amd import _lib
    assert 'guided_time.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    names = [s[0] for s in _lib.SIGNATURES]
    for name in ('wct_guided_filter_time', 'wct_guided_filter_time_batch_dev', 'wct_guided_time_max_radius'):
        assert name in names
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    for name in ('wct_guided_filter_time(', 'wct_guided_filter_time_batch_dev(', 'wct_guided_time_max_radius('):
        assert name in hdr
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_time_rule.h')).read()
    assert int(re.search(r'WCT_GUIDED_TIME_MAX_WINDOW\s+(\d+)', rule).group(1)) == oracle.MAX_WINDOW
    assert int(re.search(r'WCT_GUIDED_TIME_MAX_FRAMES\s+(\d+)', rule).group(1)) == oracle.MAX_FRAMES_T


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
def _extremes():
    """at (r, T) = (51, 1), (40, 2), (33, 3), clips of 2T + 1 frames of (2r + 2)^2 so that the central pixels have full windows of
    (2r + 1)^2 (2T + 1) pixels, the largest the rule admits: all-255 clips (the largest SII and SIp: n * 65025), 0 / 255
    checkerboards in space that alternate in time (the largest covariance and variance), and a guide of two neighbouring greys
    under a 0 / 255 frame (the largest a_q: sigma_p / (2 sqrt(eps_q)) = 63.75 at eps_q = 1), each at eps_q 1 and 65025"""
    cases = []
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    for t, r in ((1, 51), (2, 40), (3, 33)):
        f, side = 2 * t + 1, 2 * r + 2
        ff, yy, xx = np.mgrid[:f, :side, :side]
        board = ((ff + yy + xx) & 1) * 255
        greys = 100 + ((ff + xx) & 1) * 2
        for eps_q in (1, 65025):
            cases.append((rgb(np.full_like(board, 255)), rgb(np.full_like(board, 255)), r, eps_q, t))
            cases.append((rgb(board), rgb(board), r, eps_q, t))
            cases.append((rgb(board), rgb(greys), r, eps_q, t))
        cases.append((rgb(((ff + xx) & 1) * 255), rgb(greys), r, 1, t))               # a_q towards +63.75 * 2^12
        cases.append((rgb(255 - ((ff + xx) & 1) * 255), rgb(greys), r, 1, t))         # ... and towards -63.75 * 2^12
    return cases


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_time_rule_check.cpp includes csrc/guided_time_rule.h -- the functions the kernels call --, forms the
    pass-1 window sums in int32 and compares the bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into
    this process.  The signed-overflow check of UBSan on the extremes is the proof of the header's bounds."""
    cases = []
    for seed, (f, h, w, hc, wc, r, eps_q, t) in enumerate([(4, 9, 13, 9, 13, 16, 650, 3), (5, 33, 35, 33, 35, 1, 1, 1),
                                                           (5, 33, 35, 33, 35, 4, 65025, 2), (4, 16, 20, 9, 13, 3, 650, 1),
                                                           (2, 20, 24, 20, 24, 5, 7, 3), (3, 20, 24, 20, 24, 2, 650, 0)]):
        cases.append((_rand(50 + seed, (f, h, w, 3)), _rand(70 + seed, (f, hc, wc, 3)), r, eps_q, t))
    s, c = g2.clamp_case()
    cases.append((np.repeat(s[None], 3, 0), np.repeat(c[None], 3, 0), 1, 1, 1))
    cases += _extremes()
    blob = struct.pack('<i', len(cases))
    for s, c, r, eps_q, t in cases:
        blob += struct.pack('<8i', s.shape[0], s.shape[1], s.shape[2], c.shape[1], c.shape[2], r, eps_q, t)
        blob += s.tobytes() + c.tobytes() + oracle.guided_filter_time(s, c, r, eps_q, t).tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_time_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_time_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    # the full windows were met, their sums reached the neighbourhood of 2^31 and stayed under it, and so did a_q under its bound
    field = lambda name: int(out.stdout.split(name + ' ')[1].split(',')[0].split()[0])
    assert field('max n') == 5 * 81 ** 2 == 32805, out.stdout               # the largest of 31827, 32805, 31423
    assert field('max sum') == 32805 * 65025 < 2 ** 31, out.stdout
    assert 200000 < field('max |a_q|') < 2 ** 18, out.stdout
