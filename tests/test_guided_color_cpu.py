"""The colour guide of guided smoothing without a GPU: the NumPy oracle of the rule (tests/guided_color_oracle.py) against a naive
loop over windows, against the float64 colour-guide filter within the distance the rule header derives, and against the grey
oracle where the two filters coincide; the reason for the feature (an iso-luminant edge); the command lines and the Python
refusals; and the shared rule header (wct_tf_amd/csrc/guided_color_rule.h, what the kernels compile) built for the host under
AddressSanitizer + UBSan as a program of its own."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import guided_color_oracle as oracle
import guided_oracle as grey

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def _rgb(a):
    return np.repeat(np.asarray(a)[..., None], 3, -1).astype(np.uint8)


def _two_greys(h, w):
    """the guide on which the 2^-F quantisation of the covariance shows: neighbouring greys 100 | 102 in alternating columns (a
    window variance near 1 grey level squared) under a 0 / 255 frame in phase with it"""
    xx = np.mgrid[:h, :w][1]
    return _rgb((xx & 1) * 255), _rgb(100 + (xx & 1) * 2)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 4, 16])
def test_vectorised_oracle_is_the_scalar_loop(r):
    """9 x 13: at r = 16 every window is the whole image"""
    s, c = _rand(1, (9, 13, 3)), _rand(2, (9, 13, 3))
    got = oracle.guided_filter(s, c, r, 650)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.guided_filter_loop(s, c, r, 650))
    assert not np.array_equal(got, grey.guided_filter(s, c, r, 650))          # (another filter than the grey one)


def test_oracle_at_the_ends_of_eps_and_on_a_frame_larger_than_its_content():
    s, c = _rand(3, (16, 20, 3)), _rand(4, (9, 13, 3))
    for eps_q in (1, 65025):
        assert np.array_equal(oracle.guided_filter(s, c, 2, eps_q), oracle.guided_filter_loop(s, c, 2, eps_q)), eps_q
    g = oracle.guide(c, 16, 20)
    assert np.array_equal(g[9:, :13], np.broadcast_to(g[8:9, :13], (7, 13, 3))) and (g[9:, 13:] == g[8, 12]).all()
    sb, cb = _rand(5, (3, 16, 20, 3)), _rand(6, (3, 9, 13, 3))            # batched: every frame against its own content
    got = oracle.guided_filter(sb, cb, 3, 650)
    for f in range(3):
        assert np.array_equal(got[f], oracle.guided_filter(sb[f], cb[f], 3, 650))


def test_bitlength():
    v = np.array([1, 2, 3, 4, 255, 256, (1 << 43) - 1, 1 << 43, (1 << 61) + 5], np.int64)
    assert oracle.bitlength(v).tolist() == [int(x).bit_length() for x in v.tolist()]


# ---- the distance from the float64 filter ------------------------------------------------------------------------------------
def test_the_derived_distance_is_the_formula_of_the_header():
    """0.5 (the last rounding) + 2^-13 (b_q) + 3 * 255 * (2^-13 + 2^-35) (a_q and the shift of det) + the 2^-F quantisation of the
    covariances, 255 sqrt(3) h (sqrt(3) + 191.25 / sqrt(eps)) / (eps - 3h) with h = 2^-(F+1): the header's own figures at F = 4"""
    assert oracle.F == 4
    for eps_q, want in ((65025, 0.594), (650, 0.79), (65, 6.0), (1, 2940)):
        assert abs(oracle.distance(eps_q) - want) <= 0.01 * want, (eps_q, oracle.distance(eps_q))
    assert oracle.distance(1, 2) > oracle.distance(1, 4)                  # a coarser F costs


def _distance_cases():
    iso_s, iso_c, _ = oracle.isoluminant_step()
    tg_s, tg_c = _two_greys(24, 40)
    cases = [('noise', _rand(10, (33, 35, 3)), _rand(11, (33, 35, 3)), r, e) for r, e in ((1, 1), (4, 650), (5, 65025), (16, 65))]
    cases += [('isoluminant', iso_s, iso_c, r, e) for r, e in ((4, 65), (8, 650), (1, 1))]
    cases += [('two greys', tg_s, tg_c, r, 1) for r in (1, 4, 16)]
    cases += [('larger frame', _rand(12, (30, 31, 3)), _rand(13, (21, 17, 3)), r, e) for r, e in ((3, 7), (8, 65025))]
    return cases


@pytest.mark.parametrize('name,s,c,r,eps_q', _distance_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_rule_stays_within_its_derived_distance_of_the_float64_filter(name, s, c, r, eps_q):
    err = np.abs(oracle.guided_filter_unclamped(s, c, r, eps_q) - oracle.guided_filter_f64(s, c, r, eps_q)).max()
    print('%s r %d eps_q %d: distance %.4f, derived bound %.4f' % (name, r, eps_q, err, oracle.distance(eps_q)))
    assert err <= oracle.distance(eps_q), err


# ---- exact cases ---------------------------------------------------------------------------------------------------------------
def test_a_constant_frame_comes_back_exactly():
    """every c_ip is 0, so a_q = 0 and b_q = p 2^12"""
    c = _rand(14, (40, 44, 3))
    for v, r, eps_q in ((0, 1, 1), (255, 64, 65025), (77, 5, 650)):
        s = np.full((40, 44, 3), v, np.uint8)
        a_q, b_q, _, _, _ = oracle.coefficients(s, c, r, eps_q)
        assert not a_q.any() and (b_q == v << oracle.SHIFT).all()
        assert np.array_equal(oracle.guided_filter(s, c, r, eps_q), s)


def test_a_flat_guide_gives_the_box_mean_of_the_box_mean():
    s = _rand(15, (40, 44, 3))
    c = np.full((40, 44, 3), (128, 20, 250), np.uint8)
    r = 3
    n = grey.count(40, 44, r).astype(np.float64)
    got = oracle.guided_filter(s, c, r, 650).astype(np.float64)
    for ch in range(3):
        want = grey.box(grey.box(s[..., ch].astype(np.float64), r) / n, r) / n
        assert np.abs(got[..., ch] - want).max() <= 1


@pytest.mark.parametrize('e', [1, 217, 21675])
def test_on_a_grey_content_the_colour_rule_at_three_eps_is_the_grey_rule_at_eps(e):
    """R = G = B: Sigma = sigma^2 1 1^T, and (Sigma + 3 eps U)^-1 kappa has the sum sigma_Ip / (sigma^2 + eps) -- in exact arithmetic
    the colour filter at 3 eps is the grey filter at eps (the grey of a grey pixel is its value: the weights sum to 256).  The two
    rules agree within the sum of their derived distances (0.54 for the grey one)."""
    g = _rgb(_rand(16, (33, 35)))
    s = _rand(17, (33, 35, 3))
    assert np.array_equal(grey.guide(g, 33, 35), g[..., 0])
    for r in (1, 4, 16):
        d = np.abs(oracle.guided_filter_unclamped(s, g, r, 3 * e) - grey.guided_filter_unclamped(s, g, r, e)).max()
        assert d <= oracle.distance(3 * e) + 0.54, (r, d)
        f64 = np.abs(oracle.guided_filter_f64(s, g, r, 3 * e) - grey.guided_filter_f64(s, g, r, e)).max()
        assert f64 < 1e-6, (r, f64)


# ---- the reason for the feature ------------------------------------------------------------------------------------------------
def _step_and_noise(out, step):
    """of a filtered channel: the height of the step between the two columns at the edge, and the sigma of the flat sides (the
    columns at least r = 4 and a margin from the edge)"""
    w = out.shape[1]
    left, right = out[:, :w // 2], out[:, w // 2:]
    kept = right[:, 0].mean() - left[:, -1].mean()
    sigma = np.concatenate([(left[:, :-8] - step[:, :w // 2 - 8]).ravel(), (right[:, 8:] - step[:, w // 2 + 8:]).ravel()]).std()
    return kept, sigma


def test_the_colour_guide_keeps_an_isoluminant_edge_that_the_grey_guide_blurs():
    s, c, step = oracle.isoluminant_step()
    assert set(np.unique(grey.guide(c, 24, 40))) == {100, 102}            # two colours, (nearly) one grey
    _, sigma_in = _step_and_noise(s[..., 0].astype(np.float64), step)
    for f_color, f_grey in ((oracle.guided_filter, grey.guided_filter), (oracle.guided_filter_f64, grey.guided_filter_f64)):
        kept, sigma = _step_and_noise(f_color(s, c, 4, 65).astype(np.float64)[..., 0], step)
        assert kept > 0.9 * 150 and sigma < sigma_in / 5, (kept, sigma, sigma_in)
        kept_grey, _ = _step_and_noise(f_grey(s, c, 4, 65).astype(np.float64)[..., 0], step)
        assert kept_grey < 0.5 * 150, kept_grey


# ---- command lines ---------------------------------------------------------------------------------------------------------
_IMG = ['--relu-targets', 'relu1_1', '--content-path', 'c', '--out-path', 'o', '--synthetic-weights', '1', '--style-path', 's']
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1', '--style-path', 's']


def _check_image(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_guided_args(parser, args)
    return args


def _check_video(argv):
    from wct_tf_amd import stylize_video
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_guided_args(parser, args)
    return args


def test_both_command_lines_take_the_guide_and_have_it_off_by_default(capsys):
    from wct_tf_amd.stylize import guided_of
    for check, argv in ((_check_image, _IMG), (_check_video, _VID)):
        a = check(argv)
        assert a.guided_guide is None and guided_of(a) is None
        assert guided_of(check(argv + ['--guided-radius', '8'])) == (8, 650)                                    # grey, as before
        assert guided_of(check(argv + ['--guided-radius', '8', '--guided-guide', 'grey'])) == (8, 650)
        assert guided_of(check(argv + ['--guided-radius', '8', '--guided-guide', 'color'])) == (8, 650, 'color')
        assert guided_of(check(argv + ['--guided-radius', '4', '--guided-eps', '1e-9', '--guided-guide', 'color', '--passes', '2'])) == (4, 1, 'color')
        for extra in (['--guided-guide', 'color'], ['--guided-guide', 'grey'], ['--guided-guide', 'color', '--guided-radius', '0']):
            with pytest.raises(SystemExit):
                check(argv + extra)                                       # no filter to choose the guide of
            assert '--guided-guide' in capsys.readouterr().err
        for word in ('gray', 'colour', 'rgb', '1'):
            with pytest.raises(SystemExit):
                check(argv + ['--guided-radius', '8', '--guided-guide', word])
            assert '--guided-guide' in capsys.readouterr().err


def test_run_passes_hands_the_guide_on(monkeypatch):
    """one pass: the prediction gets the three-element form; several: the stand-alone op runs once at the end with guide='color'"""
    import argparse
    from wct_tf_amd import ops, stylize
    seen = []
    monkeypatch.setattr(ops, 'guided_filter_np', lambda s, c, r, e, guide='grey', ctx=None: seen.append((r, e, guide)) or oracle.guided_filter(s, c, r, e))
    content, model = _rand(20, (12, 16, 3)), argparse.Namespace(sess=None)
    calls = []

    def predict(img, colors, guided=None):
        calls.append(guided)
        return np.uint8(255 - img)

    ns = lambda **kw: argparse.Namespace(guided_radius=2, guided_eps=0.01, guided_guide='color', content_colors=False, **kw)
    stylize.run_passes(model, content, ns(passes=1), predict)
    assert calls == [(2, 650, 'color')] and not seen
    del calls[:]
    two = stylize.run_passes(model, content, ns(passes=2), predict)
    assert calls == [None, None] and seen == [(2, 650, 'color')]
    assert np.array_equal(two, oracle.guided_filter(content, content, 2, 650))


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_guided, check_guide
    from wct_tf_amd.wct import WCT
    from wct_tf_amd import _lib
    assert check_guided((4, 650)) == (4, 650) and check_guided((4, 650, 'grey')) == (4, 650, 'grey')
    assert check_guided([4, 650, 'color']) == (4, 650, 'color')
    assert (check_guide('grey'), check_guide('color')) == (_lib.GUIDE_GREY, _lib.GUIDE_COLOR)
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (16, 20, 3)), _rand(31, (9, 20, 3))
    for bad in ('colour', 'gray', 1, None, b'color'):
        for call in (lambda: ctx.guided_filter(s, c, 4, 650, guide=bad), lambda: ctx.guided_filter_batch(s[None], c[None], 4, 650, guide=bad),
                     lambda: ctx.guided_filter_batch_dev(None, 16, 20, None, 9, 20, 1, 4, 650, None, guide=bad),
                     lambda: ctx.set_guided_guide(bad), lambda: ctx.stylize(c, s, ['relu1_1'], guided=(4, 650, bad))):
            with pytest.raises(ValueError, match="'grey' or 'color'"):
                call()
    for g, word in (((0, 650, 'color'), 'radius'), ((4, 0, 'color'), 'eps_q'), ((4.5, 650, 'color'), 'integers'),
                    ((4, 650, 'color', 1), 'two integers'), ((4,), 'two integers')):
        with pytest.raises(ValueError, match=word):
            ctx.stylize(c, s, ['relu1_1'], guided=g)
    m = WCT.__new__(WCT)
    m.relu_targets = ['relu1_1']
    for call in (lambda g: m.predict(c, s, guided=g), lambda g: m.predict_frames(c[None], s, guided=g),
                 lambda g: m.predict_mix(c, [s], guided=g), lambda g: m.predict_masked(c, [s], np.zeros((9, 20)), guided=g),
                 lambda g: m.predict_frames_masked(c[None], [s], np.zeros((9, 20)), guided=g)):
        with pytest.raises(ValueError, match="'grey' or 'color'"):
            call((4, 650, 'colour'))
        with pytest.raises(ValueError, match='radius'):
            call((0, 650, 'color'))
    with pytest.raises(ValueError, match='guided is not served in bands'):
        m.predict(c, s, band_rows=16, guided=(4, 650, 'color'))


def test_constants_match_the_headers():
    from wct_tf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    assert int(re.search(r'WCT_GUIDE_GREY\s*=\s*(\d+)', hdr).group(1)) == _lib.GUIDE_GREY == 0
    assert int(re.search(r'WCT_GUIDE_COLOR\s*=\s*(\d+)', hdr).group(1)) == _lib.GUIDE_COLOR == 1
    assert _lib.GUIDES == {'grey': 0, 'color': 1}
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {'wct_guided_filter_guide', 'wct_guided_filter_guide_batch_dev', 'wct_set_guided_guide'} <= bound
    assert 'guided_color.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES
    rule = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'guided_color_rule.h')).read()
    common = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'common.h')).read()
    assert re.search(r'GUIDE_GREY = 0, GUIDE_COLOR = 1', common)
    assert int(re.search(r'WCT_GUIDED_COLOR_F\s+(\d+)', rule).group(1)) == oracle.F
    assert int(re.search(r'WCT_GUIDED_COLOR_DET_BITS\s+(\d+)', rule).group(1)) == oracle.DET_BITS
    assert int(re.search(r'WCT_GUIDED_COLOR_MAX_A\s+(\d+)', rule).group(1)) == oracle.MAX_A
    assert int(re.search(r'WCT_GUIDED_COLOR_MAX_B\s+(\d+)', rule).group(1)) == oracle.MAX_B
    assert '__int128' not in rule.split('#pragma once')[1]


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
def _extremes():
    """full 129 x 129 windows that approach the bounds the header states: 0 / 255 boards and stripes in every channel (the largest
    sums and variances) and in opposite phase between the guide's channels (the largest off-diagonal |V|), at both ends of eps_q;
    the two-greys guide under 0 / 255 stripes and their complement, and a guide that alternates in ONE channel only (one
    eigenvalue of 1 grey level squared against eps_q = 1: a_q towards sigma_p / (2 sqrt(eps_q)) = 63.75 * 2^12)"""
    n = 129
    yy, xx = np.mgrid[:n, :n]
    board, stripes = ((yy + xx) & 1) * 255, (xx & 1) * 255
    opposite = lambda a: np.stack([a, 255 - a, a], -1).astype(np.uint8)
    cases = []
    for pattern in (board, stripes):
        for eps_q in (1, 65025):
            cases.append((_rgb(pattern), _rgb(pattern), 64, eps_q))
            cases.append((_rgb(pattern), opposite(pattern), 64, eps_q))
    two = _rgb(100 + (xx & 1) * 2)
    cases.append((_rgb(stripes), two, 64, 1))
    cases.append((_rgb(255 - stripes), two, 64, 1))
    one = np.stack([100 + (xx & 1) * 2, np.full_like(xx, 100), np.full_like(xx, 100)], -1).astype(np.uint8)
    cases.append((_rgb(stripes), one, 64, 1))
    return cases


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/guided_color_rule_check.cpp includes csrc/guided_color_rule.h -- the functions the kernels call --, forms the 21
    window sums naively in int32 and compares the bytes with the oracle's: a stand-alone program, nothing sanitized is loaded into
    this process.  The signed-overflow check of UBSan on the extremes is the proof of the header's bounds."""
    cases = []
    for seed, (h, w, hc, wc, r, eps_q) in enumerate([(9, 13, 9, 13, 16, 650), (33, 35, 33, 35, 1, 1), (33, 35, 33, 35, 4, 65025),
                                                     (16, 20, 9, 13, 3, 650), (48, 48, 37, 41, 5, 7), (40, 36, 40, 36, 64, 1)]):
        cases.append((_rand(50 + seed, (h, w, 3)), _rand(70 + seed, (hc, wc, 3)), r, eps_q))
    s, c = grey.clamp_case()
    cases.append((s, c, 1, 1))
    cases += _extremes()
    blob = struct.pack('<i', len(cases))
    for s, c, r, eps_q in cases:
        blob += struct.pack('<6i', s.shape[0], s.shape[1], c.shape[0], c.shape[1], r, eps_q)
        blob += s.tobytes() + c.tobytes() + oracle.guided_filter(s, c, r, eps_q).tobytes()
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'guided_color_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'guided_color_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout
    print(out.stdout)
    max_a = int(out.stdout.split('max |a_q| ')[1].split(',')[0])
    max_b = int(out.stdout.split('max |b_q| ')[1].split(',')[0])
    bits = int(out.stdout.split('det bits ')[1].split()[0])
    # the one-channel guide reached the neighbourhood of the a_q bound, the full-range boards that of det; all under the header's
    assert 250000 < max_a < oracle.MAX_A and max_b < oracle.MAX_B and 60 <= bits <= 61, out.stdout
