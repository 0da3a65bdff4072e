"""Texture synthesis without a GPU: the NumPy oracle of the noise rule (tests/texture_oracle.py) against a byte-by-byte loop and
the known answers of the rule, the smoothing step and its borders, the statistics the rule has to meet, the command line, the
Python refusals, and the shared rule header (wct_tf_amd/csrc/noise_rule.h, what the kernel compiles) built for the host under
AddressSanitizer + UBSan as a program of its own."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import texture_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


# ---- the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('smooth', [False, True], ids=['raw', 'smooth'])
@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7)])
def test_vectorised_oracle_is_the_scalar_loop(h, w, smooth):
    for seed, sample in ((0, 0), (42, 3), (0xFFFFFFFF, 31)):
        got = oracle.noise(h, w, seed, sample, smooth)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        assert np.array_equal(got, oracle.noise_loop(h, w, seed, sample, smooth)), (seed, sample)


def test_known_answers():
    """seed 42, a 2 x 2 image, bytes in memory order"""
    assert oracle.noise(2, 2, 42, 0).reshape(-1).tolist() == [202, 213, 66, 120, 111, 31, 40, 93, 133, 193, 72, 147]
    assert oracle.noise(2, 2, 42, 3).reshape(-1).tolist() == [209, 57, 75, 233, 156, 132, 156, 171, 230, 87, 208, 106]
    assert oracle.noise_loop(2, 2, 42, 0).reshape(-1).tolist() == [202, 213, 66, 120, 111, 31, 40, 93, 133, 193, 72, 147]
    assert np.array_equal(oracle.noise_batch(2, 2, 4, 42)[3], oracle.noise(2, 2, 42, 3))


def test_smooth_keeps_a_constant_image():
    for v in (0, 1, 127, 254, 255):
        img = np.full((6, 5, 3), v, np.uint8)
        assert np.array_equal(oracle.smooth(img), img), v           # the weights sum to 256 in each direction


def test_smooth_at_both_borders_of_one_pixel_axes():
    """sym(-1) = 0 and sym(n) = n - 1: an axis of one pixel reads that pixel three times, so it smooths along the other axis only"""
    taps = np.array(oracle.TAPS, np.int64)
    row = oracle.raw(1, 9, 5, 0)
    p = np.pad(row.astype(np.int64), ((0, 0), (1, 1), (0, 0)), mode='symmetric')
    along_x = sum(taps[d] * p[:, d:d + 9] for d in range(3))
    assert np.array_equal(oracle.smooth(row), ((256 * along_x + 32768) >> 16).astype(np.uint8))
    col = oracle.raw(9, 1, 5, 1)
    assert np.array_equal(oracle.smooth(col), oracle.smooth(col.transpose(1, 0, 2)).transpose(1, 0, 2))
    one = oracle.raw(1, 1, 5, 2)
    assert np.array_equal(oracle.smooth(one), one)
    for h, w in ((1, 9), (9, 1), (1, 1), (2, 2)):
        assert np.array_equal(oracle.noise(h, w, 5, 0, True), oracle.noise_loop(h, w, 5, 0, True))
    # the border rows of a larger image repeat their own pixel, not the one two rows in (tf.pad REFLECT would)
    img = oracle.raw(6, 7, 9, 0)
    assert np.array_equal(oracle.smooth(img)[0], oracle.smooth(np.concatenate([img[:1], img]))[1])
    assert np.array_equal(oracle.smooth(img)[:, -1], oracle.smooth(np.concatenate([img, img[:, -1:]], axis=1))[:, -2])


SEEDS = [0, 1, 7, 12345, 0xFFFFFFFF]
SAMPLES = [0, 1, 31]


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize('sample', SAMPLES)
@pytest.mark.parametrize('seed', SEEDS)
def test_raw_bytes_are_uniform_and_uncorrelated(seed, sample):
    """64 x 64 x 3 = 12288 bytes: the chi-square of the byte histogram has 255 degrees of freedom (mean 255, sd 22.6) -- required
    <= 350, about four sd; the lag-1 correlations along x, along y and across channels required < 0.05 (1 / sqrt(12288) = 0.009
    is one sd).  A condition on the rule: the prototype gives 208 .. 307 and |r| < 0.03 on these fifteen cases."""
    img = oracle.noise(64, 64, seed, sample)
    hist = np.bincount(img.ravel(), minlength=256).astype(np.float64)
    expected = img.size / 256.
    chi2 = float(((hist - expected) ** 2 / expected).sum())
    rx, ry, rc = _corr(img[:, :-1], img[:, 1:]), _corr(img[:-1], img[1:]), _corr(img[..., :-1], img[..., 1:])
    print('seed %d sample %d: chi2 %.1f, lag-1 r along x %.4f, y %.4f, channels %.4f' % (seed, sample, chi2, rx, ry, rc))
    assert chi2 <= 350, chi2
    assert abs(rx) < 0.05 and abs(ry) < 0.05 and abs(rc) < 0.05, (rx, ry, rc)


def test_samples_and_seeds_give_different_images():
    """independent uniform bytes differ with probability 255 / 256 = 99.6 %: more than 95 % is required"""
    a = oracle.noise(40, 56, 7, 0)
    other_sample, other_seed = oracle.noise(40, 56, 7, 1), oracle.noise(40, 56, 8, 0)
    assert (a != other_sample).mean() > 0.95, (a != other_sample).mean()
    assert (a != other_seed).mean() > 0.95, (a != other_seed).mean()
    assert np.array_equal(a, oracle.noise(40, 56, 7, 0))            # and the same (seed, sample) the same image


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_noise_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/noise_rule_check.cpp includes csrc/noise_rule.h -- the functions the kernel calls -- and reproduces every byte
    of the oracle's images: a stand-alone program, nothing sanitized is loaded into this process."""
    cases = [(h, w, seed, sample, smooth)
             for (h, w) in ((1, 1), (2, 3), (5, 7), (1, 9), (9, 1), (17, 33))
             for (seed, sample) in ((0, 0), (42, 3), (0xFFFFFFFF, 0xFFFFFFFF), (12345, 31))
             for smooth in (0, 1)]
    blob = struct.pack('<i', len(cases))
    total = 0
    for h, w, seed, sample, smooth in cases:
        img = oracle.noise(h, w, seed, sample, bool(smooth))
        blob += struct.pack('<iiIIi', h, w, seed, sample, smooth) + img.tobytes()
        total += img.size
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'noise_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'noise_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases, %d bytes' % (len(cases), total) in out.stdout


# ---- the command line ---------------------------------------------------------------------------------------------------------
_BASE = ['--relu-targets', 'relu1_1', '--out-path', 'o', '--synthetic-weights', '1']


def _check(argv):
    from wct_tf_amd import texture
    parser = texture.build_parser()
    args = parser.parse_args(argv)
    texture.check_texture_args(parser, args)
    return args


def test_cli_defaults_and_flags():
    from wct_tf_amd import texture
    flags = {a for act in texture.build_parser()._actions for a in act.option_strings}
    for f in ['--checkpoints', '--relu-targets', '--vgg-path', '--synthetic-weights', '--wct-mode', '--device', '--style-size',
              '--crop-size', '--alpha', '--adain', '--out-path', '--style-path', '--size', '--samples', '--seed', '--passes',
              '--noise-smooth', '--batch', '--interp-styles', '--interp-weights']:
        assert f in flags, f
    assert '--content-path' not in flags and '--swap5' not in flags          # a texture has no content
    a = _check(_BASE + ['--style-path', 's.png'])
    assert (a.samples, a.seed, a.passes, a.noise_smooth, a.alpha, a.adain, a.wct_mode) == (1, 0, 3, False, 1, False, 'tf')
    assert len(a.size) == 2 and 1 <= a.batch <= 32 and a.interp_styles is None
    a = _check(_BASE + ['--interp-styles', 'a.png', 'b.png', '--interp-weights', '1', '3', '--size', '40', '56', '--samples', '4',
                        '--seed', '9', '--passes', '16', '--noise-smooth', '--batch', '32'])
    assert a.size == [40, 56] and (a.samples, a.seed, a.passes, a.noise_smooth, a.batch) == (4, 9, 16, True, 32)
    assert a.interp_weights == [1.0, 3.0] and a.style_path is None


@pytest.mark.parametrize('argv,word', [
    (['--interp-styles', 'a', 'b', '--style-path', 's'], 'replaces --style-path'),
    (['--interp-styles', 'a', 'b', '--interp-weights', '1'], '1 values for 2'),
    (['--style-path', 's', '--interp-weights', '1'], 'needs --interp-styles'),
    (['--style-path', 's', '--passes', '0'], '--passes'),
    (['--style-path', 's', '--passes', '17'], '--passes'),
    (['--style-path', 's', '--batch', '33'], '--batch'),
    (['--style-path', 's', '--batch', '0'], '--batch'),
    (['--style-path', 's', '--samples', '0'], '--samples'),
    (['--style-path', 's', '--size', '0', '8'], '--size'),
    (['--style-path', 's', '--seed', '-1'], '--seed'),
    ([], '--style-path or --interp-styles'),
], ids=lambda v: ' '.join(v) if isinstance(v, list) else None)
def test_cli_refusals(capsys, argv, word):
    with pytest.raises(SystemExit):
        _check(_BASE + argv)
    assert word in capsys.readouterr().err


def test_cli_output_names():
    from wct_tf_amd.texture import texture_name
    assert texture_name(['styles/brick.jpg'], 0, 0) == 'brick_texture_s0_0.png'
    assert texture_name(['/x/brick.jpg'], 12345, 31) == 'brick_texture_s12345_31.png'
    assert texture_name(['a.png', 'dir/b.jpeg'], 7, 2) == 'a+b_texture_s7_2.png'


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    import wct_tf_amd
    from wct_tf_amd.context import Context
    from wct_tf_amd.wct import WCT, texture_plan
    assert wct_tf_amd.texture_noise_np is wct_tf_amd.ops.texture_noise_np and 'texture_noise_np' in wct_tf_amd.__all__
    model = WCT.__new__(WCT)                             # no context behind it: a refusal that reached the library would fail loudly
    style = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match='passes'):
        model.synthesize(style, (16, 16), passes=0)
    with pytest.raises(ValueError, match='passes'):
        model.synthesize(style, (16, 16), passes=17)
    with pytest.raises(ValueError, match='empty'):
        model.synthesize(style, (0, 16))
    with pytest.raises(ValueError, match=r'\(H, W\)'):
        model.synthesize(style, 16)
    with pytest.raises(ValueError, match='list of styles'):
        model.synthesize(style, (16, 16), weights=[1, 3])
    with pytest.raises(ValueError, match='swap5'):
        model.synthesize(style, (16, 16), swap5=True)
    with pytest.raises(ValueError, match='weights'):
        model.synthesize([style, style], (16, 16), weights=[1])
    with pytest.raises(ValueError, match='seeds'):
        model.synthesize(style, (16, 16), seeds=0)
    with pytest.raises(ValueError, match='uint32'):
        model.synthesize(style, (16, 16), seed=1 << 32)
    with pytest.raises(ValueError, match='uint32'):
        model.synthesize(style, (16, 16), seeds=[0, -1])
    ctx = Context.__new__(Context)
    with pytest.raises(ValueError, match='empty'):
        ctx.texture_noise(0, 4, 1)
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.texture_noise_batch_dev(4, 4, 33, 0, 0, False, None)
    with pytest.raises(ValueError, match='1 .. 16'):
        ctx.texture_prepared_batch(4, 4, 1, 0, 0, None, ['relu1_1'], passes=0)
    # the plan of the device calls: runs of consecutive sample indices, at most `batch` each
    assert texture_plan(style, (40, 56), seeds=5, batch=2)[2:4] == ([0, 1, 2, 3, 4], [(0, 2), (2, 2), (4, 1)])
    assert texture_plan(style, (40, 56), seeds=[0, 1, 5])[3] == [(0, 2), (5, 1)]
    assert texture_plan(style, (40, 56), seeds=[3, 2, 2, 3, 4], batch=99)[3] == [(3, 1), (2, 1), (2, 3)]
    assert texture_plan(style, (40, 56), seeds=40, batch=99)[3] == [(0, 32), (32, 8)]


def test_constants_and_bounds_match_the_header():
    from wct_tf_amd import _lib
    from wct_tf_amd import build
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    for name, value in (('ADAIN', _lib.FLAG_ADAIN), ('MODE_NP', _lib.FLAG_MODE_NP), ('SWAP5', _lib.FLAG_SWAP5),
                        ('STYLE_SHARED', _lib.FLAG_STYLE_SHARED), ('IMAGES_F32', _lib.FLAG_IMAGES_F32),
                        ('CONTENT_COLORS', _lib.FLAG_CONTENT_COLORS)):
        assert int(re.search(r'WCT_FLAG_%s\s*=\s*(\d+)' % name, hdr).group(1)) == value, name
    section = hdr[hdr.index('texture synthesis'):hdr.index('decoder training')]
    assert 'B outside 1 .. %d' % _lib.BATCH_MAX in section and 'passes outside 1 .. %d' % _lib.PASSES_MAX in section
    assert (_lib.BATCH_MAX, _lib.PASSES_MAX) == (32, 16)
    for call in ('wct_texture_noise_batch_dev', 'wct_texture_noise', 'wct_texture_size', 'wct_texture_prepared_batch_dev',
                 'wct_texture_prepared'):
        assert re.search(r'%s \((webcam\.py:191-192, stylize\.py:95-97, Li et al\. sec\. 4\.3|the same lines)' % call, section), call
    assert '0x85EBCA6B' in section and '0xC2B2AE35' in section and '0x9E3779B9' in section and '27 202 27' in section
    assert 'noise.hip' in build.SOURCES
