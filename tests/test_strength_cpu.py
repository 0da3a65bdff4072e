"""Strength maps without a GPU: the NumPy oracle's ends and clamp, the shared rule header (wct_tf_amd/csrc/strength_rule.h, what
the apply kernels compile) built for the host under AddressSanitizer + UBSan as a program of its own and compared bit for bit
with NumPy, the command lines, the Python refusals and the binding."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import strength_oracle as so

CLANG = '/opt/rocm/lib/llvm/bin/clang++'
F = np.float32


def _features(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F) * F(3)


def test_the_two_ends_of_the_rule():
    y, x = _features(1, (5, 7, 8)), _features(2, (5, 7, 8))
    for alpha in (1.0, 0.8, 0.3):
        assert np.array_equal(so.blend(y, x, so.strength(alpha, np.zeros((5, 7), np.uint8))), x)      # v = 0: the content
    assert np.array_equal(so.blend(y, x, so.strength(1.0, np.full((5, 7), 255, np.uint8))), y)          # v = 255, alpha = 1: y
    a = so.strength(0.8, np.arange(256, dtype=np.uint8))
    assert a.dtype == F and a[0] == 0 and a[255] == F(0.8) and np.all(np.diff(a) > 0)
    # float32 with one rounding per operation: not the float64 value rounded once
    v = np.arange(256)
    assert np.array_equal(a, F(0.8) * (v.astype(F) / F(255)))
    assert np.any(a != F(0.8 * v / 255.0))


def test_transform_ends_against_the_reference_transforms():
    import oracle
    fc, fs = np.abs(_features(3, (6, 9, 32))), np.abs(_features(4, (7, 8, 32)))
    for kind, full in (('tf', lambda: oracle.wct_tf(fc, fs, 1.0)[0]), ('np', lambda: oracle.wct_np(fc, fs, 1.0)[0]),
                       ('adain', lambda: oracle.adain(fc, fs, 1.0)[0])):
        zero, ones = np.zeros((24, 36), np.uint8), np.full((24, 36), 255, np.uint8)
        assert np.array_equal(so.transform(fc, fs, zero, 4, 0.8, kind, f64=False), fc)
        assert np.array_equal(so.transform(fc, fs, ones, 4, 1.0, kind, f64=False), full())
        half = zero.copy()
        half[:, 20:] = 255                                           # feature columns 5 .. 8 read map column >= 20
        got = so.transform(fc, fs, half, 4, 1.0, kind, f64=False)
        assert np.array_equal(got[:, :5], fc[:, :5]) and np.array_equal(got[:, 5:], full()[:, 5:])


def test_the_clamp_at_a_map_smaller_than_the_feature_map_times_the_stride():
    smap = np.arange(7 * 10, dtype=np.uint8).reshape(7, 10)           # 3 x 4 feature pixels at stride 4 reach row 8, column 12
    got = so.level_bytes(smap, 3, 4, 4)
    assert np.array_equal(got, smap[np.ix_([0, 4, 6], [0, 4, 8, 9])])
    assert np.array_equal(so.level_strength(smap, 3, 4, 4, 0.5), F(0.5) * (got.astype(F) / F(255)))
    assert np.array_equal(so.level_bytes(smap, 7, 10, 1), smap)


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan_is_numpy_bit_for_bit(tmp_path):
    """tests/emul/strength_rule_check.cpp includes csrc/strength_rule.h -- the functions the kernels call -- and compares them
    with NumPy float32 on all 256 map values x several alphas x random x, y with +-0, denormals and large magnitudes: a
    stand-alone program, nothing sanitized is loaded into this process."""
    rng = np.random.default_rng(50)
    alphas = np.array([1.0, 0.8, 0.6, 0.5, 1 / 3, 0.1, 0.0], F)
    special = np.array([0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-38, -1e-45, 1e30, 65504.0], F)
    per = 24
    al = np.repeat(alphas, 256 * per)
    v = np.tile(np.repeat(np.arange(256, dtype=np.uint32), per), len(alphas))
    n = len(al)
    y = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 6, n)).astype(F)
    x = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 6, n)).astype(F)
    y[::per], x[1::per] = rng.choice(special, len(y[::per])), rng.choice(special, len(x[1::per]))
    y[2::per], x[2::per] = rng.choice(special, len(y[2::per])), rng.choice(special, len(x[2::per]))
    with np.errstate(over='ignore', invalid='ignore'):
        a = al * (v.astype(F) / F(255))                                # (so.strength with an alpha per record)
        out = so.blend(y, x, a)
    assert a.dtype == F and out.dtype == F
    rec = np.empty(n, dtype=[('alpha', '<f4'), ('v', '<u4'), ('y', '<f4'), ('x', '<f4'), ('a', '<f4'), ('out', '<f4')])
    rec['alpha'], rec['v'], rec['y'], rec['x'], rec['a'], rec['out'] = al, v, y, x, a, out
    idx = []
    for hm, wm, s in ((70, 86, 4), (7, 10, 4), (64, 64, 1), (9, 9, 16), (1, 1, 2)):
        for i in range(0, 24, 3):
            for j in range(0, 24, 5):
                idx.append((i, j, s, hm, wm, min(i * s, hm - 1), min(j * s, wm - 1)))
    idx = np.array(idx, '<i4')
    data = tmp_path / 'cases.bin'
    data.write_bytes(struct.pack('<i', n) + rec.tobytes() + struct.pack('<i', len(idx)) + idx.tobytes())
    exe = str(tmp_path / 'strength_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O2', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'strength_rule_check.cpp')])
    res = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert 'all checks passed: %d blends, %d indices' % (n, len(idx)) in res.stdout


# ---- command lines ----------------------------------------------------------------------------------------------------
_IMG = ['--relu-targets', 'relu1_1', '--content-path', 'c', '--out-path', 'o', '--synthetic-weights', '1']
_VID = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--synthetic-weights', '1']


def _check_image(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_interp_args(parser, args)
    stylize.check_mask_args(parser, args)
    stylize.check_color_args(parser, args)
    stylize.check_band_args(parser, args)
    stylize.check_alpha_map_args(parser, args)
    return parser, args


def _check_video(argv):
    from wct_tf_amd import stylize_video
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_mask_args(parser, args)
    stylize_video.check_warm_args(parser, args)
    stylize_video.check_color_args(parser, args)
    stylize_video.check_resize_args(parser, args)
    stylize_video.check_alpha_map_args(parser, args)
    return args


def test_alpha_map_goes_with_the_options_the_issue_names():
    assert _check_image(_IMG + ['--style-path', 's'])[1].alpha_map is None
    a = _check_image(_IMG + ['--style-path', 's', '--alpha-map', 'm.png', '--alpha', '0.7', '--adain', '--content-colors'])[1]
    assert a.alpha_map == 'm.png' and a.adain and a.content_colors
    assert _check_image(_IMG + ['--style-path', 's', '--alpha-map', 'm.png', '--wct-mode', 'np'])[1].wct_mode == 'np'
    v = _check_video(_VID + ['--style-path', 's', '--alpha-map', 'maps', '--warm-start', '--content-colors', '--device-resize',
                             '--content-size', '64'])
    assert v.alpha_map == 'maps' and v.warm_start and v.device_resize
    assert _check_video(_VID + ['--style-path', 's', '--alpha-map', 'm.png', '--adain', '--wct-mode', 'np']).adain


@pytest.mark.parametrize('extra,word', [
    (['--style-path', 's', '--swap5'], '--swap5'),
    (['--interp-styles', 'a', 'b'], '--interp-styles'),
    (['--mask-path', 'm', '--mask-styles', 'a', 'b'], '--mask-path'),
    (['--style-path', 's', '--keep-colors'], '--keep-colors'),
    (['--style-path', 's', '--passes', '2'], '--passes > 1'),
    (['--style-path', 's', '--band-rows', '64'], '--alpha-map'),
])
def test_image_command_line_refusals(capsys, extra, word):
    with pytest.raises(SystemExit):
        _check_image(_IMG + ['--alpha-map', 'm.png'] + extra)
    assert word in capsys.readouterr().err


@pytest.mark.parametrize('extra,word', [
    (['--style-path', 's', '--swap5'], '--swap5'),
    (['--mask-path', 'm', '--mask-styles', 'a', 'b'], '--mask-path'),
    (['--style-path', 's', '--keep-colors'], '--keep-colors'),
    (['--style-path', 's', '--passes', '3'], '--passes > 1'),
])
def test_video_command_line_refusals(capsys, extra, word):
    with pytest.raises(SystemExit):
        _check_video(_VID + ['--alpha-map', 'm.png'] + extra)
    assert word in capsys.readouterr().err


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_a_banded_content_is_a_parser_error(lib, capsys):
    from wct_tf_amd import stylize
    parser, args = _check_image(['--relu-targets', 'relu2_1', 'relu1_1', '--content-path', 'c', '--out-path', 'o',
                                 '--synthetic-weights', '1', '--style-path', 's', '--alpha-map', 'm.png'])
    stylize.check_content_fits(parser, args, np.empty((64, 64, 3), np.uint8), 'small.png')            # fits: no error
    with pytest.raises(SystemExit):
        stylize.check_content_fits(parser, args, np.empty((3000, 3000, 3), np.uint8), 'big.png')       # 9 MP with relu1_1
    err = capsys.readouterr().err
    assert 'big.png' in err and '--alpha-map' in err and 'bands' in err


def test_cli_maps_are_pillow_bilinear_and_matched_in_sorted_order(tmp_path):
    from PIL import Image
    from wct_tf_amd import stylize, stylize_video
    grey = np.random.default_rng(3).integers(0, 256, (20, 30)).astype(np.uint8)
    assert np.array_equal(stylize.strength_map(grey, (20, 30)), grey)
    want = np.array(Image.fromarray(grey).resize((45, 33), Image.BILINEAR))
    got = stylize.strength_map(grey, (33, 45, 3))
    assert got.dtype == np.uint8 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, want)
    d = tmp_path / 'maps'
    d.mkdir()
    for i in (10, 2, 1):
        Image.fromarray(grey).save(str(d / ('m_%d.png' % i)))
    frames = ['f1', 'f2', 'f3']
    assert [os.path.basename(p) for p in stylize_video.match_masks(str(d), frames, 'strength maps')] == ['m_1.png', 'm_2.png', 'm_10.png']
    assert stylize_video.match_masks(str(d / 'm_1.png'), frames) == [str(d / 'm_1.png')] * 3
    with pytest.raises(ValueError, match='3 strength maps'):
        stylize_video.match_masks(str(d), frames[:2], 'strength maps')


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu(lib):
    from wct_tf_amd.context import Context
    from wct_tf_amd.wct import WCT
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    c = np.zeros((16, 20, 3), np.uint8)
    good = np.zeros((16, 20), np.uint8)
    for bad, word in ((np.zeros((16, 21), np.uint8), 'shape'), (np.zeros((8, 10), np.uint8), 'shape'), (good[None], 'shape'),
                      (good.astype(np.float32), 'uint8'), (good.astype(np.int32), 'uint8'), (good > 0, 'uint8')):
        with pytest.raises(ValueError, match=word):
            ctx.stylize_prepared_strength(c, None, bad, ['relu1_1'])
        if bad.ndim == 2:
            with pytest.raises(ValueError, match=word):
                ctx.stylize_prepared_strength_batch(c[None], None, bad[None], ['relu1_1'])
    with pytest.raises(ValueError, match='2 strength maps for 3 frames'):
        ctx.stylize_prepared_strength_batch(np.stack([c] * 3), None, np.stack([good] * 2), ['relu1_1'])
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.stylize_prepared_strength_batch(np.zeros((33, 4, 4, 3), np.uint8), None, np.zeros((4, 4), np.uint8), ['relu1_1'])
    with pytest.raises(ValueError, match='shape'):      # with resize the maps are given at the resized size
        ctx.stylize_prepared_strength_batch(c[None], None, good, ['relu1_1'], resize=(8, 10))
    f = np.zeros((12, 64), np.float32)
    with pytest.raises(ValueError, match='uint8'):
        ctx.transform_strength(f, f, np.zeros((6, 8)), 3, 4, 2, 0.8, 1)
    with pytest.raises(ValueError, match='feature map'):
        ctx.transform_strength(f, f, np.zeros((6, 8), np.uint8), 3, 5, 2, 0.8, 1)
    with pytest.raises(ValueError, match='feature map'):
        ctx.adain_strength(f, f, np.zeros((6, 8), np.uint8), 3, 4, 0, 0.8)
    model = WCT.__new__(WCT)
    model.relu_targets = ['relu1_1']
    with pytest.raises(ValueError, match='shape'):
        model.predict(c, c, strength=np.zeros((16, 21), np.uint8))
    with pytest.raises(ValueError, match='uint8'):
        model.predict(c, c, strength=good.astype(np.float64))
    with pytest.raises(ValueError, match='swap5'):
        model.predict(c, c, strength=good, swap5=True)
    with pytest.raises(ValueError, match='band_rows'):
        model.predict(c, c, strength=good, band_rows=16)
    with pytest.raises(ValueError, match='limit of one launch'):
        model.predict(np.empty((3000, 3000, 3), np.uint8), c, strength=np.empty((3000, 3000), np.uint8))
    with pytest.raises(ValueError, match='shape'):
        model.predict_frames(c[None], c, strengths=np.zeros((1, 16, 21), np.uint8))
    with pytest.raises(ValueError, match='wrap'):
        model.predict_frames(c[None], c, strengths=good, wrap=True)
    with pytest.raises(ValueError, match='PreparedStyle'):
        model.predict_frames(c[None], c, strengths=good, warm=object())


def test_the_new_symbols_are_bound_and_exported(lib):
    import ctypes as C
    from wct_tf_amd import _lib
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    want = {'wct_transform_strength': 17, 'wct_adain_strength': 15, 'wct_stylize_prepared_strength': 11,
            'wct_stylize_prepared_strength_batch_dev': 12, 'wct_stylize_prepared_strength_batch_dev_warm': 13}
    for name, nargs in want.items():
        res, args = sig[name]
        assert res is C.c_int and len(args) == nargs, name
        assert hasattr(lib, name)
    t = sig['wct_transform_strength'][1]
    assert t[5] is _lib._U8 and t[12] is C.c_float and t[-1] is _lib._I        # the map, alpha, the sweeps
    b = sig['wct_stylize_prepared_strength_batch_dev'][1]
    assert b[5] is _lib._P and b[6] is _lib._P and b[-2] is C.c_uint              # device maps, the handle, the flags
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    for name in want:
        assert name + '(' in hdr
    # the argument type of the apply kernel and the launchers' map are where the issue puts them
    stages = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'wct_stages.h')).read()
    assert 'struct ApplyMapArgs : ApplyArgs' in stages
    assert 'strength_rule.h' in open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'wct.hip')).read()
