"""Luminance-only colour preservation without a GPU: the NumPy oracle of the rule against a naive loop, the four properties
the rule was chosen for, the command lines, the Python refusals, and the shared rule header (wct_tf_amd/csrc/colors_rule.h,
what the kernels compile) built for the host under AddressSanitizer + UBSan as a program of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import colors_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _rand(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint8)


def test_vectorised_oracle_is_the_scalar_loop():
    s, c = _rand(1, (48, 48, 3)), _rand(2, (37, 41, 3))
    got = oracle.content_colors(s, c)
    assert got.dtype == np.uint8 and got.shape == s.shape
    assert np.array_equal(got, oracle.content_colors_loop(s, c))
    raw = oracle.content_colors_unclamped(s, c)
    clipped = ((raw < 0) | (raw > 255)).any(-1).mean()
    assert 0.2 < clipped < 0.5, clipped               # full-range noise: about a third of the pixels exercise the clamp


def test_clamped_rows_and_columns_take_the_last_content_pixel():
    s, c = _rand(3, (16, 20, 3)), _rand(4, (9, 13, 3))
    p = oracle.clamped_content(c, 16, 20)
    assert np.array_equal(p[:9, :13], c)
    assert np.array_equal(p[9:, :13], np.broadcast_to(c[8:9], (7, 13, 3)))
    assert np.array_equal(p[:9, 13:], np.broadcast_to(c[:, 12:13], (9, 7, 3)))
    assert np.array_equal(p[9:, 13:], np.broadcast_to(c[8, 12], (7, 7, 3)))
    # batched: every frame against its own content
    sb, cb = _rand(5, (3, 16, 20, 3)), _rand(6, (3, 9, 13, 3))
    got = oracle.content_colors(sb, cb)
    for f in range(3):
        assert np.array_equal(got[f], oracle.content_colors(sb[f], cb[f]))


def test_identity_a_frame_with_its_own_colours_is_unchanged():
    c = _rand(7, (40, 44, 3))
    assert np.array_equal(oracle.content_colors(c, c), c)


def test_grey_content_gives_a_grey_frame_with_the_stylized_luminance():
    s = _rand(8, (40, 44, 3))
    grey = np.repeat(_rand(9, (40, 44, 1)), 3, axis=2)
    out = oracle.content_colors(s, grey)
    want = ((oracle.luma256(s) + 128) >> 8).astype(np.uint8)         # <= (256 * 255 + 128) >> 8 = 255: no clamp
    for ch in range(3):
        assert np.array_equal(out[..., ch], want)


def test_mid_range_images_never_clip_and_keep_chrominance_and_luminance():
    s, c = _rand(10, (48, 48, 3), 96, 160), _rand(11, (37, 41, 3), 96, 160)
    raw = oracle.content_colors_unclamped(s, c)
    assert raw.min() >= 0 and raw.max() <= 255                      # no channel clipped: the checks below leave out no pixel
    out = oracle.content_colors(s, c).astype(np.int32)
    p = oracle.clamped_content(c, 48, 48).astype(np.int32)
    assert np.array_equal(out[..., 0] - out[..., 1], p[..., 0] - p[..., 1])     # U, V: the content's
    assert np.array_equal(out[..., 2] - out[..., 1], p[..., 2] - p[..., 1])
    assert np.abs(oracle.luma256(out) - oracle.luma256(s)).max() <= 128          # Y: the stylized frame's, to half a level


def test_quantise_is_the_chain_output_rule():
    x = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, 254.999 / 255, 1 / 255, 127 / 255], np.float32)
    assert oracle.quantise(x).tolist() == [0, 0, 0, 127, 255, 255, int(np.float32(254.999 / 255) * np.float32(255)),
                                           int(np.float32(1 / 255) * np.float32(255)), int(np.float32(127 / 255) * np.float32(255))]
    # the uint8 levels survive the chain's own round trip (k / 255 in float64, cast to float32, times 255.f, truncated): the
    # fused kernel still reads the content BYTES -- one byte per sample instead of four, and no reliance on this
    k = np.arange(256)
    assert np.array_equal(oracle.quantise((k / 255.).astype(np.float32)), k)


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
    return args


def _check_video(argv):
    from wct_tf_amd import stylize_video
    parser = stylize_video.build_parser()
    args = parser.parse_args(argv)
    stylize_video.check_mask_args(parser, args)
    stylize_video.check_warm_args(parser, args)
    stylize_video.check_color_args(parser, args)
    return args


def test_both_command_lines_have_the_flag_off_by_default():
    assert _check_image(_IMG + ['--style-path', 's']).content_colors is False
    assert _check_video(_VID + ['--style-path', 's']).content_colors is False
    assert _check_image(_IMG + ['--style-path', 's', '--content-colors']).content_colors is True
    assert _check_video(_VID + ['--style-path', 's', '--content-colors']).content_colors is True


def test_flag_is_refused_with_keep_colors(capsys):
    for check, argv in ((_check_image, _IMG), (_check_video, _VID)):
        with pytest.raises(SystemExit):
            check(argv + ['--style-path', 's', '--content-colors', '--keep-colors'])
        assert 'alternatives' in capsys.readouterr().err


def test_flag_combines_with_masks_warm_start_mixes_and_prepared_styles():
    from wct_tf_amd import stylize
    a = _check_image(_IMG + ['--content-colors', '--mask-path', 'm.png', '--mask-styles', 'a', 'b'])
    assert a.content_colors and stylize.can_prepare(a)                # prepared styles stay on
    a = _check_image(_IMG + ['--content-colors', '--interp-styles', 'a', 'b', '--interp-weights', '1', '3'])
    assert a.content_colors and stylize.can_prepare(a)
    a = _check_image(_IMG + ['--content-colors', '--style-path', 's', '--swap5', '--concat', '--gpus', '2', '--passes', '2'])
    assert a.content_colors and a.swap5 and a.concat and a.gpus == 2
    a = _check_image(_IMG + ['--content-colors', '--style-path', 's', '--adain'])
    assert a.content_colors and a.adain
    assert _check_video(_VID + ['--content-colors', '--style-path', 's', '--warm-start']).warm_start
    assert _check_video(_VID + ['--content-colors', '--mask-path', 'm', '--mask-styles', 'a', 'b']).mask_path == 'm'


def test_several_passes_with_a_strided_style_swap_are_refused(capsys):
    for check, argv in ((_check_image, _IMG), (_check_video, _VID)):
        with pytest.raises(SystemExit):
            check(argv + ['--style-path', 's', '--content-colors', '--passes', '2', '--swap5', '--ss-stride', '2'])
        assert '--ss-stride 1' in capsys.readouterr().err


def test_run_passes_fuses_one_pass_and_applies_the_op_once_after_several(monkeypatch):
    """the routing of stylize.run_passes, with a stand-in for the prediction and the oracle for the op"""
    import argparse
    from wct_tf_amd import ops, stylize
    monkeypatch.setattr(ops, 'content_colors_np', lambda s, c, ctx=None: oracle.content_colors(s, c))
    content, model = _rand(20, (12, 16, 3)), argparse.Namespace(sess=None)
    calls = []

    def predict(img, colors):
        calls.append(colors)
        out = np.uint8(255 - img)
        return oracle.content_colors(out, img) if colors else out

    one = stylize.run_passes(model, content, argparse.Namespace(passes=1, content_colors=True), predict)
    assert calls == [True] and np.array_equal(one, oracle.content_colors(np.uint8(255 - content), content))
    del calls[:]
    two = stylize.run_passes(model, content, argparse.Namespace(passes=2, content_colors=True), predict)
    assert calls == [False, False] and np.array_equal(two, oracle.content_colors(content, content))     # 255 - (255 - x) = x
    del calls[:]
    plain = stylize.run_passes(model, content, argparse.Namespace(passes=2, content_colors=False), predict)
    assert calls == [False, False] and np.array_equal(plain, content)


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context
    import wct_tf_amd
    assert wct_tf_amd.content_colors_np is wct_tf_amd.ops.content_colors_np and 'content_colors_np' in wct_tf_amd.__all__
    ctx = Context.__new__(Context)                       # no device behind it: a refusal that reached the library would fail loudly
    s, c = _rand(30, (16, 20, 3)), _rand(31, (9, 20, 3))
    with pytest.raises(ValueError, match='smaller'):
        ctx.content_colors(c, s)                         # Ho < Hc
    with pytest.raises(ValueError, match='smaller'):
        ctx.content_colors(s[:, :10], c)                 # Wo < Wc
    with pytest.raises(ValueError, match='uint8'):
        ctx.content_colors(s.astype(np.float32), c)
    with pytest.raises(ValueError, match='uint8'):
        ctx.content_colors(s, c / 255.)
    with pytest.raises(ValueError, match='HxWx3'):
        ctx.content_colors(s[..., :2], c)
    with pytest.raises(ValueError, match='HxWx3'):
        ctx.content_colors(s, c[None])
    with pytest.raises(ValueError, match=r'\[B\]\[H\]\[W\]\[3\]'):
        ctx.content_colors_batch(s, c)
    with pytest.raises(ValueError, match='as many contents'):
        ctx.content_colors_batch(np.stack([s, s]), c[None])
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.content_colors_batch(np.zeros((33, 4, 4, 3), np.uint8), np.zeros((33, 4, 4, 3), np.uint8))


def test_flag_value_matches_the_header():
    import re
    from wct_tf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    assert int(re.search(r'WCT_FLAG_CONTENT_COLORS\s*=\s*(\d+)', hdr).group(1)) == _lib.FLAG_CONTENT_COLORS == 32
    assert 'colors.hip' in __import__('wct_tf_amd.build', fromlist=['SOURCES']).SOURCES


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/colors_rule_check.cpp includes csrc/colors_rule.h -- the functions the kernels call -- and compares them with
    the oracle's values: a stand-alone program, nothing sanitized is loaded into this process."""
    rng = np.random.default_rng(40)
    n = 4096
    s = rng.integers(0, 256, (n, 1, 3)).astype(np.uint8)
    c = rng.integers(0, 256, (n, 1, 3)).astype(np.uint8)
    # the corners of the range as well: the most negative and the most positive luminance difference
    s[:4, 0] = [[0, 0, 0], [255, 255, 255], [0, 0, 0], [255, 255, 255]]
    c[:4, 0] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]]
    want = oracle.content_colors(s, c)                   # (an n x 1 image: pixel i against content pixel i)
    px = np.concatenate([s, c, want], axis=2).reshape(n, 9)
    x = np.concatenate([rng.uniform(-0.5, 1.5, 2000), np.arange(256) / 255., [0., -0., 1., np.inf, -np.inf]]).astype(np.float32)
    q = oracle.quantise(x)
    data = tmp_path / 'cases.bin'
    data.write_bytes(struct.pack('<i', n) + px.tobytes() + struct.pack('<i', len(x)) + x.tobytes() + q.tobytes())
    exe = str(tmp_path / 'colors_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'colors_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d pixels, %d samples' % (n, len(x)) in out.stdout
