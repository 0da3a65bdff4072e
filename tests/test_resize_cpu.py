"""On-device resize without a GPU: the NumPy oracle of the rule (tests/resize_oracle.py) against Pillow itself -- an independent
implementation, so np.array_equal and no tolerance --, the target sizes against resize_to, the properties of the tap tables, the
shared rule header (wct_tf_amd/csrc/resize_rule.h, what the launcher and the kernel compile) built for the host under
AddressSanitizer + UBSan as a program of its own, the Python refusals and the command line."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import resize_oracle as oracle

CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _id(g):
    return '%dx%d-%dx%d' % g


# ---- the rule against Pillow -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', oracle.GEOMETRIES, ids=_id)
def test_oracle_is_pillow(geom):
    """Pins the rule to the installed Pillow: a failure on another Pillow is a finding about the rule, not a reason for a
    tolerance."""
    H, W, h, w = geom
    img = oracle.random_image(H * 7 + W, H, W)
    assert np.array_equal(oracle.resize(img, h, w), oracle.pillow(img, h, w))
    if H * W <= 1 << 18:                                            # (the constants: cheap wherever the image is small)
        for v in (0, 255):
            flat = np.full((H, W, 3), v, np.uint8)
            got = oracle.resize(flat, h, w)
            assert np.array_equal(got, oracle.pillow(flat, h, w)), v
            assert np.all(got == v), v                              # the taps of a row sum close enough to 2^22 to keep a constant


@pytest.mark.parametrize('geom', oracle.CHECKERBOARD, ids=_id)
def test_oracle_is_pillow_on_a_checkerboard(geom):
    H, W, h, w = geom
    img = oracle.checkerboard(H, W)
    assert np.array_equal(oracle.resize(img, h, w), oracle.pillow(img, h, w))


def test_an_unchanged_axis_reproduces_its_bytes():
    img = oracle.random_image(3, 64, 48)
    assert np.array_equal(oracle.resize(img, 64, 48), img)
    bounds, k = oracle.taps(64, 64)
    assert np.array_equal(bounds[:, 0], np.arange(64)) and np.all(k[:, 0] == 1 << 22) and np.all(k[:, 1:] == 0)


# ---- the target sizes --------------------------------------------------------------------------------------------------------
def test_resize_shape_is_the_shape_resize_to_gives():
    """small (h, w, s), among them products that land on .5 (h = 2, w = 3, s = 5: 3 * 2.5 = 7.5 -> round half to even: 8;
    h = 4, w = 6, s = 3: 6 * 0.75 = 4.5 -> 4)"""
    from wct_tf_amd import utils
    halves = 0
    for h in range(1, 13):
        for w in range(1, 13):
            img = np.zeros((h, w, 3), np.uint8)
            for s in (1, 2, 3, 5, 6, 7, 9, 16):
                assert utils.resize_shape(h, w, s) == utils.resize_to(img, s).shape[:2], (h, w, s)
                halves += (max(h, w) * (s / min(h, w))) % 1 == 0.5
    assert halves > 10
    assert utils.resize_shape(2, 3, 5) == (5, 8) and utils.resize_shape(4, 6, 3) == (3, 4) and utils.resize_shape(6, 4, 3) == (4, 3)
    assert utils.resize_shape(1080, 1920, 512) == (512, 910) and utils.resize_shape(96, 128, 48) == (48, 64)


# ---- the tap tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', oracle.GEOMETRIES + oracle.CHECKERBOARD, ids=_id)
def test_tap_tables(geom):
    H, W, h, w = geom
    for n_in, n_out in ((W, w), (H, h)):
        bounds, k = oracle.taps(n_in, n_out)
        ks = oracle.ksize(n_in, n_out)
        assert k.shape == (n_out, ks)
        xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert np.all(xmin >= 0) and np.all(n >= 1) and np.all(xmin + n <= n_in)
        assert np.all(n <= ks)
        assert np.all(k >= 0)
        assert np.all(np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= ks)
        for xx in range(n_out):
            assert not k[xx, n[xx]:].any()
        # what the kernel's tiles rely on: both ends of the tapped range never move backwards
        assert np.all(np.diff(xmin) >= 0) and np.all(np.diff(xmin + n) >= 0)


# ---- the shared rule header on the host, under sanitizers ------------------------------------------------------------------
HOST_CASES = [(1, 1, 3, 2), (2, 2, 1, 1), (3, 3, 1, 1), (70, 1, 35, 1), (1, 9, 4, 3), (5, 7, 96, 96), (37, 53, 24, 35),
              (300, 200, 77, 51), (64, 64, 64, 31), (64, 64, 31, 64), (64, 48, 64, 48), (1200, 8, 4, 8), (8, 1200, 8, 4),
              (100, 100, 101, 99), (97, 131, 40, 60)]


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_resize_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/resize_rule_check.cpp includes csrc/resize_rule.h -- the table function the launcher calls and the byte
    function the kernel calls -- and reproduces the oracle's tap tables, bounds and output bytes: a stand-alone program, nothing
    sanitized is loaded into this process."""
    blob = struct.pack('<i', len(HOST_CASES))
    words = total = 0
    for i, (H, W, h, w) in enumerate(HOST_CASES):
        img = oracle.checkerboard(H, W) if (H, W) == (97, 131) else oracle.random_image(i, H, W)
        (xb, kx), (yb, ky) = oracle.taps(W, w), oracle.taps(H, h)
        out = oracle.resize(img, h, w)
        blob += struct.pack('<iiii', H, W, h, w)
        for t in (xb, kx, yb, ky):
            blob += np.ascontiguousarray(t, '<i4').tobytes()
            words += t.size
        blob += img.tobytes() + out.tobytes()
        total += out.size
    data = tmp_path / 'cases.bin'
    data.write_bytes(blob)
    exe = str(tmp_path / 'resize_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'resize_rule_check.cpp')])
    run = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert 'all checks passed: %d cases, %d table words, %d bytes' % (len(HOST_CASES), words, total) in run.stdout


def test_the_table_function_states_no_contraction():
    src = open(os.path.join(ROOT, 'wct_tf_amd', 'csrc', 'resize_rule.h')).read()
    body = src[src.index('inline void wct_resize_taps'):src.index('template <typename Src>')]
    assert '#pragma clang fp contract(off)' in body
    assert '__host__ __device__' in src and 'WCT_RESIZE_HD inline uint8_t wct_resize_byte' in src


# ---- Python refusals, before any library call ------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    from wct_tf_amd.context import Context, check_resize
    from wct_tf_amd.wct import WCT
    ctx = Context.__new__(Context)                       # no library behind it: a refusal that reached it would fail loudly
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match=r'\(h, w\)'):
        ctx.resize(img, 4)
    with pytest.raises(ValueError, match='empty'):
        ctx.resize(img, (0, 4))
    with pytest.raises(ValueError, match='uint8'):
        ctx.resize(img.astype(np.float32), (4, 4))
    with pytest.raises(ValueError, match='HxWx3'):
        ctx.resize(img[None], (4, 4))
    with pytest.raises(ValueError, match=r'\[B\]\[H\]\[W\]\[3\]'):
        ctx.resize_batch(img, (4, 4))
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.resize_batch(np.zeros((33, 2, 2, 3), np.uint8), (4, 4))
    with pytest.raises(ValueError, match='1 .. 32'):
        ctx.resize_batch_dev(None, 8, 8, 33, (4, 4), None)
    with pytest.raises(ValueError, match='empty'):
        ctx.resize_batch_dev(None, 8, 8, 1, (4, -1), None)
    assert check_resize((4.0, 5)) == (4, 5)
    model = WCT.__new__(WCT)
    model.ss_stride = 2
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match='empty'):
        model.predict_frames(frames, img, resize=(0, 4))
    with pytest.raises(ValueError, match='ss_stride'):
        model.predict_frames(frames, img, swap5=True, resize=(4, 4))
    with pytest.raises(ValueError, match=r'\(h, w\)'):
        model.predict_frames_masked(frames, [img], np.zeros((8, 8), np.uint8), resize=4)
    # the label maps of a resized call are given at the resized size
    with pytest.raises(ValueError, match='mask of shape'):
        model.predict_frames_masked(frames, [img], np.zeros((8, 8), np.uint8), resize=(4, 4))


# ---- the command line ---------------------------------------------------------------------------------------------------------
_BASE = ['--relu-targets', 'relu1_1', '--in-path', 'i', '--out-path', 'o', '--style-path', 's', '--synthetic-weights', '1']


def _check(argv):
    from wct_tf_amd import stylize_video as sv
    parser = sv.build_parser()
    args = parser.parse_args(_BASE + argv)
    sv.check_color_args(parser, args)
    sv.check_resize_args(parser, args)
    return args


def test_device_resize_is_in_the_parser_and_opt_in():
    from wct_tf_amd import stylize_video as sv
    flags = {a for act in sv.build_parser()._actions for a in act.option_strings}
    assert '--device-resize' in flags
    assert _check([]).device_resize is False and _check(['--content-size', '48']).device_resize is False
    a = _check(['--device-resize', '--content-size', '48', '--content-colors', '--swap5'])
    assert a.device_resize is True
    assert sv.device_size(a, [np.zeros((96, 128, 3), np.uint8)]) == (48, 64)
    assert sv.device_size(_check(['--content-size', '48']), [np.zeros((96, 128, 3), np.uint8)]) is None


@pytest.mark.parametrize('argv,word', [
    (['--device-resize', '--content-size', '48', '--keep-colors'], '--keep-colors'),
    (['--device-resize', '--content-size', '48', '--content-colors', '--passes', '2'], '--passes 1'),
    (['--device-resize'], '--content-size > 0'),
    (['--device-resize', '--content-size', '0'], '--content-size > 0'),
    (['--device-resize', '--content-size', '48', '--swap5', '--ss-stride', '2'], '--ss-stride 1'),
], ids=lambda v: ' '.join(v) if isinstance(v, list) else None)
def test_device_resize_parser_errors(capsys, argv, word):
    with pytest.raises(SystemExit):
        _check(argv)
    err = capsys.readouterr().err
    assert '--device-resize' in err and word in err


def test_header_states_the_rule_and_the_build_lists_the_unit():
    from wct_tf_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'wct_hip.h')).read()
    section = hdr[hdr.index('On-device resize'):hdr.index('int wct_resize_batch_dev')]
    for word in ('4194304.0', '2097152', '>> 22', 'ksize = (int)ceil(support) * 2 + 1', 'B = 1 .. %d' % _lib.BATCH_MAX, '2^31',
                 'WCT_STATUS_ARG'):
        assert word in section, word
    assert 'resize.hip' in build.SOURCES
    assert {'wct_resize', 'wct_resize_batch_dev'} <= {name for name, _, _ in _lib.SIGNATURES}
