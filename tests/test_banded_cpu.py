"""Banded stylization without a GPU: the band plan (wct_band_plan) and the routing (wct_band_rows) are host code of the library;
the halos the plan returns are checked on the oracle network; csrc/pool_rule.h is checked by a stand-alone host program; and the
argument checks of --band-rows and WCT.predict(band_rows=...) run before any GPU call."""
import os
import struct
import subprocess
import types

import numpy as np
import pytest

import oracle
from conftest import ROOT
from wct_tf_amd.weights import synthetic_image, synthetic_weights

CLANG = '/opt/rocm/lib/llvm/bin/clang++'
ALL = ['relu5_1', 'relu4_1', 'relu3_1', 'relu2_1', 'relu1_1']


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_band_plan_partitions_every_height(lib):
    from wct_tf_amd.context import band_plan
    for level in range(1, 6):
        s = 1 << (level - 1)
        for band_rows in range(16, 129, 16):
            for H in range(17, 701):
                h = (H + s - 1) // s
                p = band_plan(H, 40, level, band_rows)
                assert len(p) == (H + band_rows - 1) // band_rows
                e0, e1, y0, y1, d0, d1 = p.T
                # interiors: [0, H) in image rows exactly once, every origin a multiple of 16, no empty band
                assert y0[0] == 0 and y1[-1] == H and np.array_equal(y0[1:], y1[:-1]) and np.all(y1 > y0)
                assert np.all(y0 % 16 == 0) and np.all(e0 % 16 == 0) and np.all(y1[:-1] % 16 == 0)
                # and [0, h) in feature rows exactly once
                f0, f1 = y0 // s, np.append(y1[:-1] // s, h)
                assert f0[0] == 0 and np.array_equal(f0[1:], f1[:-1]) and np.all(f1 > f0), (level, band_rows, H)
                # spans inside the image, around their interiors; decoder spans start on an even row
                assert np.all(e0 >= 0) and np.all(e1 <= H) and np.all(e0 <= y0) and np.all(e1 >= y1)
                assert np.all(d0 >= 0) and np.all(d1 <= h) and np.all(d0 <= f0) and np.all(d1 >= f1) and np.all(d0 % 2 == 0)
                assert np.all(d1 - d0 >= 2)


def test_band_plan_arguments(lib):
    import ctypes as C
    from wct_tf_amd._lib import WCTHipError
    from wct_tf_amd.context import band_plan
    assert len(band_plan(100, 40, 'relu3_1', 0)) == 1                # automatic: one band where the whole-image call runs
    assert len(band_plan(4000, 3000, 'relu1_1', 0)) == 2             # 12 MP at relu1_1: the automatic height is the cap, 2048 rows
    for bad in (8, 24, -16):
        with pytest.raises(WCTHipError, match='multiple of 16'):
            band_plan(100, 40, 'relu3_1', bad)
    n = C.c_int()
    rows = (C.c_int * 6)()
    assert lib.wct_band_plan(100, 40, 3, 16, 1, C.byref(n), rows) == -2 and n.value == 7     # no room: the count still comes back
    assert lib.wct_band_plan(16, 40, 5, 16, 1, C.byref(n), rows) == -2                       # too small for relu5_1


def test_band_rows_routing(lib):
    from wct_tf_amd._lib import WCTHipError
    from wct_tf_amd.context import band_rows
    assert band_rows(2896, 2896, ALL) == 0                           # 8 386 816 < 8 388 608 = 2^31 / 256
    assert band_rows(2900, 2900, ALL) > 0
    assert band_rows(4000, 3000, ALL[:4]) == 0                       # without relu1_1 the limit is 16.7 MP
    assert band_rows(4200, 4000, ALL[:4]) > 0
    r = band_rows(4000, 3000, ALL)
    assert r > 0 and r % 16 == 0 and r <= 2048
    assert band_rows(2900, 2900, ['relu1_1']) > 0
    with pytest.raises(WCTHipError, match='width limit'):
        band_rows(64, 400000, ['relu1_1'])


# ---- the halos, on the oracle network ------------------------------------------------------------------------------------------
HALO_CASES = [(1, 50, 20, 16), (2, 70, 22, 16), (3, 150, 26, 32), (4, 210, 20, 48), (5, 437, 36, 64)]


@pytest.fixture(scope='module')
def net():
    return synthetic_weights(3)


def _banded_encode(img, net, target, plan, s):
    parts = []
    for k, (e0, e1, y0, y1, _, _) in enumerate(plan):
        f = oracle.encode(img[e0:e1], net, [target], wino=False)[target]
        f1 = f.shape[0] + e0 // s if k == len(plan) - 1 else y1 // s
        parts.append(f[y0 // s - e0 // s:f1 - e0 // s])
    return np.concatenate(parts)


def _banded_decode(feat, net, target, plan, s, halo=True):
    parts = []
    for k, (_, _, y0, y1, d0, d1) in enumerate(plan):
        f0, f1 = y0 // s, (len(feat) if k == len(plan) - 1 else y1 // s)
        a, b = (d0, d1) if halo else (f0, f1)
        parts.append(oracle.decode(feat[a:b], net, target, wino=False)[(f0 - a) * s:(f1 - a) * s])
    return np.concatenate(parts)


@pytest.mark.parametrize('level,H,W,band_rows', HALO_CASES)
def test_the_plans_halos_reproduce_the_whole_pass_on_the_oracle(lib, net, level, H, W, band_rows):
    """Banding oracle.encode / oracle.decode (fp32, direct convolutions) by the spans of the library's plan gives the whole pass
    to 1e-5 of the largest value: numpy's GEMM blocking moves values by some 1e-7 at these shapes, a missing halo row by their
    own size -- the last assertions show that the threshold discriminates."""
    from wct_tf_amd.context import band_plan
    target = 'relu%d_1' % level
    s = 1 << (level - 1)
    plan = band_plan(H, W, target, band_rows)
    assert len(plan) > 1
    img = np.float32(synthetic_image(40 + level, H, W)) / np.float32(255)
    whole = oracle.encode(img, net, [target], wino=False)[target]
    got = _banded_encode(img, net, target, plan, s)
    assert got.shape == whole.shape
    err = np.abs(got - whole).max() / np.abs(whole).max()
    print('relu%d_1 encoder %dx%d in %d bands: %.3g' % (level, H, W, len(plan), err))
    assert err <= 1e-5
    out = oracle.decode(whole, net, target, wino=False)
    dgot = _banded_decode(whole, net, target, plan, s)
    assert dgot.shape == out.shape
    derr = np.abs(dgot - out).max() / np.abs(out).max()
    print('relu%d_1 decoder %dx%d in %d bands: %.3g' % (level, whole.shape[0], whole.shape[1], len(plan), derr))
    assert derr <= 1e-5
    if level in (3, 5):                                               # no halo at all is far outside the threshold
        none = _banded_decode(whole, net, target, plan, s, halo=False)
        assert np.abs(none - out).max() / np.abs(out).max() > 1e-2


# ---- pool_rule.h ----------------------------------------------------------------------------------------------------------------
def _pool_case(rng, K, C):
    n = rng.integers(2, 400, K)
    n[rng.integers(0, K)] = 2                                          # a chunk of two rows
    spread = rng.uniform(0.5, 2.0, C)
    base = 1e3 * spread * rng.choice([-1.0, 1.0], C)                   # means of size 1e3 x the spread
    mix = rng.standard_normal((C, C)) / np.sqrt(C)
    chunks = [base + 0.3 * spread * rng.standard_normal(C) + (rng.standard_normal((m, C)) @ mix) * spread for m in n]
    means = np.stack([c.mean(0) for c in chunks])
    covs = np.stack([np.cov(c, rowvar=False) for c in chunks])
    covs = 0.5 * (covs + covs.transpose(0, 2, 1))
    x = np.concatenate(chunks)
    if K == 1:
        return n, means, covs, means[0], covs[0]
    return n, means, covs, x.mean(0), np.cov(x, rowvar=False)


@pytest.mark.skipif(not os.path.exists(CLANG), reason='ROCm clang++ not found')
def test_pool_rule_header_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/emul/pool_rule_check.cpp includes csrc/pool_rule.h -- the functions the pooling kernels call -- and pools chunk
    statistics given in double: the result is the covariance of the concatenation (NumPy, float64) to 1e-12 of its largest entry,
    three decades above double rounding over <= 70 terms.  A stand-alone program: nothing sanitized is loaded into this process."""
    rng = np.random.default_rng(11)
    cases = [_pool_case(rng, K, 64) for K in (1, 2, 7, 33, 70)]
    data = tmp_path / 'pool_cases.bin'
    with open(data, 'wb') as f:
        f.write(struct.pack('<i', len(cases)))
        for n, means, covs, mean, cov in cases:
            f.write(struct.pack('<ii', len(n), means.shape[1]))
            f.write(np.asarray(n, '<i4').tobytes())
            for a in (means, covs, mean, cov):
                f.write(np.ascontiguousarray(a, '<f8').tobytes())
    exe = str(tmp_path / 'pool_rule_check')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tests', 'emul', 'pool_rule_check.cpp')])
    out = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'all checks passed: %d cases' % len(cases) in out.stdout


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def _parse(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(['--content-path', 'c', '--style-path', 's', '--out-path', 'o', '--synthetic-weights', '1',
                              '--relu-targets'] + ALL + argv)
    stylize.check_band_args(parser, args)
    return parser, args


def test_band_rows_option(lib, capsys):
    from wct_tf_amd import stylize
    assert _parse([])[1].band_rows == 0 and _parse(['--band-rows', '512'])[1].band_rows == 512
    for argv in (['--band-rows', '100'], ['--band-rows', '-16'], ['--band-rows', '64', '--adain'], ['--band-rows', '64', '--swap5'],
                 ['--band-rows', '64', '--interp-styles', 'a', 'b'], ['--band-rows', '64', '--mask-path', 'm', '--mask-styles', 'a']):
        with pytest.raises(SystemExit):
            _parse(argv)
        assert '--band-rows' in capsys.readouterr().err
    # a large content with an option the banded call does not serve: a clear error that names the limit and --band-rows
    parser, args = _parse(['--adain'])
    big = np.broadcast_to(np.uint8(0), (2900, 2900, 3))
    with pytest.raises(SystemExit):
        stylize.check_content_fits(parser, args, big, 'big.png')
    err = capsys.readouterr().err
    assert '--band-rows' in err and '--adain' in err and '2^31' in err
    stylize.check_content_fits(parser, args, np.broadcast_to(np.uint8(0), (512, 512, 3)), 'small.png')      # fits: nothing
    stylize.check_content_fits(*_parse([]), big, 'big.png')                                                 # served: nothing
    assert '--band-rows' not in open(os.path.join(ROOT, 'wct_tf_amd', 'stylize_video.py')).read()          # not on stylize_video


def test_predict_refuses_what_large_contents_do_not_take_before_any_gpu_call(lib):
    from wct_tf_amd.wct import WCT
    model = types.SimpleNamespace(relu_targets=ALL)
    big = np.broadcast_to(np.uint8(0), (2900, 2900, 3))
    small = np.broadcast_to(np.uint8(0), (256, 256, 3))
    route = lambda content, band_rows=None, swap5=False, adain=False, warm=None: WCT._band_route(model, content, band_rows, swap5, adain, warm)
    assert route(small) is None and route(small, adain=True) is None and route(small, warm=object()) is None
    assert route(big) == 2048 and route(small, 64) == 64 and route(big, 512) == 512
    for kw in (dict(adain=True), dict(swap5=True), dict(warm=object())):
        with pytest.raises(ValueError, match=r'2\^31.*band_rows'):
            route(big, **kw)
        with pytest.raises(ValueError, match='band_rows'):
            route(small, 64, **kw)
    for bad in (24, -16, 1.5, '64', True):
        with pytest.raises(ValueError, match='band_rows'):
            route(small, bad)
