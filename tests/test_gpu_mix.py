"""Style interpolation (Li et al. 2017, sec. 4.2) on the GPU: wct_transform_mix / wct_adain_mix / wct_stylize_mix against the
mix oracle (tests/mix_oracle.py) and the reference's wct_np (tests/golden/wct_np_mix_reference.npz), the bit-exact identities
(K = 1, one-hot weights), the ABI refusals and the CLI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mix_oracle
from conftest import GOLDEN, ROOT, rel_err, max_rel
from wct_tf_amd import _lib
from wct_tf_amd.weights import RELU_TARGETS, synthetic_features, synthetic_image, synthetic_weights

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_mix_golden  # noqa: E402

pytestmark = pytest.mark.gpu
WCT_TOL = 1e-3                       # tests/test_gpu_ops.py
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def small_ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.set_weights(synthetic_weights(5, relu_targets=SMALL))
    yield c
    c.close()


def _flat(f):
    return f.reshape(-1, f.shape[-1])


@pytest.mark.parametrize('c,hc,wc,styles', [
    (64, 32, 32, [(24, 40), (16, 16)]),
    (128, 24, 24, [(24, 24), (20, 30), (12, 40)]),
    (256, 20, 20, [(16, 30), (24, 24)]),
    (512, 24, 24, [(32, 32), (16, 20), (28, 24)]),     # 16 x 20 = 320 pixels < C
])
@pytest.mark.parametrize('mode', ['np', 'tf'])
def test_transform_mix_matches_the_mix_oracle(ctx, c, hc, wc, styles, mode):
    fc = synthetic_features(10 + c, c, hc, wc, 2.0)
    fs = [synthetic_features(20 + c + 7 * k, c, h, w, 2.0) for k, (h, w) in enumerate(styles)]
    weights = [0.5, 1.5, 1.0][:len(fs)]
    want = mix_oracle.transform_mix(fc, fs, weights, 0.8, mode)
    got, sweeps = ctx.transform_mix(_flat(fc), [_flat(f) for f in fs], weights, 0.8,
                                    _lib.WCT_NP if mode == 'np' else _lib.WCT_TF, return_sweeps=True)
    got = got.reshape(want.shape)
    e2, em = rel_err(got, want), max_rel(got, want)
    print('mix C=%d K=%d mode=%s sweeps=%s rel=%.2e max=%.2e' % (c, len(fs), mode, sweeps, e2, em))
    assert len(sweeps) == 1 + len(fs) and all(0 < s <= 14 for s in sweeps)
    assert e2 < WCT_TOL and em < 5 * WCT_TOL


def test_transform_mix_matches_the_reference_wct_np(ctx):
    z = np.load(os.path.join(GOLDEN, 'wct_np_mix_reference.npz'))
    alpha = float(z['alpha'])
    for case in make_mix_golden.CASES:
        name, c = case[:2]
        fc, fs = make_mix_golden.case_inputs(case)
        rows = z[name + '/rows']
        for weights in ((1, 1, 1), (0.2, 0.5, 0.3)):
            lam = mix_oracle.lambdas(weights, 3)
            want = sum(l * z['%s/out%d' % (name, k)].astype(np.float64) for k, l in enumerate(lam)).astype(np.float32)
            got, sweeps = ctx.transform_mix(_flat(fc), [_flat(f) for f in fs], weights, alpha, _lib.WCT_NP, return_sweeps=True)
            got = got[rows]
            print(name, weights, sweeps, 'rel %.2e max %.2e' % (rel_err(got, want), max_rel(got, want)))
            assert all(0 < s <= 14 for s in sweeps)
            assert rel_err(got, want) < WCT_TOL and max_rel(got, want) < 5 * WCT_TOL


def test_k1_is_the_single_style_call_bit_for_bit(ctx):
    for c, (hc, wc), (hs, ws) in [(64, (32, 32), (24, 40)), (512, (16, 16), (20, 24))]:
        fc = _flat(synthetic_features(30 + c, c, hc, wc, 2.0))
        fs = _flat(synthetic_features(40 + c, c, hs, ws, 2.0))
        for mode in (_lib.WCT_TF, _lib.WCT_NP):
            assert np.array_equal(ctx.transform_mix(fc, [fs], [3.0], 0.8, mode), ctx.transform(fc, fs, 0.8, mode))
        assert np.array_equal(ctx.adain_mix(fc, [fs], None, 0.7), ctx.adain(fc, fs, 0.7))


def test_adain_mix_matches_the_mix_oracle(ctx):
    for c, h, w in [(64, 40, 40), (512, 8, 8), (128, 33, 17)]:
        fc = synthetic_features(70 + c, c, h, w, 2.0)
        fs = [synthetic_features(80 + c + k, c, h + 3 * k, w + k, 2.0) for k in range(3)]
        weights = [0.2, 0.3, 0.5]
        got = ctx.adain_mix(_flat(fc), [_flat(f) for f in fs], weights, 0.7).reshape(fc.shape)
        want = mix_oracle.transform_mix(fc, fs, weights, 0.7, 'adain')
        print('adain mix', c, rel_err(got, want))
        assert rel_err(got, want) < 1e-5 and max_rel(got, want) < 1e-4


@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True)])
def test_stylize_mix_frame_identities(small_ctx, kw):
    c, a, b = synthetic_image(11, 96, 96), synthetic_image(12, 96, 96), synthetic_image(13, 80, 72)
    run = lambda styles, weights: small_ctx.stylize_mix(c, styles, weights, SMALL, alpha=0.7, **kw)
    fa, fb = small_ctx.stylize(c, a, SMALL, alpha=0.7, **kw), small_ctx.stylize(c, b, SMALL, alpha=0.7, **kw)
    assert np.array_equal(run([a], [2.0]), fa)
    assert np.array_equal(run([a, b], [1, 0]), fa)
    assert np.array_equal(run([a, b], [0, 1]), fb)
    m1, m2 = run([a, b], [1, 3]), run([a, b], [1, 3])
    assert np.array_equal(m1, m2)
    assert not np.array_equal(m1, fa) and not np.array_equal(m1, fb)


def test_stylize_mix_five_levels_512_end_to_end_on_a_well_conditioned_net():
    """The floors of test_config3_five_levels_512_end_to_end_on_a_well_conditioned_net (tests/test_gpu_pipeline.py), for a
    mix of two styles of different sizes against the fp32 mix oracle."""
    from oracle.contractive import contractive_weights
    from wct_tf_amd.context import Context
    w = contractive_weights(7)
    c = synthetic_image(1000, 512, 512)
    styles = [synthetic_image(2000, 512, 512), synthetic_image(2002, 448, 384)]
    cx = Context(0)
    try:
        cx.set_weights(w)
        got = cx.stylize_mix(c, styles, [0.3, 0.7], RELU_TARGETS, alpha=0.8)
    finally:
        cx.close()
    want = mix_oracle.stylize_mix(c, styles, [0.3, 0.7], w, RELU_TARGETS, alpha=0.8)
    d = np.abs(got.astype(int) - want.astype(int))
    psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((got.astype(np.float64) - want) ** 2), 1e-12))
    print('mix end to end: psnr %.1f dB, max LSB %d, mean LSB %.4f, frame std %.1f' % (psnr, d.max(), d.mean(), want.std()))
    assert got.shape == want.shape == (512, 512, 3) and want.std() > 15
    assert psnr > 42.0 and d.mean() <= 1.6 and d.max() <= 20


def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib = small_ctx.lib
    c = np.ascontiguousarray(synthetic_image(19, 64, 64))
    img = [np.ascontiguousarray(synthetic_image(20 + k, 64, 64)) for k in range(9)]
    lv = (C.c_int * 3)(3, 2, 1)
    out = np.zeros((64, 64, 3), np.uint8)
    u8p = lambda a: a.ctypes.data_as(_lib._U8)

    def call(k, weights, flags=0):
        ptrs = (_lib._U8 * max(k, 1))(*[u8p(a) for a in img[:max(k, 1)]])
        hs = (C.c_int * max(k, 1))(*([64] * max(k, 1)))
        w = np.ascontiguousarray(weights, np.float32) if len(weights) else np.zeros(1, np.float32)
        return lib.wct_stylize_mix(small_ctx.h, u8p(c), 64, 64, ptrs, hs, hs, k, _lib.fptr(w), lv, 3, C.c_float(0.7), flags, u8p(out))

    for k, weights, flags in ((2, [1, 1], _lib.FLAG_SWAP5), (0, [], 0), (9, [1] * 9, 0), (2, [1, -1], 0), (2, [0, 0], 0)):
        assert call(k, weights, flags) == -2, (k, weights, flags)
        assert lib.wct_last_error()
    fs = [_lib.f32(np.ones((16, 64))) for _ in range(2)]
    ns = (C.c_int * 2)(16, 16)
    o = np.zeros((16, 64), np.float32)
    assert lib.wct_transform_mix(small_ctx.h, _lib.fptr(fs[0]), 16, _lib.ptr_array(fs), ns, 2, _lib.fptr(_lib.f32([1, -1])), 64,
                                 C.c_float(1), _lib.WCT_TF, C.c_float(-1), _lib.fptr(o), None) == -2
    assert lib.wct_adain_mix(small_ctx.h, _lib.fptr(fs[0]), 16, _lib.ptr_array(fs), ns, 9, _lib.fptr(_lib.f32([1] * 9)), 64,
                             C.c_float(1), C.c_float(1e-5), _lib.fptr(o)) == -2
    before = small_ctx.stylize(c, img[0], SMALL, alpha=0.7)
    assert call(2, [1, 0]) == 0 and np.array_equal(out, before)
    assert np.array_equal(small_ctx.stylize(c, img[0], SMALL, alpha=0.7), before)


def test_cli_interp_styles_end_to_end(tmp_path):
    from wct_tf_amd import stylize, utils
    from wct_tf_amd.wct import WCT
    paths = []
    for name, seed, (h, w) in (('cat', 31, (64, 64)), ('a', 32, (64, 48)), ('b', 33, (48, 64))):
        p = str(tmp_path / (name + '.png'))
        utils.save_img(p, synthetic_image(seed, h, w))
        paths.append(p)
    out_dir = str(tmp_path / 'out')
    assert stylize.main(['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--content-path', paths[0], '--out-path', out_dir,
                         '--interp-styles', paths[1], paths[2], '--interp-weights', '1', '3']) == 1
    target = os.path.join(out_dir, 'cat_a+b.png')
    assert os.listdir(out_dir) == ['cat_a+b.png']
    model = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    want = model.predict_mix(utils.get_img(paths[0]), [utils.get_img(paths[1]), utils.get_img(paths[2])], [1, 3])
    model.sess.close()
    assert np.array_equal(utils.get_img(target), want)
