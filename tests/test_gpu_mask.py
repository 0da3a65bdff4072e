"""Spatial control (Li et al. 2017, sec. 4.2, Fig. 7) on the GPU: wct_transform_masked / wct_adain_masked / wct_stylize_masked
against the single-style calls on each region's rows (bit for bit) and the mask oracle (tests/mask_oracle.py), the device's
label partition against the host's, the ABI refusals and the CLI."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import mask_oracle
from conftest import rel_err, max_rel
from wct_tf_amd import _lib
from wct_tf_amd.weights import RELU_TARGETS, synthetic_features, synthetic_image, synthetic_weights

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
    return np.ascontiguousarray(f.reshape(-1, f.shape[-1]))


def blobs(seed, h, w, k):
    """blob-shaped random labels 0 .. k-1: the argmax of k smoothed noise fields"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((k, h, w))
    for _ in range(4):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5
    return np.uint8(np.argmax(f, 0))


def test_k1_all_zero_labels_is_the_single_style_call_bit_for_bit(ctx):
    for c, (hc, wc), (hs, ws) in [(64, (32, 32), (24, 40)), (512, (16, 16), (20, 24))]:
        fc = _flat(synthetic_features(30 + c, c, hc, wc, 2.0))
        fs = _flat(synthetic_features(40 + c, c, hs, ws, 2.0))
        zero = np.zeros(hc * wc, np.uint8)
        for mode in (_lib.WCT_TF, _lib.WCT_NP):
            got, sweeps = ctx.transform_masked(fc, [fs], zero, 0.8, mode, return_sweeps=True)
            want, wsw = ctx.transform(fc, fs, 0.8, mode, return_sweeps=True)
            assert np.array_equal(got, want) and list(sweeps) == list(wsw)
        assert np.array_equal(ctx.adain_masked(fc, [fs], zero, 0.7), ctx.adain(fc, fs, 0.7))


def _check_regions(ctx, fc, fs, labels, alpha, mode):
    """every region: bit for bit the single-style call on its rows, and within wct_transform's bound of the float64 oracle;
    a region of one row keeps it; returns the output"""
    lib_mode = _lib.WCT_NP if mode == 'np' else _lib.WCT_TF
    got, sweeps = ctx.transform_masked(fc, fs, labels, alpha, lib_mode, return_sweeps=True)
    kw64 = {'dtype': np.float64} if mode == 'tf' else {}
    for k in range(len(fs)):
        rows = labels == k
        n = int(rows.sum())
        if n == 0:
            assert sweeps[2 * k] == sweeps[2 * k + 1] == 0
            continue
        if n == 1:
            assert np.array_equal(got[rows], fc[rows]) and sweeps[2 * k] == sweeps[2 * k + 1] == 0
            continue
        want, wsw = ctx.transform(np.ascontiguousarray(fc[rows]), fs[k], alpha, lib_mode, return_sweeps=True)
        assert np.array_equal(got[rows], want), (k, n)
        assert list(sweeps[2 * k:2 * k + 2]) == list(wsw)
        o64 = mask_oracle.region_transform(np.float64(fc[rows]), np.float64(fs[k]), alpha, mode, **kw64)
        o32 = mask_oracle.region_transform(fc[rows], fs[k], alpha, mode)
        e, ref = rel_err(got[rows], o64), rel_err(o32, o64)
        print('region %d: N = %d of C = %d, %s: %.2e from the float64 oracle (float32 oracle %.2e), max %.2e' % (
            k, n, fc.shape[1], mode, e, ref, max_rel(got[rows], o64)))
        assert e < max(WCT_TOL, 4 * ref)
    return got


@pytest.mark.parametrize('c', [64, 256, 512])
@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('mode', ['tf', 'np'])
def test_each_region_is_wct_transform_on_its_rows(ctx, c, k, mode):
    hc, wc = 24, 28                                              # 672 rows: at C = 512 every region has 2 <= N_k < C
    fc = _flat(synthetic_features(50 + c, c, hc, wc, 2.0))
    fs = [_flat(synthetic_features(60 + c + k2, c, h, w, 2.0)) for k2, (h, w) in enumerate([(24, 30), (20, 26), (18, 24)][:k])]
    labels = blobs(c + k, hc, wc, 2).reshape(-1)
    if k == 3:
        labels[hc * wc // 2] = 2                                  # a region of one pixel
    n = np.bincount(labels, minlength=k)
    assert n[:2].min() >= 2 and (c < 512 or n.max() < c)
    _check_regions(ctx, fc, fs, labels, 0.8, mode)


def test_an_empty_label_and_the_other_regions(ctx):
    c, hc, wc = 128, 16, 20
    fc = _flat(synthetic_features(71, c, hc, wc, 2.0))
    fs = [_flat(synthetic_features(72 + k, c, 16, 16, 2.0)) for k in range(3)]
    labels = np.where(blobs(5, hc, wc, 2).reshape(-1) == 1, 2, 0).astype(np.uint8)   # label 1 has no pixel
    for mode in ('tf', 'np'):
        _check_regions(ctx, fc, fs, labels, 0.6, mode)


def test_changing_one_style_leaves_the_other_regions_unchanged(ctx):
    c, hc, wc = 256, 20, 20
    fc = _flat(synthetic_features(81, c, hc, wc, 2.0))
    a, b, b2 = (_flat(synthetic_features(s, c, 16, 18, 2.0)) for s in (82, 83, 84))
    labels = blobs(9, hc, wc, 2).reshape(-1)
    r0 = labels == 0
    for mode in (_lib.WCT_TF, _lib.WCT_NP):
        x, y = ctx.transform_masked(fc, [a, b], labels, 0.8, mode), ctx.transform_masked(fc, [a, b2], labels, 0.8, mode)
        assert np.array_equal(x[r0], y[r0]) and not np.array_equal(x[~r0], y[~r0])
    x, y = ctx.adain_masked(fc, [a, b], labels, 0.8), ctx.adain_masked(fc, [a, b2], labels, 0.8)
    assert np.array_equal(x[r0], y[r0]) and not np.array_equal(x[~r0], y[~r0])


def test_adain_regions(ctx):
    for c, hc, wc in [(64, 40, 40), (512, 12, 14)]:
        fc = _flat(synthetic_features(90 + c, c, hc, wc, 2.0))
        fs = [_flat(synthetic_features(91 + c + k, c, 10 + 3 * k, 12, 2.0)) for k in range(3)]
        labels = blobs(c, hc, wc, 2).reshape(-1)
        labels[0] = 2                                             # one pixel: unchanged
        got = ctx.adain_masked(fc, fs, labels, 0.7)
        for k in range(2):
            rows = labels == k
            assert np.array_equal(got[rows], ctx.adain(np.ascontiguousarray(fc[rows]), fs[k], 0.7))
            want = mask_oracle.region_transform(fc[rows], fs[k], 0.7, 'adain')
            assert rel_err(got[rows], want) < 1e-5
        assert np.array_equal(got[0], fc[0])


@pytest.mark.parametrize('hm,wm,h,w,stride,k', [(37, 45, 10, 12, 4, 3), (37, 45, 40, 48, 1, 2), (300, 700, 300, 700, 1, 5),
                                                (64, 64, 64, 64, 1, 1), (9, 9, 3, 3, 4, 8)])
def test_device_partition_is_the_hosts(ctx, hm, wm, h, w, stride, k):
    """debug check of the compaction pass: perm = the stable argsort of the level's labels, seg_off = the host's counts"""
    mask = blobs(hm + k, hm, wm, k)
    perm, seg = ctx.mask_compact(mask, h, w, stride, k)
    lab = mask_oracle.level_labels(mask, h, w, stride).reshape(-1)
    assert np.array_equal(perm, np.argsort(lab, kind='stable'))
    assert np.array_equal(seg, np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=k))]))


@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True), dict(f32=True)])
def test_stylize_masked_k1_is_stylize(small_ctx, kw):
    c, a = synthetic_image(11, 96, 80), synthetic_image(12, 72, 88)
    if kw.pop('f32', False):
        c, a = np.float32(c) + 0.25, np.float32(a) - 0.25
    zero = np.zeros(c.shape[:2], np.uint8)
    assert np.array_equal(small_ctx.stylize_masked(c, [a], zero, SMALL, alpha=0.7, **kw),
                          small_ctx.stylize(c, a, SMALL, alpha=0.7, **kw))


def test_stylize_masked_five_levels_512_end_to_end_on_a_well_conditioned_net():
    """The floors of test_config3_five_levels_512_end_to_end_on_a_well_conditioned_net (tests/test_gpu_pipeline.py) and of the
    mix's end-to-end test, for two styles of different sizes on a 3/8 | 5/8 split of the frame, against the fp32 mask oracle.
    (An exact half split gives both regions N = C = 512 rows at relu5_1: the smallest covariance eigenvalues then run down
    through the 1e-5 cut-off with no gap, and the kept count is decided by rounding -- measured 39.9 dB on this net, while that
    level's transform alone stays within 5e-5 of float64 and the four levels below it reach 52 dB)"""
    from oracle.contractive import contractive_weights
    from wct_tf_amd.context import Context
    w = contractive_weights(7)
    c = synthetic_image(1000, 512, 512)
    styles = [synthetic_image(2000, 512, 512), synthetic_image(2002, 448, 384)]
    mask = np.zeros((512, 512), np.uint8)
    mask[:, 192:] = 1                                            # relu5_1: 384 and 640 rows of C = 512
    cx = Context(0)
    try:
        cx.set_weights(w)
        got = cx.stylize_masked(c, styles, mask, RELU_TARGETS, alpha=0.8)
    finally:
        cx.close()
    want = mask_oracle.stylize_masked(c, styles, mask, w, RELU_TARGETS, alpha=0.8)
    d = np.abs(got.astype(int) - want.astype(int))
    psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((got.astype(np.float64) - want) ** 2), 1e-12))
    print('masked end to end: psnr %.1f dB, max LSB %d, mean LSB %.4f, frame std %.1f' % (psnr, d.max(), d.mean(), want.std()))
    assert got.shape == want.shape == (512, 512, 3) and want.std() > 15
    assert psnr > 42.0 and d.mean() <= 1.6 and d.max() <= 20


def test_abi_refusals_leave_the_context_usable(small_ctx):
    lib = small_ctx.lib
    c = np.ascontiguousarray(synthetic_image(19, 64, 64))
    img = [np.ascontiguousarray(synthetic_image(20 + k, 64, 64)) for k in range(9)]
    lv = (C.c_int * 3)(3, 2, 1)
    out = np.zeros((64, 64, 3), np.uint8)
    u8p = lambda a: a.ctypes.data_as(_lib._U8)

    def call(k, mask, flags=0, lv=lv):
        ptrs = (_lib._U8 * max(k, 1))(*[u8p(a) for a in img[:max(k, 1)]])
        hs = (C.c_int * max(k, 1))(*([64] * max(k, 1)))
        m = np.ascontiguousarray(mask, np.uint8)
        return lib.wct_stylize_masked(small_ctx.h, u8p(c), 64, 64, u8p(m), ptrs, hs, hs, k, lv, len(lv), C.c_float(0.7), flags, u8p(out))

    zero = np.zeros((64, 64), np.uint8)
    for k, mask, flags in ((2, zero + 2, 0), (9, zero, 0), (0, zero, 0), (2, zero, _lib.FLAG_SWAP5), (2, zero, 8)):
        assert call(k, mask, flags) == -2, (k, flags)
        assert lib.wct_last_error()
    # two faults in one call: a level out of range is refused before the decoder that is not loaded (relu4_1) is noticed
    assert call(1, zero, lv=(C.c_int * 2)(4, 7)) == -2 and b'invalid argument' in lib.wct_last_error()
    assert call(1, zero, lv=(C.c_int * 2)(4, 1)) == -3 and b'relu4_1' in lib.wct_last_error()
    fs = [_lib.f32(np.ones((16, 64))) for _ in range(9)]
    ns = (C.c_int * 9)(*([16] * 9))
    o = np.zeros((16, 64), np.float32)
    lab = np.zeros(16, np.uint8)
    lab[3] = 2
    assert lib.wct_transform_masked(small_ctx.h, _lib.fptr(fs[0]), 16, u8p(lab), _lib.ptr_array(fs), ns, 2, 64, C.c_float(1),
                                    _lib.WCT_TF, C.c_float(-1), _lib.fptr(o), None) == -2
    assert lib.wct_adain_masked(small_ctx.h, _lib.fptr(fs[0]), 16, u8p(lab * 0), _lib.ptr_array(fs), ns, 9, 64, C.c_float(1),
                                C.c_float(1e-5), _lib.fptr(o)) == -2
    before = small_ctx.stylize(c, img[0], SMALL, alpha=0.7)
    assert call(1, zero) == 0 and np.array_equal(out, before)
    assert np.array_equal(small_ctx.stylize(c, img[0], SMALL, alpha=0.7), before)


def test_cli_mask_end_to_end(tmp_path):
    from PIL import Image
    from wct_tf_amd import stylize, utils
    from wct_tf_amd.wct import WCT
    paths = []
    for name, seed, (h, w) in (('cat', 31, (64, 80)), ('a', 32, (64, 48)), ('b', 33, (48, 64))):
        p = str(tmp_path / (name + '.png'))
        utils.save_img(p, synthetic_image(seed, h, w))
        paths.append(p)
    grey = np.zeros((32, 40), np.uint8)                          # a binary mask at half the content's size
    grey[:, 18:] = 255
    mpath = str(tmp_path / 'm.png')
    Image.fromarray(grey).save(mpath)
    out_dir = str(tmp_path / 'out')
    assert stylize.main(['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--content-path', paths[0], '--out-path', out_dir,
                         '--mask-path', mpath, '--mask-styles', paths[1], paths[2]]) == 1
    assert os.listdir(out_dir) == ['cat_mask_a+b.png']
    model = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    labels = np.zeros((64, 80), np.uint8)
    labels[:, 36:] = 1
    want = model.predict_masked(utils.get_img(paths[0]), [utils.get_img(paths[1]), utils.get_img(paths[2])], labels)
    model.sess.close()
    assert np.array_equal(utils.get_img(os.path.join(out_dir, 'cat_mask_a+b.png')), want)
