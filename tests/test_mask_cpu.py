"""Spatial control (Li et al. 2017, sec. 4.2, Fig. 7), the parts that need no GPU: the mask oracle against oracle.stylize, the
level-label rule, the grey-band quantisation of the CLI, its flags, the Python validation and the ABI declarations."""
import os
import re

import numpy as np
import pytest

import oracle
import mask_oracle
from conftest import ROOT
from wct_tf_amd.weights import synthetic_image, synthetic_weights

SMALL = ['relu3_1', 'relu2_1', 'relu1_1']


@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True)])
def test_mask_oracle_k1_is_oracle_stylize(kw):
    w = synthetic_weights(5, relu_targets=SMALL)
    c, a = synthetic_image(11, 64, 48), synthetic_image(12, 40, 56)
    got = mask_oracle.stylize_masked(c, [a], np.zeros((64, 48), np.uint8), w, SMALL, alpha=0.7, **kw)
    assert np.array_equal(got, oracle.stylize(c, a, w, SMALL, alpha=0.7, **kw))


def test_mask_oracle_transform_regions():
    rng = np.random.default_rng(3)
    fc = np.float32(rng.standard_normal((40, 32)))
    styles = [np.float32(rng.standard_normal((30, 32)) + k) for k in range(3)]
    labels = np.array([0] * 20 + [1] * 19 + [2])
    out = mask_oracle.transform_masked(fc, styles, labels, 0.8, 'tf')
    assert np.array_equal(out[labels == 2], fc[labels == 2])          # one pixel: unchanged
    want0 = oracle.wct_tf(fc[:20].reshape(4, 5, 32), styles[0].reshape(5, 6, 32), 0.8).reshape(20, 32)
    assert np.allclose(out[:20], want0, rtol=1e-5, atol=1e-5)          # (the rows as a 1 x N map, the same matrix)
    np0 = oracle.wct_np(fc[:20].reshape(4, 5, 32), styles[0].reshape(5, 6, 32), 0.8).reshape(20, 32)
    assert np.allclose(mask_oracle.region_transform(fc[:20], styles[0], 0.8, 'np'), np0, rtol=1e-5, atol=1e-5)
    rows19 = mask_oracle.region_transform(fc[20:39], styles[1], 0.8, 'tf')           # a prime row count
    assert rows19.shape == (19, 32) and np.array_equal(out[20:39], rows19)


def test_level_label_rule_and_the_clamp_on_grown_maps():
    mask = np.arange(35, dtype=np.uint8).reshape(5, 7)
    got = mask_oracle.level_labels(mask, 4, 5, 2)                    # a grown 4 x 5 map at stride 2 of a 5 x 7 mask
    want = np.array([[mask[min(i * 2, 4)][min(j * 2, 6)] for j in range(5)] for i in range(4)])
    assert np.array_equal(got, want)
    assert got[3, 4] == mask[4, 6] and got[2, 3] == mask[4, 6]       # rows 6 and 8 / column 8 clamp to the last pixel
    assert np.array_equal(mask_oracle.level_labels(mask, 5, 7, 1), mask)


def test_level_geometry_of_the_content_chain():
    """the level maps a masked predict() labels: ceil pooling, then x2 upsampling, so a later level can outgrow the content"""
    from wct_tf_amd.weights import RELU_LEVEL
    H, W = 37, 45
    seen = []
    for relu in ['relu3_1', 'relu1_1']:
        l = RELU_LEVEL[relu]
        h, w = -(-H // 2 ** (l - 1)), -(-W // 2 ** (l - 1))
        seen.append((h, w))
        H, W = h * 2 ** (l - 1), w * 2 ** (l - 1)
    assert seen == [(10, 12), (40, 48)]                             # relu1_1 sees a 40 x 48 map of a 37 x 45 content
    lab = mask_oracle.level_labels(np.ones((37, 45), np.uint8), 40, 48, 1)
    assert lab.shape == (40, 48) and lab.min() == 1


def test_grey_band_quantisation():
    from wct_tf_amd.stylize import mask_labels
    grey = np.arange(256, dtype=np.uint8)[None]
    assert np.array_equal(mask_labels(np.array([[0, 255]], np.uint8), 2, (1, 2)), [[0, 1]])    # black -> S0, white -> S1
    for k in (1, 2, 3, 8):
        lab = mask_labels(grey, k, (1, 256))[0]
        assert np.array_equal(lab, np.arange(256) * k // 256) and lab.max() == k - 1
        assert np.all(np.diff(lab.astype(int)) >= 0)
    assert list(mask_labels(grey, 3, (1, 256))[0][[85, 86, 170, 171]]) == [0, 1, 1, 2]


def test_mask_resize_is_nearest():
    from wct_tf_amd.stylize import mask_labels
    grey = np.zeros((8, 8), np.uint8)
    grey[:, 4:] = 255
    lab = mask_labels(grey, 2, (16, 20))
    assert lab.shape == (16, 20) and set(np.unique(lab)) == {0, 1}
    assert np.all(lab[:, :10] == 0) and np.all(lab[:, 10:] == 1)


def _parse(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_interp_args(parser, args)
    stylize.check_mask_args(parser, args)
    return args


BASE = ['--relu-targets', 'relu1_1', '--content-path', 'c.png', '--out-path', 'o']


def test_cli_mask_flags_parse():
    args = _parse(BASE + ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.jpg'])
    assert args.mask_path == 'm.png' and args.mask_styles == ['a.png', 'b.jpg']
    args = _parse(BASE + ['--mask-path', 'm.png', '--mask-styles', 'a.png', '--swap5', '--adain', '--passes', '2'])
    assert args.mask_styles == ['a.png']
    assert _parse(BASE + ['--style-path', 's.png']).mask_path is None


@pytest.mark.parametrize('extra', [
    ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png', '--style-path', 's.png'],
    ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png', '-r', '2'],
    ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png', '--interp-styles', 'x.png', 'y.png'],
    ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png', '--concat'],
    ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png', '--swap5'],
    ['--mask-path', 'm.png', '--mask-styles'] + ['s%d.png' % k for k in range(9)],
    ['--mask-path', 'm.png'],
    ['--mask-styles', 'a.png', 'b.png'],
])
def test_cli_mask_errors(extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(BASE + extra)
    assert e.value.code == 2
    assert 'error:' in capsys.readouterr().err


def test_cli_mask_output_name():
    from wct_tf_amd.stylize import mask_name
    assert mask_name('in/cat.png', ['s/a.jpg', 't/b.png']) == 'cat_mask_a+b.png'
    assert mask_name('dog.jpg', ['x.png']) == 'dog_mask_x.jpg'


@pytest.mark.parametrize('mask,k,shape', [
    (np.array([[0, 2]]), 2, None),              # a label >= K
    (np.array([[0, -1]]), 2, None),             # negative
    (np.zeros((2, 2)), 0, None),                # K = 0
    (np.zeros((2, 2)), 9, None),                # K = 9
    (np.zeros((2, 3)), 2, (3, 2)),              # size differs from the content's
    (np.zeros((2, 2), np.float32), 2, None),    # not integer labels
])
def test_python_mask_validation(mask, k, shape):
    from wct_tf_amd import _lib
    with pytest.raises(ValueError):
        _lib.mask_labels(mask, k, shape)


def test_python_mask_validation_accepts():
    from wct_tf_amd import _lib
    m = _lib.mask_labels(np.array([[0, 1], [1, 0]], np.int64), 2, (2, 2))
    assert m.dtype == np.uint8 and m.flags['C_CONTIGUOUS'] and m.tolist() == [[0, 1], [1, 0]]
    assert _lib.mask_labels(np.zeros((3, 3), bool), 1).max() == 0


def test_predict_masked_validates_before_the_gpu():
    """WCT.predict_masked raises ValueError on bad masks, K and swap5 without touching the library (no context needed)."""
    from wct_tf_amd.wct import WCT
    model = WCT.__new__(WCT)             # no __init__: no GPU context exists, a library call would fail differently
    img = np.zeros((16, 16, 3), np.uint8)
    z = np.zeros((16, 16), np.uint8)
    for styles, mask, kw in (([img, img], z + 2, {}), ([img] * 9, z, {}), ([], z, {}), ([img, img], z[:8], {}),
                             ([img, img], z, dict(swap5=True))):
        with pytest.raises(ValueError):
            model.predict_masked(img, styles, mask, **kw)


def test_mask_symbols_declared_and_bound():
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ('wct_transform_masked', 'wct_adain_masked', 'wct_stylize_masked', 'wct_mask_compact'):
        assert re.search(r'^\s*int\s+%s\s*\(' % name, header, re.M), name
        assert name in bound, name
