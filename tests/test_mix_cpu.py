"""Style interpolation (Li et al. 2017, sec. 4.2), the parts that need no GPU: the mix oracle against oracle.stylize and
against the reference's own wct_np (tests/golden/wct_np_mix_reference.npz, tools/make_mix_golden.py), the CLI flags, the
Python weight validation and the ABI declarations."""
import os
import re
import sys

import numpy as np
import pytest

import oracle
import mix_oracle
from conftest import GOLDEN, ROOT
from wct_tf_amd.weights import synthetic_image, synthetic_weights

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_mix_golden  # noqa: E402

SMALL = ['relu3_1', 'relu2_1', 'relu1_1']


@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True)])
def test_mix_oracle_one_hot_is_oracle_stylize(kw):
    w = synthetic_weights(5, relu_targets=SMALL)
    c, a, b = synthetic_image(11, 64, 64), synthetic_image(12, 64, 64), synthetic_image(13, 48, 56)
    for weights, want_style in (((1, 0), a), ((0, 1), b), ((2.5,), a)):
        styles = [a, b] if len(weights) == 2 else [a]
        got = mix_oracle.stylize_mix(c, styles, weights, w, SMALL, alpha=0.7, **kw)
        want = oracle.stylize(c, want_style, w, SMALL, alpha=0.7, **kw)
        assert np.array_equal(got, want), (weights, kw)


def test_mix_oracle_transform_matches_the_reference_wct_np():
    z = np.load(os.path.join(GOLDEN, 'wct_np_mix_reference.npz'))
    alpha = float(z['alpha'])
    for case in make_mix_golden.CASES:
        name, c = case[:2]
        fc, styles = make_mix_golden.case_inputs(case)
        rows = z[name + '/rows']
        assert np.array_equal(rows, make_mix_golden.case_rows(case))
        refs = [z['%s/out%d' % (name, k)].astype(np.float64) for k in range(3)]
        for weights in ((1, 1, 1), (0.2, 0.5, 0.3), (3, 0, 1)):
            lam = mix_oracle.lambdas(weights, 3)
            want = sum(l * r for l, r in zip(lam, refs))
            got = mix_oracle.transform_mix(fc, styles, weights, alpha, 'np').reshape(-1, c)[rows].astype(np.float64)
            err = np.linalg.norm(got - want) / np.linalg.norm(want)
            print(name, weights, 'rel %.2e' % err)
            assert err <= 1e-5, (name, weights, err)


def _parse(argv):
    from wct_tf_amd import stylize
    parser = stylize.build_parser()
    args = parser.parse_args(argv)
    stylize.check_interp_args(parser, args)
    return args


BASE = ['--relu-targets', 'relu1_1', '--content-path', 'c.png', '--out-path', 'o']


def test_cli_interp_flags_parse():
    args = _parse(BASE + ['--interp-styles', 'a.png', 'b.jpg', '--interp-weights', '1', '3'])
    assert args.interp_styles == ['a.png', 'b.jpg'] and args.interp_weights == [1.0, 3.0]
    args = _parse(BASE + ['--interp-styles', 'a.png', 'b.jpg', 'c.jpg'])
    assert args.interp_weights is None                  # equal weights
    args = _parse(BASE + ['--style-path', 's.png'])
    assert args.interp_styles is None


@pytest.mark.parametrize('extra', [
    ['--interp-styles', 'a.png', 'b.png', '--style-path', 's.png'],
    ['--interp-styles', 'a.png', 'b.png', '-r', '2'],
    ['--interp-styles', 'a.png', 'b.png', '--interp-weights', '1'],
    ['--interp-styles', 'a.png', 'b.png', '--interp-weights', '1', '2', '3'],
    ['--interp-styles', 'a.png', 'b.png', '--interp-weights', '1', '-2'],
    ['--interp-styles', 'a.png', 'b.png', '--interp-weights', '0', '0'],
    ['--interp-styles', 'a.png', 'b.png', '--swap5'],
    ['--interp-weights', '1', '2'],
])
def test_cli_interp_errors(extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(BASE + extra)
    assert e.value.code == 2
    assert 'error:' in capsys.readouterr().err


def test_cli_interp_output_name():
    from wct_tf_amd.stylize import interp_name
    assert interp_name('in/cat.png', ['s/a.jpg', 't/b.png']) == 'cat_a+b.png'
    assert interp_name('dog.jpg', ['x.png', 'y.png', 'z.png']) == 'dog_x+y+z.jpg'


@pytest.mark.parametrize('weights,k', [([1, -1], 2), ([1, float('nan')], 2), ([0, 0], 2), ([1, 2, 3], 2), ([1], 0),
                                       ([1] * 9, 9), ([float('inf'), 1], 2)])
def test_python_weight_validation(weights, k):
    from wct_tf_amd import _lib
    with pytest.raises(ValueError):
        _lib.mix_weights(weights, k)


def test_python_weight_validation_accepts():
    from wct_tf_amd import _lib
    assert list(_lib.mix_weights(None, 3)) == [1, 1, 1]
    assert list(_lib.mix_weights([0, 2], 2)) == [0, 2]


def test_predict_mix_validates_before_the_gpu():
    """WCT.predict_mix raises ValueError on bad weights without touching the library (no context needed)."""
    from wct_tf_amd.wct import WCT
    model = WCT.__new__(WCT)             # no __init__: no GPU context exists, a library call would fail differently
    img = np.zeros((16, 16, 3), np.uint8)
    for weights in ([1, -1], [float('nan'), 1], [0, 0], [1, 2, 3]):
        with pytest.raises(ValueError):
            model.predict_mix(img, [img, img], weights)


def test_mix_symbols_declared_and_bound():
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in ('wct_transform_mix', 'wct_adain_mix', 'wct_stylize_mix'):
        assert re.search(r'^\s*int\s+%s\s*\(' % name, header, re.M), name
        assert name in bound, name
