"""Seamless textures without a GPU: the halo query (wct_wrap_halo) and the size rule (wct_wrap_check) are host code of the library;
the halos are checked on the oracle network against tests/wrap_oracle.py, which states the periodic network layer by layer; the
seam case of the GPU test is checked on the oracle's frame; and the refusals of predict_frames(wrap=True), synthesize(tile=True)
and the texture command line are raised before any GPU call."""
import ctypes as C

import numpy as np
import pytest

import oracle
import wrap_oracle
from wct_tf_amd.weights import synthetic_image, synthetic_weights

ALL = ['relu5_1', 'relu4_1', 'relu3_1', 'relu2_1', 'relu1_1']
ENC = {1: 16, 2: 16, 3: 16, 4: 48, 5: 96}
DEC = {1: (2, 2), 2: (2, 2), 3: (4, 3), 4: (4, 4), 5: (6, 5)}
# tiles no larger than 32 x 48 at the deep levels: the 96-pixel halo of relu5_1 wraps them more than once
TILE = {1: (20, 36), 2: (20, 36), 3: (20, 36), 4: (32, 48), 5: (32, 48)}


@pytest.fixture(scope='module')
def lib():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope='module')
def net():
    return synthetic_weights(3)


# ---- the halo query and the size rule ------------------------------------------------------------------------------------------
def test_halo_query_and_size_rule_need_no_gpu(lib):
    from wct_tf_amd.context import check_wrap, wrap_halo
    for level in range(1, 6):
        assert wrap_halo('relu%d_1' % level) == (ENC[level],) + DEC[level]
        assert ENC[level] % 16 == 0 and DEC[level][0] % 2 == 0
    e = C.c_int()
    assert lib.wct_wrap_halo(0, C.byref(e), C.byref(e), C.byref(e)) == -2 and lib.wct_wrap_halo(6, C.byref(e), C.byref(e), C.byref(e)) == -2
    assert lib.wct_wrap_halo(3, None, C.byref(e), C.byref(e)) == -2
    lv = (C.c_int * 5)(5, 4, 3, 2, 1)
    assert lib.wct_wrap_check(32, 48, lv, 5) == 0 and lib.wct_wrap_check(512, 512, lv, 5) == 0
    assert lib.wct_wrap_check(40, 48, lv, 5) == -2                   # 40 is no multiple of 16
    msg = lib.wct_last_error().decode()
    assert '40x48' in msg and 'relu5_1' in msg and 'multiples of 16' in msg
    assert lib.wct_wrap_check(40, 48, (C.c_int * 4)(4, 3, 2, 1), 4) == 0      # ... and fine when relu4_1 is the deepest
    assert lib.wct_wrap_check(48, 40, lv, 5) == -2 and lib.wct_wrap_check(33, 48, (C.c_int * 1)(2), 1) == -2
    assert lib.wct_wrap_check(16, 48, lv, 5) == -2 and b'too small for relu5_1' in lib.wct_last_error()      # check_min_size applies
    assert lib.wct_wrap_check(0, 48, lv, 5) == -2 and lib.wct_wrap_check(32, 48, (C.c_int * 1)(7), 1) == -2
    # the padded map, not the tile, meets the launch limit: 2896^2 fits a plain call (tests/test_banded_cpu.py), its halo does not
    assert lib.wct_wrap_check(2896, 2896, (C.c_int * 1)(1), 1) == -2 and b'2^31' in lib.wct_last_error()
    assert lib.wct_wrap_check(2848, 2848, (C.c_int * 1)(1), 1) == 0
    with pytest.raises(ValueError, match='multiples of 16'):
        check_wrap(40, 48, ALL)
    assert check_wrap(64, 96, ALL) == (64, 96)


# ---- the halos, on the oracle network ------------------------------------------------------------------------------------------
def _padded_encode(img, net, target, halo, s):
    f = oracle.encode(np.pad(img, ((halo, halo), (halo, halo), (0, 0)), mode='wrap'), net, [target], wino=False)[target]
    h, w = img.shape[0] // s, img.shape[1] // s
    return f[halo // s:halo // s + h, halo // s:halo // s + w]


def _padded_decode(feat, net, target, before, after, s):
    img = oracle.decode(np.pad(feat, ((before, after), (before, after), (0, 0)), mode='wrap'), net, target, wino=False)
    return img[before * s:(before + feat.shape[0]) * s, before * s:(before + feat.shape[1]) * s]


@pytest.mark.parametrize('level', [1, 2, 3, 4, 5])
def test_the_halos_reproduce_the_periodic_network_on_the_oracle(lib, net, level):
    """Padding by the library's halo, running the PLAIN oracle pass and cropping equals the per-layer-circular pass to 1e-5 of the
    largest value (the threshold and its reasons: tests/test_banded_cpu.py -- NumPy's GEMM blocking moves values by some 1e-7 at
    these shapes); a halo one stride short is far outside it."""
    from wct_tf_amd.context import wrap_halo
    target = 'relu%d_1' % level
    s = 1 << (level - 1)
    enc, before, after = wrap_halo(target)
    H, W = TILE[level]
    img = np.float32(synthetic_image(60 + level, H, W)) / np.float32(255)
    want = wrap_oracle.encode(img, net, target)
    got = _padded_encode(img, net, target, enc, s)
    assert got.shape == want.shape == (H // s, W // s, want.shape[2])
    err = np.abs(got - want).max() / np.abs(want).max()
    print('relu%d_1 encoder %dx%d, halo %d: %.3g' % (level, H, W, enc, err))
    assert err <= 1e-5
    out = wrap_oracle.decode(want, net, target)
    dgot = _padded_decode(want, net, target, before, after, s)
    assert dgot.shape == out.shape == (H, W, 3)
    derr = np.abs(dgot - out).max() / np.abs(out).max()
    print('relu%d_1 decoder %dx%d, halo %d / %d: %.3g' % (level, H // s, W // s, before, after, derr))
    assert derr <= 1e-5
    if level in (3, 5):
        # the layer walk needs 10 / 70 image pixels on either side of the tile (csrc/banded.hip): 12 / 80 as multiples of the stride,
        # which the library rounds up to 16 / 96.  That many still reproduce the pass; one stride -- one feature pixel -- fewer
        # do not, by the size of the values themselves, and neither does a decoder halo one feature pixel short
        need = {3: 12, 5: 80}[level]
        tight = np.abs(_padded_encode(img, net, target, need, s) - want).max() / np.abs(want).max()
        short = np.abs(_padded_encode(img, net, target, need - s, s) - want).max() / np.abs(want).max()
        dshort = np.abs(_padded_decode(want, net, target, before, after - 1, s) - out).max() / np.abs(out).max()
        print('relu%d_1 encoder halo %d: %.3g, one stride short: %.3g; decoder one short: %.3g' % (level, need, tight, short, dshort))
        assert tight <= 1e-5 and short > 1e-2 and dshort > 1e-2


def test_the_periodic_oracle_is_shift_equivariant(net):
    """the property the construction is for, on the oracle itself: a roll of the input by a multiple of the stride is the same
    roll of the features, and of the decoded image"""
    img = np.float32(synthetic_image(77, 16, 24)) / np.float32(255)
    f = wrap_oracle.encode(img, net, 'relu3_1')
    fr = wrap_oracle.encode(np.roll(img, (4, 8), (0, 1)), net, 'relu3_1')
    assert np.abs(fr - np.roll(f, (1, 2), (0, 1))).max() <= 1e-5 * np.abs(f).max()
    d = wrap_oracle.decode(f, net, 'relu3_1')
    dr = wrap_oracle.decode(np.roll(f, (1, 2), (0, 1)), net, 'relu3_1')
    assert np.abs(dr - np.roll(d, (4, 8), (0, 1))).max() <= 1e-5 * np.abs(d).max()
    plain = oracle.encode(img, net, ['relu3_1'], wino=False)['relu3_1']
    plain_r = oracle.encode(np.roll(img, (4, 8), (0, 1)), net, ['relu3_1'], wino=False)['relu3_1']
    assert np.abs(plain_r - np.roll(plain, (1, 2), (0, 1))).max() > 1e-2 * np.abs(plain).max()       # the reflect-padded net is not


# ---- the seam case of tests/test_gpu_wrap.py ------------------------------------------------------------------------------------
def test_the_seam_case_holds_on_the_oracle():
    """the tile the GPU test measures, made by the periodic oracle from the same noise: the step across either joint is no larger
    than the largest step between adjacent interior rows or columns; the plain oracle's frame is printed beside it"""
    import texture_oracle
    from oracle.contractive import contractive_weights
    case = wrap_oracle.SEAM_CASE
    w = contractive_weights(7)
    noise = texture_oracle.noise(case['size'][0], case['size'][1], case['seed'], case['sample'])
    style = synthetic_image(*case['style'])
    tile = wrap_oracle.stylize(noise, style, w, case['targets'], alpha=case['alpha'])
    joint, inner = wrap_oracle.seam_steps(tile)
    pj, pi = wrap_oracle.seam_steps(oracle.stylize(noise, style, w, case['targets'], alpha=case['alpha']))
    print('seam, oracle: tile joint %.3f interior max %.3f | plain joint %.3f interior max %.3f' % (joint, inner, pj, pi))
    assert tile.shape == noise.shape and joint <= inner


# ---- refusals, before any GPU call ------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu(lib):
    from wct_tf_amd.context import Context, PreparedStyle
    from wct_tf_amd.wct import WCT
    model = WCT.__new__(WCT)                             # no context behind it: a refusal that reached the library would fail loudly
    model.relu_targets = ALL
    handle = PreparedStyle(None, None, None, [1, 2, 3, 4, 5])
    frames = np.zeros((2, 32, 48, 3), np.uint8)
    image = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match='PreparedStyle'):
        model.predict_frames(frames, image, wrap=True)
    for kw in (dict(swap5=True), dict(warm=object()), dict(content_colors=True), dict(resize=(32, 48))):
        with pytest.raises(ValueError, match='%s is not served with wrap' % list(kw)[0]):
            model.predict_frames(frames, handle, wrap=True, **kw)
    with pytest.raises(ValueError, match='multiples of 16'):
        model.predict_frames(np.zeros((2, 40, 48, 3), np.uint8), handle, wrap=True)
    with pytest.raises(ValueError, match='too small for relu5_1'):
        model.predict_frames(np.zeros((2, 16, 48, 3), np.uint8), handle, wrap=True)
    with pytest.raises(ValueError, match=r'\[F\]\[H\]\[W\]\[3\]'):
        model.predict_frames(frames[0], handle, wrap=True)
    with pytest.raises(ValueError, match='tile takes one style'):
        model.synthesize([image, image], (32, 48), tile=True)
    with pytest.raises(ValueError, match='multiples of 16'):
        model.synthesize(image, (40, 48), tile=True)
    with pytest.raises(ValueError, match='passes'):
        model.synthesize(image, (32, 48), tile=True, passes=0)
    ctx = Context.__new__(Context)
    with pytest.raises(ValueError, match='pads'):
        ctx.wrap_pad(np.zeros((2, 2, 3), np.float32), (1, -1, 0, 0))
    with pytest.raises(ValueError, match='HxWxC'):
        ctx.wrap_pad(np.zeros((2, 2), np.float32), (1, 1, 0, 0))
    with pytest.raises(ValueError, match='multiples of 4'):
        ctx.encode_wrap(np.zeros((18, 20, 3), np.float32), 'relu3_1')
    with pytest.raises(ValueError, match='1 .. 16'):
        ctx.texture_prepared_wrap_batch(32, 48, 1, 0, 0, None, ALL, passes=0)


_BASE = ['--relu-targets', 'relu1_1', '--out-path', 'o', '--synthetic-weights', '1']


def _check(argv):
    from wct_tf_amd import texture
    parser = texture.build_parser()
    args = parser.parse_args(argv)
    texture.check_texture_args(parser, args)
    return args


def test_cli_tile_flags(capsys):
    a = _check(_BASE + ['--style-path', 's.png'])
    assert a.tile is False and a.tile_preview is None                 # without the flags: what it was
    a = _check(_BASE + ['--style-path', 's.png', '--tile', '--tile-preview', '2'])
    assert a.tile is True and a.tile_preview == 2
    assert _check(_BASE + ['--style-path', 's.png', '--tile']).tile_preview is None
    for argv, word in ((['--style-path', 's', '--tile-preview', '2'], '--tile-preview needs --tile'),
                       (['--style-path', 's', '--tile', '--tile-preview', '0'], '--tile-preview must be'),
                       (['--interp-styles', 'a', 'b', '--tile'], '--tile takes one style')):
        with pytest.raises(SystemExit):
            _check(_BASE + argv)
        assert word in capsys.readouterr().err
