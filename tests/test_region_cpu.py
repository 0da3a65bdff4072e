"""Style regions -- a prepared style from a labelled part of its image --, the parts that need no GPU: the ABI declarations, the
CLI's parser errors, the Python refusals (raised before any library call), the host-side row count, and the region oracle
against the mask oracle."""
import os
import re

import numpy as np
import pytest

import mask_oracle
import region_oracle
from conftest import ROOT
from wct_tf_amd.weights import synthetic_image, synthetic_weights

SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
NEW_SYMBOLS = ('wct_style_prepare_region', 'wct_style_prepare_regions', 'wct_style_rows', 'wct_transform_region', 'wct_adain_region')


def test_region_symbols_declared_and_bound():
    from wct_tf_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wct_hip.h')).read(), flags=re.S)
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert re.search(r'^\s*int\s+%s\s*\(' % name, header, re.M), name
        assert name in bound, name


def test_region_symbols_exported():
    from wct_tf_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def _parse(argv, video=False):
    from wct_tf_amd import stylize, stylize_video
    mod = stylize_video if video else stylize
    parser = mod.build_parser()
    args = parser.parse_args(argv)
    mod.check_mask_args(parser, args)
    stylize.check_style_mask_args(parser, args)
    return args


BASE = ['--relu-targets', 'relu1_1', '--content-path', 'c.png', '--out-path', 'o']
VBASE = ['--relu-targets', 'relu1_1', '--in-path', 'frames', '--out-path', 'o']
MASKED = ['--mask-path', 'm.png', '--mask-styles', 'a.png', 'b.png']


def test_cli_style_masks_parse():
    args = _parse(BASE + MASKED + ['--style-masks', 'am.png', '-'])
    assert args.style_masks == ['am.png', '-']
    assert _parse(BASE + MASKED).style_masks is None
    assert _parse(VBASE + MASKED + ['--style-masks', 'sm.png', 'sm.png'], video=True).style_masks == ['sm.png', 'sm.png']


@pytest.mark.parametrize('base,extra,video', [
    (BASE, ['--style-path', 's.png', '--style-masks', 'am.png'], False),                  # without --mask-styles
    (BASE, MASKED + ['--style-masks', 'am.png'], False),                                  # a count other than K
    (BASE, MASKED + ['--style-masks', 'am.png', 'bm.png', 'cm.png'], False),
    (BASE, MASKED + ['--style-masks', 'am.png', 'bm.png', '--keep-colors'], False),
    (BASE, ['--mask-path', 'm.png', '--mask-styles', 'a.png', '--style-masks', 'am.png', '--swap5'], False),
    (VBASE, ['--style-path', 's.png', '--style-masks', 'am.png'], True),
    (VBASE, MASKED + ['--style-masks', 'am.png'], True),
])
def test_cli_style_masks_errors(base, extra, video, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(base + extra, video)
    assert e.value.code == 2
    assert 'error:' in capsys.readouterr().err


def test_python_refusals_come_before_any_library_call():
    """No context exists behind these objects (no __init__): a library call would fail with AttributeError, not ValueError."""
    from wct_tf_amd.context import Context
    from wct_tf_amd.wct import WCT
    ctx = Context.__new__(Context)
    img = np.zeros((16, 24, 3), np.uint8)
    z = np.zeros((16, 24), np.uint8)
    for region in ((z[:8], 0), (z.astype(np.float32), 0), (z, 8), (z, -1), (np.zeros((24, 16), np.uint8), 0)):
        with pytest.raises(ValueError):
            ctx.prepare_style(img, SMALL, region=region)
    for label_map, k in ((z + 2, 2), (z[:, :8], 2), (z.astype(np.float64), 2), (z, 0), (z, 9)):
        with pytest.raises(ValueError):
            ctx.prepare_style_regions(img, label_map, k, SMALL)
    feat = np.zeros((4, 6, 64), np.float32)
    for labels, label in ((np.zeros((4, 5), np.uint8), 0), (np.zeros((4, 6), np.float32), 0), (np.zeros((4, 6), np.uint8), 8)):
        with pytest.raises(ValueError):
            ctx.transform_region(np.zeros((10, 64), np.float32), feat, labels, label, 0.8, 1)
        with pytest.raises(ValueError):
            ctx.adain_region(np.zeros((10, 64), np.float32), feat, labels, label, 0.8)
    model = WCT.__new__(WCT)
    model.relu_targets = SMALL
    tiny = z.copy()
    tiny[1:4, 1:4] = 1                                            # label 1: no sample at stride 4
    for styles, maps, kw in (([img, img], [z, z[:8]], {}),        # a wrong map shape
                             ([img, img], [z, z.astype(np.float32)], {}),
                             ([img, img], [z], {}),               # a count other than K
                             ([img, img], [z, tiny], {}),         # too small to carry a style
                             ([img], [z], dict(swap5=True))):
        with pytest.raises(ValueError):
            model.predict_masked(img, styles, np.zeros((16, 24), np.uint8), style_masks=maps, **kw)
    with pytest.raises(ValueError):
        model.predict_frames_masked(img[None], [img, img], z, style_masks=[z, z[:8]])


def test_cli_region_preparation_refuses_keep_colors_and_swap5():
    import argparse
    from wct_tf_amd.stylize import prepare_style_regions
    for kw in (dict(keep_colors=True, swap5=False), dict(keep_colors=False, swap5=True)):
        with pytest.raises(ValueError):
            prepare_style_regions(None, ['a.png'], [np.zeros((8, 8, 3), np.uint8)], ['am.png'], argparse.Namespace(adain=False, **kw))


def test_region_rows_is_the_level_label_rule():
    from wct_tf_amd.context import region_rows
    rng = np.random.default_rng(4)
    m = np.uint8(rng.integers(0, 3, (37, 45)))
    for relu, (h, w, s) in (('relu1_1', (37, 45, 1)), ('relu2_1', (19, 23, 2)), ('relu3_1', (10, 12, 4)), ('relu4_1', (5, 6, 8))):
        for k in range(3):
            assert region_rows(m, k, relu) == int((mask_oracle.level_labels(m, h, w, s) == k).sum()), (relu, k)
    block = np.zeros((72, 88), np.uint8)
    block[1:4, 1:4] = 1                                           # the 3 x 3 block at rows / columns 1 .. 3: no sample at stride 4
    assert [region_rows(block, 1, r) for r in SMALL] == [0, 1, 9]


@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True)])
def test_region_oracle_with_all_zero_maps_is_the_mask_oracle(kw):
    w = synthetic_weights(5, relu_targets=SMALL)
    c, a = synthetic_image(11, 64, 48), synthetic_image(12, 40, 56)
    zero = np.zeros((64, 48), np.uint8)
    got = region_oracle.stylize_regions(c, [a], [np.zeros((40, 56), np.uint8)], zero, w, SMALL, alpha=0.7, **kw)
    assert np.array_equal(got, mask_oracle.stylize_masked(c, [a], zero, w, SMALL, alpha=0.7, **kw))
    assert np.array_equal(region_oracle.stylize_regions(c, [a], [None], zero, w, SMALL, alpha=0.7, **kw), got)


def test_region_oracle_selects_the_rows_of_the_label():
    rng = np.random.default_rng(6)
    feat = np.float32(rng.standard_normal((5, 6, 32)))
    m = np.uint8(rng.integers(0, 2, (10, 12)))
    rows = region_oracle.region_rows(feat, m, 1, 2)
    want = [feat[i, j] for i in range(5) for j in range(6) if m[min(2 * i, 9), min(2 * j, 11)] == 1]
    assert rows.shape == (len(want), 32) and np.array_equal(rows, np.stack(want))
    # two styles, each from its own half: the frame differs from whole-image styles, and the unlabelled half does not matter
    w = synthetic_weights(5, relu_targets=SMALL)
    c, a, b = synthetic_image(21, 32, 32), synthetic_image(22, 32, 40), synthetic_image(23, 40, 32)
    mask = np.zeros((32, 32), np.uint8)
    mask[:, 14:] = 1
    ma, mb = np.zeros((32, 40), np.uint8), np.ones((40, 32), np.uint8)
    mb[:18] = 0
    got = region_oracle.stylize_regions(c, [a, b], [ma, mb], mask, w, SMALL, alpha=0.8)
    whole = mask_oracle.stylize_masked(c, [a, b], mask, w, SMALL, alpha=0.8)
    assert got.shape == whole.shape and not np.array_equal(got, whole)
