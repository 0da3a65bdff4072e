"""Style regions on the GPU -- a prepared style from a labelled part of its image: the op-level twins against wct_transform /
wct_adain on the selected rows (bit for bit) and the float64 oracle, region handles against plain handles and against each other,
the state cache under more keys than it holds, regions too small to carry a style, the ABI refusals, the whole predict() against
tests/region_oracle.py, and the CLI."""
import ctypes as C
import os

import numpy as np
import pytest

import mask_oracle
import region_oracle
from conftest import rel_err, max_rel
from wct_tf_amd import _lib
from wct_tf_amd.weights import RELU_TARGETS, synthetic_features, synthetic_image, synthetic_weights

pytestmark = pytest.mark.gpu
WCT_TOL = 1e-3                       # tests/test_gpu_mask.py
SMALL = ['relu3_1', 'relu2_1', 'relu1_1']
# the rows of every label of blobs(100 + c + k, 20, 26, k): >= 2 each, all below C at 512 (rank-deficient), all above it at 64
COUNTS = {(64, 2): [234, 286], (64, 3): [162, 105, 253], (256, 2): [324, 196], (256, 3): [152, 195, 173],
          (512, 2): [300, 220], (512, 3): [121, 174, 225]}
MAP_ROWS = {'relu1_1': [3129, 3207], 'relu2_1': [778, 806], 'relu3_1': [195, 201]}       # blobs(7, 72, 88, 2), per level


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
    """blob-shaped random labels 0 .. k-1: the argmax of k smoothed noise fields (tests/test_gpu_mask.py)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((k, h, w))
    for _ in range(4):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5
    return np.uint8(np.argmax(f, 0))


class Handles(object):
    """prepared styles closed on exit (None entries skipped)"""

    def __init__(self, *handles):
        self.h = [x for hs in handles for x in (hs if isinstance(hs, (list, tuple)) else [hs])]

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        for h in self.h:
            if h is not None:
                h.close()


# ---- 1. op level: the rows are selected on the device, the transform is the plain one --------------------------------------
@pytest.mark.parametrize('c', [64, 256, 512])
@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('mode', ['tf', 'np'])
def test_transform_region_is_transform_on_the_selected_rows(ctx, c, k, mode):
    fc = _flat(synthetic_features(50 + c, c, 24, 28, 2.0))
    fs = np.ascontiguousarray(synthetic_features(60 + c, c, 20, 26, 2.0).reshape(20, 26, c))
    labels = blobs(100 + c + k, 20, 26, k)
    assert list(np.bincount(labels.reshape(-1), minlength=k)) == COUNTS[c, k]
    lib_mode = _lib.WCT_NP if mode == 'np' else _lib.WCT_TF
    kw64 = {'dtype': np.float64} if mode == 'tf' else {}
    for lab in range(k):
        rows = np.ascontiguousarray(fs.reshape(-1, c)[labels.reshape(-1) == lab])
        got, sweeps = ctx.transform_region(fc, fs, labels, lab, 0.8, lib_mode, return_sweeps=True)
        want, wsw = ctx.transform(fc, rows, 0.8, lib_mode, return_sweeps=True)
        assert np.array_equal(got, want), (lab, len(rows))
        assert list(sweeps) == list(wsw)
        o64 = mask_oracle.region_transform(np.float64(fc), np.float64(rows), 0.8, mode, **kw64)
        o32 = mask_oracle.region_transform(fc, rows, 0.8, mode)
        e, ref = rel_err(got, o64), rel_err(o32, o64)
        print('label %d: Ns = %d of C = %d, %s: %.2e from the float64 oracle (float32 oracle %.2e), max %.2e' % (
            lab, len(rows), c, mode, e, ref, max_rel(got, o64)))
        assert e < max(WCT_TOL, 4 * ref)


@pytest.mark.parametrize('c', [64, 256, 512])
@pytest.mark.parametrize('k', [2, 3])
def test_adain_region_is_adain_on_the_selected_rows(ctx, c, k):
    fc = _flat(synthetic_features(50 + c, c, 24, 28, 2.0))
    fs = np.ascontiguousarray(synthetic_features(60 + c, c, 20, 26, 2.0).reshape(20, 26, c))
    labels = blobs(100 + c + k, 20, 26, k)
    for lab in range(k):
        rows = np.ascontiguousarray(fs.reshape(-1, c)[labels.reshape(-1) == lab])
        got = ctx.adain_region(fc, fs, labels, lab, 0.7)
        assert np.array_equal(got, ctx.adain(fc, rows, 0.7)), lab
        assert rel_err(got, mask_oracle.region_transform(fc, rows, 0.7, 'adain')) < 1e-5


# ---- 2. a region that is the whole image is a plain handle ------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(wct_mode='np'), dict(adain=True), dict(f32=True)])
def test_a_whole_image_region_is_the_plain_handle(small_ctx, kw):
    c, a = synthetic_image(11, 96, 80), synthetic_image(12, 72, 88)
    if kw.pop('f32', False):
        c, a = np.float32(c) + 0.25, np.float32(a) - 0.25
    zero = np.zeros((72, 88), np.uint8)
    with Handles(small_ctx.prepare_style(a, SMALL, **kw), small_ctx.prepare_style(a, SMALL, region=(zero, 0), **kw)) as (plain, region):
        assert region.region is not None and plain.region is None
        for r, (h, w) in zip(SMALL, ((18, 22), (36, 44), (72, 88))):
            assert region.rows(r) == plain.rows(r) == h * w
        assert np.array_equal(small_ctx.stylize_prepared(c, region, SMALL, alpha=0.7, **kw),
                              small_ctx.stylize_prepared(c, plain, SMALL, alpha=0.7, **kw))
        cm = np.zeros(c.shape[:2], np.uint8)
        assert np.array_equal(small_ctx.stylize_prepared_masked(c, [region], cm, SMALL, alpha=0.7, **kw),
                              small_ctx.stylize_prepared_masked(c, [plain], cm, SMALL, alpha=0.7, **kw))


# ---- 3. the K regions of one image against K single-region handles -----------------------------------------------------------
def test_prepare_style_regions_gives_the_single_region_handles(small_ctx):
    c, s = synthetic_image(13, 96, 80), synthetic_image(14, 72, 88)
    m = blobs(7, 72, 88, 2)
    cm = blobs(8, 96, 80, 2)
    group = small_ctx.prepare_style_regions(s, m, 2, SMALL)
    single = [small_ctx.prepare_style(s, SMALL, region=(m, k)) for k in range(2)]
    swapped = [small_ctx.prepare_style(s, SMALL, region=(np.uint8(1 - m), 1 - k)) for k in range(2)]
    whole = small_ctx.prepare_style(s, SMALL)
    with Handles(group, single, swapped, whole):
        assert all(h is not None for h in group)
        frames = []
        for hs in (group, single, swapped):
            for r in SMALL:
                assert [h.rows(r) for h in hs] == MAP_ROWS[r], r
            frames.append([small_ctx.stylize_prepared(c, hs[0], SMALL, alpha=0.8), small_ctx.stylize_prepared(c, hs[1], SMALL, alpha=0.8),
                           small_ctx.stylize_prepared_masked(c, hs, cm, SMALL, alpha=0.8),
                           small_ctx.stylize_prepared_masked(c, hs, cm, SMALL, alpha=0.8, adain=True)])
        for other in frames[1:]:
            for x, y in zip(frames[0], other):
                assert np.array_equal(x, y)
        # a region is not the whole image, and the two regions differ
        assert not np.array_equal(frames[0][0], frames[0][1])
        assert not np.array_equal(frames[0][0], small_ctx.stylize_prepared(c, whole, SMALL, alpha=0.8))
        # a sibling outlives the other: freed on its own, the image and the map stay with the survivor
        group[0].close()
        assert np.array_equal(small_ctx.stylize_prepared(synthetic_image(15, 160, 144), group[1], SMALL, alpha=0.8),
                              small_ctx.stylize_prepared(synthetic_image(15, 160, 144), single[1], SMALL, alpha=0.8))


# ---- 4. the cache: more keys than a level holds ------------------------------------------------------------------------------
def test_a_region_handle_refills_evicted_states_with_the_same_bits(small_ctx):
    s = synthetic_image(14, 72, 88)
    m = blobs(7, 72, 88, 2)
    contents = [synthetic_image(20 + i, h, w) for i, (h, w) in enumerate(((96, 80), (160, 144), (200, 184)))]
    with Handles(small_ctx.prepare_style(s, SMALL, region=(m, 1))) as (h,):
        first = small_ctx.stylize_prepared(contents[0], h, SMALL, alpha=0.8)
        for c in contents[1:] + contents:                        # three sizes in two modes and AdaIN: past the 4 keys of a level
            for kw in (dict(), dict(wct_mode='np'), dict(adain=True)):
                small_ctx.stylize_prepared(c, h, SMALL, alpha=0.8, **kw)
        again = small_ctx.stylize_prepared(contents[0], h, SMALL, alpha=0.8)
        assert np.array_equal(first, again)
    with Handles(small_ctx.prepare_style(s, SMALL, region=(m, 1))) as (fresh,):
        assert np.array_equal(small_ctx.stylize_prepared(contents[0], fresh, SMALL, alpha=0.8), first)


# ---- 5. regions too small to carry a style, and the other refusals --------------------------------------------------------------
def test_too_small_regions_and_the_abi_refusals_leave_the_context_usable(small_ctx):
    lib = small_ctx.lib
    s = np.ascontiguousarray(synthetic_image(14, 72, 88))
    c = synthetic_image(13, 96, 80)
    m = np.zeros((72, 88), np.uint8)
    m[1:4, 1:4] = 1                                               # label 1: 9 / 1 / 0 rows at relu1_1 / relu2_1 / relu3_1
    u8p = lambda a: a.ctypes.data_as(_lib._U8)
    lv = (C.c_int * 3)(1, 2, 3)
    with Handles(small_ctx.prepare_style_regions(s, m, 2, SMALL)) as group:
        assert group[0] is not None and group[1] is None
        assert [group[0].rows(r) for r in SMALL] == [18 * 22, 36 * 44 - 1, 72 * 88 - 9]
        before = small_ctx.stylize_prepared(c, group[0], SMALL, alpha=0.8)
    with pytest.raises(_lib.WCTHipError):
        small_ctx.prepare_style(s, SMALL, region=(m, 1))

    def region(map_, label, flags=0, levels=lv):
        h = C.c_void_p(1)
        rc = lib.wct_style_prepare_region(small_ctx.h, u8p(s), 72, 88, None if map_ is None else u8p(map_), label, levels, len(levels),
                                          flags, C.byref(h))
        assert rc == 0 or h.value is None                         # no handle on a refusal
        return rc, h

    def regions(map_, k, flags=0):
        hs = (C.c_void_p * 8)(*([1] * 8))
        rc = lib.wct_style_prepare_regions(small_ctx.h, u8p(s), 72, 88, None if map_ is None else u8p(map_), k, lv, 3, flags, hs)
        assert rc == 0 or not 1 <= k <= 8 or all(hs[j] is None for j in range(k))      # no handle on a refusal
        return rc

    rc, _ = region(m, 1)                                          # (the message names the first level that is too small)
    assert rc == -2 and b'relu2_1' in lib.wct_last_error() and b'1 rows' in lib.wct_last_error()
    rc, _ = region(m, 1, levels=(C.c_int * 2)(3, 1))
    assert rc == -2 and b'relu3_1' in lib.wct_last_error() and b'0 rows' in lib.wct_last_error()
    rc, h = region(m, 1, levels=(C.c_int * 1)(1))                 # 9 rows at relu1_1 alone: a style
    assert rc == 0 and h.value
    n = C.c_int()
    assert lib.wct_style_rows(small_ctx.h, h, 1, C.byref(n)) == 0 and n.value == 9
    assert lib.wct_style_rows(small_ctx.h, h, 2, C.byref(n)) == -2
    lib.wct_style_free(small_ctx.h, h)
    assert lib.wct_style_rows(small_ctx.h, h, 1, C.byref(n)) == -3          # freed: not a live handle
    for args in ((None, 0), (m, 8), (m, -1), (m, 0, _lib.FLAG_SWAP5), (m, 0, _lib.FLAG_STYLE_SHARED)):
        rc, _ = region(*args)
        assert rc == -2 and lib.wct_last_error(), args
    for args in ((None, 2), (m, 0), (m, 9), (m, 1), (m, 2, _lib.FLAG_SWAP5), (m, 2, _lib.FLAG_STYLE_SHARED)):   # (m, 1): a label >= K
        assert regions(*args) == -2 and lib.wct_last_error(), args
    # op level: a label with fewer than 2 rows, a label out of range, no labels
    fc, fs = np.ones((16, 64), np.float32), np.ones((4, 4, 64), np.float32)
    o = np.zeros((16, 64), np.float32)
    lab = np.zeros(16, np.uint8)
    lab[3] = 1
    for labels, label in ((lab, 1), (lab, 2), (lab, 8), (None, 0)):
        lp = None if labels is None else u8p(labels)
        assert lib.wct_transform_region(small_ctx.h, _lib.fptr(fc), 16, _lib.fptr(fs), 4, 4, 64, lp, label, C.c_float(1), _lib.WCT_TF,
                                        C.c_float(-1), _lib.fptr(o), None) == -2
        assert lib.wct_adain_region(small_ctx.h, _lib.fptr(fc), 16, _lib.fptr(fs), 4, 4, 64, lp, label, C.c_float(1), C.c_float(1e-5),
                                    _lib.fptr(o)) == -2
    with Handles(small_ctx.prepare_style(s, SMALL, region=(m, 0))) as (h0,):
        assert np.array_equal(small_ctx.stylize_prepared(c, h0, SMALL, alpha=0.8), before)


# ---- 6. the whole predict() against the oracle ------------------------------------------------------------------------------------
def test_style_regions_five_levels_512_end_to_end_on_a_well_conditioned_net():
    """The floors, net, content and content mask of test_stylize_masked_five_levels_512_end_to_end_on_a_well_conditioned_net
    (tests/test_gpu_mask.py); ONE 512 x 512 style carries both regions under a style map split at column 208 -- 416 and 608 rows
    of C = 512 at relu5_1, neither near C -- against tests/region_oracle.py."""
    from oracle.contractive import contractive_weights
    from wct_tf_amd.context import Context
    w = contractive_weights(7)
    c = synthetic_image(1000, 512, 512)
    s = synthetic_image(2000, 512, 512)
    mask = np.zeros((512, 512), np.uint8)
    mask[:, 192:] = 1
    smap = np.zeros((512, 512), np.uint8)
    smap[:, 208:] = 1
    cx = Context(0)
    try:
        cx.set_weights(w)
        with Handles(cx.prepare_style_regions(s, smap, 2, RELU_TARGETS)) as hs:
            assert [h.rows('relu5_1') for h in hs] == [416, 608]
            got = cx.stylize_prepared_masked(c, hs, mask, RELU_TARGETS, alpha=0.8)
    finally:
        cx.close()
    want = region_oracle.stylize_regions(c, [s, s], [smap, smap], mask, w, RELU_TARGETS, alpha=0.8)
    d = np.abs(got.astype(int) - want.astype(int))
    psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((got.astype(np.float64) - want) ** 2), 1e-12))
    print('style regions end to end: psnr %.1f dB, max LSB %d, mean LSB %.4f, frame std %.1f' % (psnr, d.max(), d.mean(), want.std()))
    assert got.shape == want.shape == (512, 512, 3) and want.std() > 15
    assert psnr > 42.0 and d.mean() <= 1.6 and d.max() <= 20


# ---- 7. the facade and the CLI ------------------------------------------------------------------------------------------------------
def _matrices(stats):
    return sum(v['matrices'] for v in stats.values())


def test_cli_style_masks_end_to_end(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from wct_tf_amd import stylize, utils
    from wct_tf_amd.wct import WCT
    paths = []
    for name, seed, (h, w) in (('cat', 31, (64, 80)), ('a', 32, (64, 48))):
        p = str(tmp_path / (name + '.png'))
        utils.save_img(p, synthetic_image(seed, h, w))
        paths.append(p)
    grey = np.zeros((32, 40), np.uint8)                          # the content map at half the content's size
    grey[:, 18:] = 255
    sgrey = np.zeros((64, 48), np.uint8)                         # the style map at the style's size
    sgrey[30:] = 255
    mpath, smpath = str(tmp_path / 'm.png'), str(tmp_path / 'am.png')
    Image.fromarray(grey).save(mpath)
    Image.fromarray(sgrey).save(smpath)
    calls = {'regions': 0, 'single': 0}
    regions, single = WCT.prepare_style_regions, WCT.prepare_style
    monkeypatch.setattr(WCT, 'prepare_style_regions', lambda self, *a, **k: (calls.__setitem__('regions', calls['regions'] + 1), regions(self, *a, **k))[1])
    monkeypatch.setattr(WCT, 'prepare_style', lambda self, *a, **k: (calls.__setitem__('single', calls['single'] + 1), single(self, *a, **k))[1])
    out_dir = str(tmp_path / 'out')
    base = ['--synthetic-weights', '5', '--relu-targets'] + SMALL + ['--content-path', paths[0], '--mask-path', mpath]
    # the single-photo form: one image, one map, prepared once for both regions
    assert stylize.main(base + ['--out-path', out_dir, '--mask-styles', paths[1], paths[1], '--style-masks', smpath, smpath]) == 1
    assert os.listdir(out_dir) == ['cat_mask_a+a.png'] and calls == {'regions': 1, 'single': 0}
    # a map for style 0 alone: style 1 is the whole image
    out2 = str(tmp_path / 'out2')
    assert stylize.main(base + ['--out-path', out2, '--mask-styles', paths[1], paths[1], '--style-masks', smpath, '-']) == 1
    assert calls == {'regions': 1, 'single': 2}
    monkeypatch.undo()
    model = WCT(None, SMALL, None, weights=synthetic_weights(5, relu_targets=SMALL))
    try:
        labels = np.zeros((64, 80), np.uint8)
        labels[:, 36:] = 1
        slab = np.uint8(sgrey // 128)
        a = utils.get_img(paths[1])
        want = model.predict_masked(utils.get_img(paths[0]), [a, a], labels, style_masks=[slab, slab])
        assert np.array_equal(utils.get_img(os.path.join(out_dir, 'cat_mask_a+a.png')), want)
        want2 = model.predict_masked(utils.get_img(paths[0]), [a, a], labels, style_masks=[slab, None])
        assert np.array_equal(utils.get_img(os.path.join(out2, 'cat_mask_a+a.png')), want2) and not np.array_equal(want, want2)
        assert np.array_equal(model.predict_frames_masked(utils.get_img(paths[0])[None], [a, a], labels, style_masks=[slab, slab])[0], want)
        # prepared once: one state per region and level, no more
        model.sess.eig_stats()
        with Handles(model.prepare_style_regions(a, slab, 2)) as hs:
            assert all(h is not None for h in hs) and _matrices(model.sess.eig_stats()) == 2 * len(SMALL)
        # a region too small to carry a style falls back to the whole image, with one line on stderr
        tiny = np.zeros((64, 48), np.uint8)
        tiny[1:4, 1:4] = 255
        tpath = str(tmp_path / 'tiny.png')
        Image.fromarray(tiny).save(tpath)
        capsys.readouterr()
        out3 = str(tmp_path / 'out3')
        assert stylize.main(base + ['--out-path', out3, '--mask-styles', paths[1], paths[1], '--style-masks', smpath, tpath]) == 1
        err = capsys.readouterr().err
        assert err.count('too small to carry a style') == 1
        assert np.array_equal(utils.get_img(os.path.join(out3, 'cat_mask_a+a.png')), want2)
    finally:
        model.sess.close()
