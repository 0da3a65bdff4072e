"""The per-element judge of tests/pointwise.py, checked on the CPU: the reference itself must sit well inside the derived
bounds on every input the GPU tests use (tests/test_gpu_pointwise.py), and defects of the kind a tiled kernel can have, injected
into the reference output, must be flagged at their pixel.  Each defect test also records on which side of 1e-2 the whole-map
Frobenius ratio (conftest.rel_err), the gate these kernels had at ragged sizes, falls: it passes a dropped lo operand (by four
decades) and a single pixel 40 % off; it does see the defects that put errors of the size of a value on a whole row, column or
tile edge of maps this small, without saying where."""
import numpy as np
import pytest

import oracle
import pointwise as pw
from conftest import max_rel, rel_err


@pytest.fixture(scope='module')
def encoders():
    return pw.first_encoders()


# ---- the reference inside half the bound ------------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['he', 'x64'])
def test_first_reference_and_emulation_within_half_the_bound(encoders, which):
    """float32 oracle (1x1 preprocess, then conv1_1: NOT folded) and the emulation of the split-fp16 arithmetic."""
    enc = encoders[which]
    worst = {}
    for h, w in pw.FIRST_SIZES:
        for kind in pw.FIRST_INPUTS:
            img = pw.first_image(kind, h, w)
            want, s, a = pw.first_ref(img, enc)
            f32 = oracle.encode(img, {'encoder': enc}, ['relu1_1'])['relu1_1']
            r32, at32 = pw.judge(f32, want, s, pw.TAU_FIRST, a)
            rem, atem = pw.judge(pw.first_emulate(img, enc), want, s, pw.TAU_FIRST, a)
            print('first %s %dx%d %-5s float32 oracle %.3f at %s, emulation %.3f at %s' % (which, h, w, kind, r32, at32, rem, atem))
            assert r32 <= 0.5 and rem <= 0.5, (which, h, w, kind, r32, at32, rem, atem)
            worst[kind] = max(worst.get(kind, 0), rem)
    print('first %s: worst emulation ratio per input %s' % (which, worst))


def test_last_reference_within_half_the_bound():
    for h, w, kind, seed, tap in pw.last_cases():
        feat = pw.last_features(kind, h, w)
        assert np.array_equal(feat, pw.h16(feat)) and feat.min() >= 0
        wt, b = pw.last_filters(seed, tap)
        want, s = pw.last_ref(feat, wt, b)
        r, at = pw.judge(oracle.conv3x3_reflect(feat, pw.h16(wt), b, relu=False), want, s, pw.TAU_LAST)
        print('last %dx%d %s tap %s: float32 oracle %.3f at %s' % (h, w, kind, tap, r, at))
        assert r <= 0.5, (h, w, kind, tap, r, at)


@pytest.mark.parametrize('case', pw.DIRECT_CASES, ids=lambda c: '%d-%dx%dx%d' % c[:4])
def test_direct_reference_within_half_the_bound(case):
    """The fp32 map of the float32 oracle within half the bound, unpooled and pooled; rounded to fp16 (what the kernel
    stores: up to 2^-11 |want| by itself, the whole of that term) within the bound for fp16 output.  And the tile
    configuration each shape is listed under is the one the launch policy picks."""
    c, b, h, w, cfg = case
    assert pw.tile_config(c, b, h, w) == cfg
    x, wt, bias = pw.direct_inputs(c, b, h, w)
    sel = [0, b - 1] if b > 4 else list(range(b))      # (the large batches: their first and last image; every image is an input of the same kind)
    x = x[sel]
    want, s = pw.direct_ref(x, wt, bias)
    f32 = np.stack([oracle.conv3x3_reflect(pw.h16(xi), pw.h16(wt), bias, True) for xi in x])
    assert (want == 0).mean() > 0.2                    # negative pre-activations everywhere ...
    assert (want[:, -1] == 0).any() and (want[:, :, -1] == 0).any()       # ... and on the ragged edges
    tau = pw.tau_direct(c)
    for pool in (False, True):
        g = np.stack([oracle.maxpool2x2_same(f) for f in f32]) if pool else f32
        r, at = pw.judge(g, want, s, tau, pool=pool)
        r16, at16 = pw.judge(pw.h16(g), want, s, tau, pool=pool, fp16_out=True)
        print('direct %s pool=%d: float32 oracle %.3f at %s, rounded to fp16 %.3f at %s' % (case, pool, r, at, r16, at16))
        assert r <= 0.5 and r16 <= 1.0, (case, pool, r, at, r16, at16)


def test_every_tile_configuration_is_listed():
    for c, want in ((64, {'8,64,2,2', '16,64,4,1', '32,64,4,1'}), (128, {'8,64,2,2', '16,64,4,1', '32,64,4,1', '16,128,2,2'})):
        assert {k[4] for k in pw.DIRECT_CASES if k[0] == c} == want
    # the two shapes of tests/test_gpu_ops.py::test_conv3x3 once commented as the tall tile: 24 x 12 = 288 tall tiles < 512
    assert pw.tile_config(64, 1, 360, 376) == '16,64,4,1' and pw.tile_config(64, 1, 368, 360) == '16,64,4,1'


def test_the_two_float64_convolutions_agree():
    """pointwise._conv64 switches to torch's float64 conv2d for the large maps: the same sums (of fp16 x fp16 products they are
    exact in float64 whatever the order; on fp32 operands they differ by the order alone)."""
    x, wt, bias = pw.direct_inputs(64, 2, 17, 33)
    for xx, ww in ((pw.h16(x), pw.h16(wt)), (x, wt)):
        a = pw._conv64(xx, ww, bias, False)
        b = pw._conv64(xx, ww, bias, False, torch_from=0)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-14 * np.abs(a).max()
    assert np.array_equal(pw._conv64(pw.h16(x), pw.h16(wt), bias, False), pw._conv64(pw.h16(x), pw.h16(wt), bias, False, torch_from=0))


def test_direct_reference_where_cin_differs_from_cout():
    """The direct kernel's added cases (Cin != Cout, the folded upsample, the fp32 epilogue of the tap layers): each is listed
    under the tile configuration the policy picks, and the float32 oracle sits within half of tau_direct(Cin)."""
    for ci, co, b, h, w, up, pools, cfg in pw.DIRECT_MIXED_CASES:
        s = 2 if up else 1
        assert pw.tile_config(co, b, h * s, w * s) == cfg
        x, wt, bias = pw.layer_inputs(ci, co, b, h, w)
        x = x[[0, b - 1]] if b > 4 else x
        want, sm = pw.conv_ref(pw.h16(x), pw.h16(wt), bias, relu=True, up=up)
        f32 = np.stack([oracle.conv3x3_reflect(oracle.upsample2x_nearest(pw.h16(xi)) if up else pw.h16(xi), pw.h16(wt), bias, True) for xi in x])
        assert (want[:, -1] == 0).any() and (want[:, :, -1] == 0).any()
        for pool in ((False, True) if pools else (False,)):
            g = np.stack([oracle.maxpool2x2_same(f) for f in f32]) if pool else f32
            r, at = pw.judge(g, want, sm, pw.tau_direct(ci), pool=pool)
            r16, at16 = pw.judge(pw.h16(g), want, sm, pw.tau_direct(ci), pool=pool, fp16_out=True)
            print('direct %d->%d %dx%dx%d up=%d pool=%d: float32 oracle %.3f at %s, rounded to fp16 %.3f at %s' % (ci, co, b, h, w, up, pool, r, at, r16, at16))
            assert r <= 0.5 and r16 <= 1.0, (ci, co, b, h, w, up, pool, r, r16)
    for ci, co, h, w, relu, cfg in pw.TAP_CASES:
        assert pw.tile_config(co, 1, h, w) == cfg
        x, wt, bias = pw.layer_inputs(ci, co, 1, h, w)
        want, sm = pw.conv_ref(pw.h16(x[0]), pw.h16(wt), bias, relu=relu)
        r, at = pw.judge(oracle.conv3x3_reflect(pw.h16(x[0]), pw.h16(wt), bias, relu), want, sm, pw.tau_direct(ci))
        print('tap %d->%d %dx%d relu=%d: float32 oracle %.3f at %s' % (ci, co, h, w, relu, r, at))
        assert r <= 0.5 and ((want < 0).any() or relu)
    assert {c[7] for c in pw.DIRECT_MIXED_CASES} == {'8,64,2,2', '16,128,2,2'}


# ---- the reduced-FLOP kernel: policy, coverage, reference, emulation -----------------------------------------------------------

def test_wino_cases_select_their_tile_shape_and_cover_every_edge():
    """Every case is listed under the shape launch_conv3x3_wino picks for it, and each of the three shapes occurs with an odd
    H, a last tile column one pixel wide, the upsample, the no-ReLU epilogue, filters from both packers (the device's for
    Cin < 256, the host's from 256) and more than one channel block."""
    for ci, co, b, h, w, up, norelu, cfg in pw.WINO_CASES:
        s = 2 if up else 1
        assert pw.wino_config(co, b, h * s, w * s) == cfg, (ci, co, b, h, w, up)
        assert ci % 64 == 0 and co % 64 == 0 and h * s > 1 and w * s > 1
    for cfg, bn in (('IL16', 128), ('8x128', 128), ('8x64', 64)):
        cases = [c for c in pw.WINO_CASES if c[7] == cfg]
        assert any(c[3] % 2 == 1 and not c[5] for c in cases), cfg
        assert any(c[4] % 16 == 1 and not c[5] for c in cases), cfg
        assert any(c[5] for c in cases) and any(c[6] for c in cases), cfg
        assert any(c[0] in (64, 128) for c in cases) and any(c[0] >= 256 and c[1] >= 256 for c in cases), cfg
        assert any(c[1] // bn > 1 for c in cases), cfg
    # the shared images of the two 17x33 cases
    a, b = pw.layer_inputs(256, 256, 32, 17, 33), pw.layer_inputs(256, 256, 16, 17, 33)
    assert np.array_equal(a[0][:16], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # a single image of every case selects <8,64,2,2>: the GPU test's batch == single check crosses the shapes for IL16 and 8x128
    assert all(pw.wino_config(c[1], 1, c[3] * (2 if c[5] else 1), c[4] * (2 if c[5] else 1)) == '8x64' for c in pw.WINO_CASES)


@pytest.mark.parametrize('case', pw.WINO_CASES, ids=pw.wino_case_id)
def test_wino_reference_and_emulation_within_the_bounds(case):
    """The Winograd form with exact U, T IS the layer (1e-13 of s); an fp32-accumulating emulation of the kernel's order sits
    within half of A before the fp16 store (against tau_wino s_A alone, and so against the whole bound), within A after it (the
    rounding term is the whole of the store's error), and within half of B before / B after the store; unpooled and pooled."""
    ci, co, b, h, w, up, norelu, cfg = case
    x, wt, bias = pw.layer_inputs(ci, co, b, h, w)
    x = x[[0, b - 1]] if b > 4 else x
    (pa, sa), (pb, sb) = pw.wino_ref(x, wt, bias, relu=False, up=up)
    assert (np.abs(pw.wino_exact(x, wt, bias, up) - pb) <= 1e-13 * sb).all()
    pre = np.stack([pw.wino_emulate(xi, wt, bias, relu=False, up=up) for xi in x])
    ta, tb = pw.tau_wino(ci), pw.tau_wino_b(ci)
    for relu in ((True, False) if norelu else (True,)):
        act = (lambda v: np.maximum(v, 0)) if relu else (lambda v: v)
        wa, wb, em = act(pa), act(pb), act(pre)
        if relu:
            assert (wa == 0).mean() > 0.2 and (wa[:, -1] == 0).any() and (wa[:, :, -1] == 0).any()
        for pool in ((False, True) if relu else (False,)):
            g = pw.pool_same(em) if pool else em
            r0, at0 = pw.judge(g, wa, sa, ta, pool=pool)
            r1, _ = pw.judge(g, wa, sa, ta, pool=pool, fp16_out=True)
            r2, at2 = pw.judge(pw.h16(g), wa, sa, ta, pool=pool, fp16_out=True)
            rb0, atb0 = pw.judge(g, wb, sb, tb, pool=pool)
            rb1, atb1 = pw.judge(pw.h16(g), wb, sb, tb, pool=pool, fp16_out=True)
            print('wino %s relu=%d pool=%d: A before the store %.4f (%.4f of tau s alone, at %s), after %.3f at %s; B before %.3f at %s, after %.3f at %s'
                  % (pw.wino_case_id(case), relu, pool, r1, r0, at0, r2, at2, rb0, atb0, rb1, atb1))
            assert r0 <= 0.5 and r1 <= 0.5 and r2 <= 1.0 and rb0 <= 0.5 and rb1 <= 1.0, (case, relu, pool, r0, r1, r2, rb0, rb1)


@pytest.mark.parametrize('case', pw.WINO_SUBNORMAL_CASES, ids=pw.wino_case_id)
def test_wino_subnormal_rows_are_kept(case):
    """Activations scaled by 2^-15: the emulation (which keeps fp16 subnormals, as the kernel's denormal mode does) stays inside
    A and B with the absolute term of a subnormal store; the same emulation with the subnormals of T flushed to zero does not."""
    ci, co, b, h, w, up, norelu, cfg = case
    assert pw.wino_config(co, b, h, w) == cfg
    x, wt, bias = pw.subnormal_inputs(case)
    x = x[[0, b - 1]] if b > 4 else x
    x16 = pw.h16(x)
    assert 0.3 < ((np.abs(x16) < 2.0 ** -14) & (x16 != 0)).mean() < 0.7          # (half of the inputs are exact zeros after the ReLU; nearly all the rest are subnormal)
    (wa, sa), (wb, sb) = pw.wino_ref(x, wt, bias, relu=True)
    em = np.stack([pw.wino_emulate(xi, wt, bias) for xi in x])
    r0, _ = pw.judge(em, wa, sa, pw.tau_wino(ci))
    r1, at1 = pw.judge(pw.h16(em), wa, sa, pw.tau_wino(ci), a=pw.A16_SUBNORMAL, fp16_out=True)
    rb, atb = pw.judge(pw.h16(em), wb, sb, pw.tau_wino_b(ci), a=pw.A16_SUBNORMAL, fp16_out=True)
    bad = pw.h16(np.stack([pw.wino_emulate(xi, wt, bias, defect='flush') for xi in x]))
    rf, atf = pw.judge(bad, wa, sa, pw.tau_wino(ci), a=pw.A16_SUBNORMAL, fp16_out=True)
    rfb, _ = pw.judge(bad, wb, sb, pw.tau_wino_b(ci), a=pw.A16_SUBNORMAL, fp16_out=True)
    print('wino subnormal %s: A before the store %.4f, after %.3f at %s, B %.3f at %s; T flushed: A %.3g at %s, B %.3g, rel_err %.2e'
          % (pw.wino_case_id(case), r0, r1, at1, rb, atb, rf, atf, rfb, rel_err(bad, pw.h16(em))))
    assert r0 <= 0.5 and r1 <= 1.0 and rb <= 0.5
    assert rf > 1 and rfb > 1


def test_wino_restatement_equals_the_oracles():
    """wino_ref's pair A, rounded to fp16, is oracle/net_oracle.py::conv3x3_reflect_wino_f16 (float64 sums) up to the sum order."""
    x, wt, bias = pw.layer_inputs(64, 192, 1, 5, 18)
    (wa, sa), _ = pw.wino_ref(x[0], wt, bias, relu=True)
    got = oracle.conv3x3_reflect_wino_f16(x[0], wt, bias, relu=True)
    assert pw.judge(got, wa, sa, 1e-13, fp16_out=True)[0] <= 1.0


# ---- injected defects ---------------------------------------------------------------------------------------------------

def _wino_defect(name, case, defect, mask_of, pool=False, **kw):
    """Plant `defect` in the emulation of image 0 of `case`, print the whole-map figures and the judge's, and hold the judge to
    > 1 inside the mask (a boolean map over the output's rows and columns) and <= 1 outside it, against A and against B."""
    ci, co, b, h, w, up, norelu, cfg = case
    x, wt, bias = pw.layer_inputs(ci, co, b, h, w)
    (wa, sa), (wb, sb) = pw.wino_ref(x[0], wt, bias, relu=True, up=up)
    good = pw.h16(pw.wino_emulate(x[0], wt, bias, up=up))
    bad = pw.h16(pw.wino_emulate(x[0], wt, bias, up=up, defect=defect, **kw))
    if pool:
        good, bad = pw.pool_same(good), pw.pool_same(bad)
    mask = mask_of(np.zeros(good.shape[:2], bool))
    assert np.array_equal(good[~mask], bad[~mask]) and not np.array_equal(good[mask], bad[mask])
    ra = pw.ratios(bad, wa, sa, pw.tau_wino(ci), pool=pool, fp16_out=True)
    rb = pw.ratios(bad, wb, sb, pw.tau_wino_b(ci), pool=pool, fp16_out=True)
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(ra)), ra.shape))
    print('wino defect %s, %s: A worst %.3g at %s (%.0f %% of the masked elements > 1), elsewhere %.3f; B worst %.3g, elsewhere %.3f; rel_err %.2e, max_rel %.2e'
          % (name, pw.wino_case_id(case), ra.max(), at, 100 * (ra[mask] > 1).mean(), ra[~mask].max(), rb[mask].max(), rb[~mask].max(),
             rel_err(bad, good), max_rel(bad, good)))
    assert ra[mask].max() > 1 and mask[at[:2]] and ra[~mask].max() <= 1
    assert rb[mask].max() > 1 and rb[~mask].max() <= 1
    assert pw.ratios(good, wa, sa, pw.tau_wino(ci), pool=pool, fp16_out=True).max() <= 1
    return ra, mask


def _rows_cols(rows=(), cols=()):
    def mark(m):
        for r in rows:
            m[r] = True
        for c in cols:
            m[:, c] = True
        return m
    return mark


WINO_17x33, WINO_UP, WINO_DEEP = pw.WINO_CASES[1], pw.WINO_CASES[2], pw.WINO_CASES[3]


def test_wino_defect_1_odd_last_row_pooled_against_its_dropped_partner():
    """17 rows: pooled row 8 has image row 16 alone; the kernel computes that row's partner y(17) from clamped input rows and
    must keep it out of the pool.  Here it gets in."""
    assert WINO_17x33[3:5] == (17, 33)
    _wino_defect('1 (partner row pooled)', WINO_17x33, 'partner', _rows_cols(rows=[8]), pool=True)


def test_wino_defect_2_right_halo_column_clamped():
    """W = 33: the third tile column holds one pixel, whose right neighbour is the reflection, image column 31; clamped, it is
    column 32 itself.  Only the last output column may differ."""
    ra, mask = _wino_defect('2 (right halo clamped)', WINO_17x33, 'clamp_right', _rows_cols(cols=[32]))
    assert (ra[:, 32].max(axis=1) > 1).all()              # every pixel of the column is named


def test_wino_defect_3_upsample_index_halved_before_the_reflection():
    """9x9 -> 18x18: padded index -1 is upsampled pixel 1 = source pixel 0, and 18 is 16 = source 8; halved first they become
    source -1 -> 1 and 9 -> 7.  The outermost output ring differs (row 0 through T0 only, row 17 through T3 only)."""
    assert WINO_UP[5] and WINO_UP[3:5] == (9, 9)
    _wino_defect('3 (halved before reflected)', WINO_UP, 'halve_first', _rows_cols(rows=[0, 17], cols=[0, 17]))


def test_wino_defect_4_one_frequency_with_the_wrong_sign_in_one_tile():
    """M2 enters the odd output rows of ONE tile with + instead of -: the 16-row tile (0, 1) of 18x31 and the 8-row tile (1, 1)."""
    def odd_rows(r0, r1, c0, c1):
        def mark(m):
            m[r0 + 1:r1:2, c0:c1] = True
            return m
        return mark
    _wino_defect('4 (sign of M2, 16-row tile)', WINO_DEEP, 'sign', odd_rows(0, 16, 16, 31), tile=(0, 1, 16))
    _wino_defect('4 (sign of M2, 8-row tile)', WINO_DEEP, 'sign', odd_rows(8, 16, 16, 31), tile=(1, 1, 8))


def _edge_padded_right(x, w_hwio, b):
    """The layer with the RIGHT border padded by edge replication instead of reflection (float64)."""
    x = np.asarray(x, np.float64)
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode='reflect')
    xp[:, -1] = xp[:, -2]
    h, wd, _ = x.shape
    out = np.zeros((h, wd, w_hwio.shape[3]))
    for ky in range(3):
        for kx in range(3):
            out += xp[ky:ky + h, kx:kx + wd] @ np.float64(w_hwio[ky, kx])
    return out + np.float64(b)


def test_defect_a_right_border_column_edge_replicated(encoders):
    """(a) conv_first at 31x129 and conv_last at 50x38.  Every pixel of the border column is wrong, by a large part of its value on
    inputs without spatial correlation, so the whole-map Frobenius ratio reads about 1 / sqrt(W) of that: 7e-2 on both maps here
    (3e-2 on a box-blurred 31x129 image).  This is the one defect of the five that the 1e-2 gate DOES see at these widths; it is
    on record below as `> 1e-2`.  What the judge adds is the column's name."""
    enc = encoders['he']
    img = pw.first_image('u8', 31, 129)
    want, s, a = pw.first_ref(img, enc)
    bad = np.maximum(_edge_padded_right(img, *pw.fold_first(enc)), 0)
    r, at = pw.judge(bad, want, s, pw.TAU_FIRST, a)
    print('defect a, conv_first 31x129: ratio %.3g at %s, rel_err %.2e' % (r, at, rel_err(bad, want)))
    assert r > 1 and at[1] == 128
    assert np.array_equal(bad[:, :-1], want[:, :-1])
    assert rel_err(bad, want) > 1e-2
    feat = pw.last_features('dense', 50, 38)
    wt, b = pw.last_filters(7)
    want, s = pw.last_ref(feat, wt, b)
    bad = _edge_padded_right(feat, pw.h16(wt), b)
    r, at = pw.judge(bad, want, s, pw.TAU_LAST)
    print('defect a, conv_last 50x38: ratio %.3g at %s, rel_err %.2e' % (r, at, rel_err(bad, want)))
    assert r > 1 and at[1] == 37
    assert rel_err(bad, want) > 1e-2


def test_defect_b_corner_pixel_from_its_neighbour(encoders):
    """(b) On these inputs (no spatial correlation) the neighbour differs from the corner by about its whole value, so the
    pixel's 64 channels read 1 / sqrt(50 38) = 2.3e-2 of the map's norm: the 1e-2 gate happens to see that (recorded as
    `> 1e-2`), and would on a box-blurred image too (1.1e-2).  The same pixel 40 % off reads 8e-3 and passes the gate; in the
    pooled 19x15 map of the direct kernel a 40 % corner reads 1.6e-2.  The judge names the pixel in every case."""
    enc = encoders['he']
    img = pw.first_image('u8', 50, 38)
    want, s, a = pw.first_ref(img, enc)
    for what, value, seen in (('neighbour', want[49, 36], True), ('40 % off', 0.6 * want[49, 37], False)):
        bad = want.copy()
        bad[49, 37] = value
        r, at = pw.judge(bad, want, s, pw.TAU_FIRST, a)
        print('defect b, conv_first 50x38, %s: ratio %.3g at %s, rel_err %.2e' % (what, r, at, rel_err(bad, want)))
        assert r > 1 and at[:2] == (49, 37)
        assert (rel_err(bad, want) > 1e-2) == seen
    x, wt, bias = pw.direct_inputs(64, 1, 37, 29)
    want, s = pw.direct_ref(x[0], wt, bias)
    good = pw.pool_same(want)
    bad = good.copy()
    bad[18, 14] = 0.6 * good[18, 14]
    r, at = pw.judge(bad, want, s, pw.tau_direct(64), pool=True, fp16_out=True)
    print('defect b, pooled direct 37x29, 40 %% off: ratio %.3g at %s, rel_err %.2e' % (r, at, rel_err(bad, good)))
    assert r > 1 and at[:2] == (18, 14) and rel_err(bad, good) > 1e-2


@pytest.mark.parametrize('kind', pw.FIRST_INPUTS)
def test_defect_c_lo_operand_dropped(encoders, kind):
    """(c) 11-bit products: 2^-12 relative per term, some hundred times the bound -- and 1e-4 of the map's norm."""
    for which in ('he', 'x64'):
        enc = encoders[which]
        img = pw.first_image(kind, 50, 38)
        want, s, a = pw.first_ref(img, enc)
        bad = pw.first_emulate(img, enc, drop_lo=True)
        r, at = pw.judge(bad, want, s, pw.TAU_FIRST, a)
        print('defect c, %s %s: ratio %.3g at %s, rel_err %.2e' % (which, kind, r, at, rel_err(bad, want)))
        assert r > 1 and rel_err(bad, want) < 1e-2


def test_defect_d_odd_last_row_pooled_against_a_phantom_row():
    """(d) 37 rows: pooled row 18 has image row 36 alone; here it is pooled against the row the previous 16-row tile left at
    the same place (image row 21)."""
    x, wt, bias = pw.direct_inputs(64, 1, 37, 29)
    want, s = pw.direct_ref(x[0], wt, bias)
    good = pw.pool_same(want)
    bad = good.copy()
    bad[18] = pw.pool_same(np.maximum(want[36:37], want[21:22]))[0]
    r, at = pw.judge(bad, want, s, pw.tau_direct(64), pool=True, fp16_out=True)
    print('defect d: ratio %.3g at %s, rel_err %.2e' % (r, at, rel_err(bad, good)))
    assert r > 1 and at[0] == 18
    # a whole output row of 19 is wrong, by about the size of a value: the Frobenius ratio is ~ sqrt(1/19) of that, 1.1e-1.  The
    # 1e-2 gate sees this defect when a whole row has it, and still (2e-2) when 8 pooled pixels of a 32x126 map have it (below,
    # one 16-pixel tile of the last row of 63x251): recorded as `> 1e-2`; the judge names the row and the tile
    assert rel_err(bad, good) > 1e-2
    x, wt, bias = pw.direct_inputs(64, 16, 63, 251)
    want, s = pw.direct_ref(x[0], wt, bias)
    good = pw.pool_same(want)
    bad = good.copy()
    bad[31, 8:16] = pw.pool_same(np.maximum(want[62:63, 16:32], want[47:48, 16:32]))[0]
    r, at = pw.judge(bad, want, s, pw.tau_direct(64), pool=True, fp16_out=True)
    print('defect d, one tile of 63x251: ratio %.3g at %s, rel_err %.2e' % (r, at, rel_err(bad, good)))
    assert r > 1 and at[0] == 31 and 8 <= at[1] < 16
    assert rel_err(bad, good) > 1e-2


def test_defect_e_partial_halo_tile_of_conv_last_zeroed():
    """(e) the 18x18 halo patch of a 16x16 output tile is 324 pixels = ten 32-pixel GEMM tiles and four more pixels, 320..323:
    patch row 17, columns 14..17.  Zeroed, they take the ky = 2 taps away from output row 15, columns 12..15 of the tile.  The
    decoder's filters sum to zero, so a pixel that loses a third of its taps is off by about its own deviation: with one tile
    of a 33x31 map affected the Frobenius ratio reads 3e-2 on either kind of features: seen by a 1e-2 gate at this size
    (recorded as `> 1e-2`; the decoder's only ragged-size comparison was one 32x24 map).  The judge names row 15 of the tile
    and the four columns."""
    for kind in ('dense', 'sparse'):
        _defect_e(kind)


def _defect_e(kind):
    feat = pw.last_features(kind, 33, 31)
    wt, b = pw.last_filters(8)
    want, s = pw.last_ref(feat, wt, b)
    w64 = np.float64(pw.h16(wt))
    xp = np.pad(np.float64(feat), ((1, 1), (1, 1), (0, 0)), mode='reflect')
    bad = want.copy()
    y0, x0 = 16, 0                                            # the tile at rows 16..31, columns 0..15
    for lx in range(16):
        for kx in range(3):
            if lx + kx >= 14:                                 # patch pixel (17, lx + kx) = padded image pixel (y0 + 17, x0 + lx + kx)
                bad[y0 + 15, x0 + lx] -= xp[y0 + 17, x0 + lx + kx] @ w64[2, kx]
    r, at = pw.judge(bad, want, s, pw.TAU_LAST)
    print('defect e, %s: ratio %.3g at %s, rel_err %.2e' % (kind, r, at, rel_err(bad, want)))
    assert r > 1 and at[0] == 31 and 12 <= at[1] < 16
    assert rel_err(bad, want) > 1e-2
