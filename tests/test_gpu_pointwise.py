"""The image-end and pooled conv kernels held pixel by pixel at ragged sizes (tests/pointwise.py has the criterion and the
derivation of its constants; tests/test_pointwise_cpu.py shows what it sees and that the reference sits inside half of it).

  conv_first_kernel    through ctx.encode(img, 'relu1_1'): fp32 output, no other kernel in the way
  conv_last_kernel     through ctx.decode(feat, 'relu1_1') with an identity first layer that hands the features over bit for bit
  conv3x3_mfma_kernel  through ctx.conv3x3_f16(..., algo=1) at 64 -> 64 and 128 -> 128 (conv1_2, conv2_2: the two layers that pool
                       through it), with and without the fused ceil-mode pool, once per tile configuration of launch_conv3x3;
                       at Cin != Cout with and without the folded upsample; and through ctx.conv3x3, the fp32 output of the tap layers
  conv3x3_wino_kernel  through ctx.conv3x3_f16(..., algo=2) in its three tile shapes, <16,128,1,4,IL>, <8,128,1,4> and <8,64,2,2>,
                       at ragged sizes: odd heights, last tiles one or two pixels wide, the upsample, the pool, no ReLU, both packers

Every case prints a line `pointwise <kernel> <case>: worst <err/bound> at <index>`; profiles/pointwise_margins.txt keeps those of
one run.  The asserted bound is 1: the derived one."""
import numpy as np
import pytest

import pointwise as pw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from wct_tf_amd.context import Context
    c = Context(0)
    c.first_encoder = None
    yield c
    c.close()


@pytest.fixture(scope='module')
def encoders():
    return pw.first_encoders()


@pytest.mark.parametrize('hw', pw.FIRST_SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('which', ['he', 'x64'])
def test_conv_first(ctx, encoders, which, hw):
    """Strips of four 16x16 tiles: (16, 65) has a second strip one column wide, (3, 64) exactly one strip, (17, 63) / (31, 129)
    a ragged last tile and a second tile row of 1 / 15 rows, (2, 2) and (2, 17) tiles whose halo reflects inside the patch."""
    if ctx.first_encoder != which:
        ctx.set_encoder(encoders[which])
        ctx.first_encoder = which
    for kind in pw.FIRST_INPUTS:
        img = pw.first_image(kind, *hw)
        want, s, a = pw.first_ref(img, encoders[which])
        got = ctx.encode(img, 'relu1_1')
        r, at = pw.judge(got, want, s, pw.TAU_FIRST, a)
        print('pointwise conv_first %s %dx%d %s: worst %.3f at %s' % ((which,) + hw + (kind, r, at)))
        assert r <= 1, (which, hw, kind, r, at)


@pytest.mark.parametrize('case', pw.last_cases(), ids=lambda c: '%dx%d-%s-%s' % (c[0], c[1], c[2], 'full' if c[4] is None else 'tap%d%d' % c[4]))
def test_conv_last(ctx, case):
    """One 16x16 output tile = a GEMM over the 324 pixels of its 18x18 halo patch (ten 32-pixel tiles and four pixels more), then
    nine shifted partials per output pixel; a single-tap filter set leaves one partial, so a shifted one cannot hide in a sum."""
    h, w, kind, seed, tap = case
    feat = pw.last_features(kind, h, w)
    wt, b = pw.last_filters(seed, tap)
    ident = pw.identity_conv64()
    # the hand-over: the identity layer as the decoder runs it (fp16 in, fp16 out) returns the features bit for bit
    assert np.array_equal(ctx.conv3x3_f16(feat, ident[0], ident[1], relu=True, algo=0), feat)
    ctx.set_decoder('relu1_1', [ident, (wt, b)])
    got = ctx.decode(feat, 'relu1_1')
    want, s = pw.last_ref(feat, wt, b)
    r, at = pw.judge(got, want, s, pw.TAU_LAST)
    print('pointwise conv_last %dx%d %s tap %s: worst %.3f at %s' % (h, w, kind, tap, r, at))
    assert r <= 1, (case, r, at)


def test_conv_last_hand_over_through_the_decoder(ctx):
    """The same hand-over seen from the decoder's end: a last layer whose centre tap copies channel co to output co returns
    three of the feature channels exactly, for every choice of the three."""
    feat = pw.last_features('dense', 15, 33)
    for first in (0, 31, 61):
        wt = np.zeros((3, 3, 64, 3), np.float32)
        wt[1, 1, first + np.arange(3), np.arange(3)] = 1
        ctx.set_decoder('relu1_1', [pw.identity_conv64(), (wt, np.zeros(3, np.float32))])
        assert np.array_equal(ctx.decode(feat, 'relu1_1'), feat[:, :, first:first + 3])


@pytest.mark.parametrize('case', pw.DIRECT_CASES, ids=lambda c: '%d-%dx%dx%d' % c[:4])
def test_direct_conv_with_and_without_the_fused_pool(ctx, case):
    """pointwise.DIRECT_CASES lists, per shape, the tile configuration launch_conv3x3 selects and why (the tile counts against
    its thresholds; test_pointwise_cpu.py checks the table against a restatement of the policy).  Odd heights put one image
    row into the last pooled pair-row (which relies on post-ReLU values >= 0), odd widths one column into the last pooled
    pair; a bias of -0.3 on every other channel makes about half of the pre-activations negative there.  A batch element
    must equal its single-image call bit for bit, although the batch may select another tile configuration."""
    c, b, h, w, cfg = case
    x, wt, bias = pw.direct_inputs(c, b, h, w)
    want, s = pw.direct_ref(x, wt, bias)
    for pool in (True, False):
        got = ctx.conv3x3_f16(x, wt, bias, relu=True, pool=pool, algo=1)
        r, at = pw.judge(got, want, s, pw.tau_direct(c), pool=pool, fp16_out=True)
        print('pointwise direct %d->%d <%s> %dx%dx%d pool=%d: worst %.3f at %s' % (c, c, cfg, b, h, w, pool, r, at))
        assert r <= 1, (case, pool, r, at)
        for i in sorted({0, b - 1}):
            assert np.array_equal(got[i], ctx.conv3x3_f16(x[i], wt, bias, relu=True, pool=pool, algo=1)), (case, pool, i)


@pytest.mark.parametrize('case', pw.DIRECT_MIXED_CASES, ids=lambda c: '%d-%d-%dx%dx%d%s' % (c[:5] + ('up' if c[5] else '',)))
def test_direct_conv_where_cin_differs_from_cout(ctx, case):
    """The direct kernel as the pipeline runs it between the levels: 128 -> 64 and 256 -> 128 (the decoder's narrowing layers,
    with and without the x2 upsample folded into the loader: the reflected index is halved, 18x34 and 38x14 maps with 2-wide /
    6-tall last tiles) and 64 -> 128 (conv2_1's shape) with and without the fused pool, on the 64- and the 128-channel tile."""
    ci, co, b, h, w, up, pools, cfg = case
    x, wt, bias = pw.layer_inputs(ci, co, b, h, w)
    want, s = pw.conv_ref(pw.h16(x), pw.h16(wt), bias, relu=True, up=up)
    for pool in ((True, False) if pools else (False,)):
        got = ctx.conv3x3_f16(x, wt, bias, relu=True, upsample=up, pool=pool, algo=1)
        r, at = pw.judge(got, want, s, pw.tau_direct(ci), pool=pool, fp16_out=True)
        print('pointwise direct %d->%d <%s> %dx%dx%d up=%d pool=%d: worst %.3f at %s' % (ci, co, cfg, b, h, w, up, pool, r, at))
        assert r <= 1, (case, pool, r, at)
        for i in sorted({0, b - 1} if b > 1 else ()):
            assert np.array_equal(got[i], ctx.conv3x3_f16(x[i], wt, bias, relu=True, upsample=up, pool=pool, algo=1)), (case, pool, i)


@pytest.mark.parametrize('case', pw.TAP_CASES, ids=lambda c: '%d-%d-%dx%d-relu%d' % c[:5])
def test_direct_conv_fp32_output(ctx, case):
    """The epilogue of the tap layers (conv2_1, conv3_1, conv4_1: fp32 out, here through ctx.conv3x3).  256 -> 512 is a layer
    the policy would hand to the reduced-FLOP kernel; with an fp32 output it stays on the direct one."""
    ci, co, h, w, relu, cfg = case
    x, wt, bias = pw.layer_inputs(ci, co, 1, h, w)
    want, s = pw.conv_ref(pw.h16(x[0]), pw.h16(wt), bias, relu=relu)
    got = ctx.conv3x3(x[0], wt, bias, relu=relu)
    r, at = pw.judge(got, want, s, pw.tau_direct(ci))
    print('pointwise direct fp32-out %d->%d <%s> %dx%d relu=%d: worst %.3f at %s' % (ci, co, cfg, h, w, relu, r, at))
    assert r <= 1, (case, r, at)


@pytest.mark.parametrize('case', pw.WINO_CASES, ids=pw.wino_case_id)
def test_wino_conv(ctx, case):
    """conv3x3_wino_kernel in the tile shape the case is listed under (pointwise.WINO_CASES; test_pointwise_cpu.py holds the
    table against a restatement of launch_conv3x3_wino's policy and checks what each shape is seen with).  Every element is
    held against A, the layer from the operands the kernel multiplies (fp16 T = B^T d, fp16 U as the packers round it: the
    device packer for Cin < 256, the host's from 256) with the accumulation-order bound tau_wino, and against B, the true layer,
    with the bound of one fp16 rounding of U and T.  Images 0 and B - 1 must equal their single-image calls bit for bit: those
    select <8,64,2,2>, so the equality crosses the tile shapes."""
    ci, co, b, h, w, up, norelu, cfg = case
    x, wt, bias = pw.layer_inputs(ci, co, b, h, w)
    (pa, sa), (pb, sb) = pw.wino_ref(x, wt, bias, relu=False, up=up)
    for relu, pool in [(True, True), (True, False)] + ([(False, False)] if norelu else []):
        wa, wb = (np.maximum(pa, 0), np.maximum(pb, 0)) if relu else (pa, pb)
        got = ctx.conv3x3_f16(x, wt, bias, relu=relu, upsample=up, pool=pool, algo=2)
        ra, ata = pw.judge(got, wa, sa, pw.tau_wino(ci), pool=pool, fp16_out=True)
        rb, atb = pw.judge(got, wb, sb, pw.tau_wino_b(ci), pool=pool, fp16_out=True)
        print('pointwise wino %d->%d %s %dx%dx%d up=%d relu=%d pool=%d: worst A %.3f at %s, worst B %.3f at %s'
              % (ci, co, cfg, b, h, w, up, relu, pool, ra, ata, rb, atb))
        assert ra <= 1 and rb <= 1, (case, relu, pool, ra, ata, rb, atb)
        for i in sorted({0, b - 1} if b > 1 else ()):
            assert np.array_equal(got[i], ctx.conv3x3_f16(x[i], wt, bias, relu=relu, upsample=up, pool=pool, algo=2)), (case, relu, pool, i)


@pytest.mark.parametrize('case', pw.WINO_SUBNORMAL_CASES, ids=pw.wino_case_id)
def test_wino_conv_keeps_fp16_subnormals(ctx, case):
    """Activations of 2^-15 times the usual: half of the fp16 inputs, most of T = B^T d and the outputs are fp16 subnormals.  The
    input conversion, the packed adds of the loader, the MFMA and the store must all keep them (pointwise.WINO_SUBNORMAL_CASES);
    the bound gains the absolute 2^-25 of a subnormal store and nothing else."""
    ci, co, b, h, w, up, norelu, cfg = case
    x, wt, bias = pw.subnormal_inputs(case)
    (wa, sa), (wb, sb) = pw.wino_ref(x, wt, bias, relu=True)
    for pool in (True, False):
        got = ctx.conv3x3_f16(x, wt, bias, relu=True, pool=pool, algo=2)
        ra, ata = pw.judge(got, wa, sa, pw.tau_wino(ci), a=pw.A16_SUBNORMAL, pool=pool, fp16_out=True)
        rb, atb = pw.judge(got, wb, sb, pw.tau_wino_b(ci), a=pw.A16_SUBNORMAL, pool=pool, fp16_out=True)
        print('pointwise wino-subnormal %d->%d %s %dx%dx%d pool=%d: worst A %.3f at %s, worst B %.3f at %s' % (ci, co, cfg, b, h, w, pool, ra, ata, rb, atb))
        assert ra <= 1 and rb <= 1, (case, pool, ra, ata, rb, atb)


def test_wino_tile_shapes_agree_on_shared_images(ctx):
    """256 -> 256 at 17x33: batch 32 runs <16,128,1,4,IL>, its first 16 images as a batch <8,128,1,4>, its first 2 <8,64,2,2>.
    One image row in the last tile row of each, one pixel in the last tile column; the common images agree bit for bit."""
    x, wt, bias = pw.layer_inputs(256, 256, 32, 17, 33)
    assert [pw.wino_config(256, n, 17, 33) for n in (32, 16, 2)] == ['IL16', '8x128', '8x64']
    for pool in (True, False):
        g32, g16, g2 = (ctx.conv3x3_f16(x[:n], wt, bias, relu=True, pool=pool, algo=2) for n in (32, 16, 2))
        assert np.array_equal(g32[:16], g16) and np.array_equal(g16[:2], g2), pool
