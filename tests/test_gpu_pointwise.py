"""The image-end and pooled conv kernels held pixel by pixel at ragged sizes (tests/pointwise.py has the criterion and the
derivation of its constants; tests/test_pointwise_cpu.py shows what it sees and that the reference sits inside half of it).

  conv_first_kernel    through ctx.encode(img, 'relu1_1'): fp32 output, no other kernel in the way
  conv_last_kernel     through ctx.decode(feat, 'relu1_1') with an identity first layer that hands the features over bit for bit
  conv3x3_mfma_kernel  through ctx.conv3x3_f16(..., algo=1) at 64 -> 64 and 128 -> 128 (conv1_2, conv2_2: the two layers that pool
                       through it), with and without the fused ceil-mode pool, once per tile configuration of launch_conv3x3

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
