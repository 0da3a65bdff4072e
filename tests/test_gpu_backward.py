"""The train step's gradients held element by element (tests/backward.py has the criterion and derives its constants;
tests/test_backward_cpu.py shows what it sees and that an emulation of the device's arithmetic sits inside half of it), Adam against
a float64 Adam on chosen gradients, and the device's re-pack of the trained weights against the host packer.

The forward state of a step is not re-derived: every activation the step saves is rebuilt through the op-level entry points
(ctx.encode, ctx.conv3x3_f16(algo=1), ctx.maxpool, ctx.conv3x3, and conv_last through an identity first layer), and the rebuild is
proved first: the three losses computed from it equal the returned ones to one fp32 ulp.  The backward pass is linear in that state,
so the float64 reference shares every ReLU mask, pool winner and TV sign with the device and no element is exempt.

Every case and layer prints `backward <relu> BxHxW <seeds> conv<i> dW|db: worst <err/bound> at <index>, rel L2 <...>`;
profiles/backward_margins.txt keeps the lines of one run.  The asserted ratio is 1; the rel-L2 figure is recorded only.

  relu1_1  1x3x5 (row 1 is both y == 1 and y == H - 2), 2x12x10, 3x17x33 (odd, B (H+2) (W+2) ragged against the 128-row tile):
           conv_first_dgrad, the fold, 64 -> 3 padded to 4, 64 -> 64
           1x64x64 (two slabs of exactly 2048), 1x70x90 (three slabs of 2112, the last 2076 with a 28-wide k tail), 3x34x46 (two
           slabs, the boundary inside an image row of image 1): split-K
  relu2_1  1x4x12 (2x6 features: the smallest), 2x16x12, 1x64x64 (split-K at full resolution, one slab at half): pool and upsample
           adjoints, the encoder's dgrad, N = 128 on the 128-wide tile, 128 -> 64
  relu3_1  1x8x12, 2x16x24: 256 -> 128, 128 -> 128, two upsamples, two pools, K = 2304
  relu2_1  1x8x8 on backward.tie_weights(): a constant decoded image and a non-negative encoder, every pool window a four-way tie:
           which maximum the pool adjoint picks, under a bound the second encoder pass does not inflate
"""
import numpy as np
import pytest

import backward as bw

pytestmark = pytest.mark.gpu

LOSS_KEYS = ('feature_loss', 'pixel_loss', 'tv_loss')


@pytest.fixture(scope='module')
def gpu():
    """(context, helper context for conv_last, {relu: weights}); the context holds the weights of the relu it ran last."""
    from wct_tf_amd.context import Context
    ctx, helper = Context(0), Context(0)
    ctx.relu = None
    yield ctx, helper, {}
    ctx.close()
    helper.close()


def load(gpu, case):
    ctx, helper, cache = gpu
    key = (case[0], tuple(case) == bw.TIES)
    if key not in cache:
        cache[key] = bw.case_weights(case)
    ctx.set_weights(cache[key])                    # also resets the decoder's optimiser state
    return ctx, helper, cache[key]


def step(ctx, relu, x, lw, lr=0.0):
    return ctx.train_step(relu, x, step=1, learning_rate=lr, feature_weight=lw[0], pixel_weight=lw[1], tv_weight=lw[2])


@pytest.mark.parametrize('case', bw.CASES, ids=bw.case_id)
def test_every_decoder_gradient_element_by_element(gpu, case):
    """Per case: the loss identity, then every dW and db of the step against the float64 backward pass of the rebuilt state, once
    with all three seeds live (feature 1, pixel 0.7, tv 1e-4) and once with the feature seed off, where the bound is sharp enough
    for the decoder's own adjoints (backward.SEEDS); lr = 0 leaves the weights bit-identical."""
    relu, b, h, w = case
    ctx, helper, weights = load(gpu, case)
    x = bw.case_images(b, h, w)
    st = bw.build_state(bw.GpuOps(ctx, helper), weights, relu, x)
    for seeds in sorted(bw.SEEDS):
        lw = bw.SEEDS[seeds]
        got = step(ctx, relu, x, lw)
        for key, ref in zip(LOSS_KEYS, bw.losses_from_state(st, lw)):
            print('backward %s %dx%dx%d %s %s: %.9g, from the rebuilt state %.9g' % (relu, b, h, w, seeds, key, got[key], ref))
            assert abs(np.float64(got[key]) - np.float64(ref)) <= 2.0 ** -23 * abs(np.float64(ref)), (case, seeds, key, got[key], ref)
        grads = ctx.get_decoder(relu, grads=True)
        for i, ((gw, gb), (rw, rb)) in enumerate(zip(grads, bw.backward(st, weights, lw))):
            for name, g, r in (('dW', gw, rw), ('db', gb, rb)):
                ratio, at, l2 = bw.judge_layer(g, r)
                print('backward %s %dx%dx%d %s conv%d %s: worst %.4f at %s, rel L2 %.1e' % (relu, b, h, w, seeds, i, name, ratio, at, l2))
                assert ratio <= 1, (case, seeds, i, name, ratio, at)
    for (w0, b0), (w1, b1) in zip(weights['decoder'][relu], ctx.get_decoder(relu)):
        assert np.array_equal(np.float32(w0), w1) and np.array_equal(np.float32(b0), b1)


def test_loss_weights_times_a_power_of_two_scale_everything_exactly(gpu):
    """All three loss weights times 2^k: every loss and every gradient is multiplied by exactly 2^k, bit for bit -- the power-of-two
    scaling (absmax_bits_kernel, scale_from_bits_kernel, the 1 / (sa sb) epilogue) and the scratch hand-over between
    launch_pow2_scale and the two GEMMs change nothing but the exponent."""
    relu = 'relu2_1'
    ctx, _, _ = load(gpu, (relu,))
    x = bw.case_images(2, 16, 12)
    base = step(ctx, relu, x, bw.LOSS_WEIGHTS)
    grads = ctx.get_decoder(relu, grads=True)
    for k in (-3, 5):
        f = np.float32(2.0 ** k)
        lw = tuple(np.float32(v) * f for v in bw.LOSS_WEIGHTS)
        got = step(ctx, relu, x, lw)
        for key in LOSS_KEYS:
            assert np.float32(got[key]) == np.float32(base[key]) * f, (k, key)
        for i, ((gw, gb), (w0, b0)) in enumerate(zip(ctx.get_decoder(relu, grads=True), grads)):
            assert np.array_equal(gw, w0 * f) and np.array_equal(gb, b0 * f), (k, i)


def inject(ctx, relu, layers, vec):
    """Overwrite the gradient buffer ([w0][b0][w1][b1]..., every piece 64-float aligned: the layout above ensure_train_state) with
    `vec`; returns the per-layer pieces, read back through get_decoder(grads=True) and checked against the layout."""
    ptr, count = ctx.train_grad_buffer(relu)
    assert count == len(vec)
    ctx.h2d(ptr, vec)
    back = np.empty(count, np.float32)
    ctx.d2h(back, ptr)
    assert np.array_equal(back, vec)
    got = ctx.get_decoder(relu, grads=True)
    off = 0
    for (w, b), (gw, gb) in zip(layers, got):
        for ref, g in ((w, gw), (b, gb)):
            assert np.array_equal(vec[off:off + ref.size], g.ravel())
            off += (ref.size + 63) // 64 * 64
    assert off == count
    return got


ADAM_RUNS = [('relu2_1', 16, 12, 3, {}), ('relu2_1', 16, 12, 3, dict(beta1=0.5, beta2=0.9, epsilon=1e-3)), ('relu4_1', 32, 32, 1, {})]


@pytest.mark.parametrize('run', ADAM_RUNS, ids=['relu2_1-defaults', 'relu2_1-b0.5-0.9-eps1e-3', 'relu4_1-defaults'])
def test_adam_on_chosen_gradients_and_the_repack_of_the_trained_weights(gpu, run):
    """train_step(lr = 0) creates the optimiser state; then seeded gradients (1e-12 .. 1e3 in both signs, exact zeros, values whose
    square underflows) are written into the gradient buffer and train_apply runs steps 1, 2, 3.  After each step every weight and
    bias is within u |w| + c u S of a float64 Adam that starts from the float32 weights and carries m, v in float64 (backward.adam_c
    derives c); an element whose gradients were all zero does not move.  Then the trained fp32 weights go into a fresh context
    through set_weights (the host packer): decode and stylize of the two contexts agree bit for bit, which holds
    pack_conv_frag_kernel, pack_last_frag_kernel and the bias copies at relu2_1 and pack_conv_wino_frag_kernel at relu4_1 (whose
    >= 256-channel layers the pipeline hands to the reduced-FLOP kernel at any map size) against api_weights.hip::pack_conv."""
    from wct_tf_amd.context import Context
    from wct_tf_amd.weights import synthetic_image
    relu, h, w, steps, kw = run
    weights = bw.case_weights((relu,))
    ctx = Context(0)
    ctx.set_weights(weights)
    step(ctx, relu, bw.case_images(1, h, w), bw.LOSS_WEIGHTS)
    count = ctx.train_grad_buffer(relu)[1]
    layers = ctx.get_decoder(relu)
    mom = [[np.zeros(a.shape) for a in (lw_, lw_, lw_, lb, lb, lb)] for lw_, lb in layers]       # m, v, M of w; m, v, M of b
    never = np.arange(count) % 7 == 3                                    # zero in every step: zero moments
    ref_kw = dict(b1=kw.get('beta1', 0.9), b2=kw.get('beta2', 0.999), eps=kw.get('epsilon', 1e-8))
    for t in range(1, steps + 1):
        vec = bw.adam_gradients(1000 * t + h, count)
        vec[never] = 0
        grads = inject(ctx, relu, layers, vec)
        ctx.train_apply(relu, t, 1e-3, **kw)
        after = ctx.get_decoder(relu)
        worst, beyond, stills = 0.0, 0.0, 0
        for i, ((w0, b0), (gw, gb), (w1, b1)) in enumerate(zip(layers, grads, after)):
            for j, (p0, g, p1) in enumerate(((w0, gw, w1), (b0, gb, b1))):
                m, v, mabs = mom[i][3 * j:3 * j + 3]
                want, m, v, mabs, store, stepb = bw.adam_ref(p0, g, m, v, mabs, t, 1e-3, **ref_kw)
                mom[i][3 * j:3 * j + 3] = m, v, mabs
                err = np.abs(np.float64(p1) - want)
                ratio = err / (store + stepb)
                worst = max(worst, float(ratio.max()))
                beyond = max(beyond, float((np.maximum(err - store, 0) / np.maximum(stepb, 1e-300)).max()))
                assert ratio.max() <= 1, (run, t, i, j, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
                still = mabs == 0
                stills += int(still.sum())
                assert np.array_equal(p1[still], p0[still]), (run, t, i, j)
        assert stills > 0
        print('adam %s %s step %d: worst %.3f of the bound; beyond the rounding of the stored weight %.3f of the bound of the step, c = %.0f'
              % (relu, kw or 'defaults', t, worst, beyond, bw.adam_c(np.float32(ref_kw['b1']), np.float32(ref_kw['b2']), t)))
        layers = after
    # ---- the re-pack: the device's fragments of the trained weights against the host packer's
    assert any(not np.array_equal(w0, np.float32(w1)) for (w0, _), (w1, _) in zip(layers, weights['decoder'][relu]))
    fresh = Context(0)
    fresh.set_weights({'encoder': weights['encoder'], 'decoder': {relu: layers}})
    if relu == 'relu4_1':                                                # the policy hands this decoder's wide layers to the reduced-FLOP kernel
        from oracle.net_oracle import wino_layer
        w0, b0 = layers[0]
        assert wino_layer(*w0.shape[2:])
        x = np.maximum(np.random.default_rng(4).standard_normal((h // 8, w // 8, w0.shape[2])), 0).astype(np.float32)
        y0 = ctx.conv3x3_f16(x, w0, b0, algo=0)
        assert np.array_equal(y0, ctx.conv3x3_f16(x, w0, b0, algo=2)) and not np.array_equal(y0, ctx.conv3x3_f16(x, w0, b0, algo=1))
    content, style = synthetic_image(3, 2 * h, 2 * w), synthetic_image(4, 2 * h, 2 * w)
    feat = ctx.encode(np.float32(content) / 255., relu)
    assert np.array_equal(ctx.decode(feat, relu), fresh.decode(feat, relu))
    adain = relu == 'relu4_1'                                            # 8x8 features at 512 channels: no covariance to whiten
    assert np.array_equal(ctx.stylize(content, style, [relu], alpha=0.8, adain=adain), fresh.stylize(content, style, [relu], alpha=0.8, adain=adain))
    ctx.close()
    fresh.close()
