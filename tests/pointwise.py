"""Per-element judge for one conv layer  y = act(b + sum_k w_k x_k)  (helper, not collected).

The Frobenius ratio of a whole map (conftest.rel_err) cannot see one wrong pixel: a corner of a 50x38 map that is 40 % off
reads 0.4 / sqrt(1900) = 9e-3.  Here every output element is held against its own bound

    |got - want| <= tau * s + a            s = |b| + sum_k |w_k| |x_k|

with `want` and `s` in float64: `want` is the layer of oracle/net_oracle.py (reflect pad, 3x3 conv, bias, optional ReLU,
optional x2 nearest upsample) restated with float64 sums, `s` the same conv run on |w|, |x| and |b|.  ReLU is 1-Lipschitz and
changes nothing; a ceil-mode pooled output takes the largest bound of its window (|max a_i - max b_i| <= max |a_i - b_i|);
an fp16 output adds its own rounding, 2^-11 |want|.

The constants are derived from the arithmetic, not measured on a GPU:

 * fp16-operand layers (csrc/conv.hip conv3x3_mfma_kernel, conv_last_kernel): `want` is computed from the fp16-rounded
   activations and filters, so every product is exact in fp32 and the only error is the fp32 accumulation of n terms in some
   order, at most n 2^-24 s.  n = 9 Cin + 1 for the direct kernel, 64 + 10 for conv_last (64 channels per partial, then the
   bias and nine partials).  tau = 2 n 2^-24: the factor 2 covers an MFMA whose internal adds are not individually rounded
   to nearest.  a = 0.
 * conv_first_kernel: `want` from the fp32 image and the folded (preprocess o conv1_1) filters.  Operands are fp16 hi + lo
   pairs (22 bits each, relative 2^-22 per operand), lo * lo is dropped (2^-24 relative) and 27 terms are accumulated three
   times in fp32 (81 adds and the bias, < 82 2^-24 = 2^-17.6 in the worst order, ~sqrt(82) 2^-24 = 2^-20.8 typically).
   tau = 2^-19.  a = 2^-24 sum_k |w_k|: the lo half of a pixel value below 2^-2 is an fp16 subnormal (spacing 2^-24), so it
   carries an absolute error of up to 2^-25 per pixel value whatever the value.
   tests/test_pointwise_cpu.py runs a NumPy emulation of this arithmetic and holds it to HALF the bound.
 * the reduced-FLOP kernel (csrc/conv_wino.hip conv3x3_wino_kernel, Winograd F(2,3) along y; wino_ref below) is held twice.
   A, against its own roundings: `want_A` is the layer in the kernel's form, y(2r) = M0 + M1 + M2, y(2r+1) = M1 - M2 - M3,
   M_f = sum_{kx,c} U_f[kx] T_f[x + kx], from the operands the kernel multiplies: T_f = fp16(B^T d) of the fp16 activations (one
   correctly rounded add per value, v_pk_add_f16; the file is compiled with the fp16 denormal mode that PRESERVES subnormals
   -- .amdhsa_float_denorm_mode_16_64 3 -- so nothing is flushed, as in the oracle's restatement) and U_f[kx] =
   fp16(float(sum_ky G[f][ky] g[ky][kx])), the sum in double, as BOTH packers round it (api_weights.hip::pack_conv on the host,
   train.hip::pack_conv_wino_frag_kernel on the device: the same three terms in the same order; the products by 0.5 are exact,
   so a contracted multiply-add changes nothing).  Every product is exact in fp32; what is left is the fp32 accumulation.
   With s_f = sum_{kx,c} |U_f| |T_f| (+ |b| for f = 1, where the bias rides), frequency f accumulates 3 Cin products (and the
   bias) in its own register: at most (3 Cin + 1) 2^-24 s_f in the worst order.  An output row combines three frequencies, and
   s_A = |b| + the row's three sums = s_f + s_f' + s_f'', so the three accumulations together err by at most (3 Cin + 1) 2^-24
   s_A -- the count does not multiply by three, each frequency is charged against its own share -- and the two combining adds
   by 2^-24 s_A each: n = 3 Cin + 3.  tau_wino = 2 n 2^-24, doubled like tau_direct for an MFMA whose internal adds are not
   individually rounded to nearest.  The fp16 store adds 2^-11 |want_A|.
   B, against the true layer: `want_B` is the plain float64 conv of the fp16 activations with the fp32 filters (equal to the
   Winograd form with exact U and T: the CPU test holds that identity to 1e-13), s_B the same sum with exact U and T, and
   tau_B = 2^-10 + 2^-22 + tau_wino (1 + 2^-10): one fp16 rounding each of U and T (2^-11 + 2^-11), their product term, and the
   accumulation on the rounded operands.  B is loose (1e-3 of s); it is there so that a mistake shared by the kernel and the
   restatement (a wrong G, a swapped frequency) cannot pass.  (An fp16-subnormal U, |U| < 2^-14, is rounded to 2^-25 absolute,
   not 2^-11 relative: at most 2^-25 |T| per such term, four decades under tau_B s_B on any filter set used here.)
   tests/test_pointwise_cpu.py runs a NumPy emulation of the kernel's order (chunk of 32 channels, f, kx, k-step of 16 into an
   fp32 running sum, bias starting M1) and holds it to half of A before the fp16 store, to A after it, and to half of B.
"""
import numpy as np

TAU_FIRST = 2.0 ** -19
EPS16 = 2.0 ** -11                # fp16 round-to-nearest, relative


def tau_direct(cin):
    return 2.0 * (9 * cin + 1) * 2.0 ** -24


TAU_LAST = 2.0 * (64 + 10) * 2.0 ** -24


def tau_wino(cin):
    return 2.0 * (3 * cin + 3) * 2.0 ** -24


def tau_wino_b(cin):
    return 2.0 ** -10 + 2.0 ** -22 + tau_wino(cin) * (1 + 2.0 ** -10)


def h16(a):
    """Round to fp16 (nearest even, as the device's conversions do), back in float32."""
    return np.asarray(a, np.float16).astype(np.float32)


def _conv64(x, w, b, up, torch_from=1 << 30):
    """Reflect pad, 3x3 conv, bias in float64: nine matrix products in NumPy; from `torch_from` multiply-adds on the same sum
    by torch.nn.functional.conv2d in float64 on the CPU, which is some three times quicker (the CPU test holds the two equal)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    if up:
        x = np.repeat(np.repeat(x, 2, axis=-3), 2, axis=-2)
    lead = x.shape[:-3]
    h, wd, cin = x.shape[-3:]
    cout = w.shape[3]
    xp = np.pad(x, [(0, 0)] * len(lead) + [(1, 1), (1, 1), (0, 0)], mode='reflect')
    if x.size * 9 * cout >= torch_from:
        import torch
        xt = torch.from_numpy(xp.reshape((-1, h + 2, wd + 2, cin))).permute(0, 3, 1, 2)
        y = torch.nn.functional.conv2d(xt, torch.from_numpy(w).permute(3, 2, 0, 1).contiguous(), torch.from_numpy(np.asarray(b, np.float64)))
        return y.permute(0, 2, 3, 1).contiguous().numpy().reshape(lead + (h, wd, cout))
    out = np.zeros((int(np.prod(lead, dtype=np.int64)) * h * wd, cout), np.float64)
    for ky in range(3):
        for kx in range(3):
            out += np.ascontiguousarray(xp[..., ky:ky + h, kx:kx + wd, :]).reshape(-1, cin) @ w[ky, kx]
    return out.reshape(lead + (h, wd, cout)) + np.asarray(b, np.float64)


def conv_ref(x, w_hwio, b, relu=True, up=False):
    """(want, s) in float64 for x [..., H, W, Cin], w [3][3][Cin][Cout], b [Cout]."""
    want = _conv64(x, w_hwio, b, up)
    if relu:
        want = np.maximum(want, 0)
    return want, _conv64(np.abs(x), np.abs(w_hwio), np.abs(b), up)


def pool_same(a, fill=-np.inf):
    """2x2/2 ceil-mode max-pool on [..., H, W, C]: the odd last row / column pools over the cells that exist."""
    a = np.asarray(a)
    lead = a.shape[:-3]
    h, w, c = a.shape[-3:]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    p = np.full(lead + (ho * 2, wo * 2, c), fill, a.dtype)
    p[..., :h, :w, :] = a
    return p.reshape(lead + (ho, 2, wo, 2, c)).max(axis=(-4, -2))


def judge(got, want, s, tau, a=0.0, pool=False, fp16_out=False):
    """Worst err / bound over all elements and its index (y, x, c) (with a leading batch index for a 4-d map)."""
    ratio = ratios(got, want, s, tau, a, pool, fp16_out)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


def ratios(got, want, s, tau, a=0.0, pool=False, fp16_out=False):
    """err / bound of every element (what judge takes the maximum of)."""
    bound = tau * np.asarray(s, np.float64) + a
    want = np.asarray(want, np.float64)
    if pool:
        want, bound = pool_same(want), pool_same(bound)
    if fp16_out:
        bound = bound + EPS16 * np.abs(want)
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return np.where(np.isfinite(got), ratio, np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# conv1_1 with the folded preprocess (conv_first_kernel)
# ---------------------------------------------------------------------------------------------------------------------
FIRST_SIZES = [(2, 2), (2, 17), (3, 64), (16, 65), (17, 63), (31, 129), (50, 38)]
FIRST_INPUTS = ['u8', 'dark', 'float', 'span']


def first_image(kind, h, w):
    rng = np.random.default_rng(1000 * h + w + 17 * FIRST_INPUTS.index(kind))
    if kind == 'u8':                                   # the uint8 grid over 255
        return np.float32(rng.integers(0, 256, (h, w, 3)) / 255.)
    if kind == 'dark':                                 # 0..8 over 255 with exact zeros: every lo half is an fp16 subnormal
        v = rng.integers(0, 9, (h, w, 3))
        v[rng.random((h, w, 3)) < 0.3] = 0
        return np.float32(v / 255.)
    if kind == 'float':
        return np.float32(rng.uniform(-0.1, 1.1, (h, w, 3)))
    return np.float32(10.0 ** rng.uniform(-7, 0, (h, w, 3)))      # 'span': 1e-7 .. 1


def first_encoders():
    """{'he': the encoder of synthetic_weights(42), 'x64': conv1_1 scaled x64 with flipped signs and a bias of order one}."""
    from wct_tf_amd.weights import synthetic_weights
    enc = synthetic_weights(seed=42, relu_targets=['relu1_1'])['encoder']
    rng = np.random.default_rng(64)
    w, _ = enc['conv1_1']
    big = dict(enc)
    big['conv1_1'] = (np.float32(w * 64 * rng.choice([-1.0, 1.0], w.shape[:3] + (1,))), np.float32(rng.standard_normal(64)))
    return {'he': enc, 'x64': big}


def fold_first(enc):
    """The folded filters [3][3][3][64] and bias [64] as wct_set_encoder builds them (float64 sums, stored as float32)."""
    pw = np.asarray(enc['preprocess'][0], np.float64).reshape(3, 3)          # [in][out]
    pb = np.asarray(enc['preprocess'][1], np.float64)
    w1 = np.asarray(enc['conv1_1'][0], np.float64)
    fw = np.einsum('ip,yxpo->yxio', pw, w1)
    fb = np.asarray(enc['conv1_1'][1], np.float64) + np.einsum('p,yxpo->o', pb, w1)
    return np.float32(fw), np.float32(fb)


def first_ref(img, enc):
    """(want, s, a) of relu1_1 for an fp32 image."""
    fw, fb = fold_first(enc)
    want, s = conv_ref(img, fw, fb, relu=True)
    return want, s, 2.0 ** -24 * np.abs(np.float64(fw)).sum(axis=(0, 1, 2))


def first_emulate(img, enc, drop_lo=False):
    """conv_first_kernel's arithmetic in NumPy: image values and folded filters split into fp16 hi + lo, per k-step of 16 the
    products w_lo x_hi, w_hi x_lo, w_hi x_hi (each exact in fp32) added to an fp32 running sum, k = ky 9 + kx 3 + c; bias,
    ReLU.  drop_lo: the defect of an 11-bit product (the image's lo half never multiplied)."""
    fw, fb = fold_first(enc)
    x = np.pad(np.asarray(img, np.float32), ((1, 1), (1, 1), (0, 0)), mode='reflect')
    h, w = img.shape[:2]
    xh = h16(x)
    xl = np.zeros_like(xh) if drop_lo else h16(x - xh)
    wh = h16(fw)
    wl = h16(fw - wh)
    acc = np.zeros((h, w, 64), np.float32)
    ks = [(ky, kx, c) for ky in range(3) for kx in range(3) for c in range(3)]
    for step in (ks[:16], ks[16:]):
        for a, b in ((wl, xh), (wh, xl), (wh, xh)):
            for ky, kx, c in step:
                acc += b[ky:ky + h, kx:kx + w, c, None] * a[ky, kx, c]
    return np.maximum(acc + fb, np.float32(0))


# ---------------------------------------------------------------------------------------------------------------------
# decoder output conv 64 -> 3 (conv_last_kernel), reached through an identity first layer
# ---------------------------------------------------------------------------------------------------------------------
LAST_SIZES = [(2, 2), (2, 17), (17, 2), (16, 16), (15, 33), (33, 31), (50, 38)]


def identity_conv64():
    w = np.zeros((3, 3, 64, 64), np.float32)
    w[1, 1, np.arange(64), np.arange(64)] = 1
    return w, np.zeros(64, np.float32)


def last_features(kind, h, w):
    """Non-negative fp16-exact maps: 'sparse' = 80 % zeros, 'dense' = every value > 0 with channel scales over 3 decades."""
    rng = np.random.default_rng(100 * h + w + (kind == 'dense'))
    if kind == 'sparse':
        f = np.abs(rng.standard_normal((h, w, 64))) * (rng.random((h, w, 64)) < 0.2)
    else:
        f = rng.uniform(0.25, 1.0, (h, w, 64)) * 10.0 ** rng.uniform(-1.5, 1.5, 64)
    return h16(f)


def last_filters(seed, tap=None):
    """He-normal 64 -> 3 filters with a bias; tap = (ky, kx) keeps that tap alone."""
    rng = np.random.default_rng(seed)
    w = np.float32(rng.standard_normal((3, 3, 64, 3)) * np.sqrt(2.0 / 576))
    if tap is not None:
        keep = np.zeros((3, 3, 1, 1), np.float32)
        keep[tap] = 1
        w = w * keep
    return w, np.float32(0.5 + 0.05 * rng.standard_normal(3))


def last_cases():
    """(h, w, feature kind, filter seed, tap or None): every size with both feature kinds on full filters and with one single-tap
    set, all nine taps at (15, 33)."""
    out = []
    for i, (h, w) in enumerate(LAST_SIZES):
        out += [(h, w, 'sparse', 7, None), (h, w, 'dense', 8, None)]
        taps = [divmod(t, 3) for t in (range(9) if (h, w) == (15, 33) else [(2 * i + 1) % 9])]
        out += [(h, w, 'dense' if k % 2 else 'sparse', 9, t) for k, t in enumerate(taps)]
    return out


def last_ref(feat, w, b):
    return conv_ref(feat, h16(w), b, relu=False)


# ---------------------------------------------------------------------------------------------------------------------
# the direct kernel at 64 -> 64 and 128 -> 128, with and without the fused ceil-mode pool
# ---------------------------------------------------------------------------------------------------------------------
# (channels, B, H, W, tile configuration launch_conv3x3 selects).  With t16 = ceil(W/16) ceil(H/16) B and t32 = ceil(W/16) ceil(H/32) B
# the policy reads (csrc/conv.hip): Cout % 128 == 0 and t16 Cout/128 >= 512 -> <16,128,2,2>; t32 Cout/64 >= 512 -> <32,64,4,1>;
# Cout % 128 == 0 and t16 Cout/128 >= 256 -> <16,128,2,2>; t16 Cout/64 >= 256 -> <16,64,4,1>; else <8,64,2,2>.
SMALL_SHAPES = [(1, 2, 2), (1, 3, 3), (1, 5, 18), (2, 17, 33), (1, 37, 29), (3, 33, 16)]     # t16 <= 9: all <8,64,2,2>
DIRECT_CASES = [(c,) + s + ('8,64,2,2',) for c in (64, 128) for s in SMALL_SHAPES] + [
    (64, 3, 23, 35, '8,64,2,2'),          # t16 = 3 2 3 = 18 < 256
    (64, 16, 49, 63, '16,64,4,1'),        # t32 = 4 2 16 = 128 < 512, t16 = 4 4 16 = 256 >= 256; the 4th tile row holds one image row
    (64, 16, 63, 251, '32,64,4,1'),       # t32 = 16 2 16 = 512 >= 512
    (128, 3, 23, 35, '8,64,2,2'),         # t16 = 18: 18 < 256, 2 18 < 256
    (128, 8, 49, 63, '16,64,4,1'),        # t16 = 4 4 8 = 128 (< 256, 2 128 >= 256), t32 = 4 2 8 = 64 (2 64 < 512)
    (128, 64, 33, 17, '32,64,4,1'),       # t16 = 2 3 64 = 384 < 512, t32 = 2 2 64 = 256, 2 256 >= 512; the 2nd tile row holds one image row
    (128, 4, 125, 123, '16,128,2,2'),     # t16 = 8 8 4 = 256 (< 512), t32 = 8 4 4 = 128 (2 128 < 512), t16 >= 256
]


def tile_config(cout, b, h, w):
    """launch_conv3x3's choice for a layer the direct kernel runs (restated from csrc/conv.hip, see DIRECT_CASES)."""
    tx = -(-w // 16)
    t16, t32 = tx * -(-h // 16) * b, tx * -(-h // 32) * b
    if cout % 128 == 0 and t16 * (cout // 128) >= 512:
        return '16,128,2,2'
    if t32 * (cout // 64) >= 512:
        return '32,64,4,1'
    if cout % 128 == 0 and t16 * (cout // 128) >= 256:
        return '16,128,2,2'
    if t16 * (cout // 64) >= 256:
        return '16,64,4,1'
    return '8,64,2,2'


def direct_inputs(c, b, h, w):
    """Post-ReLU activations, He-normal filters, a bias of -0.3 on every other channel: about half of the pre-activations
    are negative everywhere, the ragged edge included, so a pooled edge that saw a value from before the ReLU, or a stale
    one, differs from the reference."""
    rng = np.random.default_rng(c * 7919 + b * 131 + h * 17 + w)
    x = np.maximum(rng.standard_normal((b, h, w, c)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, c, c)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
    bias = np.float32(rng.standard_normal(c) * 0.1)
    bias[1::2] = -0.3
    return x, wt, bias


def direct_ref(x, wt, bias):
    return conv_ref(h16(x), h16(wt), bias, relu=True)


def layer_inputs(cin, cout, b, h, w):
    """direct_inputs for Cin != Cout.  The seed leaves the batch out and the images are drawn last, so a smaller batch of the
    same layer and size holds the first images of a larger one."""
    rng = np.random.default_rng(cin * 7919 + cout * 611 + h * 17 + w)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    bias = np.float32(rng.standard_normal(cout) * 0.1)
    bias[1::2] = -0.3
    x = np.maximum(rng.standard_normal((b, h, w, cin)), 0).astype(np.float32)
    return x, wt, bias


# the direct kernel where Cin != Cout (fp16 output, conv3x3_f16 algo=1):
# (Cin, Cout, B, source H, source W, upsample, pools too, tile configuration).  t16 counts the tiles of the upsampled map.
DIRECT_MIXED_CASES = [(ci, co, 1, h, w, up, False, '8,64,2,2')       # t16 <= 2 3 = 6: encoder's conv3_1 / decoder's 256->128, 128->64
                      for ci, co in ((128, 64), (256, 128)) for h, w in ((9, 17), (19, 7)) for up in (False, True)] + [
    (64, 128, 2, 17, 33, False, True, '8,64,2,2'),        # t16 = 3 2 2 = 12: conv2_1's shape with the fused pool
    (64, 128, 16, 49, 63, False, True, '16,128,2,2'),     # t16 = 4 4 16 = 256 (< 512), t32 = 4 2 16 = 128 (2 128 < 512), t16 >= 256
]
# the tap layers' epilogue (fp32 output, ctx.conv3x3, one image): (Cin, Cout, H, W, relu, tile configuration)
TAP_CASES = [(ci, co, h, w, True, '8,64,2,2') for ci, co in ((64, 128), (128, 256), (256, 512)) for h, w in ((37, 29), (17, 33))] + [
    (128, 256, 37, 29, False, '8,64,2,2')]                # t16 <= 3 2 = 6, Cout/64 <= 8: 48 < 256


# ---------------------------------------------------------------------------------------------------------------------
# the reduced-FLOP kernel (csrc/conv_wino.hip) in its three tile shapes
# ---------------------------------------------------------------------------------------------------------------------
def wino_config(cout, b, h, w):
    """launch_conv3x3_wino's choice (restated from csrc/conv_wino.hip); h, w after the upsample."""
    tx = -(-w // 16)
    if cout % 128 == 0 and tx * -(-h // 16) * b * (cout // 128) >= 256:
        return 'IL16'                  # conv3x3_wino_walk_kernel<16,128,1,4>
    if cout % 128 == 0 and tx * -(-h // 8) * b * (cout // 128) >= 256:
        return '8x128'                 # <8,128,1,4>
    return '8x64'                      # <8,64,2,2>


# (Cin, Cout, B, source H, source W, upsample, also once without ReLU, tile shape).  Counts are tx ty B Cout/128.
WINO_CASES = [
    (64, 512, 16, 23, 29, False, False, 'IL16'),       # 2 2 16 4 = 256.  device packer; ONE K-pair iteration; 7 rows in tile row 2
    (256, 256, 32, 17, 33, False, False, 'IL16'),      # 3 2 32 2 = 384.  host packer; one image row in tile row 2, one pixel in tile column 3
    (128, 512, 16, 9, 9, True, False, 'IL16'),         # 18x18: 2 2 16 4 = 256.  upsample; 2-wide and 2-tall last tiles
    (512, 512, 16, 18, 31, False, True, 'IL16'),       # 2 2 16 4 = 256.  deep K: 8 K-pair iterations; the no-ReLU epilogue
    (64, 512, 8, 25, 29, False, False, '8x128'),       # 16-row: 2 2 8 4 = 128; 8-row: 2 4 8 4 = 256.  one image row in tile row 4
    (256, 256, 16, 17, 33, False, False, '8x128'),     # 3 2 16 2 = 192; 3 3 16 2 = 288.  the first 16 images of the IL16 case of this size
    (128, 512, 8, 13, 9, True, False, '8x128'),        # 26x18: 2 2 8 4 = 128; 2 4 8 4 = 256.  upsample
    (512, 256, 16, 23, 35, False, True, '8x128'),      # 3 2 16 2 = 192; 3 3 16 2 = 288.  the decoder's 512 -> 256; no ReLU
] + [(ci, co) + s + (False, s == (2, 17, 33), '8x64') for ci, co in ((256, 256), (64, 192)) for s in SMALL_SHAPES] + [
    (64, 192, 2, 13, 9, True, False, '8x64'),          # 26x18 upsampled, Cout no multiple of 128
    (64, 192, 16, 49, 63, False, False, '8x64'),       # 4 4 16 = 256 tiles: IL16's grid if Cout were a multiple of 128
]


# The same layers on activations (and a bias) scaled by 2^-15: about half of the fp16 inputs and most of T = B^T d are fp16
# subnormals.  conv_wino.hip is compiled with the denormal mode that keeps them (module docstring); a loader that flushed T would
# lose up to 2^-14 |U| per term against a bound of tau_wino s_A ~ 1e-5 of one such term's sum.  Outputs are subnormal too: their
# store rounds to the subnormal spacing 2^-24, an absolute 2^-25 whatever the value, which is `a` for these cases alone.
SUBNORMAL_SCALE = 2.0 ** -15
A16_SUBNORMAL = 2.0 ** -25
WINO_SUBNORMAL_CASES = [
    (64, 512, 16, 23, 29, False, False, 'IL16'),
    (64, 512, 8, 25, 29, False, False, '8x128'),
    (64, 192, 1, 5, 18, False, False, '8x64'),
]


def subnormal_inputs(case):
    x, wt, bias = layer_inputs(*case[:5])
    return np.float32(x * SUBNORMAL_SCALE), wt, np.float32(bias * SUBNORMAL_SCALE)


def wino_case_id(c):
    return '%d-%d-%dx%dx%d%s-%s' % (c[:5] + ('up' if c[5] else '', c[7]))


_WINO_BT = ((0, 2, -1), (1, 2, 1), (2, 1, -1), (1, 3, -1))        # T_f = d_i + sign d_j: d0 - d2, d1 + d2, d2 - d1, d1 - d3


def _wino_rows(x, up, defect=None):
    """The four padded input rows 2r + i of every pair-row r, [..., ceil(H/2), W + 2, Cin] each, and H.  An odd last row has a
    partner row the kernel computes and drops: its d3 is the clamped reflection of row H + 1, image row H - 3."""
    x = np.asarray(x, np.float64)
    pad = [(0, 0)] * (x.ndim - 3) + [(1, 1), (1, 1), (0, 0)]
    if up and defect == 'halve_first':                     # DEFECT: (i >> 1) reflected in the source instead of reflect(i) >> 1
        xp = np.pad(x, pad, mode='reflect')
        for ax in (-3, -2):
            xp = np.moveaxis(xp, ax, 0)
            xp = np.concatenate([xp[:1], np.repeat(xp[1:-1], 2, axis=0), xp[-1:]], 0)
            xp = np.moveaxis(xp, 0, ax)
    else:
        if up:
            x = np.repeat(np.repeat(x, 2, axis=-3), 2, axis=-2)
        xp = np.pad(x, pad, mode='reflect')
    if defect == 'clamp_right':                            # DEFECT: the right halo column is image column W - 1, not W - 2
        xp[..., :, -1, :] = xp[..., :, -2, :]
    h = xp.shape[-3] - 2
    if h & 1:
        xp = np.concatenate([xp, xp[..., h - 2:h - 1, :, :]], -3)
    he = h + (h & 1)
    return [xp[..., i:i + he:2, :, :] for i in range(4)], h


def _wino_t(rows):
    return [rows[i] + sg * rows[j] for i, j, sg in _WINO_BT]


def wino_u(w_hwio):
    """(exact U in float64, U as both packers round it) [4][3][Cin][Cout]: the sum over ky in double, term by term in their
    order, rounded to fp32 and then to fp16."""
    g = np.asarray(w_hwio, np.float32).astype(np.float64)
    u = np.stack([g[0], (0.5 * g[0] + 0.5 * g[1]) + 0.5 * g[2], (0.5 * g[0] - 0.5 * g[1]) + 0.5 * g[2], g[2]])
    return u, u.astype(np.float32).astype(np.float16).astype(np.float64)


def _wino_m(t, u, w):
    """M_f = sum_{kx, c} U_f[kx] T_f[x + kx] for f = 0..3 in float64, [..., pair-rows, W, Cout] each."""
    out = []
    for f in range(4):
        lead = t[f].shape[:-2]
        m = 0
        for kx in range(3):
            m = m + np.ascontiguousarray(t[f][..., kx:kx + w, :]).reshape(-1, t[f].shape[-1]) @ u[f, kx]
        out.append(m.reshape(lead + (w, u.shape[-1])))
    return out


def _wino_combine(m, h, signed=True):
    """y(2r) = M0 + M1 + M2, y(2r+1) = M1 - M2 - M3 (signed=False: the sums of the absolute terms), the first h rows."""
    e = m[0] + m[1] + m[2]
    o = m[1] - m[2] - m[3] if signed else m[1] + m[2] + m[3]
    y = np.stack([e, o], -3)                               # [..., pr, 2, W, C]
    return y.reshape(e.shape[:-3] + (2 * e.shape[-3],) + e.shape[-2:])[..., :h, :, :]


def wino_ref(x, w_hwio, b, relu=True, up=False):
    """((want_A, s_A), (want_B, s_B)) in float64 for x [..., H, W, Cin] (source size if up): A the layer from the operands the
    kernel multiplies (fp16 T, fp16 U), B the true layer of the fp16 activations and the fp32 filters with the sum of the
    exact |U| |T| (module docstring).  ReLU acts on `want` alone."""
    x16 = np.float64(h16(x))
    b64 = np.asarray(b, np.float64)
    rows, h = _wino_rows(x16, up)
    w = rows[0].shape[-2] - 2
    te = _wino_t(rows)
    tr = [t.astype(np.float16).astype(np.float64) for t in te]
    ue, ur = wino_u(w_hwio)
    want_a = _wino_combine(_wino_m(tr, ur, w), h) + b64
    s_a = _wino_combine(_wino_m([np.abs(t) for t in tr], np.abs(ur), w), h, signed=False) + np.abs(b64)
    want_b = _conv64(x16, np.asarray(w_hwio, np.float32), b64, up)
    s_b = _wino_combine(_wino_m([np.abs(t) for t in te], np.abs(ue), w), h, signed=False) + np.abs(b64)
    if relu:
        want_a, want_b = np.maximum(want_a, 0), np.maximum(want_b, 0)
    return (want_a, s_a), (want_b, s_b)


def wino_exact(x, w_hwio, b, up=False):
    """The Winograd form with exact U and T in float64, no ReLU: equal to the plain conv (the CPU test holds the identity)."""
    rows, h = _wino_rows(np.float64(h16(x)), up)
    return _wino_combine(_wino_m(_wino_t(rows), wino_u(w_hwio)[0], rows[0].shape[-2] - 2), h) + np.asarray(b, np.float64)


def wino_emulate(x, w_hwio, b, relu=True, up=False, defect=None, tile=(0, 0, 16)):
    """conv3x3_wino_kernel's arithmetic in NumPy for ONE image, the fp32 map before the fp16 store: fp16 T and U, per frequency an
    fp32 running sum that starts at the bias for f = 1 and takes whole k-steps of 16 channels (each an exact sum, as of an MFMA)
    in the kernel's order: chunk of 32 channels, f, kx, k-step; then (M0 + M1) + M2 and (M1 - M2) - M3 in fp32, ReLU.
    defect: 'halve_first' / 'clamp_right' (see _wino_rows); 'flush': subnormal T flushed to zero; 'partner': the dropped partner row of an odd last row is returned
    too (H + 1 rows: what a pool without the row mask would see); 'sign': M2 enters the odd rows of the tile (ty, tx, rows per
    tile) with + instead of -."""
    rows, h = _wino_rows(np.float64(h16(x)), up, defect)
    t = [v.astype(np.float16).astype(np.float64) for v in _wino_t(rows)]
    if defect == 'flush':                                  # DEFECT: fp16 subnormals of T flushed to zero
        t = [np.where(np.abs(v) < 2.0 ** -14, 0.0, v) for v in t]
    u = wino_u(w_hwio)[1]
    pr, w, cin, cout = t[0].shape[0], t[0].shape[1] - 2, u.shape[2], u.shape[3]
    acc = [np.zeros((pr * w, cout), np.float32) for _ in range(4)]
    acc[1] += np.asarray(b, np.float32)
    for c0 in range(0, cin, 32):
        for f in range(4):
            for kx in range(3):
                for c in (c0, c0 + 16):
                    acc[f] += (np.ascontiguousarray(t[f][:, kx:kx + w, c:c + 16]).reshape(-1, 16) @ u[f, kx, c:c + 16]).astype(np.float32)
    m = [a.reshape(pr, w, cout) for a in acc]
    e = (m[0] + m[1]) + m[2]
    o = (m[1] - m[2]) - m[3]
    if defect == 'sign':
        ty, tx, th = tile
        rs, cs = slice(ty * th // 2, (ty + 1) * th // 2), slice(tx * 16, (tx + 1) * 16)
        o[rs, cs] = (m[1][rs, cs] + m[2][rs, cs]) - m[3][rs, cs]
    y = np.stack([e, o], 1).reshape(2 * pr, w, cout)
    if defect != 'partner':
        y = y[:h]
    return np.maximum(y, np.float32(0)) if relu else y
