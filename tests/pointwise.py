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
"""
import numpy as np

TAU_FIRST = 2.0 ** -19
EPS16 = 2.0 ** -11                # fp16 round-to-nearest, relative


def tau_direct(cin):
    return 2.0 * (9 * cin + 1) * 2.0 ** -24


TAU_LAST = 2.0 * (64 + 10) * 2.0 ** -24


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
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


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
