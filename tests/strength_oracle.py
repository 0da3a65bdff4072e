"""CPU oracle of strength maps (TEST INFRASTRUCTURE ONLY): a per-pixel style strength, the K = 1 case of soft spatial control.
A strength map is a uint8 image of the content's size -- 255 the call's alpha, 0 "keep the content features" -- and at level l
(stride s = 2^(l-1)) feature pixel (i, j) reads v = smap[min(i s, H - 1)][min(j s, W - 1)], the rule of the label maps
(tests/mask_oracle.py).  Per feature row, with y the level's transform at alpha = 1 (statistics over the whole map):

    a   = alpha * (float(v) / 255.f)              float32, each operation rounded once
    out = a * y + (1.f - a) * x                   float32: two products, one difference, one sum, never fused

which is ops.py:83, :133 and :293 of the reference with alpha replaced by a.  `blend` is that rule in NumPy float32, bit for bit
what csrc/strength_rule.h computes; `transform` and `stylize` restate a level and the whole predict() on oracle.wct_oracle and
oracle.net_oracle, in float64 where the reference functions take it.
"""
import numpy as np

import oracle
from oracle import net_oracle

F = np.float32


def level_bytes(smap, h, w, stride):
    """the map bytes [h][w] of a level's feature map: smap[min(i * stride, H - 1)][min(j * stride, W - 1)]"""
    smap = np.asarray(smap)
    ii = np.minimum(np.arange(h) * stride, smap.shape[0] - 1)
    jj = np.minimum(np.arange(w) * stride, smap.shape[1] - 1)
    return smap[np.ix_(ii, jj)]


def strength(alpha, v):
    """a = alpha * (float(v) / 255.f) in float32, elementwise over the bytes v"""
    return F(alpha) * (np.asarray(v).astype(F) / F(255))


def level_strength(smap, h, w, stride, alpha):
    """the strengths a [h][w] float32 of a level's feature pixels"""
    return strength(alpha, level_bytes(smap, h, w, stride))


def blend(y, x, a):
    """out = a * y + (1 - a) * x in float32, every operation rounded once; a broadcasts over the channels ([...] against [...][C])"""
    y, x, a = np.asarray(y, F), np.asarray(x, F), np.asarray(a, F)
    if a.ndim == y.ndim - 1:
        a = a[..., None]
    ay = a * y
    keep = F(1) - a
    kx = keep * x
    return ay + kx


def _adain64(fc, fs):
    """ops.py:282-294 at alpha = 1 in float64 (oracle.adain computes in float32 whatever it is given)"""
    x, s = np.float64(fc), np.float64(fs)
    mu_c, var_c = x.mean((0, 1)), x.var((0, 1))
    mu_s, var_s = s.mean((0, 1)), s.var((0, 1))
    return (x - mu_c) / np.sqrt(var_c + 1e-5) * np.sqrt(var_s) + mu_s


def full_transform(fc, fs, kind='tf', f64=True):
    """y: the level's transform of fc [h][w][C] against fs [hs][ws][C] at alpha = 1 -- in float64 arithmetic (f64), or as the
    reference computes it"""
    if kind == 'adain':
        return _adain64(fc, fs) if f64 else oracle.adain(fc, fs, 1.0)[0]
    if kind == 'tf':
        return oracle.wct_tf(fc, fs, 1.0, dtype=np.float64 if f64 else np.float32)[0]
    return oracle.wct_np(np.float64(fc), np.float64(fs), 1.0)[0] if f64 else oracle.wct_np(fc, fs, 1.0)[0]


def transform(fc, fs, smap, stride, alpha, kind='tf', f64=True):
    """One level with a strength map: fc [h][w][C], fs [hs][ws][C], smap [H][W] uint8 sampled at `stride`.  f64: the transform and
    the blend in float64 (the yardstick); else the reference's float32 transform and the float32 rule."""
    fc = np.asarray(fc, F)
    h, w = fc.shape[:2]
    y = full_transform(fc, np.asarray(fs, F), kind, f64)
    v = level_bytes(smap, h, w, stride)
    if not f64:
        return blend(y, fc, strength(alpha, v))
    a = (float(alpha) * (v.astype(np.float64) / 255.0))[..., None]
    return a * np.float64(y) + (1.0 - a) * np.float64(fc)


def stylize(content, style, smap, wts, relu_targets, alpha=1.0, adain=False, wct_mode='tf', f64=True):
    """WCT.predict(strength=smap) through the test-mode graph: oracle.stylize with every level's transform replaced by the
    strength one (one style pass with all taps; level i > 0 encodes clip(previous decoded, 0, 1)).  smap None: the plain call --
    an all-255 map, alpha in every row -- through the same code, which is the yardstick of the end-to-end test."""
    kind = 'adain' if adain else wct_mode
    c01 = np.float32(net_oracle.preprocess(content))
    style_feats = net_oracle.encode(np.float32(net_oracle.preprocess(style)), wts, relu_targets)
    if smap is None:
        smap = np.full(np.shape(content)[:2], 255, np.uint8)
    x = c01
    for i, relu in enumerate(relu_targets):
        if i > 0:
            x = np.clip(x, 0, 1)
        fc = net_oracle.encode(x, wts, [relu])[relu]
        h, w, c = fc.shape[-3:]
        t = transform(fc.reshape(h, w, c), np.squeeze(style_feats[relu]), smap, 2 ** (int(relu[4]) - 1), alpha, kind, f64)
        x = net_oracle.decode(np.float32(t), wts, relu)
    return net_oracle.postprocess(x)
