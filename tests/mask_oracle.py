"""CPU oracle of spatial control (TEST INFRASTRUCTURE ONLY): Li et al. 2017, sec. 4.2 and Fig. 7 -- a label map picks the style
of each content region,

    out[rows of k] = T(content[rows of k], style k, alpha)      (rows of a label with < 2 pixels: unchanged)

restated on oracle.wct_oracle (T = wct_tf, wct_np or adain, each on the region's rows alone) and, for the whole predict(), on
oracle.net_oracle's encode / decode the way oracle.stylize chains them (oracle.stylize has no hook for a mask).  At level l
(stride s = 2^(l-1)) feature pixel (i, j) has the label mask[min(i s, H - 1)][min(j s, W - 1)].
"""
import numpy as np

import oracle
from oracle import net_oracle, wct_oracle

_T = {'tf': oracle.wct_tf, 'np': oracle.wct_np, 'adain': oracle.adain}


def level_labels(mask, h, w, stride):
    """labels [h][w] of a level's feature map: mask[min(i * stride, H - 1)][min(j * stride, W - 1)]"""
    mask = np.asarray(mask)
    ii = np.minimum(np.arange(h) * stride, mask.shape[0] - 1)
    jj = np.minimum(np.arange(w) * stride, mask.shape[1] - 1)
    return mask[np.ix_(ii, jj)]


_flatten_chw = wct_oracle._flatten_chw


def _flatten_rows(feat):
    """wct_oracle._flatten_chw, which also takes a region's rows [N][C] (a 1 x N map: its squeeze would drop the 1)"""
    f = np.asarray(feat)
    if f.ndim == 2:
        return np.ascontiguousarray(f.T), (1, f.shape[0], f.shape[1])
    return _flatten_chw(feat)


def region_transform(rows, style, alpha, kind='tf', **kw):
    """T of oracle.wct_oracle on a region's rows [N][C] (any N >= 2) -> [N][C]"""
    rows = np.asarray(rows)
    c = rows.shape[-1]
    if kind == 'adain':
        return _T[kind](rows.reshape(1, 1, -1, c), np.asarray(style).reshape(1, 1, -1, c), alpha, **kw).reshape(-1, c)
    wct_oracle._flatten_chw = _flatten_rows
    try:
        return _T[kind](rows, np.asarray(style).reshape(-1, c), alpha, **kw).reshape(-1, c)
    finally:
        wct_oracle._flatten_chw = _flatten_chw


def transform_masked(fc, styles, labels, alpha, kind='tf'):
    """the masked transform of one level: fc [h][w][C] (or [N][C]), labels [h][w] (or [N]), styles K feature maps"""
    fc = np.asarray(fc, np.float32)
    c = fc.shape[-1]
    labels = np.asarray(labels).reshape(-1)
    flat = fc.reshape(-1, c)
    out = flat.copy()
    for k, fs in enumerate(styles):
        rows = labels == k
        if rows.sum() < 2:
            continue
        if rows.all() and fc.ndim == 3:                           # one region: T on the map itself, as oracle.stylize calls it
            out = np.asarray(_T[kind](fc, fs, alpha), np.float32).reshape(-1, c)
        else:
            out[rows] = region_transform(flat[rows], np.asarray(fs, np.float32), alpha, kind)
    return out.reshape(fc.shape)


def stylize_masked(content, styles, mask, wts, relu_targets, alpha=1.0, adain=False, wct_mode='tf', fp16_storage=False):
    """WCT.predict_masked through the test-mode graph: oracle.stylize with every level's transform replaced by the masked one
    (one style pass per style with all taps; level i > 0 encodes clip(previous decoded, 0, 1))."""
    kind = 'adain' if adain else wct_mode
    c01 = np.float32(net_oracle.preprocess(content))
    style_feats = [net_oracle.encode(np.float32(net_oracle.preprocess(s)), wts, relu_targets, fp16_storage) for s in styles]
    x = c01
    for i, relu in enumerate(relu_targets):
        if i > 0:
            x = np.clip(x, 0, 1)
        fc = net_oracle.encode(x, wts, [relu], fp16_storage)[relu]
        h, w, c = fc.shape[-3:]
        labels = level_labels(mask, h, w, 2 ** (int(relu[4]) - 1))
        t = transform_masked(fc.reshape(h, w, c), [sf[relu] for sf in style_feats], labels, alpha, kind)
        x = net_oracle.decode(t, wts, relu, fp16_storage)
    return net_oracle.postprocess(x)
