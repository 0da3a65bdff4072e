"""CPU oracle of a style mix (TEST INFRASTRUCTURE ONLY): Li et al. 2017, sec. 4.2,

    lambda_k = w_k / sum(w),   mix(fc) = sum_k lambda_k T(fc, fs_k, alpha)

restated on oracle.wct_oracle (T = wct_tf, wct_np or adain) and, for the whole predict(), on oracle.net_oracle's
encode / decode the way oracle.stylize chains them (oracle.stylize has no hook for a mix).  The sum runs in float32, k in
order, from zero -- so one-hot weights give oracle.stylize's frame bit for bit.
"""
import numpy as np

import oracle
from oracle import net_oracle

_T = {'tf': oracle.wct_tf, 'np': oracle.wct_np, 'adain': oracle.adain}


def lambdas(weights, k):
    """lambda_k = w_k / sum(w) of the float32 weights the library receives (None: equal)"""
    w = np.ones(k) if weights is None else np.asarray(np.asarray(weights, np.float32), np.float64)
    assert w.shape == (k,) and np.all(w >= 0) and w.sum() > 0
    return w / w.sum()


def mix(terms, weights):
    """sum_k lambda_k terms[k] in float32, k in order, from zero"""
    lam = lambdas(weights, len(terms))
    acc = np.zeros_like(np.asarray(terms[0], np.float32))
    for l, t in zip(lam, terms):
        acc = acc + np.float32(l) * np.asarray(t, np.float32)
    return acc


def transform_mix(fc, styles, weights, alpha, kind='tf'):
    """the mixed transform of one level: kind 'tf' / 'np' (wct_tf / wct_np) or 'adain'; features [1][h][w][C]"""
    return mix([_T[kind](fc, fs, alpha) for fs in styles], weights)


def stylize_mix(content, styles, weights, wts, relu_targets, alpha=1.0, adain=False, wct_mode='tf', fp16_storage=False):
    """WCT.predict_mix through the test-mode graph: oracle.stylize with every level's transform replaced by the mix
    (one style pass per style with all taps; level i > 0 encodes clip(previous decoded, 0, 1))."""
    kind = 'adain' if adain else wct_mode
    c01 = np.float32(net_oracle.preprocess(content))
    style_feats = [net_oracle.encode(np.float32(net_oracle.preprocess(s)), wts, relu_targets, fp16_storage) for s in styles]
    x = c01
    for i, relu in enumerate(relu_targets):
        if i > 0:
            x = np.clip(x, 0, 1)
        fc = net_oracle.encode(x, wts, [relu], fp16_storage)[relu]
        t = transform_mix(fc, [sf[relu] for sf in style_feats], weights, alpha, kind)[0]
        x = net_oracle.decode(t, wts, relu, fp16_storage)
    return net_oracle.postprocess(x)
