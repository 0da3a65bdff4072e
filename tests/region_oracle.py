"""CPU oracle of style regions (TEST INFRASTRUCTURE ONLY): spatial control whose styles are labelled PARTS of their images.  Built
on tests/mask_oracle.py: the whole predict() is mask_oracle.stylize_masked, except that style k's features of a level are the
rows of label k of ITS label map,

    feat.reshape(-1, C)[level_labels(map_k, h, w, stride) == k]            (map_k None: the whole map, as stylize_masked)

by the content side's rule: feature pixel (i, j) at stride s = 2^(l-1) has the label map[min(i s, Hs - 1)][min(j s, Ws - 1)].  The
encoder sees the whole style image; only the rows entering the statistics are selected.
"""
import numpy as np

from oracle import net_oracle
from mask_oracle import level_labels, transform_masked


def region_rows(feat, style_map, label, stride):
    """the rows [n][C] of `label` of a style feature map [h][w][C] under style_map (None, or every row selected: the map itself)"""
    if style_map is None:
        return feat
    h, w, c = feat.shape[-3:]
    sel = level_labels(style_map, h, w, stride).reshape(-1) == label
    return feat if sel.all() else np.ascontiguousarray(feat.reshape(-1, c)[sel])


def stylize_regions(content, styles, style_maps, mask, wts, relu_targets, alpha=1.0, adain=False, wct_mode='tf', fp16_storage=False):
    """WCT.predict_masked(content, styles, mask, style_masks=style_maps) through the test-mode graph"""
    kind = 'adain' if adain else wct_mode
    c01 = np.float32(net_oracle.preprocess(content))
    style_feats = [net_oracle.encode(np.float32(net_oracle.preprocess(s)), wts, relu_targets, fp16_storage) for s in styles]
    x = c01
    for i, relu in enumerate(relu_targets):
        if i > 0:
            x = np.clip(x, 0, 1)
        fc = net_oracle.encode(x, wts, [relu], fp16_storage)[relu]
        h, w, c = fc.shape[-3:]
        stride = 2 ** (int(relu[4]) - 1)
        labels = level_labels(mask, h, w, stride)
        fs = []
        for k, sf in enumerate(style_feats):
            f = np.asarray(sf[relu])
            f = f.reshape(f.shape[-3:])
            fs.append(region_rows(f, style_maps[k], k, stride))
        if all(f.ndim == 3 for f in fs):                          # whole maps only: mask_oracle.stylize_masked's own call
            t = transform_masked(fc.reshape(h, w, c), fs, labels, alpha, kind)
        else:                                                     # rows: every region goes through region_transform
            t = transform_masked(fc.reshape(-1, c), fs, labels.reshape(-1), alpha, kind).reshape(h, w, c)
        x = net_oracle.decode(t, wts, relu, fp16_storage)
    return net_oracle.postprocess(x)
