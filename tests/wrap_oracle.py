"""NumPy statement of the PERIODIC network (include/wct_hip.h, "seamless textures"), independent of the pad-and-crop construction
the library uses: every 3x3 conv of oracle.net_oracle's layer lists is applied to its own input continued periodically by one
pixel (np.pad(mode='wrap')) and cropped by one, so the conv's own reflect pad only ever touches the discarded ring; pools and
upsamples run on even sizes, where they commute with a shift by their stride.  The transform is the oracle's own, on one period.
The style side is the plain network's: a prepared style is encoded as any style is.  float32, direct convolutions."""
import numpy as np

import oracle
from oracle import net_oracle

# the seam case shared by tests/test_wrap_cpu.py (on the oracle) and tests/test_gpu_wrap.py (on the device): one pass over the noise
# (seed, sample) of `size` on the contractive net (oracle/contractive.py, seed 7), style = synthetic_image(*style)
SEAM_CASE = dict(seed=11, sample=0, size=(64, 96), style=(902, 80, 96), targets=['relu3_1', 'relu2_1', 'relu1_1'], alpha=0.8)
LEVEL = {'relu1_1': 1, 'relu2_1': 2, 'relu3_1': 3, 'relu4_1': 4, 'relu5_1': 5}


def conv3x3_circular(x, w_hwio, b, relu=True):
    """the 3x3 conv on a torus: the layer's own function on the map continued by one pixel, the ring dropped"""
    xp = np.pad(np.asarray(x, np.float32), ((1, 1), (1, 1), (0, 0)), mode='wrap')
    return net_oracle.conv3x3_reflect(xp, w_hwio, b, relu=relu)[1:-1, 1:-1]


def encode(img01, weights, target):
    """relu<l>_1 of the periodic VGG on an HxWx3 image in [0,1]; H and W multiples of 2^(l-1)"""
    enc = weights['encoder']
    s = 1 << (LEVEL[target] - 1)
    assert img01.shape[0] % s == 0 and img01.shape[1] % s == 0, 'ceil-mode pooling of an odd size is not periodic'
    x = net_oracle.conv1x1(np.asarray(img01, np.float32), *enc['preprocess'])
    for layer in net_oracle.ENCODER_LAYERS:
        if layer[0] == 'C':
            x = conv3x3_circular(x, enc[layer[1]][0], enc[layer[1]][1])
            if 'relu' + layer[1][4:] == target:
                return x
        else:
            assert x.shape[0] % 2 == 0 and x.shape[1] % 2 == 0
            x = net_oracle.maxpool2x2_same(x)
    raise ValueError(target)


def decode(feat, weights, target):
    """the periodic mirror decoder of `target`"""
    x = np.asarray(feat, np.float32)
    params = iter(weights['decoder'][target])
    for kind, _, _, relu in net_oracle.decoder_layers(target):
        if kind == 'C':
            w, b = next(params)
            x = conv3x3_circular(x, w, b, relu=relu)
        else:
            x = net_oracle.upsample2x_nearest(x)
    return x


def stylize(content, style, weights, relu_targets, alpha=1.0, adain=False, wct_mode='tf'):
    """oracle.stylize with the content chain on a torus: uint8 HxWx3, the size of the content"""
    s01 = np.float32(oracle.preprocess(style))
    style_feats = oracle.encode(s01, weights, relu_targets)
    x = np.float32(oracle.preprocess(content))
    for i, relu in enumerate(relu_targets):
        if i > 0:
            x = np.clip(x, 0, 1)
        fc, fs = encode(x, weights, relu), style_feats[relu]
        if adain:
            t = oracle.adain(fc, fs, alpha)[0]
        elif wct_mode == 'tf':
            t = oracle.wct_tf(fc, fs, alpha)[0]
        else:
            t = oracle.wct_np(fc, fs, alpha)[0]
        x = decode(t, weights, relu)
    return oracle.postprocess(x)


def seam_steps(frame):
    """The mean absolute step across the two joints of a tile laid beside itself (last row against first row, last column
    against first column), and the largest mean step between adjacent interior rows / columns of the same frame."""
    f = np.asarray(frame).astype(np.float64)
    rows = np.abs(f[1:] - f[:-1]).mean(axis=(1, 2))
    cols = np.abs(f[:, 1:] - f[:, :-1]).mean(axis=(0, 2))
    joint = max(np.abs(f[0] - f[-1]).mean(), np.abs(f[:, 0] - f[:, -1]).mean())
    return float(joint), float(max(rows.max(), cols.max()))
