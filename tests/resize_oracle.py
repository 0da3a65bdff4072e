"""NumPy restatement of the bilinear resize rule (wct_tf_amd/csrc/resize_rule.h, include/wct_hip.h): Pillow's 8-bit resampler.
Python floats are IEEE doubles and nothing here is fused, so the taps are the ones the host function builds; the accumulation is
int64 (the rule's int32 never overflows: the taps of a row sum to 2^22 +- ksize)."""
import math

import numpy as np

BITS = 22

# (H, W, h, w): the geometries the rule was pinned to Pillow on
GEOMETRIES = [
    (1080, 1920, 512, 910), (720, 1280, 512, 910), (2000, 3000, 512, 768), (480, 640, 240, 320),
    (37, 53, 512, 733), (5, 7, 96, 96), (1, 1, 3, 2),
    (300, 200, 77, 51), (37, 53, 24, 35), (96, 128, 48, 64),
    (64, 64, 64, 31), (513, 511, 512, 512), (100, 100, 101, 99), (64, 48, 64, 48),
    (1200, 8, 4, 8), (8, 1200, 8, 4), (300, 5, 1, 5), (70, 1, 35, 1), (1, 9, 4, 3), (3, 3, 1, 1), (2, 2, 1, 1),
]
CHECKERBOARD = [(97, 131, 40, 60), (97, 131, 200, 300), (97, 131, 97, 60)]


def ksize(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def taps(n_in, n_out):
    """-> (bounds int32 [out][2] = (xmin, n), k int32 [out][ksize], zero past n)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = []
        ww = 0.0
        for x in range(n):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
            ww += w[-1]
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, n)
    return bounds, k


def _axis0(a, n_out):
    """resize along axis 0 of a uint8 array [n_in][...]"""
    bounds, k = taps(a.shape[0], n_out)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    src = a.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = np.tensordot(k[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0)) + (1 << (BITS - 1))
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(img, h, w):
    """img uint8 [H][W][3] -> [h][w][3]: along x into a uint8 intermediate [H][w][3], then along y"""
    a = np.ascontiguousarray(img, np.uint8)
    mid = _axis0(a.transpose(1, 0, 2), w).transpose(1, 0, 2)
    return np.ascontiguousarray(_axis0(mid, h))


def pillow(img, h, w):
    from PIL import Image
    return np.array(Image.fromarray(np.ascontiguousarray(img, np.uint8)).resize((w, h), Image.BILINEAR))


def random_image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
