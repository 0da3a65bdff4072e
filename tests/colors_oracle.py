"""NumPy restatement of the luminance-only colour rule (include/wct_hip.h, wct_content_colors), independent of the library:

    p      = c[min(y, Hc-1)][min(x, Wc-1)]
    Y(q)   = 77 q.R + 150 q.G + 29 q.B
    d      = Y(s[y][x]) - Y(p)
    out.ch = clamp((256 p.ch + d + 128) >> 8, 0, 255)

`content_colors` is the vectorised form the tests compare against; `content_colors_loop` is a deliberately naive per-pixel
loop in Python integers that only cross-checks the first.  `quantise` is the output rule of the stylize chain,
uint8(clip(x, 0, 1) * 255.f) truncating, in float32 -- what WCT_FLAG_IMAGES_F32 applies to a float content."""
import numpy as np

WEIGHTS = (77, 150, 29)


def luma256(img):
    """Y x 256 of uint8 [...][3] as int32"""
    a = np.asarray(img).astype(np.int32)
    return WEIGHTS[0] * a[..., 0] + WEIGHTS[1] * a[..., 1] + WEIGHTS[2] * a[..., 2]


def clamped_content(content, ho, wo):
    """the content pixel of every output pixel: [...][ho][wo][3], index (min(y, Hc-1), min(x, Wc-1))"""
    c = np.asarray(content)
    hc, wc = c.shape[-3], c.shape[-2]
    assert ho >= hc and wo >= wc
    ys = np.minimum(np.arange(ho), hc - 1)
    xs = np.minimum(np.arange(wo), wc - 1)
    return c[..., ys[:, None], xs[None, :], :]


def content_colors_unclamped(stylized, content):
    """the rule before the clamp to 0 .. 255, int32 [...][Ho][Wo][3] (the property tests look at it)"""
    s = np.asarray(stylized)
    assert s.dtype == np.uint8 and np.asarray(content).dtype == np.uint8
    p = clamped_content(content, s.shape[-3], s.shape[-2]).astype(np.int32)
    d = luma256(s) - luma256(p)
    return (256 * p + d[..., None] + 128) >> 8           # numpy's >> on negative int32 is arithmetic: floor


def content_colors(stylized, content):
    """uint8 [...][Ho][Wo][3] stylized, uint8 [...][Hc][Wc][3] content (leading batch dimensions equal) -> uint8"""
    return np.clip(content_colors_unclamped(stylized, content), 0, 255).astype(np.uint8)


def content_colors_loop(stylized, content):
    """one frame, pixel by pixel, in Python integers (// floors like the arithmetic shift)"""
    s, c = np.asarray(stylized), np.asarray(content)
    ho, wo, _ = s.shape
    hc, wc, _ = c.shape
    out = np.zeros_like(s)
    for y in range(ho):
        for x in range(wo):
            sp = [int(v) for v in s[y, x]]
            p = [int(v) for v in c[min(y, hc - 1), min(x, wc - 1)]]
            d = sum(w * v for w, v in zip(WEIGHTS, sp)) - sum(w * v for w, v in zip(WEIGHTS, p))
            for ch in range(3):
                out[y, x, ch] = max(0, min(255, (256 * p[ch] + d + 128) // 256))
    return out


def quantise(img01):
    """float image in [0,1] -> uint8 by the chain's output rule, in float32"""
    x = np.asarray(img01, np.float32)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
