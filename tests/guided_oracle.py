"""NumPy restatement of the guided-smoothing rule (include/wct_hip.h, wct_guided_filter; wct_tf_amd/csrc/guided_rule.h),
independent of the library:

    rdiv(a, b) = floor((2a + b) / (2b))
    I          = (77 p.R + 150 p.G + 29 p.B + 128) >> 8,  p = c[min(y, Hc-1)][min(x, Wc-1)]
    window     = rows max(0, y-r) .. min(H-1, y+r) x the same in x, n pixels
    pass 1     a_q = rdiv((n SIp - SI Sp) 2^12, n SII - SI^2 + eps_q n^2),  b_q = rdiv(Sp 2^12 - a_q SI, n)
    pass 2     out = clamp(rdiv(I sum a_q + sum b_q, n 2^12), 0, 255)

`guided_filter` is the vectorised int64 form (2-D cumulative sums) the tests compare against; `guided_filter_loop` is a
deliberately naive loop over windows in Python integers that only cross-checks the first; `guided_filter_f64` is the float64
guided filter of He et al. with the same guide and box, the yardstick of the rule's error."""
import numpy as np

from colors_oracle import clamped_content, luma256

SHIFT = 12
MAX_RADIUS, MAX_EPS = 64, 65025


def eps_q_of(eps):
    """eps of the [0,1]^2 convention in grey levels squared"""
    return max(1, int(round(float(eps) * 65025)))


def rdiv(a, b):
    """floor((2a + b) / (2b)) on int64 arrays (numpy's // floors) or Python integers"""
    return (2 * a + b) // (2 * b)


def guide(content, ho, wo):
    """the guide of every output pixel, int64 [...][ho][wo] in 0 .. 255"""
    return ((luma256(clamped_content(content, ho, wo)) + 128) >> 8).astype(np.int64)


def box(a, r):
    """window sums of int64 / float64 [...][H][W] over the (2r+1)^2 box cut at the border, by 2-D cumulative sums"""
    h, w = a.shape[-2], a.shape[-1]
    p = np.zeros(a.shape[:-2] + (h + 1, w + 1), a.dtype)
    p[..., 1:, 1:] = a.cumsum(-2).cumsum(-1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r, h - 1) + 1
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r, w - 1) + 1
    return (p[..., y1[:, None], x1[None, :]] - p[..., y0[:, None], x1[None, :]]
            - p[..., y1[:, None], x0[None, :]] + p[..., y0[:, None], x0[None, :]])


def count(h, w, r):
    return box(np.ones((h, w), np.int64), r)


def _check(s, c, r, eps_q):
    assert s.dtype == np.uint8 and c.dtype == np.uint8 and s.shape[-1] == 3 and c.shape[-1] == 3
    assert 1 <= r <= MAX_RADIUS and 1 <= eps_q <= MAX_EPS


def coefficients(stylized, content, r, eps_q):
    """pass 1: (a_q, b_q) int64 [...][H][W][3], and the guide and n it used"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q)
    h, w = s.shape[-3], s.shape[-2]
    I, n = guide(c, h, w), count(h, w, r)
    SI, SII = box(I, r), box(I * I, r)
    a_q, b_q = [], []
    for ch in range(3):
        p = s[..., ch].astype(np.int64)
        Sp, SIp = box(p, r), box(I * p, r)
        a = rdiv((n * SIp - SI * Sp) << SHIFT, n * SII - SI * SI + eps_q * n * n)
        a_q.append(a)
        b_q.append(rdiv((Sp << SHIFT) - a * SI, n))
    return np.stack(a_q, -1), np.stack(b_q, -1), I, n


def guided_filter_unclamped(stylized, content, r, eps_q):
    """the rule before the clamp to 0 .. 255, int64 [...][H][W][3]"""
    a_q, b_q, I, n = coefficients(stylized, content, r, eps_q)
    return np.stack([rdiv(box(a_q[..., ch], r) * I + box(b_q[..., ch], r), n << SHIFT) for ch in range(3)], -1)


def guided_filter(stylized, content, r, eps_q):
    """uint8 [...][H][W][3] stylized, uint8 [...][Hc][Wc][3] content (leading batch dimensions equal) -> uint8"""
    return np.clip(guided_filter_unclamped(stylized, content, r, eps_q), 0, 255).astype(np.uint8)


def guided_filter_loop(stylized, content, r, eps_q):
    """one frame, window by window, in Python integers"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q)
    h, w, _ = s.shape
    hc, wc, _ = c.shape
    I = [[(sum(k * int(v) for k, v in zip((77, 150, 29), c[min(y, hc - 1), min(x, wc - 1)])) + 128) >> 8 for x in range(w)]
         for y in range(h)]

    def window(y, x):
        return [(yy, xx) for yy in range(max(0, y - r), min(h - 1, y + r) + 1) for xx in range(max(0, x - r), min(w - 1, x + r) + 1)]

    ab = {}
    for y in range(h):
        for x in range(w):
            win = window(y, x)
            n = len(win)
            SI, SII = sum(I[yy][xx] for yy, xx in win), sum(I[yy][xx] ** 2 for yy, xx in win)
            for ch in range(3):
                Sp = sum(int(s[yy, xx, ch]) for yy, xx in win)
                SIp = sum(I[yy][xx] * int(s[yy, xx, ch]) for yy, xx in win)
                a = rdiv((n * SIp - SI * Sp) << SHIFT, n * SII - SI * SI + eps_q * n * n)
                ab[y, x, ch] = (a, rdiv((Sp << SHIFT) - a * SI, n))
    out = np.zeros_like(s)
    for y in range(h):
        for x in range(w):
            win = window(y, x)
            for ch in range(3):
                SA, SB = sum(ab[yy, xx, ch][0] for yy, xx in win), sum(ab[yy, xx, ch][1] for yy, xx in win)
                out[y, x, ch] = max(0, min(255, rdiv(SA * I[y][x] + SB, len(win) << SHIFT)))
    return out


def guided_filter_f64(stylized, content, r, eps_q):
    """He et al.'s guided filter in float64 with the rule's guide, box and eps (grey levels squared), before any rounding"""
    s, c = np.asarray(stylized), np.asarray(content)
    h, w = s.shape[-3], s.shape[-2]
    I, n = guide(c, h, w).astype(np.float64), count(h, w, r).astype(np.float64)
    mI = box(I, r) / n
    var = box(I * I, r) / n - mI * mI
    out = []
    for ch in range(3):
        p = s[..., ch].astype(np.float64)
        mp = box(p, r) / n
        a = (box(I * p, r) / n - mI * mp) / (var + eps_q)
        b = mp - a * mI
        out.append(box(a, r) / n * I + box(b, r) / n)
    return np.stack(out, -1)


def clamp_case(seed=0, h=24, w=28):
    """an input whose filtered values leave 0 .. 255: a guide of 100 .. 105 with a few outliers of +5 .. +60, and s an amplified
    copy of it (at r = 1, eps_q = 1 the local line through an outlier overshoots at its neighbours)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(100, 106, (h, w)).astype(np.int64)
    out = rng.random((h, w)) < 0.06
    g = g + out * rng.integers(5, 61, (h, w))
    c = np.repeat(g[..., None], 3, -1).astype(np.uint8)
    s = np.clip((g[..., None] - 100) * np.array([4, 5, 6]) + np.array([0, 10, 20]), 0, 255).astype(np.uint8)
    return s, c
