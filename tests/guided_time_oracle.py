"""NumPy restatement of temporal guided smoothing (include/wct_hip.h, wct_guided_filter_time; wct_tf_amd/csrc/guided_time_rule.h),
independent of the library: the rule of guided_oracle with its box extended along time.

    clip       s [F][H][W][3], c [F][Hc][Wc][3]; T frames on each side, 0 .. 3
    window     the box of guided_oracle at (y, x) in each frame of max(0, f-T) .. min(F-1, f+T), n pixels
    pass 1     a_q, b_q of (f, y, x) from the sums over that window, by guided_oracle's formulas with this n
    pass 2     out = clamp(rdiv(I(f, y, x) sum a_q + sum b_q, n 2^12), 0, 255), the sums over the same window
    valid      guided_oracle's radius and eps_q, 0 <= T <= 3, (2r + 1)^2 (2T + 1) <= 33025

`guided_filter_time` is the vectorised int64 form: guided_oracle.box in each frame, then a cumulative sum along axis 0.
`guided_filter_time_loop` is a deliberately naive loop over 3-D windows in Python integers that only cross-checks the first;
`guided_filter_time_f64` is the float64 guided filter with the same guide and 3-D box, the yardstick of the rule's error;
`guided_filter_time_chunked` filters a clip chunk by chunk with a halo of frames on each side, as a caller of the device call
does for a clip longer than 32 frames."""
import numpy as np

import guided_oracle as g2

MAX_FRAMES_T = 3
MAX_WINDOW = 33025                          # floor(2^31 / 65025)
MAX_RADIUS = (64, 51, 40, 33)               # at T = 0 .. 3


def params_ok(r, eps_q, t):
    return 1 <= r <= g2.MAX_RADIUS and 1 <= eps_q <= g2.MAX_EPS and 0 <= t <= MAX_FRAMES_T and (2 * r + 1) ** 2 * (2 * t + 1) <= MAX_WINDOW


def tbox(a, t):
    """sums of [F][...] over frames max(0, f-t) .. min(F-1, f+t), by a cumulative sum along axis 0"""
    f = a.shape[0]
    p = np.zeros((f + 1,) + a.shape[1:], a.dtype)
    p[1:] = a.cumsum(0)
    lo, hi = np.maximum(np.arange(f) - t, 0), np.minimum(np.arange(f) + t, f - 1) + 1
    return p[hi] - p[lo]


def box3(a, r, t):
    """window sums of int64 / float64 [F][H][W] over the 3-D box cut at the borders and at the clip's ends"""
    return tbox(g2.box(a, r), t)


def count3(f, h, w, r, t):
    return box3(np.ones((f, h, w), np.int64), r, t)


def _check(s, c, r, eps_q, t):
    assert s.dtype == np.uint8 and c.dtype == np.uint8 and s.ndim == 4 and c.ndim == 4 and s.shape[-1] == 3 and c.shape[-1] == 3
    assert s.shape[0] == c.shape[0] and params_ok(r, eps_q, t), (s.shape, c.shape, r, eps_q, t)


def coefficients(stylized, content, r, eps_q, t):
    """pass 1: (a_q, b_q) int64 [F][H][W][3], and the guide and n it used"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t)
    f, h, w = s.shape[:3]
    I, n = g2.guide(c, h, w), count3(f, h, w, r, t)
    SI, SII = box3(I, r, t), box3(I * I, r, t)
    a_q, b_q = [], []
    for ch in range(3):
        p = s[..., ch].astype(np.int64)
        Sp, SIp = box3(p, r, t), box3(I * p, r, t)
        a = g2.rdiv((n * SIp - SI * Sp) << g2.SHIFT, n * SII - SI * SI + eps_q * n * n)
        a_q.append(a)
        b_q.append(g2.rdiv((Sp << g2.SHIFT) - a * SI, n))
    return np.stack(a_q, -1), np.stack(b_q, -1), I, n


def guided_filter_time_unclamped(stylized, content, r, eps_q, t):
    """the rule before the clamp to 0 .. 255, int64 [F][H][W][3]"""
    a_q, b_q, I, n = coefficients(stylized, content, r, eps_q, t)
    return np.stack([g2.rdiv(box3(a_q[..., ch], r, t) * I + box3(b_q[..., ch], r, t), n << g2.SHIFT) for ch in range(3)], -1)


def guided_filter_time(stylized, content, r, eps_q, t):
    """uint8 [F][H][W][3] stylized clip, uint8 [F][Hc][Wc][3] contents -> uint8 [F][H][W][3]"""
    return np.clip(guided_filter_time_unclamped(stylized, content, r, eps_q, t), 0, 255).astype(np.uint8)


def guided_filter_time_loop(stylized, content, r, eps_q, t):
    """window by window, in Python integers"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t)
    nf, h, w, _ = s.shape
    hc, wc = c.shape[1:3]
    I = [[[(sum(k * int(v) for k, v in zip((77, 150, 29), c[f, min(y, hc - 1), min(x, wc - 1)])) + 128) >> 8 for x in range(w)]
          for y in range(h)] for f in range(nf)]

    def window(f, y, x):
        return [(ff, yy, xx) for ff in range(max(0, f - t), min(nf - 1, f + t) + 1) for yy in range(max(0, y - r), min(h - 1, y + r) + 1)
                for xx in range(max(0, x - r), min(w - 1, x + r) + 1)]

    ab = {}
    for f in range(nf):
        for y in range(h):
            for x in range(w):
                win = window(f, y, x)
                n = len(win)
                SI, SII = sum(I[ff][yy][xx] for ff, yy, xx in win), sum(I[ff][yy][xx] ** 2 for ff, yy, xx in win)
                for ch in range(3):
                    Sp = sum(int(s[ff, yy, xx, ch]) for ff, yy, xx in win)
                    SIp = sum(I[ff][yy][xx] * int(s[ff, yy, xx, ch]) for ff, yy, xx in win)
                    a = g2.rdiv((n * SIp - SI * Sp) << g2.SHIFT, n * SII - SI * SI + eps_q * n * n)
                    ab[f, y, x, ch] = (a, g2.rdiv((Sp << g2.SHIFT) - a * SI, n))
    out = np.zeros_like(s)
    for f in range(nf):
        for y in range(h):
            for x in range(w):
                win = window(f, y, x)
                for ch in range(3):
                    SA, SB = sum(ab[p + (ch,)][0] for p in win), sum(ab[p + (ch,)][1] for p in win)
                    out[f, y, x, ch] = max(0, min(255, g2.rdiv(SA * I[f][y][x] + SB, len(win) << g2.SHIFT)))
    return out


def guided_filter_time_f64(stylized, content, r, eps_q, t):
    """He et al.'s guided filter in float64 over the 3-D box with the rule's guide and eps (grey levels squared), before any rounding"""
    s, c = np.asarray(stylized), np.asarray(content)
    f, h, w = s.shape[:3]
    I, n = g2.guide(c, h, w).astype(np.float64), count3(f, h, w, r, t).astype(np.float64)
    mI = box3(I, r, t) / n
    var = box3(I * I, r, t) / n - mI * mI
    out = []
    for ch in range(3):
        p = s[..., ch].astype(np.float64)
        mp = box3(p, r, t) / n
        a = (box3(I * p, r, t) / n - mI * mp) / (var + eps_q)
        b = mp - a * mI
        out.append(box3(a, r, t) / n * I + box3(b, r, t) / n)
    return np.stack(out, -1)


def guided_filter_time_chunked(stylized, content, r, eps_q, t, chunk, halo, op=guided_filter_time):
    """the clip filtered in chunks of `chunk` output frames, each as a clip of its own with `halo` frames on each side (fewer at
    the clip's ends): the whole clip's bytes when halo >= 2 t"""
    s, c = np.asarray(stylized), np.asarray(content)
    out = np.empty_like(s)
    for f0 in range(0, len(s), chunk):
        f1 = min(len(s), f0 + chunk)
        g0, g1 = max(0, f0 - halo), min(len(s), f1 + halo)
        out[f0:f1] = op(s[g0:g1], c[g0:g1], r, eps_q, t)[f0 - g0:f1 - g0]
    return out


def flicker_case(seed=0, frames=12, h=48, w=64, sigma=20, move=0):
    """a guide that steps from 50 to 200 (the step moving `move` px per frame) and frames of that step plus independent gaussian
    noise of `sigma` per frame -> (s, c, clean), uint8 [F][h][w][3] and the noise-free frames float64 [F][h][w]"""
    rng = np.random.default_rng(seed)
    edge = w // 2 - move * (frames // 2) + move * np.arange(frames)
    clean = np.where(np.arange(w)[None, None, :] < edge[:, None, None], 50.0, 200.0) * np.ones((frames, h, w))
    noisy = np.clip(np.rint(clean + rng.normal(0, sigma, clean.shape)), 0, 255)
    rgb = lambda a: np.repeat(a[..., None], 3, -1).astype(np.uint8)
    return rgb(noisy), rgb(clean), clean
