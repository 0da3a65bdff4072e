"""NumPy restatement of temporal guided upsampling (include/wct_hip.h, wct_guided_upsample_time;
wct_tf_amd/csrc/guided_up_time_rule.h), independent of the library and built on guided_motion_oracle's and guided_up_oracle's pieces:

    1. a_q, b_q of (f, y, x) on the small clip   guided_motion_oracle.coefficients (the shifted 3-D window; equal positions: the
                                                 window of guided_time_oracle)
    2. am = rdiv(box3(a_q), n), bm = rdiv(box3(b_q), n)   over the same window                              (2^-12 units)
    3. guided_up_oracle's taps and sum on frame f's own means and frame f's full content

`guided_upsample_time` is the vectorised int64 form the tests compare against; `guided_upsample_time_loop` a deliberately naive
loop over windows in Python integers that only cross-checks it on tiny clips; `guided_upsample_time_f64` the float64 fast guided
filter with the same guide, window and half-pixel bilinear map, the yardstick of the rule's error, and `bound` the rule's stated
distance from it; `guided_upsample_time_chunked` delivers a clip chunk by chunk with a halo of SMALL frames on each side, as a
caller of the device call does for a clip longer than 32 frames."""
import numpy as np

import guided_oracle as g2
import guided_motion_oracle as gm
import guided_up_oracle as gu


def _pos(positions, frames):
    return np.zeros((frames, 2), np.int32) if positions is None else np.asarray(positions)


def means(stylized, contents_small, r, eps_q, t, positions=None):
    """step 2: (am, bm) int64 [F][h][w][3]"""
    pos = _pos(positions, len(stylized))
    a_q, b_q, _, n = gm.coefficients(stylized, contents_small, r, eps_q, t, pos)
    am = np.stack([g2.rdiv(gm.box3(a_q[..., ch], r, t, pos), n) for ch in range(3)], -1)
    bm = np.stack([g2.rdiv(gm.box3(b_q[..., ch], r, t, pos), n) for ch in range(3)], -1)
    return am, bm


def corners(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """per full pixel and channel the four values am_k I + bm_k (2^-12 units), int64 [4][F][H][W][3], and their weights
    int64 [4][H][W] (sum 65536)"""
    c, C = np.asarray(contents_small), np.asarray(contents_full)
    assert C.dtype == np.uint8 and C.ndim == 4 and C.shape[-1] == 3 and len(C) == len(c)
    hc, wc = c.shape[1:3]
    H, W = C.shape[1:3]
    assert H >= hc and W >= wc
    am, bm = means(stylized, c, r, eps_q, t, positions)
    I = g2.guide(C, H, W)[..., None]
    y0, y1, fy = gu.axis(H, hc)
    x0, x1, fx = gu.axis(W, wc)
    vals, wts = [], []
    for ys, wy in ((y0, gu.ONE - fy), (y1, fy)):
        for xs, wx in ((x0, gu.ONE - fx), (x1, fx)):
            vals.append(am[:, ys[:, None], xs[None, :], :] * I + bm[:, ys[:, None], xs[None, :], :])
            wts.append(wy[:, None] * wx[None, :])
    return np.stack(vals), np.stack(wts)


def guided_upsample_time_unclamped(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """the rule before the clamp, int64 [F][H][W][3]"""
    vals, wts = corners(stylized, contents_small, contents_full, r, eps_q, t, positions)
    v = sum(vals[k] * wts[k][..., None] for k in range(4))
    return (v + (1 << (g2.SHIFT + 2 * gu.WBITS - 1))) >> (g2.SHIFT + 2 * gu.WBITS)


def guided_upsample_time(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """uint8 [F][h][w][3] small frames, [F][hc][wc][3] small contents, [F][H][W][3] full contents, int positions [F][2] or None
    -> uint8 [F][H][W][3]"""
    return np.clip(guided_upsample_time_unclamped(stylized, contents_small, contents_full, r, eps_q, t, positions), 0, 255).astype(np.uint8)


def guided_upsample_time_loop(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """window by window and pixel by pixel, in Python integers"""
    s, c, C = np.asarray(stylized), np.asarray(contents_small), np.asarray(contents_full)
    nf, h, w, _ = s.shape
    hc, wc = c.shape[1:3]
    H, W = C.shape[1:3]
    pos = [(int(a), int(b)) for a, b in _pos(positions, nf)]
    luma = lambda p: (sum(k * int(v) for k, v in zip((77, 150, 29), p)) + 128) >> 8
    I = [[[luma(c[f, min(y, hc - 1), min(x, wc - 1)]) for x in range(w)] for y in range(h)] for f in range(nf)]

    def window(f, y, x):
        win = []
        for g in range(max(0, f - t), min(nf - 1, f + t) + 1):
            cy, cx = y + pos[g][0] - pos[f][0], x + pos[g][1] - pos[f][1]
            win += [(g, yy, xx) for yy in range(max(0, cy - r), min(h - 1, cy + r) + 1) for xx in range(max(0, cx - r), min(w - 1, cx + r) + 1)]
        return win

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
    m = {}
    for f in range(nf):
        for y in range(hc):
            for x in range(wc):
                win = window(f, y, x)
                n = len(win)
                for ch in range(3):
                    sa, sb = sum(ab[p + (ch,)][0] for p in win), sum(ab[p + (ch,)][1] for p in win)
                    m[f, y, x, ch] = ((2 * sa + n) // (2 * n), (2 * sb + n) // (2 * n))

    def tap(P, N, mm):
        tt = min(max((2 * P + 1) * mm - N, 0), 2 * N * (mm - 1))
        p0 = tt // (2 * N)
        return p0, min(p0 + 1, mm - 1), (2 * (tt - p0 * 2 * N) * 256 + 2 * N) // (4 * N)

    out = np.zeros_like(C)
    for f in range(nf):
        for Y in range(H):
            y0, y1, fy = tap(Y, H, hc)
            for X in range(W):
                x0, x1, fx = tap(X, W, wc)
                J = luma(C[f, Y, X])
                for ch in range(3):
                    v = 0
                    for yy, wy in ((y0, 256 - fy), (y1, fy)):
                        for xx, wx in ((x0, 256 - fx), (x1, fx)):
                            a, b = m[f, yy, xx, ch]
                            v += wy * wx * (a * J + b)
                    out[f, Y, X, ch] = max(0, min(255, (v + (1 << 27)) >> 28))
    return out


def guided_upsample_time_f64(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """the fast guided filter in float64, before any rounding: He et al.'s a, b on the small clip with the rule's guide, shifted 3-D
    window and eps; their means over the same window; bilinear interpolation on half-pixel centres over the content extent
    hc x wc; a I + b on the full guide of the frame"""
    s, c, C = np.asarray(stylized), np.asarray(contents_small), np.asarray(contents_full)
    nf, h, w = s.shape[:3]
    hc, wc = c.shape[1:3]
    H, W = C.shape[1:3]
    pos = _pos(positions, nf)
    box = lambda a: gm.box3(a, r, t, pos)
    I, n = g2.guide(c, h, w).astype(np.float64), gm.count3(nf, h, w, r, t, pos).astype(np.float64)
    mI = box(I) / n
    var = box(I * I) / n - mI * mI
    IF = g2.guide(C, H, W).astype(np.float64)

    def frac(N, m):
        src = np.clip((np.arange(N) + 0.5) * m / N - 0.5, 0, m - 1)
        p0 = np.minimum(np.floor(src).astype(np.int64), m - 1)
        return p0, np.minimum(p0 + 1, m - 1), src - p0

    y0, y1, fy = frac(H, hc)
    x0, x1, fx = frac(W, wc)

    def interp(m):
        top = m[:, y0[:, None], x0[None, :]] * (1 - fx) + m[:, y0[:, None], x1[None, :]] * fx
        bot = m[:, y1[:, None], x0[None, :]] * (1 - fx) + m[:, y1[:, None], x1[None, :]] * fx
        return top * (1 - fy)[:, None] + bot * fy[:, None]

    out = []
    for ch in range(3):
        p = s[..., ch].astype(np.float64)
        mp = box(p) / n
        a = (box(I * p) / n - mI * mp) / (var + eps_q)
        b = mp - a * mI
        out.append(interp(box(a) / n) * IF + interp(box(b) / n))
    return np.stack(out, -1)


def bound(stylized, contents_small, contents_full, r, eps_q, t, positions=None):
    """the rule's stated distance from guided_upsample_time_f64 per pixel and channel, before the clamp (guided_up_time_rule.h):
    0.5 + 256 2^-12 + D 2^-8, D the spread of the pixel's four am_k I + bm_k in grey levels"""
    vals, _ = corners(stylized, contents_small, contents_full, r, eps_q, t, positions)
    D = (vals.max(0) - vals.min(0)).astype(np.float64) / (1 << g2.SHIFT)
    return 0.5 + 256.0 / (1 << g2.SHIFT) + D / (1 << gu.WBITS)


def guided_upsample_time_chunked(stylized, contents_small, contents_full, r, eps_q, t, chunk, halo, positions=None):
    """the clip delivered in chunks of `chunk` frames, each from a clip of its own with `halo` SMALL frames on each side, its slice
    of the positions, and the full contents of the delivered frames only: the whole clip's bytes when halo >= 2 t"""
    s, c, C = np.asarray(stylized), np.asarray(contents_small), np.asarray(contents_full)
    pos = _pos(positions, len(s))
    out = np.empty_like(C)
    for f0 in range(0, len(s), chunk):
        f1 = min(len(s), f0 + chunk)
        g0, g1 = max(0, f0 - halo), min(len(s), f1 + halo)
        am, bm = means(s[g0:g1], c[g0:g1], r, eps_q, t, pos[g0:g1])
        out[f0:f1] = deliver(am[f0 - g0:f1 - g0], bm[f0 - g0:f1 - g0], c.shape[1], c.shape[2], C[f0:f1])
    return out


def deliver(am, bm, hc, wc, contents_full):
    """step 3 alone: the means of some frames and the full contents of those frames -> uint8 [.][H][W][3]"""
    C = np.asarray(contents_full)
    H, W = C.shape[1:3]
    I = g2.guide(C, H, W)[..., None]
    y0, y1, fy = gu.axis(H, hc)
    x0, x1, fx = gu.axis(W, wc)
    v = 0
    for ys, wy in ((y0, gu.ONE - fy), (y1, fy)):
        for xs, wx in ((x0, gu.ONE - fx), (x1, fx)):
            v = v + (am[:, ys[:, None], xs[None, :], :] * I + bm[:, ys[:, None], xs[None, :], :]) * (wy[:, None] * wx[None, :])[..., None]
    return np.clip((v + (1 << (g2.SHIFT + 2 * gu.WBITS - 1))) >> (g2.SHIFT + 2 * gu.WBITS), 0, 255).astype(np.uint8)


def clip_case(seed, frames, h, w, hc, wc, H, W):
    """a seeded clip: guided_up_oracle.case per frame (its own seed each), stacked -> (s, c, C)"""
    parts = [gu.case(seed * 100 + f, h, w, hc, wc, H, W) for f in range(frames)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def noise_clip(seed, frames, h, w, hc, wc, H, W):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (frames,) + shp + (3,)).astype(np.uint8) for shp in ((h, w), (hc, wc), (H, W)))


def zigzag(frames, step):
    """positions that go forth and back by `step` = (sy, sx) per frame"""
    return gm.positions_of([(step[0] * (-1) ** f, step[1] * (-1) ** f) for f in range(frames - 1)])


# ---- the case the feature was built for -----------------------------------------------------------------------------------------
def flicker_case(frames=12, H=96, W=128, ratio=4, edge=66, seed=0):
    """a static 50 | 200 step at full column `edge` (off the small grid); the small content is the rounded ratio x ratio block
    mean; the small frame is that content plus N(0, 20) noise, rounded and clipped; grey replicated to RGB -> (s, c, C)"""
    rgb = lambda a: np.repeat(np.clip(np.rint(a), 0, 255)[..., None], 3, -1).astype(np.uint8)
    full = np.full((H, W), 50.0)
    full[:, edge:] = 200.0
    small = np.rint(full.reshape(H // ratio, ratio, W // ratio, ratio).mean((1, 3)))
    rng = np.random.default_rng(seed)
    s = rgb(small[None] + rng.normal(0, 20, (frames,) + small.shape))
    return s, rgb(np.repeat(small[None], frames, 0)), rgb(np.repeat(full[None], frames, 0))


def flicker(out, cols=42):
    """mean |difference between consecutive frames| over columns < cols of frames 2 .. 9"""
    v = out[2:10, :, :cols, 0].astype(np.float64)
    return float(np.abs(np.diff(v, axis=0)).mean())


def edge_jump(out, edge=66):
    """(mean, smallest over rows and frames) of the jump between full columns edge - 1 and edge"""
    d = out[:, :, edge, 0].astype(np.float64) - out[:, :, edge - 1, 0].astype(np.float64)
    return float(d.mean()), float(d.min())
