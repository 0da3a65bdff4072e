"""NumPy restatement of guided upsampling under the colour guide (include/wct_hip.h, wct_guided_upsample_guide with
WCT_GUIDE_COLOR; wct_tf_amd/csrc/guided_up_color_rule.h), independent of the library and built on the pieces of its two parents:

    1. a_q[i][p], b_q[p] on h x w   guided_color_oracle.coefficients (pass 1 of the colour-guide filter, unchanged)
    2. am[i][p] = rdiv(box(a_q[i][p]), n), bm[p] = rdiv(box(b_q[p]), n)                      (2^-12 units)
    3. per axis the taps of guided_up_oracle.axis;  I = the three bytes of the FULL content's pixel
       v_p = sum_k w_k (sum_i am_k[i][p] I_i + bm_k[p]),  out_p = clamp((v_p + 2^27) >> 28, 0, 255)

`guided_upsample` is the vectorised int64 form the tests compare against; `guided_upsample_loop` is a deliberately naive loop in
Python integers that only cross-checks the first; `guided_upsample_f64` is the float64 fast guided filter (He & Sun 2015) with the
colour guide (np.linalg.solve on the small pair's window covariances), the same box and half-pixel bilinear map, the yardstick of
the rule's error; `bound` is the rule's stated distance from it and `bound_parts` the same without its eps-dependent term."""
import numpy as np

import guided_color_oracle as color
from guided_oracle import SHIFT, box, count, rdiv
from guided_up_oracle import ONE, WBITS, axis

MAX_A, MAX_B = color.MAX_A, color.MAX_B      # the header's bounds of |am| and |bm|: those of a_q and b_q
MAX_V = 29100000000000                       # ... and of |v|: 65536 (3 * 288400 * 255 + 2.22e8) < 2.91e13


def means(stylized, content_small, r, eps_q):
    """step 2: am int64 [...][h][w][3][3] (guide channel, frame channel) and bm [...][h][w][3]"""
    a_q, b_q, _, n, _ = color.coefficients(stylized, content_small, r, eps_q)
    am = np.stack([np.stack([rdiv(box(a_q[..., i, p], r), n) for p in range(3)], -1) for i in range(3)], -2)
    bm = np.stack([rdiv(box(b_q[..., p], r), n) for p in range(3)], -1)
    return am, bm


def corners(stylized, content_small, content_full, r, eps_q):
    """per full pixel and channel the four values sum_i am_k[i][p] I_i + bm_k[p] (2^-12 units), int64 [4][...][H][W][3], and their
    weights int64 [4][H][W] (sum 65536)"""
    c, C = np.asarray(content_small), np.asarray(content_full)
    assert C.dtype == np.uint8 and C.shape[-1] == 3
    hc, wc = c.shape[-3], c.shape[-2]
    H, W = C.shape[-3], C.shape[-2]
    assert H >= hc and W >= wc
    am, bm = means(stylized, c, r, eps_q)
    I = C.astype(np.int64)
    y0, y1, fy = axis(H, hc)
    x0, x1, fx = axis(W, wc)
    vals, wts = [], []
    for ys, wy in ((y0, ONE - fy), (y1, fy)):
        for xs, wx in ((x0, ONE - fx), (x1, fx)):
            a, b = am[..., ys[:, None], xs[None, :], :, :], bm[..., ys[:, None], xs[None, :], :]
            vals.append((a * I[..., :, None]).sum(-2) + b)
            wts.append(wy[:, None] * wx[None, :])
    return np.stack(vals), np.stack(wts)


def guided_upsample_sum(stylized, content_small, content_full, r, eps_q):
    """v of step 3, int64 [...][H][W][3]"""
    vals, wts = corners(stylized, content_small, content_full, r, eps_q)
    return sum(vals[k] * wts[k][..., None] for k in range(4))


def guided_upsample_unclamped(stylized, content_small, content_full, r, eps_q):
    """the rule before the clamp, int64 [...][H][W][3]"""
    v = guided_upsample_sum(stylized, content_small, content_full, r, eps_q)
    return (v + (1 << (SHIFT + 2 * WBITS - 1))) >> (SHIFT + 2 * WBITS)


def guided_upsample(stylized, content_small, content_full, r, eps_q):
    """uint8 [...][h][w][3] small frames, [...][hc][wc][3] small contents, [...][H][W][3] full contents -> uint8 [...][H][W][3]"""
    return np.clip(guided_upsample_unclamped(stylized, content_small, content_full, r, eps_q), 0, 255).astype(np.uint8)


def guided_upsample_loop(stylized, content_small, content_full, r, eps_q):
    """one frame, pixel by pixel, in Python integers"""
    s, c, C = np.asarray(stylized), np.asarray(content_small), np.asarray(content_full)
    h, w, _ = s.shape
    hc, wc, _ = c.shape
    H, W, _ = C.shape
    a_q, b_q, _, _, _ = color.coefficients(s, c, r, eps_q)

    def mean(y, x):
        win = [(yy, xx) for yy in range(max(0, y - r), min(h - 1, y + r) + 1) for xx in range(max(0, x - r), min(w - 1, x + r) + 1)]
        n = len(win)
        a = [[(2 * sum(int(a_q[yy, xx, i, p]) for yy, xx in win) + n) // (2 * n) for p in range(3)] for i in range(3)]
        b = [(2 * sum(int(b_q[yy, xx, p]) for yy, xx in win) + n) // (2 * n) for p in range(3)]
        return a, b

    m = {(y, x): mean(y, x) for y in range(hc) for x in range(wc)}

    def tap(P, N, mm):
        t = min(max((2 * P + 1) * mm - N, 0), 2 * N * (mm - 1))
        p0 = t // (2 * N)
        f = (2 * (t - p0 * 2 * N) * 256 + 2 * N) // (4 * N)
        return p0, min(p0 + 1, mm - 1), f

    out = np.zeros_like(C)
    for Y in range(H):
        y0, y1, fy = tap(Y, H, hc)
        for X in range(W):
            x0, x1, fx = tap(X, W, wc)
            I = [int(v) for v in C[Y, X]]
            for p in range(3):
                v = 0
                for yy, wy in ((y0, 256 - fy), (y1, fy)):
                    for xx, wx in ((x0, 256 - fx), (x1, fx)):
                        a, b = m[yy, xx]
                        v += wy * wx * (sum(a[i][p] * I[i] for i in range(3)) + b[p])
                out[Y, X, p] = max(0, min(255, (v + (1 << 27)) >> 28))
    return out


def guided_upsample_f64(stylized, content_small, content_full, r, eps_q):
    """the fast guided filter with the colour guide in float64, before any rounding: He et al.'s a (np.linalg.solve on the window
    covariances of the small pair) and b with the rule's guide, box and eps; their window means; bilinear interpolation on
    half-pixel centres over the content extent hc x wc; sum_i a_i I_i + b on the full content"""
    s, c, C = np.asarray(stylized), np.asarray(content_small), np.asarray(content_full)
    h, w = s.shape[-3], s.shape[-2]
    hc, wc = c.shape[-3], c.shape[-2]
    H, W = C.shape[-3], C.shape[-2]
    I, n = color.guide(c, h, w).astype(np.float64), count(h, w, r).astype(np.float64)
    P = s.astype(np.float64)
    mI = np.stack([box(I[..., i], r) / n for i in range(3)], -1)
    mp = np.stack([box(P[..., p], r) / n for p in range(3)], -1)
    cov = np.stack([np.stack([box(I[..., i] * I[..., j], r) / n for j in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mI[..., None, :] + eps_q * np.eye(3)
    kap = np.stack([np.stack([box(I[..., i] * P[..., p], r) / n for p in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mp[..., None, :]
    a = np.linalg.solve(cov, kap)                                                     # [...][h][w][i][p]
    b = mp - (a * mI[..., :, None]).sum(-2)
    IF = C.astype(np.float64)

    def frac(N, m):
        src = np.clip((np.arange(N) + 0.5) * m / N - 0.5, 0, m - 1)
        p0 = np.minimum(np.floor(src).astype(np.int64), m - 1)
        return p0, np.minimum(p0 + 1, m - 1), src - p0

    y0, y1, fy = frac(H, hc)
    x0, x1, fx = frac(W, wc)

    def interp(m):
        top = m[..., y0[:, None], x0[None, :]] * (1 - fx) + m[..., y0[:, None], x1[None, :]] * fx
        bot = m[..., y1[:, None], x0[None, :]] * (1 - fx) + m[..., y1[:, None], x1[None, :]] * fx
        return top * (1 - fy)[:, None] + bot * fy[:, None]

    return np.stack([sum(interp(box(a[..., i, p], r) / n) * IF[..., i] for i in range(3)) + interp(box(b[..., p], r) / n)
                     for p in range(3)], -1)


def eps_term(eps_q, f=color.F):
    """the eps-dependent term of guided_color_rule.h, eq. (1), against a guide pixel 255 sqrt(3) from the window's mean"""
    h = 2.0 ** -(f + 1)
    return 255 * 3 ** 0.5 * h * (3 ** 0.5 + 191.25 / eps_q ** 0.5) / (eps_q - 3 * h)


def bound_parts(stylized, content_small, content_full, r, eps_q):
    """0.5 + 766 2^-12 + D 2^-8 per pixel and channel, D the spread of the pixel's four corner values in grey levels: the
    rule's distance from guided_upsample_f64 without its eps-dependent term (not a bound by itself)"""
    vals, _ = corners(stylized, content_small, content_full, r, eps_q)
    D = (vals.max(0) - vals.min(0)).astype(np.float64) / (1 << SHIFT)
    return 0.5 + 766.0 / (1 << SHIFT) + D / (1 << WBITS)


def bound(stylized, content_small, content_full, r, eps_q):
    """the rule's stated distance from guided_upsample_f64 per pixel and channel, before the clamp (guided_up_color_rule.h):
    0.5 + 766 2^-12 + 765 2^-35 + D 2^-8 + eps_term(eps_q)"""
    return bound_parts(stylized, content_small, content_full, r, eps_q) + 765 * 2.0 ** -35 + eps_term(eps_q)


def isoluminant_step(H=96, W=160, ratio=8, edge=83, seed=40):
    """the reason for the colour guide under upsampling: a full content of two colours whose greys are 102 | 100 with the step at
    column `edge`, off the small grid; the small content by ratio x ratio box means; the small frame the box-mean 50 | 200 step
    plus +-20 uniform noise on all three channels alike -> (small frame, small content, full content)"""
    C = np.empty((H, W, 3), np.uint8)
    C[:, :edge], C[:, edge:] = (200, 60, 60), (20, 141, 100)
    S = np.full((H, W), 50.0)
    S[:, edge:] = 200
    c = np.round(C.reshape(H // ratio, ratio, W // ratio, ratio, 3).mean((1, 3))).astype(np.uint8)
    step = np.round(S.reshape(H // ratio, ratio, W // ratio, ratio).mean((1, 3))).astype(np.int64)
    noise = np.random.default_rng(seed).integers(-20, 21, step.shape)
    s = np.clip(step + noise, 0, 255)[..., None].repeat(3, -1).astype(np.uint8)
    return s, c, C
