"""NumPy restatement of the guided-upsampling rule (include/wct_hip.h, wct_guided_upsample; wct_tf_amd/csrc/guided_up_rule.h),
independent of the library and built on guided_oracle's pieces:

    1. a_q, b_q on h x w      guided_oracle.coefficients (pass 1 of the guided filter, unchanged)
    2. am = rdiv(box(a_q), n), bm = rdiv(box(b_q), n)                                     (2^-12 units)
    3. per axis  t = clamp((2P + 1) m - N, 0, 2N (m - 1)), p0 = t div 2N, f = rdiv((t - p0 2N) 256, 2N), p1 = min(p0 + 1, m - 1)
       v = sum_k w_k (am_k I + bm_k),  out = clamp((v + 2^27) >> 28, 0, 255),  I the guide of the FULL content's pixel

`guided_upsample` is the vectorised int64 form the tests compare against; `guided_upsample_loop` is a deliberately naive loop in
Python integers that only cross-checks the first; `guided_upsample_f64` is the float64 fast guided filter (He & Sun 2015) with the
same guide, box and half-pixel bilinear map, the yardstick of the rule's error, and `bound` the rule's stated distance from it."""
import numpy as np

from guided_oracle import SHIFT, box, coefficients, count, guide, rdiv

WBITS = 8
ONE = 1 << WBITS

# the cases both test files share, (h, w, hc, wc, H, W, r, eps_q): equal sizes, odd ratios, a frame larger than its content, the two
# axes at different ratios, both ends of r and eps_q
CASES = [(9, 13, 9, 13, 9, 13, 2, 650), (9, 13, 9, 13, 40, 61, 2, 650), (33, 35, 33, 35, 264, 280, 4, 1),
         (16, 20, 9, 13, 50, 70, 3, 650), (48, 48, 48, 48, 200, 100, 8, 65025), (33, 35, 33, 35, 67, 71, 1, 1),
         (30, 31, 30, 31, 240, 250, 16, 7)]


def axis(N, m):
    """the taps of every full coordinate 0 .. N - 1 on a small axis of m: int64 arrays (p0, p1, f)"""
    P = np.arange(N, dtype=np.int64)
    t = np.clip((2 * P + 1) * m - N, 0, 2 * N * (m - 1))
    p0 = t // (2 * N)
    f = rdiv((t - p0 * 2 * N) * ONE, 2 * N)
    return p0, np.minimum(p0 + 1, m - 1), f


def means(stylized, content_small, r, eps_q):
    """step 2: (am, bm) int64 [...][h][w][3]"""
    a_q, b_q, _, n = coefficients(stylized, content_small, r, eps_q)
    am = np.stack([rdiv(box(a_q[..., ch], r), n) for ch in range(3)], -1)
    bm = np.stack([rdiv(box(b_q[..., ch], r), n) for ch in range(3)], -1)
    return am, bm


def corners(stylized, content_small, content_full, r, eps_q):
    """per full pixel and channel the four values am_k I + bm_k (2^-12 units), int64 [4][...][H][W][3], and their weights
    int64 [4][H][W] (sum 65536)"""
    c, C = np.asarray(content_small), np.asarray(content_full)
    assert C.dtype == np.uint8 and C.shape[-1] == 3
    hc, wc = c.shape[-3], c.shape[-2]
    H, W = C.shape[-3], C.shape[-2]
    assert H >= hc and W >= wc
    am, bm = means(stylized, c, r, eps_q)
    I = guide(C, H, W)[..., None]
    y0, y1, fy = axis(H, hc)
    x0, x1, fx = axis(W, wc)
    vals, wts = [], []
    for ys, wy in ((y0, ONE - fy), (y1, fy)):
        for xs, wx in ((x0, ONE - fx), (x1, fx)):
            vals.append(am[..., ys[:, None], xs[None, :], :] * I + bm[..., ys[:, None], xs[None, :], :])
            wts.append(wy[:, None] * wx[None, :])
    return np.stack(vals), np.stack(wts)


def guided_upsample_unclamped(stylized, content_small, content_full, r, eps_q):
    """the rule before the clamp, int64 [...][H][W][3]"""
    vals, wts = corners(stylized, content_small, content_full, r, eps_q)
    v = sum(vals[k] * wts[k][..., None] for k in range(4))
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
    a_q, b_q, _, _ = coefficients(s, c, r, eps_q)

    def mean(y, x, ch):
        ys, xs = range(max(0, y - r), min(h - 1, y + r) + 1), range(max(0, x - r), min(w - 1, x + r) + 1)
        n = len(ys) * len(xs)
        sa, sb = sum(int(a_q[yy, xx, ch]) for yy in ys for xx in xs), sum(int(b_q[yy, xx, ch]) for yy in ys for xx in xs)
        return (2 * sa + n) // (2 * n), (2 * sb + n) // (2 * n)

    m = {(y, x, ch): mean(y, x, ch) for y in range(hc) for x in range(wc) for ch in range(3)}

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
            I = (sum(k * int(v) for k, v in zip((77, 150, 29), C[Y, X])) + 128) >> 8
            for ch in range(3):
                v = 0
                for yy, wy in ((y0, 256 - fy), (y1, fy)):
                    for xx, wx in ((x0, 256 - fx), (x1, fx)):
                        a, b = m[yy, xx, ch]
                        v += wy * wx * (a * I + b)
                out[Y, X, ch] = max(0, min(255, (v + (1 << 27)) >> 28))
    return out


def guided_upsample_f64(stylized, content_small, content_full, r, eps_q):
    """the fast guided filter in float64, before any rounding: He et al.'s a, b on the small pair with the rule's guide, box and
    eps; their window means; bilinear interpolation on half-pixel centres over the content extent hc x wc; a I + b on the full guide"""
    s, c, C = np.asarray(stylized), np.asarray(content_small), np.asarray(content_full)
    h, w = s.shape[-3], s.shape[-2]
    hc, wc = c.shape[-3], c.shape[-2]
    H, W = C.shape[-3], C.shape[-2]
    I, n = guide(c, h, w).astype(np.float64), count(h, w, r).astype(np.float64)
    mI = box(I, r) / n
    var = box(I * I, r) / n - mI * mI
    IF = guide(C, H, W).astype(np.float64)

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

    out = []
    for ch in range(3):
        p = s[..., ch].astype(np.float64)
        mp = box(p, r) / n
        a = (box(I * p, r) / n - mI * mp) / (var + eps_q)
        b = mp - a * mI
        out.append(interp(box(a, r) / n) * IF + interp(box(b, r) / n))
    return np.stack(out, -1)


def bound(stylized, content_small, content_full, r, eps_q):
    """the rule's stated distance from guided_upsample_f64 per pixel and channel, before the clamp (guided_up_rule.h):
    0.5 + 256 2^-12 + D 2^-8, D the spread of the pixel's four am_k I + bm_k in grey levels"""
    vals, _ = corners(stylized, content_small, content_full, r, eps_q)
    D = (vals.max(0) - vals.min(0)).astype(np.float64) / (1 << SHIFT)
    return 0.5 + 256.0 / (1 << SHIFT) + D / (1 << WBITS)


def bilinear_f64(img, H, W):
    """a float64 half-pixel bilinear upscale of [h][w][3] to [H][W][3]: what an ordinary up-scaler does to a filtered small frame"""
    a = np.asarray(img, np.float64)
    h, w = a.shape[0], a.shape[1]
    ys = np.clip((np.arange(H) + 0.5) * h / H - 0.5, 0, h - 1)
    xs = np.clip((np.arange(W) + 0.5) * w / W - 0.5, 0, w - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = a[y0][:, x0] * (1 - fx) + a[y0][:, x1] * fx
    bot = a[y1][:, x0] * (1 - fx) + a[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def case(seed, h, w, hc, wc, H, W):
    """a seeded test case: a smooth full content with edges and noise, its small version by box sampling, a noisy small frame"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 90 + 60 * np.sin(yy / 9.0)[..., None] + 50 * np.cos(xx / 7.0)[..., None] + np.array([0, 20, -20])
    base = base + 70 * ((xx > W * 0.45) & (yy > H * 0.3))[..., None]
    C = np.clip(base + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
    ys = np.minimum((np.arange(hc) * H) // hc, H - 1)
    xs = np.minimum((np.arange(wc) * W) // wc, W - 1)
    c = np.ascontiguousarray(C[ys][:, xs])
    s = rng.integers(0, 256, (h, w, 3)).astype(np.int64)
    s[:hc, :wc] = (s[:hc, :wc] + 2 * c[..., ::-1].astype(np.int64)) // 3
    return s.astype(np.uint8), c, C
