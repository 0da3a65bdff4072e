"""NumPy restatement of temporal guided smoothing along camera motion (include/wct_hip.h, wct_guided_filter_motion and
wct_motion_global; wct_tf_amd/csrc/guided_motion_rule.h), independent of the library: the rule of guided_time_oracle with the
window of every neighbouring frame shifted by one global integer translation per frame, and the estimator of those translations.

    positions  pos [F][2] (py, px); the scene point at (y, x) of frame f is at (y + pos[g][0] - pos[f][0], x + pos[g][1] -
               pos[f][1]) of frame g; only differences count; every step between consecutive frames within 16 on both axes
    window     in each frame g of max(0, f-T) .. min(F-1, f+T) the (2r+1)^2 box centred at the shifted pixel, cut at the borders,
               possibly empty; n = the pixels of all of them
    pass 1, 2  guided_time_oracle's, with these windows and this n
    estimator  per pair of consecutive contents the step (dy, dx), |dy|, |dx| <= R, of the smallest SAD / cnt of the grey guides
               over the even (y, x) of frame f whose (y + dy, x + dx) lies in frame f + 1, compared as SAD cnt' < SAD' cnt; ties go
               to the smaller (dy^2 + dx^2, dy, dx); positions are the running sum from (0, 0)

`guided_filter_motion` is the vectorised int64 form (a 2-D prefix sum read at clipped, possibly empty ranges),
`guided_filter_motion_loop` a deliberately naive loop over windows in Python integers that only cross-checks it on tiny clips."""
import numpy as np

import guided_oracle as g2
import guided_time_oracle as gt

MAX_STEP = 16
MAX_SEARCH = 16


def positions_ok(pos, frames):
    p = np.asarray(pos)
    return p.shape == (frames, 2) and np.issubdtype(p.dtype, np.integer) and \
        (frames < 2 or np.abs(np.diff(p.astype(np.int64), axis=0)).max() <= MAX_STEP)


def positions_of(steps):
    """positions [len(steps) + 1][2] from (0, 0) by the steps between consecutive frames"""
    return np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(np.asarray(steps, np.int64).reshape(-1, 2), 0)]).astype(np.int32)


def box_shift(a, r, dy, dx):
    """[H][W] -> the sums of `a` over the (2r+1)^2 box centred at (y + dy, x + dx), cut at the borders: 0 where it lies outside"""
    h, w = a.shape
    p = np.zeros((h + 1, w + 1), a.dtype)
    p[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(h) + dy - r, 0, h), np.clip(np.arange(h) + dy + r + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) + dx - r, 0, w), np.clip(np.arange(w) + dx + r + 1, 0, w)
    y1, x1 = np.maximum(y1, y0), np.maximum(x1, x0)                   # an empty range sums to nothing
    return p[y1[:, None], x1[None, :]] - p[y0[:, None], x1[None, :]] - p[y1[:, None], x0[None, :]] + p[y0[:, None], x0[None, :]]


def box3(a, r, t, pos):
    """window sums of int64 / float64 [F][H][W] over the shifted boxes of the frames of the time window"""
    f = a.shape[0]
    pos = np.asarray(pos, np.int64)
    out = np.zeros_like(a)
    for i in range(f):
        for g in range(max(0, i - t), min(f - 1, i + t) + 1):
            out[i] += box_shift(a[g], r, int(pos[g, 0] - pos[i, 0]), int(pos[g, 1] - pos[i, 1]))
    return out


def count3(f, h, w, r, t, pos):
    return box3(np.ones((f, h, w), np.int64), r, t, pos)


def _check(s, c, r, eps_q, t, pos):
    gt._check(s, c, r, eps_q, t)
    assert positions_ok(pos, s.shape[0]), pos


def coefficients(stylized, content, r, eps_q, t, pos):
    """pass 1: (a_q, b_q) int64 [F][H][W][3], and the guide and n it used"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t, pos)
    f, h, w = s.shape[:3]
    I, n = g2.guide(c, h, w), count3(f, h, w, r, t, pos)
    SI, SII = box3(I, r, t, pos), box3(I * I, r, t, pos)
    a_q, b_q = [], []
    for ch in range(3):
        p = s[..., ch].astype(np.int64)
        Sp, SIp = box3(p, r, t, pos), box3(I * p, r, t, pos)
        a = g2.rdiv((n * SIp - SI * Sp) << g2.SHIFT, n * SII - SI * SI + eps_q * n * n)
        a_q.append(a)
        b_q.append(g2.rdiv((Sp << g2.SHIFT) - a * SI, n))
    return np.stack(a_q, -1), np.stack(b_q, -1), I, n


def guided_filter_motion(stylized, content, r, eps_q, t, pos):
    """uint8 [F][H][W][3] stylized clip, uint8 [F][Hc][Wc][3] contents, int positions [F][2] -> uint8 [F][H][W][3]"""
    a_q, b_q, I, n = coefficients(stylized, content, r, eps_q, t, pos)
    raw = np.stack([g2.rdiv(box3(a_q[..., ch], r, t, pos) * I + box3(b_q[..., ch], r, t, pos), n << g2.SHIFT) for ch in range(3)], -1)
    return np.clip(raw, 0, 255).astype(np.uint8)


def guided_filter_motion_loop(stylized, content, r, eps_q, t, pos):
    """window by window, in Python integers"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t, pos)
    nf, h, w, _ = s.shape
    hc, wc = c.shape[1:3]
    pos = [(int(a), int(b)) for a, b in pos]
    I = [[[(sum(k * int(v) for k, v in zip((77, 150, 29), c[f, min(y, hc - 1), min(x, wc - 1)])) + 128) >> 8 for x in range(w)]
          for y in range(h)] for f in range(nf)]

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
    out = np.zeros_like(s)
    for f in range(nf):
        for y in range(h):
            for x in range(w):
                win = window(f, y, x)
                for ch in range(3):
                    SA, SB = sum(ab[p + (ch,)][0] for p in win), sum(ab[p + (ch,)][1] for p in win)
                    out[f, y, x, ch] = max(0, min(255, g2.rdiv(SA * I[f][y][x] + SB, len(win) << g2.SHIFT)))
    return out


def guided_filter_motion_chunked(stylized, content, r, eps_q, t, pos, chunk, halo):
    """the clip filtered in chunks of `chunk` output frames, each as a clip of its own with `halo` frames on each side and its
    slice of the positions: the whole clip's bytes when halo >= 2 t"""
    s, c, pos = np.asarray(stylized), np.asarray(content), np.asarray(pos)
    out = np.empty_like(s)
    for f0 in range(0, len(s), chunk):
        f1 = min(len(s), f0 + chunk)
        g0, g1 = max(0, f0 - halo), min(len(s), f1 + halo)
        out[f0:f1] = guided_filter_motion(s[g0:g1], c[g0:g1], r, eps_q, t, pos[g0:g1])[f0 - g0:f1 - g0]
    return out


# ---- the estimator --------------------------------------------------------------------------------------------------------------
def search_ok(search, hc, wc):
    return 1 <= search <= MAX_SEARCH and hc >= 4 * search and wc >= 4 * search and hc * wc <= 1 << 28


def sad_count(i0, i1, dy, dx):
    """(SAD, cnt) of candidate (dy, dx) on int64 guide planes [Hc][Wc]"""
    h, w = i0.shape
    ys = np.arange(0, h, 2)
    ys = ys[(ys + dy >= 0) & (ys + dy < h)]
    xs = np.arange(0, w, 2)
    xs = xs[(xs + dx >= 0) & (xs + dx < w)]
    a, b = i0[ys[:, None], xs[None, :]], i1[(ys + dy)[:, None], (xs + dx)[None, :]]
    return int(np.abs(a - b).sum()), len(ys) * len(xs)


def estimate_step(i0, i1, search):
    best = None
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            sad, cnt = sad_count(i0, i1, dy, dx)
            key = (dy * dy + dx * dx, dy, dx)
            if best is None or sad * best[1] < best[0] * cnt or (sad * best[1] == best[0] * cnt and key < best[2]):
                best = (sad, cnt, key)                    # Python integers: no overflow to think about
    return best[2][1], best[2][2]


def estimate_positions(contents, search=8):
    """uint8 [F][Hc][Wc][3] -> int32 positions [F][2] from (0, 0)"""
    c = np.asarray(contents)
    assert c.dtype == np.uint8 and c.ndim == 4 and c.shape[3] == 3 and search_ok(search, c.shape[1], c.shape[2]), (c.shape, search)
    I = g2.guide(c, c.shape[1], c.shape[2])
    return positions_of([estimate_step(I[f], I[f + 1], search) for f in range(len(c) - 1)])


# ---- the case the feature was built for -----------------------------------------------------------------------------------------
def pan_case(step, seed=0, frames=12, h=48, w=64):
    """a camera that pans over a checkerboard (cells of 23 x 17 px, 60 | 190) by step = (sy, sx) px per frame: frame f is the
    h x w crop of the canvas at origin (12 + sy f, 4 + sx f); contents = crop + N(0, 2), stylized = crop + N(0, 20), rounded and
    clipped, grey replicated to RGB -> (stylized, contents, clean float64 [F][h][w], the true positions [F][2]: steps of (-sy, -sx))"""
    sy, sx = step
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h + 40, :w + 80]
    canvas = np.where((xx // 23 + yy // 17) % 2 == 0, 60.0, 190.0)
    clean = np.stack([canvas[12 + sy * f:12 + sy * f + h, 4 + sx * f:4 + sx * f + w] for f in range(frames)])
    assert clean.shape == (frames, h, w)
    rgb = lambda a: np.repeat(np.clip(np.rint(a), 0, 255)[..., None], 3, -1).astype(np.uint8)
    contents = rgb(clean + rng.normal(0, 2, clean.shape))
    stylized = rgb(clean + rng.normal(0, 20, clean.shape))
    return stylized, contents, clean, positions_of([(-sy, -sx)] * (frames - 1))


def flicker_along(out, step_pos, h, w):
    """mean |out_f(p) - out_{f+1}(p + d)| along the motion d = step_pos (the step of the positions), over rows 10 .. h - 10,
    columns 20 .. w - 20 and frames 2 .. F - 4"""
    v = out[..., 0].astype(np.float64)
    dy, dx = step_pos
    return float(np.mean([np.abs(v[f, 10:h - 10, 20:w - 20] - v[f + 1, 10 + dy:h - 10 + dy, 20 + dx:w - 20 + dx]).mean()
                          for f in range(2, len(v) - 3)]))


def error_against(out, clean, h, w):
    """mean |out - clean| over the same rows, columns and frames"""
    v = out[..., 0].astype(np.float64)
    return float(np.abs(v[2:len(v) - 3, 10:h - 10, 20:w - 20] - clean[2:len(v) - 3, 10:h - 10, 20:w - 20]).mean())
