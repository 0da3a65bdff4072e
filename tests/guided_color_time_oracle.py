"""NumPy restatement of temporal guided smoothing with the colour guide (include/wct_hip.h, wct_guided_filter_time_guide with
WCT_GUIDE_COLOR; wct_tf_amd/csrc/guided_color_time_rule.h), independent of the library: the 21 sums and the 3 x 3 solve of
guided_color_oracle over the 3-D, optionally shifted, window of guided_motion_oracle.

    window     in each frame g of max(0, f-T) .. min(F-1, f+T) the (2r+1)^2 box centred at the shifted pixel, cut at the borders,
               possibly empty; n = the pixels of all of them; positions None = all zero = the window of guided_time_oracle
    pass 1     guided_color_oracle._solve on the sums over that window
    pass 2     out_p = clamp(rdiv(sum_i I_i sum a_q[i][p] + sum b_q[p], n 2^12), 0, 255), the sums over the same window

`guided_filter` is the vectorised int64 form the tests compare against; `guided_filter_loop` a naive loop over windows in Python
integers that only cross-checks it on tiny clips; `guided_filter_f64` the float64 colour-guide filter on the same 3-D shifted box
(np.linalg.solve), the yardstick of the rule's error; `guided_filter_chunked` the clip in chunks with halos."""
import numpy as np

import guided_color_oracle as gc
import guided_motion_oracle as gm
import guided_time_oracle as gt
from guided_oracle import SHIFT, rdiv

PAIRS = gc.PAIRS


def _pos(pos, frames):
    p = np.zeros((frames, 2), np.int64) if pos is None else np.asarray(pos)
    assert gm.positions_ok(p, frames), p
    return p.astype(np.int64)


def _check(s, c, r, eps_q, t):
    gt._check(s, c, r, eps_q, t)


def coefficients(stylized, content, r, eps_q, t, pos=None):
    """pass 1: a_q int64 [F][H][W][3][3] (guide channel, frame channel), b_q [F][H][W][3], the guide, n and bitlength(det)"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t)
    f, h, w = s.shape[:3]
    pos = _pos(pos, f)
    I, n = gc.guide(c, h, w), gm.count3(f, h, w, r, t, pos)
    P = s.astype(np.int64)
    b3 = lambda a: gm.box3(np.ascontiguousarray(a), r, t, pos)
    SI = [b3(I[..., i]) for i in range(3)]
    SIJ = {(i, j): b3(I[..., i] * I[..., j]) for i, j in PAIRS}
    Sp = [b3(P[..., p]) for p in range(3)]
    SIp = [[b3(I[..., i] * P[..., p]) for p in range(3)] for i in range(3)]
    a_q, b_q, bits = gc._solve(n, SI, SIJ, Sp, SIp, eps_q)
    return np.stack([np.stack(row, -1) for row in a_q], -2), np.stack(b_q, -1), I, n, bits


def guided_filter_unclamped(stylized, content, r, eps_q, t, pos=None):
    """the rule before the clamp to 0 .. 255, int64 [F][H][W][3]"""
    a_q, b_q, I, n, _ = coefficients(stylized, content, r, eps_q, t, pos)
    pos = _pos(pos, len(I))
    b3 = lambda a: gm.box3(np.ascontiguousarray(a), r, t, pos)
    return np.stack([rdiv(sum(b3(a_q[..., i, p]) * I[..., i] for i in range(3)) + b3(b_q[..., p]), n << SHIFT) for p in range(3)], -1)


def guided_filter(stylized, content, r, eps_q, t, pos=None):
    """uint8 [F][H][W][3] stylized clip, uint8 [F][Hc][Wc][3] contents, int positions [F][2] or None -> uint8 [F][H][W][3]"""
    return np.clip(guided_filter_unclamped(stylized, content, r, eps_q, t, pos), 0, 255).astype(np.uint8)


def guided_filter_loop(stylized, content, r, eps_q, t, pos=None):
    """window by window, in Python integers"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q, t)
    nf, h, w, _ = s.shape
    hc, wc = c.shape[1:3]
    pos = [(int(a), int(b)) for a, b in _pos(pos, nf)]
    I = [[[[int(v) for v in c[f, min(y, hc - 1), min(x, wc - 1)]] for x in range(w)] for y in range(h)] for f in range(nf)]
    P = [[[[int(v) for v in s[f, y, x]] for x in range(w)] for y in range(h)] for f in range(nf)]

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
                SI = [sum(I[g][yy][xx][i] for g, yy, xx in win) for i in range(3)]
                SIJ = {(i, j): sum(I[g][yy][xx][i] * I[g][yy][xx][j] for g, yy, xx in win) for i, j in PAIRS}
                Sp = [sum(P[g][yy][xx][p] for g, yy, xx in win) for p in range(3)]
                SIp = [[sum(I[g][yy][xx][i] * P[g][yy][xx][p] for g, yy, xx in win) for p in range(3)] for i in range(3)]
                ab[f, y, x] = gc._solve(len(win), SI, SIJ, Sp, SIp, eps_q)[:2]
    out = np.zeros_like(s)
    for f in range(nf):
        for y in range(h):
            for x in range(w):
                win = window(f, y, x)
                for p in range(3):
                    v = sum(ab[q][1][p] for q in win)
                    for i in range(3):
                        v += sum(ab[q][0][i][p] for q in win) * I[f][y][x][i]
                    out[f, y, x, p] = max(0, min(255, rdiv(v, len(win) << SHIFT)))
    return out


def guided_filter_f64(stylized, content, r, eps_q, t, pos=None):
    """He et al.'s colour-guide filter (eqs. 19-21) in float64 on the same 3-D shifted box, before any rounding"""
    s, c = np.asarray(stylized), np.asarray(content)
    f, h, w = s.shape[:3]
    pos = _pos(pos, f)
    I, n = gc.guide(c, h, w).astype(np.float64), gm.count3(f, h, w, r, t, pos).astype(np.float64)
    P = s.astype(np.float64)
    b3 = lambda a: gm.box3(np.ascontiguousarray(a), r, t, pos)
    mI = np.stack([b3(I[..., i]) / n for i in range(3)], -1)
    mp = np.stack([b3(P[..., p]) / n for p in range(3)], -1)
    cov = np.stack([np.stack([b3(I[..., i] * I[..., j]) / n for j in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mI[..., None, :] + eps_q * np.eye(3)
    kap = np.stack([np.stack([b3(I[..., i] * P[..., p]) / n for p in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mp[..., None, :]
    a = np.linalg.solve(cov, kap)
    b = mp - (a * mI[..., :, None]).sum(-2)
    return np.stack([sum(b3(a[..., i, p]) / n * I[..., i] for i in range(3)) + b3(b[..., p]) / n for p in range(3)], -1)


def guided_filter_chunked(stylized, content, r, eps_q, t, pos, chunk, halo):
    """the clip filtered in chunks of `chunk` output frames, each as a clip of its own with `halo` frames on each side and its
    slice of the positions: the whole clip's bytes when halo >= 2 t"""
    s, c = np.asarray(stylized), np.asarray(content)
    out = np.empty_like(s)
    for f0 in range(0, len(s), chunk):
        f1 = min(len(s), f0 + chunk)
        g0, g1 = max(0, f0 - halo), min(len(s), f1 + halo)
        out[f0:f1] = guided_filter(s[g0:g1], c[g0:g1], r, eps_q, t, None if pos is None else np.asarray(pos)[g0:g1])[f0 - g0:f1 - g0]
    return out


# ---- the case the feature was built for -----------------------------------------------------------------------------------------
def isoluminant_clip(seed, frames=12, h=48, w=64, sigma=20):
    """a static content of two colours of (nearly) equal luminance, (200, 60, 60) | (20, 141, 100) -- grey guides 102 | 100 -- under
    a 50 | 200 step with N(0, sigma) noise of its own in every frame -> (stylized [F][h][w][3], contents, the clean step [h][w])"""
    rng = np.random.default_rng(seed)
    left = np.arange(w) < w // 2
    c = np.where(left[None, :, None], np.array([200, 60, 60]), np.array([20, 141, 100])) * np.ones((frames, h, 1, 1), np.int64)
    step = np.where(left, 50.0, 200.0)[None, :].repeat(h, 0)
    s = np.clip(np.rint(step[None] + rng.normal(0, sigma, (frames, h, w))), 0, 255)[..., None].repeat(3, -1)
    return s.astype(np.uint8), c.astype(np.uint8), step


def flicker_flat(out, w):
    """mean |out_f - out_{f+1}| on the flat left side (rows 10 .. -10, columns 8 .. w/2 - 8), frames 3 .. F - 4"""
    v = out[..., 0].astype(np.float64)
    return float(np.mean([np.abs(v[f, 10:-10, 8:w // 2 - 8] - v[f + 1, 10:-10, 8:w // 2 - 8]).mean() for f in range(3, len(v) - 4)]))


def edge_jump(out, w):
    """(mean, smallest) jump out[.., w/2] - out[.., w/2 - 1] across the edge over rows 10 .. -10 and frames 3 .. F - 4"""
    v = out[..., 0].astype(np.float64)
    j = v[3:len(v) - 3, 10:-10, w // 2] - v[3:len(v) - 3, 10:-10, w // 2 - 1]
    return float(j.mean()), float(j.min())


def error_against(out, clean):
    """mean |out - clean| over rows 10 .. -10 and frames 3 .. F - 4"""
    v = out[..., 0].astype(np.float64)
    return float(np.abs(v[3:len(v) - 3, 10:-10] - clean[None, 10:-10]).mean())
