"""NumPy restatement of the colour-guide rule of guided smoothing (include/wct_hip.h, wct_guided_filter_guide with
WCT_GUIDE_COLOR; wct_tf_amd/csrc/guided_color_rule.h), independent of the library.  rdiv, box, count and the clamp are those of
guided_oracle.py:

    I          = the three bytes of c[min(y, Hc-1)][min(x, Wc-1)]
    pass 1     V_ij = rdiv(2^F (n S_ij - S_i S_j), n^2), M = V + 2^F eps_q U, c_ip = rdiv(2^F (n S_ip - S_i S_p), n^2), F = 4
               adj = adjugate(M), det = sum_j M_0j adj_0j, u_ip = sum_j adj_ij c_jp, k = max(0, bitlength(det) - 43)
               a_q[i][p] = rdiv((u_ip >> k) 2^12, det >> k),  b_q[p] = rdiv(S_p 2^12 - sum_i a_q[i][p] S_i, n)
    pass 2     out_p = clamp(rdiv(sum_i I_i sum a_q[i][p] + sum b_q[p], n 2^12), 0, 255)

`guided_filter` is the vectorised int64 form the tests compare against; `guided_filter_loop` is a naive loop over windows in
Python integers (no width at all) that only cross-checks the first; `guided_filter_f64` is the float64 colour-guide filter of He
et al. (np.linalg.solve on the window covariances, the same box), the yardstick of the rule's error; `distance` is the bound the
rule header derives for it."""
import numpy as np

from colors_oracle import clamped_content
from guided_oracle import SHIFT, MAX_RADIUS, MAX_EPS, rdiv, box, count

F = 4
DET_BITS = 43
MAX_A, MAX_B = 288400, 222000000       # the header's bounds of |a_q| and |b_q|
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def distance(eps_q, f=F):
    """the header's derived distance from the float64 filter, before the clamp"""
    h = 2.0 ** -(f + 1)
    return 0.5 + 2.0 ** -13 + 765 * (2.0 ** -13 + 2.0 ** -35) + 255 * 3 ** 0.5 * h * (3 ** 0.5 + 191.25 / eps_q ** 0.5) / (eps_q - 3 * h)


def guide(content, ho, wo):
    """the guide of every output pixel, int64 [...][ho][wo][3]"""
    return clamped_content(content, ho, wo).astype(np.int64)


def _check(s, c, r, eps_q):
    assert s.dtype == np.uint8 and c.dtype == np.uint8 and s.shape[-1] == 3 and c.shape[-1] == 3
    assert 1 <= r <= MAX_RADIUS and 1 <= eps_q <= MAX_EPS


def bitlength(v):
    """bits of positive int64 values"""
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for b in (32, 16, 8, 4, 2, 1):
        big = (v >> b) > 0
        out += big * b
        v = np.where(big, v >> b, v)
    return out + (v > 0)


def _solve(n, SI, SIJ, Sp, SIp, eps_q):
    """pass 1 of any number of pixels from their window sums (int64 arrays, or Python integers): SI [3], SIJ {pair: sum},
    Sp [3], SIp [3][3] -> a_q [3][3] (guide channel, frame channel), b_q [3], bitlength(det)"""
    n2, one = n * n, 1 << F
    V = {ij: rdiv(one * (n * SIJ[ij] - SI[ij[0]] * SI[ij[1]]), n2) for ij in PAIRS}
    M00, M11, M22 = (V[i, i] + one * eps_q for i in range(3))
    V01, V02, V12 = V[0, 1], V[0, 2], V[1, 2]
    a00, a01, a02 = M11 * M22 - V12 * V12, V02 * V12 - V01 * M22, V01 * V12 - V02 * M11
    a11, a12, a22 = M00 * M22 - V02 * V02, V01 * V02 - V12 * M00, M00 * M11 - V01 * V01
    adj = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    det = M00 * a00 + V01 * a01 + V02 * a02
    bits = bitlength(det) if isinstance(det, np.ndarray) else int(det).bit_length()
    k = np.maximum(bits - DET_BITS, 0) if isinstance(det, np.ndarray) else max(bits - DET_BITS, 0)
    dk = det >> k
    a_q, b_q = [[None] * 3 for _ in range(3)], []
    for p in range(3):
        c = [rdiv(one * (n * SIp[i][p] - SI[i] * Sp[p]), n2) for i in range(3)]
        acc = Sp[p] << SHIFT
        for i in range(3):
            u = adj[i][0] * c[0] + adj[i][1] * c[1] + adj[i][2] * c[2]
            a_q[i][p] = rdiv((u >> k) << SHIFT, dk)
            acc = acc - a_q[i][p] * SI[i]
        b_q.append(rdiv(acc, n))
    return a_q, b_q, bits


def coefficients(stylized, content, r, eps_q):
    """pass 1: a_q int64 [...][H][W][3][3] (guide channel, frame channel), b_q [...][H][W][3], the guide, n and bitlength(det)"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q)
    h, w = s.shape[-3], s.shape[-2]
    I, n = guide(c, h, w), count(h, w, r)
    P = s.astype(np.int64)
    SI = [box(I[..., i], r) for i in range(3)]
    SIJ = {(i, j): box(I[..., i] * I[..., j], r) for i, j in PAIRS}
    Sp = [box(P[..., p], r) for p in range(3)]
    SIp = [[box(I[..., i] * P[..., p], r) for p in range(3)] for i in range(3)]
    a_q, b_q, bits = _solve(n, SI, SIJ, Sp, SIp, eps_q)
    return np.stack([np.stack(row, -1) for row in a_q], -2), np.stack(b_q, -1), I, n, bits


def guided_filter_unclamped(stylized, content, r, eps_q):
    """the rule before the clamp to 0 .. 255, int64 [...][H][W][3]"""
    a_q, b_q, I, n, _ = coefficients(stylized, content, r, eps_q)
    return np.stack([rdiv(sum(box(a_q[..., i, p], r) * I[..., i] for i in range(3)) + box(b_q[..., p], r), n << SHIFT)
                     for p in range(3)], -1)


def guided_filter(stylized, content, r, eps_q):
    """uint8 [...][H][W][3] stylized, uint8 [...][Hc][Wc][3] content (leading batch dimensions equal) -> uint8"""
    return np.clip(guided_filter_unclamped(stylized, content, r, eps_q), 0, 255).astype(np.uint8)


def guided_filter_loop(stylized, content, r, eps_q):
    """one frame, window by window, in Python integers"""
    s, c = np.asarray(stylized), np.asarray(content)
    _check(s, c, r, eps_q)
    h, w, _ = s.shape
    hc, wc, _ = c.shape
    I = [[[int(v) for v in c[min(y, hc - 1), min(x, wc - 1)]] for x in range(w)] for y in range(h)]
    P = [[[int(v) for v in s[y, x]] for x in range(w)] for y in range(h)]

    def window(y, x):
        return [(yy, xx) for yy in range(max(0, y - r), min(h - 1, y + r) + 1) for xx in range(max(0, x - r), min(w - 1, x + r) + 1)]

    ab = {}
    for y in range(h):
        for x in range(w):
            win = window(y, x)
            SI = [sum(I[yy][xx][i] for yy, xx in win) for i in range(3)]
            SIJ = {(i, j): sum(I[yy][xx][i] * I[yy][xx][j] for yy, xx in win) for i, j in PAIRS}
            Sp = [sum(P[yy][xx][p] for yy, xx in win) for p in range(3)]
            SIp = [[sum(I[yy][xx][i] * P[yy][xx][p] for yy, xx in win) for p in range(3)] for i in range(3)]
            ab[y, x] = _solve(len(win), SI, SIJ, Sp, SIp, eps_q)[:2]
    out = np.zeros_like(s)
    for y in range(h):
        for x in range(w):
            win = window(y, x)
            for p in range(3):
                v = sum(ab[yy, xx][1][p] for yy, xx in win)
                for i in range(3):
                    v += sum(ab[yy, xx][0][i][p] for yy, xx in win) * I[y][x][i]
                out[y, x, p] = max(0, min(255, rdiv(v, len(win) << SHIFT)))
    return out


def guided_filter_f64(stylized, content, r, eps_q):
    """He et al.'s colour-guide filter (eqs. 19-21) in float64 with the rule's guide, box and eps (grey levels squared), before any
    rounding: np.linalg.solve on the window covariances"""
    s, c = np.asarray(stylized), np.asarray(content)
    h, w = s.shape[-3], s.shape[-2]
    I, n = guide(c, h, w).astype(np.float64), count(h, w, r).astype(np.float64)
    P = s.astype(np.float64)
    mI = np.stack([box(I[..., i], r) / n for i in range(3)], -1)                                    # [...][H][W][3]
    mp = np.stack([box(P[..., p], r) / n for p in range(3)], -1)
    cov = np.stack([np.stack([box(I[..., i] * I[..., j], r) / n for j in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mI[..., None, :] + eps_q * np.eye(3)
    kap = np.stack([np.stack([box(I[..., i] * P[..., p], r) / n for p in range(3)], -1) for i in range(3)], -2) \
        - mI[..., :, None] * mp[..., None, :]                                                       # [...][H][W][i][p]
    a = np.linalg.solve(cov, kap)
    b = mp - (a * mI[..., :, None]).sum(-2)
    return np.stack([sum(box(a[..., i, p], r) / n * I[..., i] for i in range(3)) + box(b[..., p], r) / n for p in range(3)], -1)


def isoluminant_step(h=24, w=40, seed=0):
    """the reason for the colour guide: a content of two colours whose grey guides are 102 | 100, under a 50 | 200 step with
    +-20 uniform noise -> (stylized, content, the clean step [h][w])"""
    rng = np.random.default_rng(seed)
    left = np.arange(w) < w // 2
    c = np.where(left[None, :, None], np.array([200, 60, 60]), np.array([20, 141, 100])) * np.ones((h, 1, 1), np.int64)
    step = np.where(left, 50, 200)[None, :].repeat(h, 0)
    s = (step + rng.integers(-20, 21, (h, w)))[..., None].repeat(3, -1)
    return s.astype(np.uint8), c.astype(np.uint8), step
