"""Op-level mirror of the reference's ops.py / coral.py / utils.py surface, running
on libwct_hip.so.  Same names, argument meaning and array conventions:

  wct_np(content, style, alpha=0.6, eps=1e-5)   ops.py:92   1xHxWxC in, float32 1xHxWxC out
  wct_tf(content, style, alpha, eps=1e-8)       ops.py:24
  adain(content_features, style_features, alpha, epsilon=1e-5)   ops.py:282
  coral_numpy(source, target)                   coral.py:13 (float64)
  preserve_colors_np(style_rgb, content_rgb)    utils.py:87
and, without a counterpart in the reference,
  content_colors_np(stylized_rgb, content_rgb)  luminance-only colour preservation (Gatys et al. 2016), applied to a result
  guided_filter_np(stylized_rgb, content_rgb, radius, eps_q, guide)   guided smoothing of a result with its content as guide (He et al.)
  guided_upsample_np(stylized, content_small, content_full, radius, eps_q, guide)   a small result delivered at the full content's size (He & Sun)
  guided_upsample_time_np(stylized, contents_small, contents_full, radius, eps_q, frames_t, positions)   a small clip delivered at full size, the box across frames (NumPy, on the host)
  motion_global_np(contents, search)   one global integer translation per frame of a clip, for guided_filter_time_np(positions=)
  texture_noise_np(h, w, seed, sample=0, smooth=False)   the seeded noise image a texture starts from (webcam.py:191-192 --noise)
"""
import numpy as np

from . import _lib
from .context import default_context


def _flat(feat):
    f = np.squeeze(np.asarray(feat))            # batch must be 1 (ops.py:32-33,98-99)
    if f.ndim != 3:
        raise ValueError('WCT needs a single 1xHxWxC feature map, got shape %s' % (np.shape(feat),))
    h, w, c = f.shape
    return np.ascontiguousarray(f.reshape(h * w, c), np.float32), (h, w, c)


def wct_np(content, style, alpha=0.6, eps=1e-5, ctx=None):
    ctx = ctx or default_context()
    fc, (h, w, c) = _flat(content)
    fs, _ = _flat(style)
    out = ctx.transform(fc, fs, alpha, _lib.WCT_NP, eps)
    return out.reshape(1, h, w, c)


def wct_tf(content, style, alpha, eps=1e-8, ctx=None):
    ctx = ctx or default_context()
    fc, (h, w, c) = _flat(content)
    fs, _ = _flat(style)
    out = ctx.transform(fc, fs, alpha, _lib.WCT_TF, eps)
    return out.reshape(1, h, w, c)


def adain(content_features, style_features, alpha, epsilon=1e-5, ctx=None):
    ctx = ctx or default_context()
    x = np.asarray(content_features, np.float32)
    s = np.asarray(style_features, np.float32)
    if x.ndim == 3:
        x = x[None]
    if s.ndim == 3:
        s = s[None]
    if x.shape[0] != 1 or s.shape[0] != 1:
        raise ValueError('batch must be 1')
    _, h, w, c = x.shape
    out = ctx.adain(x.reshape(h * w, c), s.reshape(-1, c), alpha, epsilon)
    return out.reshape(1, h, w, c)


def wct_style_swap(content, style, alpha, patch_size=3, stride=1, eps=1e-8, ctx=None):
    """ops.py:145: 1xHxWxC content/style encodings -> float32 1xHxWxC"""
    ctx = ctx or default_context()
    c = np.squeeze(np.asarray(content, np.float32))
    s = np.squeeze(np.asarray(style, np.float32))
    if c.ndim != 3 or s.ndim != 3:
        raise ValueError('style swap needs single 1xHxWxC feature maps')
    return ctx.style_swap(c, s, alpha, patch_size, stride, eps)[None]


def _moments_from_sums(sums, npix):
    """mean / population std / (Xn Xn^T + I) of img/255 from the exact integer moments."""
    s1 = sums[:3] / 255.0
    idx = {(0, 0): 3, (0, 1): 4, (0, 2): 5, (1, 1): 6, (1, 2): 7, (2, 2): 8}
    s2 = np.empty((3, 3))
    for (i, j), k in idx.items():
        s2[i, j] = s2[j, i] = sums[k] / (255.0 * 255.0)
    mean = s1 / npix
    cov = s2 - npix * np.outer(mean, mean)           # sum (x-m)(x-m)^T
    std = np.sqrt(np.diag(cov) / npix)                # population std (coral.py:23,27)
    cov_eye = cov / np.outer(std, std) + np.eye(3)    # coral.py:30-31 (not divided by N)
    return mean, std, cov_eye


def _mat_sqrt(x):
    # coral.py:8-11 verbatim in meaning: U sqrt(D) V.T with V = numpy's third SVD output (V^H);
    # the value depends on LAPACK's singular-vector signs, hence LAPACK on the host (see
    # include/wct_hip.h, wct_coral_stats).
    u, d, v = np.linalg.svd(x)
    return u.dot(np.diag(np.sqrt(d))).dot(v.T)


def _coral(source_u8, target_u8, ctx, want_f64, want_u8):
    src = np.ascontiguousarray(source_u8, np.uint8)
    tgt = np.ascontiguousarray(target_u8, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3 or tgt.ndim != 3 or tgt.shape[2] != 3:
        raise ValueError('CORAL needs HxWx3 images')
    ms, ss, cs = _moments_from_sums(ctx.coral_stats(src), src.shape[0] * src.shape[1])
    mt, st, ct = _moments_from_sums(ctx.coral_stats(tgt), tgt.shape[0] * tgt.shape[1])
    m = _mat_sqrt(ct).dot(np.linalg.inv(_mat_sqrt(cs)))          # coral.py:33
    return ctx.coral_apply(src, m, ms, ss, mt, st, want_f64=want_f64, want_u8=want_u8)


def coral_numpy(source, target, ctx=None):
    """source/target: HxWx3 images in [0,1] that are uint8 images / 255 (the only way the
    reference calls it, utils.py:88).  Returns float64 HxWx3."""
    ctx = ctx or default_context()
    s8 = np.rint(np.asarray(source, np.float64) * 255.0)
    t8 = np.rint(np.asarray(target, np.float64) * 255.0)
    if np.abs(s8 / 255.0 - source).max() > 1e-12 or np.abs(t8 / 255.0 - target).max() > 1e-12:
        raise ValueError('coral_numpy on the GPU path takes uint8-valued images / 255 (utils.py:88)')
    return _coral(s8.astype(np.uint8), t8.astype(np.uint8), ctx, True, False)[1]


def preserve_colors_np(style_rgb, content_rgb, ctx=None):
    ctx = ctx or default_context()
    return _coral(style_rgb, content_rgb, ctx, False, True)[0]


def content_colors_np(stylized_rgb, content_rgb, ctx=None):
    """The other way to keep a content's colours (Gatys et al. 2016, luminance-only transfer, post hoc): uint8 HxWx3 images, the
    stylized one at least as large as the content -> uint8, the luminance of `stylized_rgb` on the colours of `content_rgb`
    (the integer rule of include/wct_hip.h, wct_content_colors).  preserve_colors_np recolours the STYLE before stylizing; this
    recolours the RESULT, so the style side does not depend on the content."""
    ctx = ctx or default_context()
    return ctx.content_colors(stylized_rgb, content_rgb)


def guided_filter_np(stylized, content, radius, eps_q, guide='grey', ctx=None):
    """Guided smoothing of a result (He, Sun, Tang, "Guided Image Filtering"; the post-step of Li et al. 2018's fast photorealistic
    variant): uint8 HxWx3 images, the stylized one at least as large as the content -> uint8, `stylized` filtered over a
    (2 radius + 1)^2 box with `content` as guide: guide='grey', its grey, or guide='color', its three channels, which also keeps
    an edge between two colours of equal luminance (the integer rules of include/wct_hip.h, wct_guided_filter_guide).  radius
    1 .. 64; eps_q 1 .. 65025 in grey levels squared (_lib.guided_eps_q(eps) for an eps of the [0,1]^2 convention)."""
    ctx = ctx or default_context()
    return ctx.guided_filter(stylized, content, radius, eps_q, guide=guide)


def guided_upsample_np(stylized, content_small, content_full, radius, eps_q, ctx=None, guide='grey'):
    """Guided upsampling of a small result (He, Sun, "Fast Guided Filter"): uint8 HxWx3 images -- the small stylized frame, the
    small content it was made from (never larger than the frame) and the full content (never smaller than the small one) -> uint8
    at the full content's size.  The guided filter's coefficients a, b of the small pair are averaged, interpolated and evaluated
    against the full content, so the frame gets every edge of the full content at full sharpness (the integer rule of
    include/wct_hip.h, wct_guided_upsample_guide).  radius 1 .. 64 and eps_q 1 .. 65025 as in guided_filter_np, in pixels of the
    small frame.  guide: 'grey', or 'color' as in guided_filter_np: the three channels of the contents, which brings back an edge
    between two colours of equal luminance.  Not served: down-scaling."""
    ctx = ctx or default_context()
    return ctx.guided_upsample(stylized, content_small, content_full, radius, eps_q, guide=guide)


def guided_upsample_time_np(stylized, contents_small, contents_full, radius, eps_q, frames_t, positions=None):
    """Temporal guided upsampling of a small stylized clip, the rule of include/wct_hip.h (wct_guided_upsample_time) written out in
    NumPy int64 -- it runs on the host, without the library, and gives the bytes of Context.guided_upsample_time_clip: uint8 small
    frames [F][h][w][3], the small contents [F][hc][wc][3] they were made from and the full contents [F][H][W][3] of any F -> uint8
    [F][H][W][3].  The coefficients of guided_upsample_np and their means are formed over the (2 radius + 1)^2 box in each of the
    frames_t (0 .. 3) frames on each side of a frame, as guided_filter_time_np forms them, so flat static areas stop flickering;
    frame f is then interpolated and evaluated against its own full content, which returns every edge at full sharpness.
    frames_t = 0, or one frame, is guided_upsample_np per frame.  radius 1 .. 64 / 51 / 40 / 33 at frames_t 0 / 1 / 2 / 3, in pixels
    of the small frame.  positions: int [F][2] (py, px) in pixels of the small frame, as motion_global_np estimates them on the
    small contents; None: no shift.  The grey guide only.  Not served: the colour guide along time, down-scaling."""
    from .context import _upsample_time_clip, check_guided_motion, check_guided_time
    s, c, full = _upsample_time_clip(stylized, contents_small, contents_full)
    r, e, t = check_guided_time(radius, eps_q, frames_t)
    nf, h, w = s.shape[:3]
    hc, wc = c.shape[1:3]
    hf, wf = full.shape[1:3]
    pos = (np.zeros((nf, 2), np.int32) if positions is None else check_guided_motion(positions, nf)).astype(np.int64)
    rdiv = lambda a, b: (2 * a + b) // (2 * b)
    luma = lambda img: (img.astype(np.int64) @ np.array([77, 150, 29], np.int64) + 128) >> 8

    def box3(a):                                      # [F][h][w] -> the sums over the shifted boxes of the frames of the time window
        p = np.zeros((nf, h + 1, w + 1), np.int64)
        p[:, 1:, 1:] = a.cumsum(1).cumsum(2)
        out = np.zeros_like(a)
        for f in range(nf):
            for g in range(max(0, f - t), min(nf - 1, f + t) + 1):
                cy, cx = np.arange(h) + pos[g, 0] - pos[f, 0], np.arange(w) + pos[g, 1] - pos[f, 1]
                y0, x0 = np.clip(cy - r, 0, h), np.clip(cx - r, 0, w)
                y1, x1 = np.maximum(np.clip(cy + r + 1, 0, h), y0), np.maximum(np.clip(cx + r + 1, 0, w), x0)
                q = p[g]
                out[f] += q[y1[:, None], x1[None, :]] - q[y0[:, None], x1[None, :]] - q[y1[:, None], x0[None, :]] + q[y0[:, None], x0[None, :]]
        return out

    def taps(n, m):                                   # the axis taps of guided_upsample_np
        P = np.arange(n, dtype=np.int64)
        tt = np.clip((2 * P + 1) * m - n, 0, 2 * n * (m - 1))
        p0 = tt // (2 * n)
        return p0, np.minimum(p0 + 1, m - 1), rdiv((tt - p0 * 2 * n) * 256, 2 * n)

    guide = luma(c[:, np.minimum(np.arange(h), hc - 1)][:, :, np.minimum(np.arange(w), wc - 1)])
    n = box3(np.ones((nf, h, w), np.int64))
    si, sii = box3(guide), box3(guide * guide)
    y0, y1, fy = taps(hf, hc)
    x0, x1, fx = taps(wf, wc)
    big = luma(full)
    out = np.empty_like(full)
    for ch in range(3):
        p = s[..., ch].astype(np.int64)
        sp, sip = box3(p), box3(guide * p)
        a_q = rdiv((n * sip - si * sp) << 12, n * sii - si * si + e * n * n)
        b_q = rdiv((sp << 12) - a_q * si, n)
        am, bm = rdiv(box3(a_q), n), rdiv(box3(b_q), n)
        v = 0
        for ys, wy in ((y0, 256 - fy), (y1, fy)):
            for xs, wx in ((x0, 256 - fx), (x1, fx)):
                v = v + (am[:, ys[:, None], xs[None, :]] * big + bm[:, ys[:, None], xs[None, :]]) * (wy[:, None] * wx[None, :])
        out[..., ch] = np.clip((v + (1 << 27)) >> 28, 0, 255)
    return out


def guided_filter_time_np(stylized, contents, radius, eps_q, frames_t, ctx=None, positions=None, guide='grey'):
    """Temporal guided smoothing of a stylized clip, against the flicker of frames that were stylized one by one: uint8
    [F][Ho][Wo][3] frames and [F][Hc][Wc][3] contents of any F -> uint8 [F][Ho][Wo][3], guided_filter_np's grey-guide filter with
    its box extended over the frames_t (0 .. 3) frames on each side of a frame and cut at the clip's ends (the integer rule of
    include/wct_hip.h, wct_guided_filter_time).  Where the content stands still the frames are averaged along time; where it
    moves the result follows the content.  Without positions there is no motion compensation: a flat region that pans is averaged
    too.  radius 1 .. 64 / 51 / 40 / 33 at frames_t 0 / 1 / 2 / 3.  A clip of more than 32 frames goes in chunks of 32 - 4 frames_t
    frames with halos of 2 frames_t and gives the whole clip's bytes.
    positions: int [F][2] (py, px), one global translation per frame, as motion_global_np estimates them: the window in every
    neighbouring frame is shifted by the difference of the positions (wct_guided_filter_motion), so a clip that pans is averaged
    along its motion.  Steps between consecutive frames of at most 16 on both axes.
    guide: 'grey', or 'color' -- the three content channels as guide (wct_guided_filter_time_guide), with or without positions: the
    clip keeps an edge between two colours of equal luminance, which the grey guide blurs, and still stops flickering."""
    ctx = ctx or default_context()
    return ctx.guided_filter_time_clip(stylized, contents, radius, eps_q, frames_t, positions=positions, guide=guide)


def motion_global_np(contents, search=8, ctx=None):
    """One global integer translation per frame of a clip (wct_motion_global): uint8 [F][Hc][Wc][3] contents of any F -> int32
    [F][2] positions (py, px) from (0, 0), the sum of the steps between consecutive frames.  A step is the (dy, dx), |dy|, |dx| <=
    search (1 .. 16), with the smallest mean absolute difference of the grey guides over the even pixels, by exhaustive search; at
    equality the smallest step.  Both sides of a frame at least 4 search.  Not served: per-block or dense motion, sub-pixel
    shifts, rotation and zoom."""
    ctx = ctx or default_context()
    return ctx.motion_global(contents, search)


def texture_noise_np(h, w, seed, sample=0, smooth=False, ctx=None):
    """The noise image that texture synthesis starts from (Li et al. 2017, sec. 4.3) -> uint8 [h][w][3].  The reference draws it
    with `np.random.randint(0, 256, shape, np.uint8)` (webcam.py:191-192); here it is the seeded integer rule of include/wct_hip.h
    (wct_texture_noise), made on the device: the same (seed, sample) gives the same bytes anywhere, and every sample of a seed is
    an independent image.  smooth: the 27 202 27 filter along y and x, the gaussian_filter(sigma=0.5) of stylize.py:95-97."""
    ctx = ctx or default_context()
    return ctx.texture_noise(h, w, seed, sample, smooth)
