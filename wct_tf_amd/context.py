"""Python handle on one wct_ctx (one GPU, one HIP stream) -- the session object
that replaces the reference's tf.Session (wct.py:29-58).  Every method is a
thin ctypes call into libwct_hip.so; no arithmetic of the path happens here.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f32, fptr, u8
from .weights import ENCODER_CONVS, RELU_LEVEL, decoder_plan

_LEVEL_C = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}


def _levels(relu_targets):
    out = []
    for r in relu_targets:
        if isinstance(r, str):
            if r not in RELU_LEVEL:
                raise ValueError('unknown relu target %r' % (r,))
            out.append(RELU_LEVEL[r])
        else:
            out.append(int(r))
    return out


def _flags(adain=False, wct_mode='tf', swap5=False, images_f32=False, shared_style=False, content_colors=False, guided=False):
    """The flag word of a stylize call (WCT_FLAG_*, include/wct_hip.h)."""
    return (_lib.FLAG_ADAIN if adain else 0) | (_lib.FLAG_MODE_NP if wct_mode == 'np' else 0) | \
        (_lib.FLAG_SWAP5 if swap5 else 0) | (_lib.FLAG_IMAGES_F32 if images_f32 else 0) | \
        (_lib.FLAG_STYLE_SHARED if shared_style else 0) | (_lib.FLAG_CONTENT_COLORS if content_colors else 0) | \
        (_lib.FLAG_GUIDED if guided else 0)


def _feature_args(content, styles, validate):
    """A content [Nc][C] and K styles [Ns_k][C] as float32, the caller's own validate(content, K) (its result is returned), the
    shape check, and the style row counts as a C int array."""
    c = f32(content)
    ss = [f32(s) for s in styles]
    v = validate(c, len(ss))
    if c.ndim != 2 or any(s.ndim != 2 or s.shape[1] != c.shape[1] for s in ss):
        raise ValueError('expected [N][C] feature matrices with equal C')
    return c, ss, v, (C.c_int * len(ss))(*[s.shape[0] for s in ss])


def _color_images(stylized, content, ndim):
    """The refusals of content_colors, before any library call: uint8 arrays [...][H][W][3] of `ndim` dimensions, the stylized
    frame at least as large as the content.  -> both as contiguous uint8"""
    s, c = np.asarray(stylized), np.asarray(content)
    for name, a in (('stylized', s), ('content', c)):
        if a.dtype != np.uint8:
            raise ValueError('content_colors takes uint8 images, the %s one is %s' % (name, a.dtype))
        if a.ndim != ndim or a.shape[-1] != 3 or a.size == 0:
            raise ValueError('content_colors takes %s images, the %s one has shape %s' % ('[B][H][W][3]' if ndim == 4 else 'HxWx3', name, a.shape))
    if s.shape[-3] < c.shape[-3] or s.shape[-2] < c.shape[-2]:
        raise ValueError('the stylized frame %dx%d is smaller than its content %dx%d' % (s.shape[-3], s.shape[-2], c.shape[-3], c.shape[-2]))
    return u8(s), u8(c)


def check_guide(guide):
    """The guide of guided smoothing by name, 'grey' or 'color' -> WCT_GUIDE_GREY or WCT_GUIDE_COLOR"""
    if not isinstance(guide, str) or guide not in _lib.GUIDES:
        raise ValueError("the guided guide is 'grey' or 'color', got %r" % (guide,))
    return _lib.GUIDES[guide]


def check_guided(guided):
    """The refusals of guided=(radius, eps_q) or (radius, eps_q, guide), before any library call: two integers, the radius 1 .. 64
    and eps_q 1 .. 65025 (grey levels squared; _lib.guided_eps_q converts an eps of the [0,1]^2 convention), and the guide 'grey'
    (what the two-element form means) or 'color'.  -> (radius, eps_q), or (radius, eps_q, guide) as it was given"""
    try:
        g = tuple(guided)
        r, e = g[:2] if len(g) == 3 else g
        if int(r) != r or int(e) != e:
            raise TypeError
        r, e = int(r), int(e)
    except (TypeError, ValueError):
        raise ValueError("guided is (radius, eps_q), two integers, or (radius, eps_q, 'grey' or 'color'), got %r" % (guided,))
    if not 1 <= r <= _lib.GUIDED_MAX_RADIUS:
        raise ValueError('the guided radius must be 1 .. %d, got %d' % (_lib.GUIDED_MAX_RADIUS, r))
    if not 1 <= e <= _lib.GUIDED_MAX_EPS:
        raise ValueError('the guided eps_q must be 1 .. %d (grey levels squared), got %d' % (_lib.GUIDED_MAX_EPS, e))
    if len(g) == 3:
        check_guide(g[2])
        return r, e, g[2]
    return r, e


def check_guided_time(radius, eps_q, frames_t):
    """The refusals of temporal guided smoothing's parameters, before any library call: check_guided's, frames_t an integer
    0 .. 3 and the radius within the limit for it (_lib.GUIDED_TIME_MAX_RADIUS: (2 radius + 1)^2 (2 frames_t + 1) <= 33025).
    -> (radius, eps_q, frames_t)"""
    r, e = check_guided((radius, eps_q))
    try:
        if int(frames_t) != frames_t:
            raise TypeError
        t = int(frames_t)
    except (TypeError, ValueError):
        raise ValueError('guided_frames is an integer 0 .. %d, got %r' % (len(_lib.GUIDED_TIME_MAX_RADIUS) - 1, frames_t))
    if not 0 <= t < len(_lib.GUIDED_TIME_MAX_RADIUS):
        raise ValueError('guided_frames must be 0 .. %d frames on each side, got %d' % (len(_lib.GUIDED_TIME_MAX_RADIUS) - 1, t))
    if r > _lib.GUIDED_TIME_MAX_RADIUS[t]:
        raise ValueError('the guided radius must be 1 .. %d with guided_frames %d, got %d' % (_lib.GUIDED_TIME_MAX_RADIUS[t], t, r))
    return r, e, t


def check_guided_motion(positions, frames):
    """The refusals of positions= of temporal guided smoothing along motion, before any library call: an integer array
    [frames][2] of (py, px) whose steps between consecutive frames are within _lib.MOTION_MAX_RANGE on both axes
    -> contiguous int32 [frames][2]"""
    try:
        p = np.asarray(positions)
    except Exception:
        raise ValueError('positions is an integer array [frames][2] of (py, px), got %r' % (positions,))
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError('positions is an integer array [frames][2] of (py, px), got dtype %s' % p.dtype)
    if p.ndim != 2 or p.shape != (int(frames), 2):
        raise ValueError('positions is [frames][2], one (py, px) per frame: expected (%d, 2), got %s' % (frames, p.shape))
    p = p.astype(np.int64)
    if np.abs(p).max() >= 1 << 30:
        raise ValueError('positions must be below 2^30 in size')
    step = np.abs(np.diff(p, axis=0))
    if step.size and step.max() > _lib.MOTION_MAX_RANGE:
        f = int(np.argmax(step.max(1) > _lib.MOTION_MAX_RANGE))
        raise ValueError('positions: the step from frame %d to %d is %s, must be within %d on both axes'
                         % (f, f + 1, tuple(int(v) for v in p[f + 1] - p[f]), _lib.MOTION_MAX_RANGE))
    return np.ascontiguousarray(p, np.int32)


def check_motion_search(search, hc, wc):
    """The refusals of the estimator's search range, before any library call: an integer 1 .. 16, both sides of the content at
    least 4 search, at most 2^28 pixels -> search"""
    try:
        if int(search) != search:
            raise TypeError
        r = int(search)
    except (TypeError, ValueError):
        raise ValueError('the motion search range is an integer 1 .. %d, got %r' % (_lib.MOTION_MAX_RANGE, search))
    if not 1 <= r <= _lib.MOTION_MAX_RANGE:
        raise ValueError('the motion search range must be 1 .. %d, got %d' % (_lib.MOTION_MAX_RANGE, r))
    if hc < 4 * r or wc < 4 * r:
        raise ValueError('a motion search range of %d needs contents of at least %d x %d, got %d x %d' % (r, 4 * r, 4 * r, hc, wc))
    if hc * wc > _lib.MOTION_MAX_PIXELS:
        raise ValueError('motion estimation takes contents of at most 2^28 pixels, got %d x %d' % (hc, wc))
    return r


def _guided_clip(stylized, contents):
    """The refusals of a clip and its contents, before any library call -> both as contiguous uint8 [F][..][..][3], F >= 1"""
    try:
        s, c = _color_images(stylized, contents, 4)
    except ValueError as e:
        raise ValueError(str(e).replace('content_colors', 'guided_filter_time'))
    if s.shape[0] != c.shape[0]:
        raise ValueError('a clip takes as many contents as frames, got %d and %d' % (s.shape[0], c.shape[0]))
    return s, c


def _guided_images(stylized, content, ndim):
    """The refusals of guided_filter's images, before any library call (those of content_colors) -> both as contiguous uint8"""
    try:
        return _color_images(stylized, content, ndim)
    except ValueError as e:
        raise ValueError(str(e).replace('content_colors', 'guided_filter'))


def check_guided_upsample(guided_upsample):
    """The refusals of guided_upsample=(short_side, radius, eps_q) or (short_side, radius, eps_q, guide), before any library call:
    three integers, the short side of the working size at least 1, the radius and eps_q those of check_guided (in pixels of the
    working size), and the guide 'grey' (what the three-element form means) or 'color'.
    -> (short_side, radius, eps_q), or (short_side, radius, eps_q, guide) as it was given"""
    try:
        g = tuple(guided_upsample)
        side, r, e = g[:3] if len(g) == 4 else g
        if int(side) != side:
            raise TypeError
        side = int(side)
    except (TypeError, ValueError):
        raise ValueError("guided_upsample is (short_side, radius, eps_q), three integers, or (short_side, radius, eps_q, 'grey' or "
                         "'color'), got %r" % (guided_upsample,))
    if side < 1:
        raise ValueError('the short side of guided_upsample must be at least 1, got %d' % side)
    r, e = check_guided((r, e))
    if len(g) == 4:
        check_guide(g[3])
        return side, r, e, g[3]
    return side, r, e


def upsample_work_size(h, w, short_side):
    """The working size of an h x w content under guided_upsample: utils.resize_shape(h, w, short_side), or the content's own size
    when its short side is short_side or less already (it is then worked on as it is: the op never scales down)"""
    if min(h, w) <= short_side:
        return int(h), int(w)
    from .utils import resize_shape
    return tuple(int(v) for v in resize_shape(h, w, short_side))


def _upsample_images(stylized, content_small, content_full, ndim):
    """The refusals of guided_upsample's images, before any library call: three uint8 arrays [...][.][.][3] of `ndim` dimensions,
    the small frame at least as large as the small content, the full content at least as large as the small one
    -> the three as contiguous uint8"""
    arrs = []
    for name, a in (('stylized', stylized), ('content_small', content_small), ('content_full', content_full)):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise ValueError('guided_upsample takes uint8 images, %s is %s' % (name, a.dtype))
        if a.ndim != ndim or a.shape[-1] != 3 or a.size == 0:
            raise ValueError('guided_upsample takes %s images, %s has shape %s' % ('[B][H][W][3]' if ndim == 4 else 'HxWx3', name, a.shape))
        arrs.append(u8(a))
    s, c, f = arrs
    if s.shape[-3] < c.shape[-3] or s.shape[-2] < c.shape[-2]:
        raise ValueError('stylized %dx%d is smaller than content_small %dx%d' % (s.shape[-3], s.shape[-2], c.shape[-3], c.shape[-2]))
    if f.shape[-3] < c.shape[-3] or f.shape[-2] < c.shape[-2]:
        raise ValueError('content_full %dx%d is smaller than content_small %dx%d: guided_upsample does not scale down'
                         % (f.shape[-3], f.shape[-2], c.shape[-3], c.shape[-2]))
    if ndim == 4 and not (s.shape[0] == c.shape[0] == f.shape[0] and 1 <= s.shape[0] <= _lib.BATCH_MAX):
        raise ValueError('a batch takes 1 .. %d frames and as many contents of either size, got %d, %d and %d'
                         % (_lib.BATCH_MAX, s.shape[0], c.shape[0], f.shape[0]))
    return s, c, f


def _upsample_time_full(contents_full, frames, contents_small):
    """The refusals of the full contents of `frames` delivered frames, before any library call -> contiguous uint8 [frames][H][W][3]"""
    f = np.asarray(contents_full)
    if f.dtype != np.uint8:
        raise ValueError('guided_upsample_time takes uint8 images, contents_full is %s' % f.dtype)
    if f.ndim != 4 or f.shape[-1] != 3 or f.size == 0:
        raise ValueError('guided_upsample_time takes [F][H][W][3] images, contents_full has shape %s' % (f.shape,))
    if f.shape[0] != frames:
        raise ValueError('guided_upsample_time takes one full content per delivered frame, got %d for %d frames' % (f.shape[0], frames))
    c = contents_small
    if f.shape[1] < c.shape[1] or f.shape[2] < c.shape[2]:
        raise ValueError('contents_full %dx%d is smaller than contents_small %dx%d: guided_upsample_time does not scale down'
                         % (f.shape[1], f.shape[2], c.shape[1], c.shape[2]))
    return u8(f)


def _upsample_time_clip(stylized, contents_small, contents_full):
    """The refusals of a clip of small frames, its small and its full contents, before any library call: three uint8 arrays
    [F][.][.][3] with the same F >= 1, the small frame at least as large as the small content, the full content at least as large
    as the small one -> the three as contiguous uint8"""
    try:
        s, c = _guided_clip(stylized, contents_small)
    except ValueError as e:
        raise ValueError(str(e).replace('guided_filter_time', 'guided_upsample_time'))
    return s, c, _upsample_time_full(contents_full, s.shape[0], c)


def upsample_time_chunk(hf, wf, frames_t):
    """The delivered frames of one chunk of guided_upsample_time_clip at full size hf x wf: 32 - 4 frames_t (the resident clip
    with its halos is at most 32 small frames), lowered where that many full frames would reach 2^31 bytes"""
    per = int(hf) * int(wf) * 3
    if per >= 1 << 31:
        raise ValueError('a full content of %dx%dx3 passes 2^31 bytes' % (hf, wf))
    return max(1, min(_lib.BATCH_MAX - 4 * int(frames_t), ((1 << 31) - 1) // per))


def check_work_size(work_size, h, w):
    """The working size (hc, wc) of a stylize_prepared_upsampled call on h x w contents: two positive integers, neither above the
    content's.  -> (hc, wc)"""
    hc, wc = check_resize(work_size)
    if hc > h or wc > w:
        raise ValueError('the working size %dx%d is larger than the %dx%d content: guided_upsample does not scale down' % (hc, wc, h, w))
    return hc, wc


def check_texture(size, passes=1, batch=1, seed=0, first_sample=0):
    """The refusals of a texture call, before any library call: a size (H, W) of two positive integers, 1 .. PASSES_MAX passes,
    1 .. BATCH_MAX samples per call, seed and sample indices that are uint32.  -> (H, W)"""
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('a texture size is (H, W), got %r' % (size,))
    if h < 1 or w < 1:
        raise ValueError('an empty texture size %dx%d' % (h, w))
    if not 1 <= int(passes) <= _lib.PASSES_MAX:
        raise ValueError('a texture takes 1 .. %d passes, got %d' % (_lib.PASSES_MAX, passes))
    if not 1 <= int(batch) <= _lib.BATCH_MAX:
        raise ValueError('a batch takes 1 .. %d samples, got %d' % (_lib.BATCH_MAX, batch))
    if not 0 <= int(seed) < 1 << 32 or not 0 <= int(first_sample) or not int(first_sample) + int(batch) <= 1 << 32:
        raise ValueError('seed and sample indices are uint32, got seed %d, samples %d .. %d' %
                         (seed, first_sample, int(first_sample) + int(batch) - 1))
    return h, w


def check_resize(size, frames=None, ndim=4):
    """The refusals of a resize, before any library call: a target size (h, w) of two positive integers and, given `frames`, a
    non-empty uint8 array [B][H][W][3] (ndim 4; B <= BATCH_MAX) or HxWx3 (ndim 3).  -> (h, w), or (h, w, frames contiguous)"""
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('a resize target is (h, w), got %r' % (size,))
    if h < 1 or w < 1:
        raise ValueError('an empty resize target %dx%d' % (h, w))
    if frames is None:
        return h, w
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise ValueError('resize takes uint8 images, got %s' % a.dtype)
    if a.ndim != ndim or a.shape[-1] != 3 or a.size == 0:
        raise ValueError('resize takes %s images, got shape %s' % ('[B][H][W][3]' if ndim == 4 else 'HxWx3', a.shape))
    if ndim == 4 and not 1 <= a.shape[0] <= _lib.BATCH_MAX:
        raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, a.shape[0]))
    return h, w, u8(a)


def _image_arrays(images):
    """Pointers, heights and widths of K images as C arrays."""
    k = len(images)
    return ((_lib._U8 * k)(*[s.ctypes.data_as(_lib._U8) for s in images]), (C.c_int * k)(*[s.shape[0] for s in images]),
            (C.c_int * k)(*[s.shape[1] for s in images]))


class PreparedStyle(object):
    """A style whose style side -- encoder pass, statistics, covariances, eigendecompositions, colouring matrices -- is kept on
    the device (wct_style, include/wct_hip.h): Context.prepare_style makes one, the stylize_prepared* calls take it in the place
    of a style image and give the image-based call's frame bit for bit.  Owned by its context (closing the context closes it);
    close() or a `with` block releases it earlier.  `image` is the style as it was handed in.  `region` is None, or the
    (label_map, label) of a style region: the statistics of every level come from the feature rows of that label alone."""

    def __init__(self, ctx, handle, image, levels, region=None):
        self.ctx, self.h, self.image, self.levels, self.region = ctx, handle, image, frozenset(levels), region

    def rows(self, relu_target):
        """the feature rows the statistics of `relu_target` use (wct_style_rows): h * w of the style's map, or the region's"""
        if self.closed:
            raise ValueError('the prepared style is closed')
        n = C.c_int()
        check(self.ctx.lib.wct_style_rows(self.ctx.h, self.h, _levels([relu_target])[0], C.byref(n)))
        return n.value

    @property
    def closed(self):
        return self.h is None or self.ctx is None or not getattr(self.ctx, 'h', None)

    def close(self):
        if not self.closed:
            self.ctx.lib.wct_style_free(self.ctx.h, self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_prepared(ctx, styles, relu_targets, swap5=False):
    """The refusals of a call that takes prepared styles, raised before any library call: swap5, a closed handle, a handle of
    another context, levels the handle was not prepared for, and -- last -- an object whose `h` is not the wct_style pointer
    prepare_style stores (TypeError: the library takes addresses, and a made-up one must never reach it)."""
    if swap5:
        raise ValueError('swap5 takes a style image: style-swap needs the style\'s relu5_1 patches, which a prepared style does not hold')
    lv = _levels(relu_targets)
    for s in styles:
        if not isinstance(s, PreparedStyle):
            raise TypeError('expected a PreparedStyle, got %s' % type(s).__name__)
        if s.closed:
            raise ValueError('the prepared style is closed')
        if s.ctx is not ctx:
            raise ValueError('the prepared style belongs to another context')
        if not set(lv) <= s.levels:
            raise ValueError('the prepared style serves relu levels %s, not %s' % (sorted(s.levels), sorted(set(lv))))
    for s in styles:
        if not isinstance(s.h, C.c_void_p):
            raise TypeError('the prepared style holds %s, not a wct_style pointer' % type(s.h).__name__)
    return lv


class WarmState(object):
    """A video warm start (wct_warm, include/wct_hip.h): per relu level the eigenvector basis of the last frame a call stylized
    with it, from which the content eigensolves of the next call start.  Context.warm_state makes one; the stylize_prepared*
    calls and Context.transform take it as `warm=`.  A fresh state, and one after reset(), solves cold -- today's frames bit for
    bit; warm frames meet the same tolerances but are not bit-identical to cold ones.  Owned by its context; close() or a
    `with` block releases it earlier."""

    def __init__(self, ctx, handle, levels):
        self.ctx, self.h, self.levels = ctx, handle, frozenset(levels)

    @property
    def closed(self):
        return self.h is None or self.ctx is None or not getattr(self.ctx, 'h', None)

    def close(self):
        if not self.closed:
            self.ctx.lib.wct_warm_free(self.ctx.h, self.h)
        self.h = None

    def _live(self):
        if self.closed:
            raise ValueError('the warm state is closed')

    def reset(self):
        """Every level invalid: the next call solves cold."""
        self._live()
        check(self.ctx.lib.wct_warm_reset(self.ctx.h, self.h))

    def _basis(self, level, want):
        self._live()
        lv = _levels([level])[0]
        if lv not in self.levels:
            raise ValueError('the warm state serves relu levels %s, not %d' % (sorted(self.levels), lv))
        valid = C.c_int()
        v = np.empty((_LEVEL_C[lv], _LEVEL_C[lv]), np.float32) if want else None
        check(self.ctx.lib.wct_warm_basis(self.ctx.h, self.h, lv, C.byref(valid), fptr(v) if want else None))
        return bool(valid.value), v

    def valid(self, level):
        """Does `level` ('relu3_1' or 3) hold a basis?"""
        return self._basis(level, False)[0]

    def basis(self, level):
        """The stored C x C basis of `level` (eigenvectors in columns), or None while the level is invalid."""
        ok, v = self._basis(level, True)
        return v if ok else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_warm(ctx, warm, relu_targets, adain=False, swap5=False, level_set=True):
    """The refusals of a call that takes a warm state, raised before any library call: AdaIN (no eigensolve) and swap5, an object
    that is not a WarmState, a closed one, another context's, and a call whose levels are not the state's."""
    if not isinstance(warm, WarmState):
        raise TypeError('expected a WarmState, got %s' % type(warm).__name__)
    if adain:
        raise ValueError('a warm state starts eigensolves: AdaIN has none')
    if swap5:
        raise ValueError('a warm state goes with a prepared style, which does not serve swap5')
    if warm.closed:
        raise ValueError('the warm state is closed')
    if warm.ctx is not ctx:
        raise ValueError('the warm state belongs to another context')
    lv = set(_levels(relu_targets))
    if (lv != warm.levels) if level_set else not lv <= warm.levels:
        raise ValueError('the warm state serves relu levels %s, not %s' % (sorted(warm.levels), sorted(lv)))
    if not isinstance(warm.h, C.c_void_p):
        raise TypeError('the warm state holds %s, not a wct_warm pointer' % type(warm.h).__name__)


def check_band_rows(band_rows):
    """band_rows as the banded calls take it: an int, 0 (automatic) or a positive multiple of 16 -- checked before any GPU call"""
    if isinstance(band_rows, bool) or not isinstance(band_rows, (int, np.integer)):
        raise ValueError('band_rows must be an int, got %r' % (band_rows,))
    if band_rows < 0 or band_rows % 16:
        raise ValueError('band_rows must be 0 (automatic) or a positive multiple of 16, got %d' % band_rows)
    return int(band_rows)


def band_rows(hc, wc, relu_targets):
    """wct_band_rows: 0 when the whole-image calls take an hc x wc content with the levels `relu_targets`, else the automatic
    band height of the banded call.  Host code only: no context, no GPU."""
    lv = _levels(relu_targets)
    out = C.c_int()
    check(_lib.load().wct_band_rows(int(hc), int(wc), (C.c_int * len(lv))(*lv), len(lv), C.byref(out)))
    return out.value


def band_plan(h, w, relu_target, band_rows=0):
    """wct_band_plan: the bands of one level on an h x w input as an int array [n_bands][6] -- the encoder span and the interior
    in image rows, the decoder span in feature rows.  Host code only."""
    level = _levels([relu_target])[0]
    lib = _lib.load()
    n = C.c_int()
    check(lib.wct_band_plan(int(h), int(w), level, int(band_rows), 0, C.byref(n), None))
    rows = np.zeros((n.value, 6), np.int32)
    check(lib.wct_band_plan(int(h), int(w), level, int(band_rows), n.value, C.byref(n), rows.ctypes.data_as(_lib._I)))
    return rows


def wrap_halo(relu_target):
    """wct_wrap_halo: the wrap-around halo of one level as (enc, dec_before, dec_after) -- image pixels on every side of the
    encoder's input, feature pixels in front of and behind the decoder's.  Host code only: no context, no GPU."""
    level = _levels([relu_target])[0]
    e, d0, d1 = C.c_int(), C.c_int(), C.c_int()
    check(_lib.load().wct_wrap_halo(level, C.byref(e), C.byref(d0), C.byref(d1)))
    return e.value, d0.value, d1.value


def check_wrap(h, w, relu_targets):
    """The size rule of the wrap calls, before any GPU call (wct_wrap_check, host code only): h and w multiples of the deepest
    level's stride, the tile large enough for that level, its padded maps inside one launch -- else ValueError with the
    library's message.  -> (h, w)"""
    lv = _levels(relu_targets)
    lib = _lib.load()
    if lib.wct_wrap_check(int(h), int(w), (C.c_int * len(lv))(*lv), len(lv)) != 0:
        raise ValueError(lib.wct_last_error().decode())
    return int(h), int(w)


def region_rows(label_map, label, relu_target):
    """The feature rows a style region has at `relu_target`, by the library's rule (include/wct_hip.h): feature pixel (i, j) of the
    ceil-pooled h x w map has the label label_map[min(i s, H - 1)][min(j s, W - 1)], s = 2^(level - 1).  No GPU call."""
    m = np.asarray(label_map)
    l = _levels([relu_target])[0]
    h, w = m.shape
    for _ in range(l - 1):
        h, w = (h + 1) // 2, (w + 1) // 2
    s = 1 << (l - 1)
    rows = np.minimum(np.arange(h) * s, m.shape[0] - 1)
    cols = np.minimum(np.arange(w) * s, m.shape[1] - 1)
    return int(np.count_nonzero(m[np.ix_(rows, cols)] == label))


def split_styles(styles):
    """(handles, images) of a list of styles: one of the two is empty, a list that mixes PreparedStyle objects and images is a
    ValueError."""
    handles = [s for s in styles if isinstance(s, PreparedStyle)]
    if handles and len(handles) != len(styles):
        raise ValueError('give either style images or prepared styles, not a mix of both')
    return handles, ([] if handles else list(styles))


class Context(object):
    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.wct_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.loaded_decoders = set()
        self.encoder_loaded = False

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wct_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.wct_sync(self.h))
        self._masks_in_flight = []               # (stylize_prepared_masked_batch_dev: every upload has run)

    def stream_handle(self):
        """The context's hipStream_t as an integer (torch.cuda.ExternalStream(handle) wraps it)."""
        p = C.c_void_p()
        check(self.lib.wct_get_stream(self.h, C.byref(p)))
        return p.value or 0

    # ---- weights ---------------------------------------------------------
    def set_encoder(self, enc):
        pre_w, pre_b = enc['preprocess']
        pw = f32(np.asarray(pre_w).reshape(3, 3))
        pb = f32(pre_b)
        ws = [f32(enc[name][0]) for name, _, _ in ENCODER_CONVS]
        bs = [f32(enc[name][1]) for name, _, _ in ENCODER_CONVS]
        for (name, cin, cout), w in zip(ENCODER_CONVS, ws):
            if w.shape != (3, 3, cin, cout):
                raise ValueError('%s: expected HWIO %s, got %s' % (name, (3, 3, cin, cout), w.shape))
        check(self.lib.wct_set_encoder(self.h, fptr(pw), fptr(pb), _lib.ptr_array(ws), _lib.ptr_array(bs), len(ws)))
        self.encoder_loaded = True

    def set_decoder(self, relu_target, layers):
        level = _levels([relu_target])[0]
        plan = [p for p in decoder_plan('relu%d_1' % level) if p[0] == 'C']
        if len(layers) != len(plan):
            raise ValueError('decoder relu%d_1 needs %d conv layers, got %d' % (level, len(plan), len(layers)))
        ws = [f32(w) for w, _ in layers]
        bs = [f32(b) for _, b in layers]
        for (_, cin, cout, _), w in zip(plan, ws):
            if w.shape != (3, 3, cin, cout):
                raise ValueError('decoder relu%d_1: expected HWIO %s, got %s' % (level, (3, 3, cin, cout), w.shape))
        check(self.lib.wct_set_decoder(self.h, level, _lib.ptr_array(ws), _lib.ptr_array(bs), len(ws)))
        self.loaded_decoders.add(level)

    def set_weights(self, weights):
        self.set_encoder(weights['encoder'])
        for relu, layers in weights['decoder'].items():
            self.set_decoder(relu, layers)

    # ---- op level ----------------------------------------------------------
    def transform(self, content, style, alpha, mode, eps=-1.0, return_sweeps=False, warm=None, level=None):
        """content [Nc][C], style [Ns][C] float32 -> [Nc][C].  warm (a WarmState) with level: the content eigensolve starts from
        the state's basis of that level (wct_transform_warm; the reference eps only)."""
        c = f32(content)
        s = f32(style)
        if c.ndim != 2 or s.ndim != 2 or c.shape[1] != s.shape[1]:
            raise ValueError('expected [N][C] feature matrices with equal C')
        out = np.empty_like(c)
        sweeps = (C.c_int * 2)()
        self.last_sweeps = sweeps            # negative entries: that eigensolve failed (the call raises WCTNotConverged)
        if warm is not None:
            if level is None:
                raise ValueError('transform(warm=...) needs the level whose basis it starts from')
            if eps >= 0:
                raise ValueError('transform(warm=...) takes the reference eps only')
            check_warm(self, warm, [level], level_set=False)
            check(self.lib.wct_transform_warm(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], c.shape[1], float(alpha),
                                              _lib.FLAG_MODE_NP if int(mode) == _lib.WCT_NP else 0, warm.h, _levels([level])[0],
                                              fptr(out), sweeps))
            return (out, list(sweeps)) if return_sweeps else out
        check(self.lib.wct_transform(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], c.shape[1],
                                     float(alpha), int(mode), float(eps), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def adain(self, content, style, alpha, epsilon=1e-5):
        c = f32(content)
        s = f32(style)
        out = np.empty_like(c)
        check(self.lib.wct_adain(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], c.shape[1],
                                 float(alpha), float(epsilon), fptr(out)))
        return out

    @staticmethod
    def _region_level(content, style, labels, label):
        """The arguments of a one-level region call, checked before any GPU call: content [Nc][C], style [hs][ws][C] float32,
        labels [hs][ws] integers, label 0 .. 7."""
        c, s = f32(content), f32(style)
        if c.ndim != 2 or s.ndim != 3 or c.shape[1] != s.shape[2]:
            raise ValueError('expected content [N][C] and a style feature map [hs][ws][C] with equal C')
        return c, s, _lib.style_region_map(labels, s.shape[:2], label=label)

    def transform_region(self, content, style, labels, label, alpha, mode, eps=-1.0, return_sweeps=False):
        """transform() on a style region (wct_transform_region): style [hs][ws][C] a feature map, labels [hs][ws] -- the style
        rows are those of `label`, selected on the device: transform(content, style[labels == label]) bit for bit."""
        c, s, m = self._region_level(content, style, labels, label)
        out = np.empty_like(c)
        sweeps = (C.c_int * 2)()
        self.last_sweeps = sweeps
        check(self.lib.wct_transform_region(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], s.shape[1], c.shape[1],
                                            m.ctypes.data_as(_lib._U8), int(label), float(alpha), int(mode), float(eps), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def adain_region(self, content, style, labels, label, alpha, epsilon=1e-5):
        """adain() on a style region (wct_adain_region): as transform_region."""
        c, s, m = self._region_level(content, style, labels, label)
        out = np.empty_like(c)
        check(self.lib.wct_adain_region(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], s.shape[1], c.shape[1],
                                        m.ctypes.data_as(_lib._U8), int(label), float(alpha), float(epsilon), fptr(out)))
        return out

    @staticmethod
    def _strength_level(content, smap, h, w, stride):
        """The arguments of a one-level strength call, checked before any GPU call: content [h*w][C] float32, smap [Hm][Wm] uint8."""
        c = f32(content)
        m = np.asarray(smap)
        if m.ndim != 2:
            raise ValueError('expected an [H][W] strength map, got shape %s' % (m.shape,))
        m = _lib.strength_map(m, m.shape)
        if c.ndim != 2 or int(h) < 1 or int(w) < 1 or int(stride) < 1 or c.shape[0] != int(h) * int(w):
            raise ValueError('content of shape %s is not the [h*w][C] rows of a %dx%d feature map' % (c.shape, h, w))
        return c, m

    def transform_strength(self, content, style, smap, h, w, stride, alpha, mode, eps=-1.0, return_sweeps=False):
        """transform() with a strength map (wct_transform_strength): content [h*w][C] the rows of an h x w feature map, smap
        [Hm][Wm] uint8 sampled at `stride` -- row (i, j) takes a = alpha * smap[min(i stride, Hm-1)][min(j stride, Wm-1)] / 255 and
        leaves as a * transform(content, style, 1.0)[row] + (1 - a) * content[row], in float32."""
        c, m = self._strength_level(content, smap, h, w, stride)
        s = f32(style)
        if s.ndim != 2 or c.shape[1] != s.shape[1]:
            raise ValueError('expected [N][C] feature matrices with equal C')
        out = np.empty_like(c)
        sweeps = (C.c_int * 2)()
        self.last_sweeps = sweeps
        check(self.lib.wct_transform_strength(self.h, fptr(c), c.shape[0], int(h), int(w), m.ctypes.data_as(_lib._U8), m.shape[0],
                                              m.shape[1], int(stride), fptr(s), s.shape[0], c.shape[1], float(alpha), int(mode),
                                              float(eps), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def adain_strength(self, content, style, smap, h, w, stride, alpha, epsilon=1e-5):
        """adain() with a strength map (wct_adain_strength): as transform_strength."""
        c, m = self._strength_level(content, smap, h, w, stride)
        s = f32(style)
        out = np.empty_like(c)
        check(self.lib.wct_adain_strength(self.h, fptr(c), c.shape[0], int(h), int(w), m.ctypes.data_as(_lib._U8), m.shape[0],
                                          m.shape[1], int(stride), fptr(s), s.shape[0], c.shape[1], float(alpha), float(epsilon),
                                          fptr(out)))
        return out

    def transform_mix(self, content, styles, weights, alpha, mode, eps=-1.0, return_sweeps=False):
        """Style mix (wct_transform_mix): content [Nc][C], styles K x [Ns_k][C] float32, weights [K] (None: equal) ->
        sum_k lambda_k transform(content, styles[k]) [Nc][C], lambda = weights / sum(weights).  Sweeps: content, then style k."""
        c, ss, w, ns = _feature_args(content, styles, lambda c, k: _lib.mix_weights(weights, k))
        out = np.empty_like(c)
        sweeps = (C.c_int * (1 + len(ss)))()
        self.last_sweeps = sweeps
        check(self.lib.wct_transform_mix(self.h, fptr(c), c.shape[0], _lib.ptr_array(ss), ns, len(ss), fptr(w), c.shape[1],
                                         float(alpha), int(mode), float(eps), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def adain_mix(self, content, styles, weights, alpha, epsilon=1e-5):
        """AdaIN with a style mix (wct_adain_mix): the style's deviation and mean are the lambda-weighted ones."""
        c, ss, w, ns = _feature_args(content, styles, lambda c, k: _lib.mix_weights(weights, k))
        out = np.empty_like(c)
        check(self.lib.wct_adain_mix(self.h, fptr(c), c.shape[0], _lib.ptr_array(ss), ns, len(ss), fptr(w), c.shape[1],
                                     float(alpha), float(epsilon), fptr(out)))
        return out

    def transform_masked(self, content, styles, labels, alpha, mode, eps=-1.0, return_sweeps=False):
        """Spatial control (wct_transform_masked): content [Nc][C], styles K x [Ns_k][C] float32, labels [Nc] in 0 .. K-1 ->
        [Nc][C], the rows of label k transformed with style k alone.  Sweeps [2K]: label k's content at 2k, style at 2k + 1
        (0: a label with fewer than 2 rows)."""
        c, ss, lab, ns = _feature_args(content, styles, lambda c, k: _lib.mask_labels(labels, k, (c.shape[0],)))
        out = np.empty_like(c)
        sweeps = (C.c_int * (2 * len(ss)))()
        self.last_sweeps = sweeps
        check(self.lib.wct_transform_masked(self.h, fptr(c), c.shape[0], lab.ctypes.data_as(_lib._U8), _lib.ptr_array(ss), ns,
                                            len(ss), c.shape[1], float(alpha), int(mode), float(eps), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def adain_masked(self, content, styles, labels, alpha, epsilon=1e-5):
        """AdaIN with spatial control (wct_adain_masked): the rows of label k take region k's moments and style k's."""
        c, ss, lab, ns = _feature_args(content, styles, lambda c, k: _lib.mask_labels(labels, k, (c.shape[0],)))
        out = np.empty_like(c)
        check(self.lib.wct_adain_masked(self.h, fptr(c), c.shape[0], lab.ctypes.data_as(_lib._U8), _lib.ptr_array(ss), ns,
                                        len(ss), c.shape[1], float(alpha), float(epsilon), fptr(out)))
        return out

    def mask_compact(self, mask, h, w, stride, k):
        """The device's stable partition of an h x w feature map's rows by label (wct_mask_compact) -> (perm [h*w], seg_off [k+1])"""
        m = _lib.mask_labels(mask, k)
        if m.ndim != 2:
            raise ValueError('expected an [H][W] label map')
        perm = np.empty(h * w, np.int32)
        seg = np.empty(k + 1, np.int32)
        check(self.lib.wct_mask_compact(self.h, m.ctypes.data_as(_lib._U8), m.shape[0], m.shape[1], int(h), int(w), int(stride),
                                        int(k), perm.ctypes.data_as(_lib._I), seg.ctypes.data_as(_lib._I)))
        return perm, seg

    def mask_compact_batch(self, masks, h, w, stride, k):
        """mask_compact for B label maps [B][H][W] in one launch of each pass (wct_mask_compact_batch) -> (perm [B][h*w],
        seg_off [B][k+1])"""
        m = _lib.mask_labels(masks, k)
        if m.ndim != 3:
            raise ValueError('expected [B][H][W] label maps')
        perm = np.empty((m.shape[0], h * w), np.int32)
        seg = np.empty((m.shape[0], k + 1), np.int32)
        check(self.lib.wct_mask_compact_batch(self.h, m.ctypes.data_as(_lib._U8), m.shape[0], m.shape[1], m.shape[2], int(h), int(w),
                                              int(stride), int(k), perm.ctypes.data_as(_lib._I), seg.ctypes.data_as(_lib._I)))
        return perm, seg

    def style_swap(self, content, style, alpha, patch_size=3, stride=1, eps=-1.0):
        """content [hc][wc][C], style [hs][ws][C] float32 -> [hc][wc][C] (ops.py:145-278)"""
        c = f32(content)
        s = f32(style)
        out = np.empty_like(c)
        check(self.lib.wct_style_swap(self.h, fptr(c), c.shape[0], c.shape[1], fptr(s), s.shape[0], s.shape[1],
                                      c.shape[2], float(alpha), int(patch_size), int(stride), float(eps), fptr(out)))
        return out

    def set_style_swap(self, ss_alpha=0.6, patch_size=3, stride=1):
        check(self.lib.wct_set_style_swap(self.h, float(ss_alpha), int(patch_size), int(stride)))

    def eigh(self, mats, return_sweeps=False, symmetrize=True):
        """mats [n][C][C] (or [C][C]) -> (evals [n][C], evecs [n][C][C]) through wct_eigh.  symmetrize=False hands the float32
        array to the ABI as given (what a C caller does)."""
        a = f32(mats)
        if a.ndim == 2:
            a = a[None]
        # wct_eigh takes the UPPER triangle as authoritative and mirrors it into the lower one on its staged copy
        # (include/wct_hip.h), so it needs no symmetric input.  The default solves (a + a^T) / 2, the matrix a NumPy caller
        # means by a nearly symmetric `a`; it leaves a symmetric input unchanged.
        if symmetrize:
            a = 0.5 * (a + a.transpose(0, 2, 1))
        a = np.ascontiguousarray(a, np.float32)
        n, c, _ = a.shape
        evals = np.empty((n, c), np.float32)
        evecs = np.empty((n, c, c), np.float32)
        sweeps = (C.c_int * n)()
        self.last_sweeps = sweeps
        check(self.lib.wct_eigh(self.h, fptr(a), c, n, fptr(evals), fptr(evecs), sweeps))
        return (evals, evecs, list(sweeps)) if return_sweeps else (evals, evecs)

    def conv3x3(self, x, w_hwio, bias, relu=True, upsample=False):
        x = f32(x)
        w = f32(w_hwio)
        b = f32(bias)
        h, wd, cin = x.shape
        cout = w.shape[3]
        s = 2 if upsample else 1
        y = np.empty((h * s, wd * s, cout), np.float32)
        check(self.lib.wct_conv3x3(self.h, fptr(x), h, wd, cin, fptr(w), fptr(b), cout, int(relu), int(upsample), fptr(y)))
        return y

    def conv3x3_f16(self, x, w_hwio, bias, relu=True, upsample=False, pool=False, algo=0):
        """One 3x3 layer as the stylize pipeline runs it (fp16 activations out, optional fused 'same' max-pool) on a batch
        x [B][H][W][Cin] (or [H][W][Cin]); algo 0 = the pipeline's kernel for this shape, 1 = direct, 2 = Winograd F(2,3)."""
        x = f32(x)
        single = x.ndim == 3
        if single:
            x = x[None]
        w = f32(w_hwio)
        b = f32(bias)
        n, h, wd, cin = x.shape
        cout = w.shape[3]
        s = 2 if upsample else 1
        ho, wo = h * s, wd * s
        if pool:
            ho, wo = (ho + 1) // 2, (wo + 1) // 2
        y = np.empty((n, ho, wo, cout), np.float32)
        check(self.lib.wct_conv3x3_f16(self.h, fptr(x), n, h, wd, cin, fptr(w), fptr(b), cout, int(relu), int(upsample), int(pool),
                                       int(algo), fptr(y)))
        return y[0] if single else y

    def maxpool(self, x):
        x = f32(x)
        h, w, c = x.shape
        y = np.empty(((h + 1) // 2, (w + 1) // 2, c), np.float32)
        check(self.lib.wct_maxpool(self.h, fptr(x), h, w, c, fptr(y)))
        return y

    def encode(self, img01, relu_target):
        level = _levels([relu_target])[0]
        x = f32(img01)
        h, w, _ = x.shape
        hh, ww = h, w
        for _ in range(level - 1):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
        feat = np.empty((hh, ww, _LEVEL_C[level]), np.float32)
        check(self.lib.wct_encode(self.h, fptr(x), h, w, level, fptr(feat)))
        return feat

    def decode(self, feat, relu_target):
        level = _levels([relu_target])[0]
        f = f32(feat)
        h, w, _ = f.shape
        s = 1 << (level - 1)
        img = np.empty((h * s, w * s, 3), np.float32)
        check(self.lib.wct_decode(self.h, fptr(f), h, w, level, fptr(img)))
        return img

    def encode_banded(self, img01, relu_target, band_rows=0):
        """encode() band by band (wct_encode_banded; band_rows 0: automatic): the same map, bit for bit, and maps past its limit"""
        level = _levels([relu_target])[0]
        x = f32(img01)
        h, w, _ = x.shape
        hh, ww = h, w
        for _ in range(level - 1):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
        feat = np.empty((hh, ww, _LEVEL_C[level]), np.float32)
        check(self.lib.wct_encode_banded(self.h, fptr(x), h, w, level, int(band_rows), fptr(feat)))
        return feat

    def decode_banded(self, feat, relu_target, band_rows=0):
        """decode() band by band (wct_decode_banded; band_rows 0: automatic): the same image, bit for bit"""
        level = _levels([relu_target])[0]
        f = f32(feat)
        h, w, _ = f.shape
        s = 1 << (level - 1)
        img = np.empty((h * s, w * s, 3), np.float32)
        check(self.lib.wct_decode_banded(self.h, fptr(f), h, w, level, int(band_rows), fptr(img)))
        return img

    # ---- wrap-around halos: the periodic network on the unchanged kernels ------------------------
    def wrap_halo(self, relu_target):
        """The wrap-around halo of one level as (enc, dec_before, dec_after) (wrap_halo)"""
        return wrap_halo(relu_target)

    def wrap_pad_batch_dev(self, in_dev, batch, h, w, c, pads, out_dev):
        """`batch` fp32 maps [batch][h][w][c] resident in HBM extended periodically by pads = (top, bottom, left, right) into out_dev
        (wct_wrap_pad_batch_dev): one launch, asynchronous."""
        t, b, l, r = (int(v) for v in pads)
        check(self.lib.wct_wrap_pad_batch_dev(self.h, in_dev, int(batch), int(h), int(w), int(c), t, b, l, r, out_dev))

    def wrap_pad(self, x, pads):
        """x [H][W][C] fp32 -> np.pad(x, ((top, bottom), (left, right), (0, 0)), mode='wrap') for pads = (top, bottom, left,
        right), on the device (wct_wrap_pad): the kernel of the wrap calls alone."""
        a = f32(x)
        if a.ndim != 3 or a.size == 0:
            raise ValueError('wrap_pad takes an HxWxC map, got shape %s' % (a.shape,))
        t, b, l, r = (int(v) for v in pads)
        if min(t, b, l, r) < 0:
            raise ValueError('pads must be >= 0, got %r' % (pads,))
        h, w, c = a.shape
        y = np.empty((t + h + b, l + w + r, c), np.float32)
        check(self.lib.wct_wrap_pad(self.h, fptr(a), h, w, c, t, b, l, r, fptr(y)))
        return y

    def encode_wrap(self, img01, relu_target):
        """encode() on a torus (wct_encode_wrap): the map of the image extended periodically by the level's halo, its interior
        kept -- encode(np.pad(img01, halo, mode='wrap')) cropped, bit for bit.  H and W multiples of the level's stride."""
        level = _levels([relu_target])[0]
        x = f32(img01)
        h, w, _ = x.shape
        check_wrap(h, w, [level])
        s = 1 << (level - 1)
        feat = np.empty((h // s, w // s, _LEVEL_C[level]), np.float32)
        check(self.lib.wct_encode_wrap(self.h, fptr(x), h, w, level, fptr(feat)))
        return feat

    def decode_wrap(self, feat, relu_target):
        """decode() on a torus (wct_decode_wrap): the image of the map extended periodically by the level's halo, its interior kept"""
        level = _levels([relu_target])[0]
        f = f32(feat)
        h, w, _ = f.shape
        s = 1 << (level - 1)
        img = np.empty((h * s, w * s, 3), np.float32)
        check(self.lib.wct_decode_wrap(self.h, fptr(f), h, w, level, fptr(img)))
        return img

    def transform_chunked(self, content, style, alpha, mode, chunk_rows, eps=-1.0, return_sweeps=False):
        """transform() with the content statistics pooled over chunks of chunk_rows rows (wct_transform_chunked); 0, or at
        least the content's rows: one chunk, transform()'s output bit for bit"""
        c = f32(content)
        s = f32(style)
        if c.ndim != 2 or s.ndim != 2 or c.shape[1] != s.shape[1]:
            raise ValueError('expected [N][C] feature matrices with equal C')
        out = np.empty_like(c)
        sweeps = (C.c_int * 2)()
        self.last_sweeps = sweeps
        check(self.lib.wct_transform_chunked(self.h, fptr(c), c.shape[0], fptr(s), s.shape[0], c.shape[1], float(alpha), int(mode),
                                             float(eps), int(chunk_rows), fptr(out), sweeps))
        return (out, list(sweeps)) if return_sweeps else out

    def coral_stats(self, img_u8):
        a = u8(img_u8)
        sums = (C.c_double * 9)()
        check(self.lib.wct_coral_stats(self.h, a.ctypes.data_as(_lib._U8), a.shape[0], a.shape[1], sums))
        return np.array(list(sums), np.float64)

    def coral_apply(self, src_u8, m, src_mean, src_std, tgt_mean, tgt_std, want_f64=True, want_u8=True):
        a = u8(src_u8)
        h, w, _ = a.shape
        dd = lambda v: np.ascontiguousarray(v, np.float64).ctypes.data_as(_lib._D)
        arrs = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (m, src_mean, src_std, tgt_mean, tgt_std)]
        out8 = np.empty((h, w, 3), np.uint8) if want_u8 else None
        out64 = np.empty((h, w, 3), np.float64) if want_f64 else None
        check(self.lib.wct_coral_apply(
            self.h, a.ctypes.data_as(_lib._U8), h, w, *[x.ctypes.data_as(_lib._D) for x in arrs],
            out8.ctypes.data_as(_lib._U8) if want_u8 else None,
            out64.ctypes.data_as(_lib._D) if want_f64 else None))
        return out8, out64

    def content_colors(self, stylized_u8, content_u8):
        """Luminance-only colour preservation (wct_content_colors): stylized [Ho][Wo][3] and content [Hc][Wc][3] uint8, Ho >= Hc
        and Wo >= Wc -> uint8 [Ho][Wo][3], the luminance of `stylized` on the colours of `content` (pixel (y, x) takes content
        pixel (min(y, Hc - 1), min(x, Wc - 1)))."""
        s, c = _color_images(stylized_u8, content_u8, 3)
        out = np.empty_like(s)
        check(self.lib.wct_content_colors(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], c.ctypes.data_as(_lib._U8),
                                          c.shape[0], c.shape[1], out.ctypes.data_as(_lib._U8)))
        return out

    def content_colors_batch_dev(self, stylized_dev, ho, wo, content_dev, hc, wc, batch, out_dev):
        """content_colors for B frames resident in HBM (wct_content_colors_batch_dev): asynchronous; out_dev may be stylized_dev."""
        check(self.lib.wct_content_colors_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc), int(batch),
                                                    out_dev))

    def content_colors_batch(self, stylized_u8, contents_u8):
        """Host arrays in, host array out: stylized [B][Ho][Wo][3] and contents [B][Hc][Wc][3] uint8 (B <= 32) -> [B][Ho][Wo][3]."""
        s, c = _color_images(stylized_u8, contents_u8, 4)
        if s.shape[0] != c.shape[0] or not 1 <= s.shape[0] <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames and as many contents, got %d and %d' % (_lib.BATCH_MAX, s.shape[0], c.shape[0]))
        return self._host_batch([s, c], np.empty_like(s), in_place=True, enqueue=lambda ds, dc: self.content_colors_batch_dev(
            ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], ds))

    # ---- guided smoothing: the photo mode ---------------------------------------------------
    def set_guided(self, radius, eps_q):
        """The radius and eps_q that WCT_FLAG_GUIDED filters with (wct_set_guided)"""
        r, e = check_guided((radius, eps_q))
        check(self.lib.wct_set_guided(self.h, r, e))

    def set_guided_guide(self, guide):
        """The guide that WCT_FLAG_GUIDED filters through, 'grey' (the initial one) or 'color' (wct_set_guided_guide)"""
        g = check_guide(guide)
        check(self.lib.wct_set_guided_guide(self.h, g))

    def _set_guided(self, guided):
        """guided=(radius, eps_q[, guide]) of a stylize call: None -> False; else the settings go to the library -> True (the flag).
        The two-element form means the grey guide."""
        if guided is None:
            return False
        g = check_guided(guided)
        self.set_guided(g[0], g[1])
        self.set_guided_guide(g[2] if len(g) == 3 else 'grey')
        return True

    def guided_filter(self, stylized_u8, content_u8, radius, eps_q, guide='grey'):
        """Guided smoothing (wct_guided_filter_guide; He, Sun, Tang, "Guided Image Filtering"): stylized [Ho][Wo][3] and content
        [Hc][Wc][3] uint8, Ho >= Hc and Wo >= Wc -> uint8 [Ho][Wo][3], `stylized` filtered with `content` as guide (pixel (y, x)
        takes content pixel (min(y, Hc - 1), min(x, Wc - 1))) over a (2 radius + 1)^2 box; eps_q in grey levels squared.  guide:
        'grey', the grey of the content, or 'color', its three channels (a 3 x 3 solve per pixel, which sees an edge between two
        colours of equal luminance).  The integer rules of include/wct_hip.h."""
        s, c = _guided_images(stylized_u8, content_u8, 3)
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        out = np.empty_like(s)
        check(self.lib.wct_guided_filter_guide(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], c.ctypes.data_as(_lib._U8),
                                               c.shape[0], c.shape[1], r, e, g, out.ctypes.data_as(_lib._U8)))
        return out

    def guided_filter_batch_dev(self, stylized_dev, ho, wo, content_dev, hc, wc, batch, radius, eps_q, out_dev, guide='grey'):
        """guided_filter for B frames resident in HBM (wct_guided_filter_guide_batch_dev): asynchronous; out_dev may be stylized_dev."""
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        check(self.lib.wct_guided_filter_guide_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc), int(batch),
                                                         r, e, g, out_dev))

    def guided_filter_batch(self, stylized_u8, contents_u8, radius, eps_q, guide='grey'):
        """Host arrays in, host array out: stylized [B][Ho][Wo][3] and contents [B][Hc][Wc][3] uint8 (B <= 32) -> [B][Ho][Wo][3]."""
        s, c = _guided_images(stylized_u8, contents_u8, 4)
        r, e = check_guided((radius, eps_q))
        check_guide(guide)
        if s.shape[0] != c.shape[0] or not 1 <= s.shape[0] <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames and as many contents, got %d and %d' % (_lib.BATCH_MAX, s.shape[0], c.shape[0]))
        return self._host_batch([s, c], np.empty_like(s), in_place=True, enqueue=lambda ds, dc: self.guided_filter_batch_dev(
            ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r, e, ds, guide=guide))

    # ---- guided upsampling: a small frame delivered at the full content's size ----------------
    def guided_upsample(self, stylized_u8, content_small_u8, content_full_u8, radius, eps_q, guide='grey'):
        """Guided upsampling (wct_guided_upsample_guide; He, Sun, "Fast Guided Filter"): the small stylized frame [h][w][3], the small
        content [hc][wc][3] it was made from (hc <= h, wc <= w) and the full content [H][W][3] (H >= hc, W >= wc), all uint8 ->
        uint8 [H][W][3]: the guided filter's coefficients of the small pair, interpolated and evaluated against the full content.
        radius and eps_q as in guided_filter, in pixels of the small frame.  guide: 'grey', the grey of the contents, or 'color',
        their three channels (which brings back an edge between two colours of equal luminance).  The integer rules of
        include/wct_hip.h."""
        s, c, f = _upsample_images(stylized_u8, content_small_u8, content_full_u8, 3)
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        out = np.empty_like(f)
        check(self.lib.wct_guided_upsample_guide(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], c.ctypes.data_as(_lib._U8),
                                                 c.shape[0], c.shape[1], f.ctypes.data_as(_lib._U8), f.shape[0], f.shape[1], r, e, g,
                                                 out.ctypes.data_as(_lib._U8)))
        return out

    def guided_upsample_batch_dev(self, stylized_dev, h, w, content_small_dev, hc, wc, content_full_dev, hf, wf, batch, radius, eps_q,
                                  out_dev, guide='grey'):
        """guided_upsample for B frames resident in HBM (wct_guided_upsample_guide_batch_dev): asynchronous; out_dev overlaps no
        input."""
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        check(self.lib.wct_guided_upsample_guide_batch_dev(self.h, stylized_dev, int(h), int(w), content_small_dev, int(hc), int(wc),
                                                           content_full_dev, int(hf), int(wf), int(batch), r, e, g, out_dev))

    def guided_upsample_batch(self, stylized_u8, contents_small_u8, contents_full_u8, radius, eps_q, guide='grey'):
        """Host arrays in, host array out: [B][h][w][3], [B][hc][wc][3] and [B][H][W][3] uint8 (B <= 32) -> [B][H][W][3]."""
        s, c, f = _upsample_images(stylized_u8, contents_small_u8, contents_full_u8, 4)
        r, e = check_guided((radius, eps_q))
        check_guide(guide)
        return self._host_batch([s, c, f], np.empty_like(f), enqueue=lambda ds, dc, df, do: self.guided_upsample_batch_dev(
            ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], df, f.shape[1], f.shape[2], s.shape[0], r, e, do, guide=guide))

    def stylize_prepared_upsampled(self, content, style, relu_targets, work_size, radius, eps_q, alpha=1.0, adain=False, wct_mode='tf',
                                   content_colors=False, guide='grey'):
        """Stylize small, deliver at the content's size (wct_stylize_prepared_upsampled_guide): the uint8 content [H][W][3] is resized
        on the device to work_size (hc, wc), stylized with the PreparedStyle, upsampled against the full content (guided_upsample with
        radius, eps_q and guide) and, with content_colors, recoloured at full size -> uint8 [H][W][3], the composition of resize,
        stylize_prepared, guided_upsample and content_colors bit for bit.  work_size equal to the content's size skips the resize."""
        check_prepared(self, [style], relu_targets)
        c = np.asarray(content)
        if c.dtype != np.uint8 or c.ndim != 3 or c.shape[-1] != 3 or c.size == 0:
            raise ValueError('stylize_prepared_upsampled takes a uint8 HxWx3 content, got %s %s' % (c.dtype, c.shape))
        c = u8(c)
        hc, wc = check_work_size(work_size, c.shape[0], c.shape[1])
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        lv = _levels(relu_targets)
        out = np.empty_like(c)
        check(self.lib.wct_stylize_prepared_upsampled_guide(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], hc, wc, style.h,
                                                            (C.c_int * len(lv))(*lv), len(lv), float(alpha),
                                                            _flags(adain, wct_mode, content_colors=content_colors), r, e, g,
                                                            out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_upsampled_batch_dev(self, content_dev, hf, wf, batch, work_size, style, relu_targets, radius, eps_q, alpha, out_dev,
                                             adain=False, wct_mode='tf', content_colors=False, guide='grey'):
        """stylize_prepared_upsampled for B full contents [B][H][W][3] resident in HBM -> out_dev [B][H][W][3]; asynchronous
        (wct_stylize_prepared_upsampled_guide_batch_dev)."""
        lv = check_prepared(self, [style], relu_targets)
        hc, wc = check_work_size(work_size, hf, wf)
        r, e = check_guided((radius, eps_q))
        g = check_guide(guide)
        check(self.lib.wct_stylize_prepared_upsampled_guide_batch_dev(self.h, content_dev, int(hf), int(wf), int(batch), hc, wc, style.h,
                                                                      (C.c_int * len(lv))(*lv), len(lv), float(alpha),
                                                                      _flags(adain, wct_mode, content_colors=content_colors), r, e, g,
                                                                      out_dev))

    def stylize_prepared_upsampled_batch(self, contents_u8, style, relu_targets, work_size, radius, eps_q, alpha=1.0, adain=False,
                                         wct_mode='tf', content_colors=False, guide='grey'):
        """Host arrays in, host array out: full contents [B][H][W][3] uint8 (B <= 32) -> [B][H][W][3] uint8."""
        check_prepared(self, [style], relu_targets)
        _, _, c = check_resize((1, 1), contents_u8)
        hc, wc = check_work_size(work_size, c.shape[1], c.shape[2])
        check_guided((radius, eps_q))
        check_guide(guide)
        return self._host_batch([c], np.empty_like(c), enqueue=lambda dc, do: self.stylize_prepared_upsampled_batch_dev(
            dc, c.shape[1], c.shape[2], c.shape[0], (hc, wc), style, relu_targets, radius, eps_q, alpha, do, adain=adain,
            wct_mode=wct_mode, content_colors=content_colors, guide=guide))

    # ---- temporal guided smoothing: the filter's box across frames --------------------------
    def guided_filter_time(self, stylized_u8, contents_u8, radius, eps_q, frames_t, positions=None, guide='grey'):
        """Temporal guided smoothing of a clip (wct_guided_filter_time): stylized [F][Ho][Wo][3] and contents [F][Hc][Wc][3] uint8,
        F <= 32 -> uint8 [F][Ho][Wo][3], the grey-guide filter of guided_filter with its box extended over the frames_t (0 .. 3)
        frames on each side of a frame, cut at the clip's ends.  frames_t = 0 is guided_filter_batch.  The radius is at most
        64 / 51 / 40 / 33 at frames_t 0 / 1 / 2 / 3.  A longer clip: ops.guided_filter_time_np.
        positions: int [F][2] (py, px), one global translation per frame (motion_global estimates them) -- the window in every
        neighbouring frame is shifted by the difference of the positions (wct_guided_filter_motion); None: no shift.
        guide: 'grey', or 'color' -- the three content channels as guide along time, with or without positions
        (wct_guided_filter_time_guide), which keeps an edge between two colours of equal luminance."""
        s, c = _guided_clip(stylized_u8, contents_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        g = check_guide(guide)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        if not 1 <= s.shape[0] <= _lib.BATCH_MAX:
            raise ValueError('a clip takes 1 .. %d frames in one call, got %d (ops.guided_filter_time_np takes any length)'
                             % (_lib.BATCH_MAX, s.shape[0]))
        out = np.empty_like(s)
        if g != _lib.GUIDE_GREY:
            check(self.lib.wct_guided_filter_time_guide(self.h, s.ctypes.data_as(_lib._U8), s.shape[1], s.shape[2],
                                                        c.ctypes.data_as(_lib._U8), c.shape[1], c.shape[2], s.shape[0], r, e, t, g,
                                                        None if pos is None else pos.ctypes.data_as(_lib._I),
                                                        out.ctypes.data_as(_lib._U8)))
            return out
        if pos is not None:
            check(self.lib.wct_guided_filter_motion(self.h, s.ctypes.data_as(_lib._U8), s.shape[1], s.shape[2], c.ctypes.data_as(_lib._U8),
                                                    c.shape[1], c.shape[2], s.shape[0], r, e, t, pos.ctypes.data_as(_lib._I),
                                                    out.ctypes.data_as(_lib._U8)))
            return out
        check(self.lib.wct_guided_filter_time(self.h, s.ctypes.data_as(_lib._U8), s.shape[1], s.shape[2], c.ctypes.data_as(_lib._U8),
                                              c.shape[1], c.shape[2], s.shape[0], r, e, t, out.ctypes.data_as(_lib._U8)))
        return out

    def guided_filter_time_batch_dev(self, stylized_dev, ho, wo, content_dev, hc, wc, frames, radius, eps_q, frames_t, f0, f1, out_dev,
                                     guide='grey'):
        """Frames f0 .. f1 - 1 of the clip of `frames` frames resident in HBM, filtered along time as a clip of its own
        (wct_guided_filter_time_batch_dev) -> out_dev [f1 - f0][ho][wo][3]: asynchronous; out_dev may be the address of frame f0 of
        stylized_dev.  The bytes of a longer video need 2 frames_t real frames of halo on each side of [f0, f1).  guide 'color':
        the colour guide along time (wct_guided_filter_time_guide_batch_dev with null positions)."""
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        g = check_guide(guide)
        if not (1 <= int(frames) <= _lib.BATCH_MAX and 0 <= int(f0) < int(f1) <= int(frames)):
            raise ValueError('a clip takes 1 .. %d frames and a range 0 <= f0 < f1 <= frames, got %d frames and [%d, %d)'
                             % (_lib.BATCH_MAX, frames, f0, f1))
        if g != _lib.GUIDE_GREY:
            check(self.lib.wct_guided_filter_time_guide_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc),
                                                                  int(frames), r, e, t, g, None, int(f0), int(f1), out_dev))
            return
        check(self.lib.wct_guided_filter_time_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc), int(frames),
                                                        r, e, t, int(f0), int(f1), out_dev))

    def guided_filter_motion_batch_dev(self, stylized_dev, ho, wo, content_dev, hc, wc, frames, radius, eps_q, frames_t, positions, f0, f1,
                                       out_dev, guide='grey'):
        """guided_filter_time_batch_dev with positions int [frames][2] (host): the window of every neighbouring frame shifted by
        the difference of the positions (wct_guided_filter_motion_batch_dev).  Asynchronous; the same aliasing and halo.  guide
        'color': the colour guide along motion (wct_guided_filter_time_guide_batch_dev with these positions)."""
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        g = check_guide(guide)
        if not (1 <= int(frames) <= _lib.BATCH_MAX and 0 <= int(f0) < int(f1) <= int(frames)):
            raise ValueError('a clip takes 1 .. %d frames and a range 0 <= f0 < f1 <= frames, got %d frames and [%d, %d)'
                             % (_lib.BATCH_MAX, frames, f0, f1))
        pos = check_guided_motion(positions, frames)
        if g != _lib.GUIDE_GREY:
            check(self.lib.wct_guided_filter_time_guide_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc),
                                                                  int(frames), r, e, t, g, pos.ctypes.data_as(_lib._I), int(f0), int(f1),
                                                                  out_dev))
            return
        check(self.lib.wct_guided_filter_motion_batch_dev(self.h, stylized_dev, int(ho), int(wo), content_dev, int(hc), int(wc), int(frames),
                                                          r, e, t, pos.ctypes.data_as(_lib._I), int(f0), int(f1), out_dev))

    def motion_global_batch_dev(self, content_dev, hc, wc, frames, search=8):
        """The positions of `frames` contents resident in HBM (wct_motion_global_batch_dev) -> int32 [frames][2]: three launches,
        then it blocks on the result."""
        r = check_motion_search(search, int(hc), int(wc))
        if not 1 <= int(frames) <= _lib.BATCH_MAX:
            raise ValueError('motion estimation takes 1 .. %d frames in one call, got %d' % (_lib.BATCH_MAX, frames))
        pos = np.zeros((int(frames), 2), np.int32)
        check(self.lib.wct_motion_global_batch_dev(self.h, content_dev, int(hc), int(wc), int(frames), r, pos.ctypes.data_as(_lib._I)))
        return pos

    def motion_global(self, contents_u8, search=8):
        """One global integer translation per frame of a clip, from its contents [F][Hc][Wc][3] uint8 of any F (wct_motion_global):
        for every pair of consecutive frames the step (dy, dx), |dy|, |dx| <= search, with the smallest mean absolute difference of
        the grey guides over the even pixels (ties: the smallest step), summed up from (0, 0) -> int32 [F][2], what positions= of
        guided_filter_time takes.  A longer clip goes in chunks of 32 frames that share one frame.  A scene cut yields an
        arbitrary step."""
        c = np.ascontiguousarray(contents_u8)
        if c.dtype != np.uint8 or c.ndim != 4 or c.shape[3] != 3 or c.shape[0] < 1:
            raise ValueError('motion_global takes uint8 contents [F][H][W][3], got %s %s' % (c.dtype, c.shape))
        r = check_motion_search(search, c.shape[1], c.shape[2])
        pos = np.zeros((c.shape[0], 2), np.int32)
        for f0 in range(0, max(1, c.shape[0] - 1), _lib.BATCH_MAX - 1):
            part = np.ascontiguousarray(c[f0:f0 + _lib.BATCH_MAX])
            got = np.zeros((part.shape[0], 2), np.int32)
            check(self.lib.wct_motion_global(self.h, part.ctypes.data_as(_lib._U8), c.shape[1], c.shape[2], part.shape[0], r,
                                             got.ctypes.data_as(_lib._I)))
            pos[f0:f0 + part.shape[0]] = got + pos[f0]
        return pos

    def guided_time_max_radius(self, frames_t):
        """The largest radius of temporal guided smoothing with frames_t frames on each side (wct_guided_time_max_radius): the
        entries of _lib.GUIDED_TIME_MAX_RADIUS; 0 for a frames_t outside 0 .. 3"""
        return int(self.lib.wct_guided_time_max_radius(int(frames_t)))

    def guided_filter_time_clip(self, stylized_u8, contents_u8, radius, eps_q, frames_t, positions=None, guide='grey'):
        """guided_filter_time for a clip of any length: chunks of at most 32 - 4 frames_t output frames, each uploaded with
        2 frames_t frames of halo on each side (fewer at the clip's ends) and filtered as a clip of its own -- the whole clip's
        bytes, since a frame depends on no frame further than 2 frames_t away.  positions [F][2]: sliced with every chunk (only
        their differences count).  guide: as in guided_filter_time."""
        s, c = _guided_clip(stylized_u8, contents_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        check_guide(guide)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        n, step, out = s.shape[0], _lib.BATCH_MAX - 4 * t, np.empty_like(s)
        for f0 in range(0, n, step):
            f1 = min(n, f0 + step)
            g0, g1 = max(0, f0 - 2 * t), min(n, f1 + 2 * t)
            self.guided_filter_time_range(s[g0:g1], c[g0:g1], r, e, t, f0 - g0, f1 - g0, out=out[f0:f1],
                                          positions=None if pos is None else pos[g0:g1], guide=guide)
        return out

    def guided_filter_time_range(self, stylized_u8, contents_u8, radius, eps_q, frames_t, f0, f1, out=None, positions=None, guide='grey'):
        """Host arrays in, host array out: frames f0 .. f1 - 1 of the clip stylized [F][Ho][Wo][3] with contents [F][Hc][Wc][3]
        (F <= 32), filtered along time as guided_filter_time_batch_dev does (with positions [F][2]: as
        guided_filter_motion_batch_dev does) -> uint8 [f1 - f0][Ho][Wo][3].  guide: as in guided_filter_time."""
        s, c = _guided_clip(stylized_u8, contents_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        check_guide(guide)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        if not (1 <= s.shape[0] <= _lib.BATCH_MAX and 0 <= f0 < f1 <= s.shape[0]):
            raise ValueError('a clip takes 1 .. %d frames and a range 0 <= f0 < f1 <= frames, got %d frames and [%d, %d)'
                             % (_lib.BATCH_MAX, s.shape[0], f0, f1))
        out = np.empty((f1 - f0,) + s.shape[1:], np.uint8) if out is None else out
        if pos is not None:
            return self._host_batch([s, c], out, enqueue=lambda ds, dc, do: self.guided_filter_motion_batch_dev(
                ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r, e, t, pos, f0, f1, do, guide=guide))
        return self._host_batch([s, c], out, enqueue=lambda ds, dc, do: self.guided_filter_time_batch_dev(
            ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], s.shape[0], r, e, t, f0, f1, do, guide=guide))

    # ---- temporal guided upsampling: the box across frames, delivered at full size -----------
    def guided_upsample_time(self, stylized_u8, contents_small_u8, contents_full_u8, radius, eps_q, frames_t, positions=None):
        """Temporal guided upsampling of a clip (wct_guided_upsample_time): small stylized frames [F][h][w][3], the small contents
        [F][hc][wc][3] they were made from and the full contents [F][H][W][3], all uint8, F <= 32 -> uint8 [F][H][W][3]:
        guided_upsample with its coefficients and their means formed over the frames_t (0 .. 3) frames on each side of a frame as
        guided_filter_time forms them; frame f is then delivered against its own full content.  frames_t = 0, or one frame, is
        guided_upsample_batch bit for bit.  The radius is at most 64 / 51 / 40 / 33 at frames_t 0 / 1 / 2 / 3.  The grey guide.
        positions: int [F][2] (py, px) in pixels of the SMALL frame, as in guided_filter_time; None: no shift.  A longer clip:
        guided_upsample_time_clip."""
        s, c, f = _upsample_time_clip(stylized_u8, contents_small_u8, contents_full_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        if not 1 <= s.shape[0] <= _lib.BATCH_MAX:
            raise ValueError('a clip takes 1 .. %d frames in one call, got %d (guided_upsample_time_clip takes any length)'
                             % (_lib.BATCH_MAX, s.shape[0]))
        out = np.empty_like(f)
        check(self.lib.wct_guided_upsample_time(self.h, s.ctypes.data_as(_lib._U8), s.shape[1], s.shape[2], c.ctypes.data_as(_lib._U8),
                                                c.shape[1], c.shape[2], f.ctypes.data_as(_lib._U8), f.shape[1], f.shape[2], s.shape[0],
                                                r, e, t, None if pos is None else pos.ctypes.data_as(_lib._I),
                                                out.ctypes.data_as(_lib._U8)))
        return out

    def guided_upsample_time_batch_dev(self, stylized_dev, h, w, content_small_dev, hc, wc, content_full_dev, hf, wf, frames, radius, eps_q,
                                       frames_t, f0, f1, out_dev, positions=None):
        """Frames f0 .. f1 - 1 of the clip of `frames` SMALL frames resident in HBM, delivered at full size
        (wct_guided_upsample_time_batch_dev): content_full_dev [f1 - f0][hf][wf][3] holds the full contents of the delivered frames
        only -> out_dev [f1 - f0][hf][wf][3].  Asynchronous; out_dev overlaps no input.  positions: int [frames][2] (host) or None.
        The bytes of a longer video need 2 frames_t real small frames of halo on each side of [f0, f1)."""
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        if not (1 <= int(frames) <= _lib.BATCH_MAX and 0 <= int(f0) < int(f1) <= int(frames)):
            raise ValueError('a clip takes 1 .. %d frames and a range 0 <= f0 < f1 <= frames, got %d frames and [%d, %d)'
                             % (_lib.BATCH_MAX, frames, f0, f1))
        pos = None if positions is None else check_guided_motion(positions, frames)
        check(self.lib.wct_guided_upsample_time_batch_dev(self.h, stylized_dev, int(h), int(w), content_small_dev, int(hc), int(wc),
                                                          content_full_dev, int(hf), int(wf), int(frames), r, e, t,
                                                          None if pos is None else pos.ctypes.data_as(_lib._I), int(f0), int(f1), out_dev))

    def guided_upsample_time_range(self, stylized_u8, contents_small_u8, contents_full_u8, radius, eps_q, frames_t, f0, f1, out=None,
                                   positions=None):
        """Host arrays in, host array out: frames f0 .. f1 - 1 of the clip of small frames [F][h][w][3] with small contents
        [F][hc][wc][3] (F <= 32), delivered against contents_full [f1 - f0][H][W][3], the full contents of those frames only ->
        uint8 [f1 - f0][H][W][3]"""
        s, c = _guided_clip(stylized_u8, contents_small_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        if not (1 <= s.shape[0] <= _lib.BATCH_MAX and 0 <= f0 < f1 <= s.shape[0]):
            raise ValueError('a clip takes 1 .. %d frames and a range 0 <= f0 < f1 <= frames, got %d frames and [%d, %d)'
                             % (_lib.BATCH_MAX, s.shape[0], f0, f1))
        f = _upsample_time_full(contents_full_u8, f1 - f0, c)
        out = np.empty_like(f) if out is None else out
        return self._host_batch([s, c, f], out, enqueue=lambda ds, dc, df, do: self.guided_upsample_time_batch_dev(
            ds, s.shape[1], s.shape[2], dc, c.shape[1], c.shape[2], df, f.shape[1], f.shape[2], s.shape[0], r, e, t, f0, f1, do,
            positions=pos))

    def guided_upsample_time_clip(self, stylized_u8, contents_small_u8, contents_full_u8, radius, eps_q, frames_t, positions=None):
        """guided_upsample_time for a clip of any length: chunks of at most 32 - 4 frames_t delivered frames -- fewer where that many
        full frames would reach 2^31 bytes --, each uploaded with 2 frames_t SMALL frames of halo on each side (fewer at the clip's
        ends) and the full contents of its own frames only.  The whole clip's bytes, whatever the chunking: a frame depends on no
        small frame further than 2 frames_t away and on its own full content."""
        s, c, f = _upsample_time_clip(stylized_u8, contents_small_u8, contents_full_u8)
        r, e, t = check_guided_time(radius, eps_q, frames_t)
        pos = None if positions is None else check_guided_motion(positions, s.shape[0])
        step = upsample_time_chunk(f.shape[1], f.shape[2], t)
        n, out = s.shape[0], np.empty_like(f)
        for f0 in range(0, n, step):
            f1 = min(n, f0 + step)
            g0, g1 = max(0, f0 - 2 * t), min(n, f1 + 2 * t)
            self.guided_upsample_time_range(s[g0:g1], c[g0:g1], f[f0:f1], r, e, t, f0 - g0, f1 - g0, out=out[f0:f1],
                                            positions=None if pos is None else pos[g0:g1])
        return out

    # ---- on-device resize: Pillow's bilinear bytes ------------------------------------------
    def resize(self, img_u8, size):
        """img [H][W][3] uint8 -> uint8 [h][w][3] for size = (h, w) (wct_resize; the integer rule of include/wct_hip.h): the bytes
        of Image.fromarray(img).resize((w, h), Image.BILINEAR), i.e. of utils._imresize."""
        h, w, a = check_resize(size, img_u8, ndim=3)
        out = np.empty((h, w, 3), np.uint8)
        check(self.lib.wct_resize(self.h, a.ctypes.data_as(_lib._U8), a.shape[0], a.shape[1], h, w, out.ctypes.data_as(_lib._U8)))
        return out

    def resize_batch_dev(self, in_dev, hi, wi, batch, size, out_dev):
        """`batch` frames [batch][hi][wi][3] resident in HBM -> [batch][h][w][3] at out_dev (wct_resize_batch_dev): one launch,
        asynchronous; out_dev must not overlap in_dev."""
        h, w = check_resize(size)
        if not 1 <= int(batch) <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, batch))
        check(self.lib.wct_resize_batch_dev(self.h, in_dev, int(hi), int(wi), int(batch), h, w, out_dev))

    def resize_batch(self, frames_u8, size):
        """Host arrays in, host array out: frames [B][H][W][3] uint8 (B <= 32) -> [B][h][w][3]; frame f is resize(frames[f], size)."""
        h, w, a = check_resize(size, frames_u8)
        out = np.empty((a.shape[0], h, w, 3), np.uint8)
        return self._host_batch([a], out, lambda di, do: self.resize_batch_dev(di, a.shape[1], a.shape[2], a.shape[0], (h, w), do))

    # ---- texture synthesis: seeded noise on the device, the passes chained there -----
    def texture_noise(self, h, w, seed, sample=0, smooth=False):
        """The noise image `sample` of `seed` (wct_texture_noise; the integer rule of include/wct_hip.h) -> uint8 [h][w][3].
        smooth: the rule's 27 202 27 filter along y and x (stylize.py:95-97); off is webcam.py:192's plain noise."""
        h, w = check_texture((h, w), seed=seed, first_sample=sample)
        out = np.empty((h, w, 3), np.uint8)
        check(self.lib.wct_texture_noise(self.h, h, w, int(seed), int(sample), int(bool(smooth)), out.ctypes.data_as(_lib._U8)))
        return out

    def texture_noise_batch_dev(self, h, w, batch, seed, first_sample, smooth, out_dev):
        """`batch` noise images [batch][h][w][3] into device memory at any byte address (wct_texture_noise_batch_dev): image b is
        sample first_sample + b.  One launch, asynchronous."""
        h, w = check_texture((h, w), batch=batch, seed=seed, first_sample=first_sample)
        check(self.lib.wct_texture_noise_batch_dev(self.h, h, w, int(batch), int(seed), int(first_sample), int(bool(smooth)), out_dev))

    def texture_size(self, h, w, relu_targets, passes=1):
        """The frame size of a texture from h x w noise after `passes` passes (wct_texture_size)."""
        lv = _levels(relu_targets)
        ho, wo = C.c_int(), C.c_int()
        check(self.lib.wct_texture_size(int(h), int(w), (C.c_int * len(lv))(*lv), len(lv), int(passes), C.byref(ho), C.byref(wo)))
        return ho.value, wo.value

    def texture_prepared_batch_dev(self, h, w, batch, seed, first_sample, style, relu_targets, passes, alpha, out_dev, adain=False,
                                   wct_mode='tf', smooth=False):
        """Texture samples first_sample .. first_sample + batch - 1 of `seed` on a PreparedStyle, into device memory
        [batch][Ho][Wo][3] (texture_size): the noise is made on the device and the `passes` passes feed each other there
        (wct_texture_prepared_batch_dev).  Asynchronous."""
        h, w = check_texture((h, w), passes, batch, seed, first_sample)
        lv = check_prepared(self, [style], relu_targets)
        check(self.lib.wct_texture_prepared_batch_dev(self.h, h, w, int(batch), int(seed), int(first_sample), int(bool(smooth)), style.h,
                                                      (C.c_int * len(lv))(*lv), len(lv), int(passes), float(alpha),
                                                      _flags(adain, wct_mode), out_dev))

    def texture_prepared_batch(self, h, w, batch, seed, first_sample, style, relu_targets, passes=3, alpha=1.0, adain=False,
                               wct_mode='tf', smooth=False):
        """texture_prepared_batch_dev with the frames brought to the host -> uint8 [batch][Ho][Wo][3].  Sample f equals the noise
        texture_noise(h, w, seed, first_sample + f) through `passes` chained stylize_prepared_batch calls, bit for bit."""
        h, w = check_texture((h, w), passes, batch, seed, first_sample)
        check_prepared(self, [style], relu_targets)
        ho, wo = self.texture_size(h, w, relu_targets, passes)
        out = np.empty((int(batch), ho, wo, 3), np.uint8)
        return self._host_batch([], out, lambda do: self.texture_prepared_batch_dev(
            h, w, batch, seed, first_sample, style, relu_targets, passes, alpha, do, adain=adain, wct_mode=wct_mode, smooth=smooth))

    def texture_prepared(self, h, w, seed, sample, style, relu_targets, passes=3, alpha=1.0, adain=False, wct_mode='tf', smooth=False):
        """One texture sample -> uint8 [Ho][Wo][3] (wct_texture_prepared, blocking): texture_prepared_batch with one sample."""
        h, w = check_texture((h, w), passes, 1, seed, sample)
        lv = check_prepared(self, [style], relu_targets)
        ho, wo = self.texture_size(h, w, relu_targets, passes)
        out = np.empty((ho, wo, 3), np.uint8)
        check(self.lib.wct_texture_prepared(self.h, h, w, int(seed), int(sample), int(bool(smooth)), style.h, (C.c_int * len(lv))(*lv),
                                            len(lv), int(passes), float(alpha), _flags(adain, wct_mode), out.ctypes.data_as(_lib._U8)))
        return out

    def texture_prepared_wrap_batch_dev(self, h, w, batch, seed, first_sample, style, relu_targets, passes, alpha, out_dev, adain=False,
                                        wct_mode='tf', smooth=False):
        """texture_prepared_batch_dev on a torus (wct_texture_prepared_wrap_batch_dev): seamless tiles [batch][h][w][3] into device
        memory -- the same noise, `passes` runs of the wrap chain.  h and w multiples of the deepest level's stride.  Asynchronous."""
        h, w = check_texture((h, w), passes, batch, seed, first_sample)
        lv = check_prepared(self, [style], relu_targets)
        check_wrap(h, w, lv)
        check(self.lib.wct_texture_prepared_wrap_batch_dev(self.h, h, w, int(batch), int(seed), int(first_sample), int(bool(smooth)),
                                                           style.h, (C.c_int * len(lv))(*lv), len(lv), int(passes), float(alpha),
                                                           _flags(adain, wct_mode), out_dev))

    def texture_prepared_wrap_batch(self, h, w, batch, seed, first_sample, style, relu_targets, passes=3, alpha=1.0, adain=False,
                                    wct_mode='tf', smooth=False):
        """texture_prepared_wrap_batch_dev with the tiles brought to the host -> uint8 [batch][h][w][3].  Sample f equals the noise
        texture_noise(h, w, seed, first_sample + f) through `passes` chained stylize_prepared_wrap_batch calls, bit for bit."""
        h, w = check_texture((h, w), passes, batch, seed, first_sample)
        check_wrap(h, w, check_prepared(self, [style], relu_targets))
        out = np.empty((int(batch), h, w, 3), np.uint8)
        return self._host_batch([], out, lambda do: self.texture_prepared_wrap_batch_dev(
            h, w, batch, seed, first_sample, style, relu_targets, passes, alpha, do, adain=adain, wct_mode=wct_mode, smooth=smooth))

    def texture_prepared_wrap(self, h, w, seed, sample, style, relu_targets, passes=3, alpha=1.0, adain=False, wct_mode='tf',
                              smooth=False):
        """One seamless tile -> uint8 [h][w][3] (wct_texture_prepared_wrap, blocking): texture_prepared_wrap_batch with one sample."""
        h, w = check_texture((h, w), passes, 1, seed, sample)
        lv = check_prepared(self, [style], relu_targets)
        check_wrap(h, w, lv)
        out = np.empty((h, w, 3), np.uint8)
        check(self.lib.wct_texture_prepared_wrap(self.h, h, w, int(seed), int(sample), int(bool(smooth)), style.h,
                                                 (C.c_int * len(lv))(*lv), len(lv), int(passes), float(alpha), _flags(adain, wct_mode),
                                                 out.ctypes.data_as(_lib._U8)))
        return out

    # ---- the hot path ------------------------------------------------------
    def output_size(self, hc, wc, relu_targets):
        lv = _levels(relu_targets)
        arr = (C.c_int * len(lv))(*lv)
        ho, wo = C.c_int(), C.c_int()
        check(self.lib.wct_output_size(hc, wc, arr, len(lv), C.byref(ho), C.byref(wo)))
        return ho.value, wo.value

    def stylize(self, content, style, relu_targets, alpha=1.0, adain=False, wct_mode='tf', swap5=False, content_colors=False, guided=None):
        """One predict(): HxWx3 images in [0,255] in, uint8 out.  uint8 inputs go to the library as they are (the /255
        runs on the device); anything else is preprocessed exactly as the reference does -- `image / 255.` in float64
        (wct.py:60-64), cast to the float32 the graph's placeholders hold (model.py:43-44) -- and handed over as float32
        images in [0,1] (WCT_FLAG_IMAGES_F32): a float image is NOT rounded to integer levels.
        content_colors (here and in every stylize* method): the frame keeps its luminance and takes the colours of its content
        (WCT_FLAG_CONTENT_COLORS) -- content_colors(the plain frame, content) bit for bit, fused into the last launch."""
        c, (s,), _, arr, out, flags = self._stylize_args(content, [style], None, relu_targets, adain, wct_mode, swap5, content_colors, guided)
        check(self.lib.wct_stylize(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1],
                                   s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], arr, len(arr),
                                   float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    def _stylize_args(self, content, styles, validate, relu_targets, adain, wct_mode, swap5, content_colors=False, guided=None):
        """The common arguments of the stylize calls: the caller's own validate(content, K) first (None: none; its result is
        returned), then the images -- all uint8 go as they are, otherwise every image is `/ 255.` in float64 and handed over as
        float32 in [0,1] -- the levels as a C int array, the output image and the flag word."""
        guided = None if guided is None else check_guided(guided)              # ValueError before any library call
        content = np.asarray(content)
        styles = [np.asarray(s) for s in styles]
        v = validate(content, len(styles)) if validate else None
        as_f32 = content.dtype != np.uint8 or any(s.dtype != np.uint8 for s in styles)
        if as_f32:
            c = np.ascontiguousarray(np.asarray(content / 255.), np.float32)
            ss = [np.ascontiguousarray(np.asarray(s / 255.), np.float32) for s in styles]
        else:
            c, ss = u8(content), [u8(s) for s in styles]
        lv = _levels(relu_targets)
        ho, wo = self.output_size(c.shape[0], c.shape[1], lv)
        flags = _flags(adain, wct_mode, swap5, images_f32=as_f32, content_colors=content_colors, guided=self._set_guided(guided))
        return c, ss, v, (C.c_int * len(lv))(*lv), np.empty((ho, wo, 3), np.uint8), flags

    # ---- prepared styles -----------------------------------------------------
    @staticmethod
    def _style_image(style):
        """a style image as prepare_style hands it over: -> (the array as given, its device form, images_f32)"""
        img = np.asarray(style)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError('expected an HxWx3 style image, got shape %s' % (img.shape,))
        as_f32 = img.dtype != np.uint8
        return img, (np.ascontiguousarray(np.asarray(img / 255.), np.float32) if as_f32 else u8(img)), as_f32

    def prepare_style(self, style, relu_targets, adain=False, wct_mode='tf', region=None):
        """The style side of `style` (HxWx3 in [0,255]) for the levels `relu_targets`, kept on the device -> PreparedStyle.
        uint8 goes as it is, anything else `/ 255.` in float64 and handed over as float32, exactly as Context.stylize does with
        its style.  adain / wct_mode only pick what is computed up front: a handle serves either mode and AdaIN.
        region=(label_map, label): a style region (wct_style_prepare_region) -- label_map [H][W] integers of the style's size,
        and the statistics of every level come from the feature rows of `label` (0 .. 7) alone; the encoder still sees the
        whole image.  A region with fewer than 2 rows at a level is refused by the library."""
        img, s, as_f32 = self._style_image(style)
        lv = sorted(set(_levels(relu_targets)))
        flags = _flags(adain, wct_mode, images_f32=as_f32)
        h = C.c_void_p()
        if region is not None:
            label_map, label = region
            m = _lib.style_region_map(label_map, img.shape[:2], label=label)   # ValueError before any library call
            check(self.lib.wct_style_prepare_region(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], m.ctypes.data_as(_lib._U8),
                                                    int(label), (C.c_int * len(lv))(*lv), len(lv), flags, C.byref(h)))
            return PreparedStyle(self, h, img, lv, region=(m, int(label)))
        check(self.lib.wct_style_prepare(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], (C.c_int * len(lv))(*lv), len(lv),
                                         flags, C.byref(h)))
        return PreparedStyle(self, h, img, lv)

    def prepare_style_regions(self, style, label_map, k, relu_targets, adain=False, wct_mode='tf'):
        """The k regions of ONE style image as prepared styles (wct_style_prepare_regions): label_map [H][W] integers 0 .. k - 1 of
        the style's size -> a list of k entries, entry j the PreparedStyle prepare_style(style, region=(label_map, j)) gives, bit
        for bit -- from one upload, one encoder pass and one partition per level for all of them -- or None for a label with
        fewer than 2 feature rows at some level, which cannot carry a style."""
        img, s, as_f32 = self._style_image(style)
        m = _lib.style_region_map(label_map, img.shape[:2], k=k)               # ValueError before any library call
        lv = sorted(set(_levels(relu_targets)))
        flags = _flags(adain, wct_mode, images_f32=as_f32)
        hs = (C.c_void_p * int(k))()
        check(self.lib.wct_style_prepare_regions(self.h, s.ctypes.data_as(_lib._U8), s.shape[0], s.shape[1], m.ctypes.data_as(_lib._U8),
                                                 int(k), (C.c_int * len(lv))(*lv), len(lv), flags, hs))
        return [PreparedStyle(self, C.c_void_p(hs[j]), img, lv, region=(m, j)) if hs[j] else None for j in range(int(k))]

    def _prepared_args(self, content, relu_targets, adain, wct_mode, content_colors=False, guided=None):
        """content, levels, output and flags of a call with prepared styles (the content as in stylize)"""
        guided = None if guided is None else check_guided(guided)              # ValueError before any library call
        content = np.asarray(content)
        as_f32 = content.dtype != np.uint8
        c = np.ascontiguousarray(np.asarray(content / 255.), np.float32) if as_f32 else u8(content)
        lv = _levels(relu_targets)
        ho, wo = self.output_size(c.shape[0], c.shape[1], lv)
        flags = _flags(adain, wct_mode, images_f32=as_f32, content_colors=content_colors, guided=self._set_guided(guided))
        return c, (C.c_int * len(lv))(*lv), np.empty((ho, wo, 3), np.uint8), flags

    def warm_state(self, relu_targets):
        """A WarmState for the levels `relu_targets` (wct_warm_create): every level invalid until a call has used it."""
        lv = sorted(set(_levels(relu_targets)))
        h = C.c_void_p()
        check(self.lib.wct_warm_create(self.h, (C.c_int * len(lv))(*lv), len(lv), C.byref(h)))
        return WarmState(self, h, lv)

    def stylize_prepared(self, content, style, relu_targets, alpha=1.0, adain=False, wct_mode='tf', warm=None, content_colors=False, guided=None):
        """stylize() with a PreparedStyle in the place of the style image: the same frame, bit for bit.  warm (a WarmState):
        the content eigensolves start from the state's bases, which then take this frame's."""
        check_prepared(self, [style], relu_targets)
        if warm is not None:
            check_warm(self, warm, relu_targets, adain)
        c, arr, out, flags = self._prepared_args(content, relu_targets, adain, wct_mode, content_colors, guided)
        if warm is not None:
            check(self.lib.wct_stylize_prepared_warm(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], style.h, arr,
                                                     len(arr), float(alpha), flags, warm.h, out.ctypes.data_as(_lib._U8)))
            return out
        check(self.lib.wct_stylize_prepared(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], style.h, arr, len(arr),
                                            float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    def band_rows(self, hc, wc, relu_targets):
        """0 when the whole-image calls take an hc x wc content with these levels, else the automatic band height (band_rows)"""
        return band_rows(hc, wc, relu_targets)

    def band_plan(self, h, w, relu_target, band_rows=0):
        """The bands of one level on an h x w input (band_plan)"""
        return band_plan(h, w, relu_target, band_rows)

    def stylize_prepared_banded(self, content, style, relu_targets, alpha=1.0, wct_mode='tf', band_rows=0, stat_rows=0,
                                content_colors=False):
        """stylize_prepared() in bands of band_rows image rows (a multiple of 16; 0: automatic) with the content statistics
        pooled over chunks of stat_rows feature rows (0: the fewest that fit): contents of any size.  Where stylize_prepared()
        runs, stat_rows = 0 gives its frame bit for bit.  WCT only: no AdaIN, warm state, mix or mask."""
        check_prepared(self, [style], relu_targets)
        check_band_rows(band_rows)
        if int(stat_rows) < 0:
            raise ValueError('stat_rows must be >= 0, got %r' % (stat_rows,))
        c, arr, out, flags = self._prepared_args(content, relu_targets, False, wct_mode, content_colors)
        check(self.lib.wct_stylize_prepared_banded(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], style.h, arr, len(arr),
                                                   float(alpha), flags, int(band_rows), int(stat_rows), out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_mix(self, content, styles, weights, relu_targets, alpha=1.0, adain=False, wct_mode='tf', content_colors=False, guided=None):
        """stylize_mix() with K PreparedStyle objects in the place of the K images: the same frame, bit for bit."""
        w = _lib.mix_weights(weights, len(styles))
        check_prepared(self, styles, relu_targets)
        c, arr, out, flags = self._prepared_args(content, relu_targets, adain, wct_mode, content_colors, guided)
        hs = (C.c_void_p * len(styles))(*[s.h.value for s in styles])
        check(self.lib.wct_stylize_prepared_mix(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], hs, len(styles), fptr(w),
                                                arr, len(arr), float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_batch_dev(self, content_dev, hc, wc, batch, style, relu_targets, alpha, out_dev, adain=False, wct_mode='tf',
                                   warm=None, content_colors=False, guided=None):
        """stylize_batch_dev(shared_style=True) with a PreparedStyle: B contents resident in HBM, asynchronous.  warm (a
        WarmState): all B frames start from the state's bases, which then take those of frame B - 1."""
        lv = check_prepared(self, [style], relu_targets)
        flags = _flags(adain, wct_mode, content_colors=content_colors, guided=self._set_guided(guided))
        if warm is not None:
            check_warm(self, warm, relu_targets, adain)
            check(self.lib.wct_stylize_prepared_batch_dev_warm(self.h, content_dev, hc, wc, batch, style.h, (C.c_int * len(lv))(*lv),
                                                               len(lv), float(alpha), flags, warm.h, out_dev))
            return
        check(self.lib.wct_stylize_prepared_batch_dev(self.h, content_dev, hc, wc, batch, style.h, (C.c_int * len(lv))(*lv), len(lv),
                                                      float(alpha), flags, out_dev))

    def stylize_prepared_batch(self, contents_u8, style, relu_targets, alpha=1.0, adain=False, wct_mode='tf', warm=None,
                               content_colors=False, guided=None, resize=None):
        """stylize_batch() with a PreparedStyle: contents [B][H][W][3] uint8 (B <= 32) -> [B][Ho][Wo][3] uint8.  warm: as in
        stylize_prepared_batch_dev.  resize (h, w): the contents are raw frames, resized on the device (resize_batch_dev) into
        the content buffer the call -- and content_colors -- reads: the frames of the call on utils._imresize(frame, (h, w))."""
        check_prepared(self, [style], relu_targets)
        if warm is not None:
            check_warm(self, warm, relu_targets, adain)
        if resize is not None:
            hc, wc, c = check_resize(resize, contents_u8)
        else:
            c = u8(contents_u8)
            assert c.ndim == 4 and c.shape[3] == 3
            hc, wc = c.shape[1:3]
        B = c.shape[0]
        ho, wo = self.output_size(hc, wc, relu_targets)
        out = np.empty((B, ho, wo, 3), np.uint8)
        enqueue = lambda dc, do: self.stylize_prepared_batch_dev(
            dc, hc, wc, B, style, relu_targets, alpha, do, adain=adain, wct_mode=wct_mode, warm=warm, content_colors=content_colors, guided=guided)
        if resize is not None:
            return self._host_batch_resized(c, (hc, wc), [], out, enqueue)
        return self._host_batch([c], out, enqueue)

    def stylize_prepared_strength(self, content, style, smap, relu_targets, alpha=1.0, adain=False, wct_mode='tf', content_colors=False, guided=None):
        """stylize_prepared() with a strength map (wct_stylize_prepared_strength): smap [H][W] uint8 of the content's size, 255 the
        call's alpha, 0 "keep the content features"; every level samples it at its own stride.  An all-255 map gives
        stylize_prepared's frame at alpha = 1 bit for bit."""
        c0 = np.asarray(content)
        m = _lib.strength_map(smap, c0.shape[:2])
        check_prepared(self, [style], relu_targets)
        c, arr, out, flags = self._prepared_args(c0, relu_targets, adain, wct_mode, content_colors, guided)
        check(self.lib.wct_stylize_prepared_strength(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1],
                                                     m.ctypes.data_as(_lib._U8), style.h, arr, len(arr), float(alpha), flags,
                                                     out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_strength_batch_dev(self, content_dev, hc, wc, batch, smaps_dev, style, relu_targets, alpha, out_dev,
                                            adain=False, wct_mode='tf', warm=None, content_colors=False, guided=None):
        """stylize_prepared_batch_dev with one strength map per frame, smaps_dev [B][hc][wc] uint8 resident in HBM.  Asynchronous:
        nothing of the maps is read on the host.  Frame f is stylize_prepared_strength(frame f, map f)."""
        if not 1 <= int(batch) <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, batch))
        lv = check_prepared(self, [style], relu_targets)
        flags = _flags(adain, wct_mode, content_colors=content_colors, guided=self._set_guided(guided))
        arr = (C.c_int * len(lv))(*lv)
        if warm is not None:
            check_warm(self, warm, relu_targets, adain)
            check(self.lib.wct_stylize_prepared_strength_batch_dev_warm(self.h, content_dev, hc, wc, int(batch), smaps_dev, style.h, arr,
                                                                        len(lv), float(alpha), flags, warm.h, out_dev))
            return
        check(self.lib.wct_stylize_prepared_strength_batch_dev(self.h, content_dev, hc, wc, int(batch), smaps_dev, style.h, arr, len(lv),
                                                               float(alpha), flags, out_dev))

    def stylize_prepared_strength_batch(self, contents_u8, style, smaps, relu_targets, alpha=1.0, adain=False, wct_mode='tf', warm=None,
                                        content_colors=False, guided=None, resize=None):
        """Host arrays in, host array out: contents [B][H][W][3] uint8 (B <= 32), smaps [B][H][W] uint8 (or one [H][W] map for
        all) -> [B][Ho][Wo][3] uint8.  warm and resize (h, w): as in stylize_prepared_batch; the maps are given at the resized
        size."""
        if resize is not None:
            hc, wc, c = check_resize(resize, contents_u8)
        else:
            c = u8(contents_u8)
            if c.ndim != 4 or c.shape[3] != 3:
                raise ValueError('expected [B][H][W][3] frames, got shape %s' % (c.shape,))
            hc, wc = c.shape[1:3]
        B = c.shape[0]
        if not 1 <= B <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, B))
        m = _lib.strength_maps_frames(smaps, B, (hc, wc))
        check_prepared(self, [style], relu_targets)
        if warm is not None:
            check_warm(self, warm, relu_targets, adain)
        ho, wo = self.output_size(hc, wc, relu_targets)
        out = np.empty((B, ho, wo, 3), np.uint8)
        enqueue = lambda dc, dm, do: self.stylize_prepared_strength_batch_dev(
            dc, hc, wc, B, dm, style, relu_targets, alpha, do, adain=adain, wct_mode=wct_mode, warm=warm, content_colors=content_colors, guided=guided)
        if resize is not None:
            return self._host_batch_resized(c, (hc, wc), [m], out, enqueue)
        return self._host_batch([c, m], out, enqueue)

    def stylize_prepared_wrap_batch_dev(self, content_dev, hc, wc, batch, style, relu_targets, alpha, out_dev, adain=False, wct_mode='tf'):
        """stylize_prepared_batch_dev on a torus (wct_stylize_prepared_wrap_batch_dev): every encoder and decoder of the chain sees
        its input extended periodically, so a periodic content gives a periodic frame [batch][hc][wc][3].  Asynchronous."""
        lv = check_prepared(self, [style], relu_targets)
        check_wrap(hc, wc, lv)
        check(self.lib.wct_stylize_prepared_wrap_batch_dev(self.h, content_dev, int(hc), int(wc), int(batch), style.h,
                                                           (C.c_int * len(lv))(*lv), len(lv), float(alpha), _flags(adain, wct_mode), out_dev))

    def stylize_prepared_wrap_batch(self, frames, style, relu_targets, alpha=1.0, adain=False, wct_mode='tf'):
        """stylize_prepared_wrap_batch_dev with host arrays: frames [B][H][W][3] uint8 (B <= 32; H and W multiples of the deepest
        level's stride) -> [B][H][W][3] uint8.  No mix, mask, warm state, style-swap or content colours on this path."""
        lv = check_prepared(self, [style], relu_targets)
        c = np.asarray(frames)
        if c.dtype != np.uint8 or c.ndim != 4 or c.shape[3] != 3 or not 1 <= c.shape[0] <= _lib.BATCH_MAX:
            raise ValueError('expected 1 .. %d uint8 frames [B][H][W][3], got %s of shape %s' % (_lib.BATCH_MAX, c.dtype, c.shape))
        c = u8(c)
        hc, wc = check_wrap(c.shape[1], c.shape[2], lv)
        return self._host_batch([c], np.empty_like(c), lambda dc, do: self.stylize_prepared_wrap_batch_dev(
            dc, hc, wc, c.shape[0], style, relu_targets, alpha, do, adain=adain, wct_mode=wct_mode))

    def stylize_prepared_wrap(self, content, style, relu_targets, alpha=1.0, adain=False, wct_mode='tf'):
        """One tile through wct_stylize_prepared_wrap (blocking): content HxWx3 in [0,255] as in stylize_prepared -> uint8 HxWx3"""
        lv = check_prepared(self, [style], relu_targets)
        check_wrap(np.shape(content)[0], np.shape(content)[1], lv)
        c, arr, out, flags = self._prepared_args(content, relu_targets, adain, wct_mode)
        check(self.lib.wct_stylize_prepared_wrap(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], style.h, arr, len(arr),
                                                 float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_masked(self, content, styles, mask, relu_targets, alpha=1.0, adain=False, wct_mode='tf', content_colors=False, guided=None):
        """stylize_masked() with K PreparedStyle objects in the place of the K images: the same frame, bit for bit."""
        c0 = np.asarray(content)
        m = _lib.mask_labels(mask, len(styles), c0.shape[:2])
        check_prepared(self, styles, relu_targets)
        c, arr, out, flags = self._prepared_args(c0, relu_targets, adain, wct_mode, content_colors, guided)
        hs = (C.c_void_p * len(styles))(*[s.h.value for s in styles])
        check(self.lib.wct_stylize_prepared_masked(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1],
                                                   m.ctypes.data_as(_lib._U8), hs, len(styles), arr, len(arr), float(alpha), flags,
                                                   out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_prepared_masked_batch_dev(self, content_dev, hc, wc, batch, masks, styles, relu_targets, alpha, out_dev,
                                          adain=False, wct_mode='tf', content_colors=False, guided=None):
        """Spatial control of B uint8 frames resident in HBM, one label map per frame: `masks` [B][hc][wc] (or one [hc][wc] map
        for all) is a HOST array, the K PreparedStyle objects are shared by all frames.  Asynchronous; frame f is
        stylize_prepared_masked(frame f, masks[f])."""
        if not 1 <= int(batch) <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, batch))
        m = _lib.mask_labels_frames(masks, len(styles), int(batch), (hc, wc))
        lv = check_prepared(self, styles, relu_targets)
        flags = _flags(adain, wct_mode, content_colors=content_colors, guided=self._set_guided(guided))
        hs = (C.c_void_p * len(styles))(*[s.h.value for s in styles])
        # the upload is enqueued on the stream: the maps stay alive until sync() (include/wct_hip.h)
        self._masks_in_flight = getattr(self, '_masks_in_flight', []) + [m]
        check(self.lib.wct_stylize_prepared_masked_batch_dev(self.h, content_dev, hc, wc, int(batch), m.ctypes.data_as(_lib._U8), hs,
                                                             len(styles), (C.c_int * len(lv))(*lv), len(lv), float(alpha), flags,
                                                             out_dev))

    def stylize_prepared_masked_batch(self, contents_u8, styles, masks, relu_targets, alpha=1.0, adain=False, wct_mode='tf',
                                      content_colors=False, guided=None, resize=None):
        """Host arrays in, host array out: contents [B][H][W][3] uint8 (B <= 32), masks [B][H][W] (or one [H][W] map for all),
        K PreparedStyle objects -> [B][Ho][Wo][3] uint8.  resize (h, w): as in stylize_prepared_batch; the label maps are given
        at the resized size."""
        if resize is not None:
            hc, wc, c = check_resize(resize, contents_u8)
        else:
            c = u8(contents_u8)
            if c.ndim != 4 or c.shape[3] != 3:
                raise ValueError('expected [B][H][W][3] frames, got shape %s' % (c.shape,))
            hc, wc = c.shape[1:3]
        B = c.shape[0]
        if not 1 <= B <= _lib.BATCH_MAX:
            raise ValueError('a batch takes 1 .. %d frames, got %d' % (_lib.BATCH_MAX, B))
        m = _lib.mask_labels_frames(masks, len(styles), B, (hc, wc))
        check_prepared(self, styles, relu_targets)
        ho, wo = self.output_size(hc, wc, relu_targets)
        out = np.empty((B, ho, wo, 3), np.uint8)
        enqueue = lambda dc, do: self.stylize_prepared_masked_batch_dev(
            dc, hc, wc, B, m, styles, relu_targets, alpha, do, adain=adain, wct_mode=wct_mode, content_colors=content_colors, guided=guided)
        if resize is not None:
            return self._host_batch_resized(c, (hc, wc), [], out, enqueue)
        return self._host_batch([c], out, enqueue)

    def stylize_mix(self, content, styles, weights, relu_targets, alpha=1.0, adain=False, wct_mode='tf', swap5=False,
                    content_colors=False, guided=None):
        """One predict() with a style mix at every level (wct_stylize_mix): `styles` is a list of K HxWx3 images (sizes may
        differ), `weights` [K] (None: equal).  Inputs as in stylize: all uint8 go as they are, otherwise every image is
        `/ 255.` in float64 and handed over as float32 in [0,1]."""
        c, ss, w, arr, out, flags = self._stylize_args(content, styles, lambda c, k: _lib.mix_weights(weights, k), relu_targets,
                                                       adain, wct_mode, swap5, content_colors, guided)
        ptrs, hs, ws = _image_arrays(ss)
        check(self.lib.wct_stylize_mix(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], ptrs, hs, ws, len(ss), fptr(w),
                                       arr, len(arr), float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    def stylize_masked(self, content, styles, mask, relu_targets, alpha=1.0, adain=False, wct_mode='tf', swap5=False,
                       content_colors=False, guided=None):
        """One predict() with spatial control at every level (wct_stylize_masked): `mask` [H][W] labels 0 .. K-1 of the content
        pixels, `styles` a list of K HxWx3 images (sizes may differ).  Inputs as in stylize: all uint8 go as they are,
        otherwise every image is `/ 255.` in float64 and handed over as float32 in [0,1]."""
        c, ss, m, arr, out, flags = self._stylize_args(content, styles, lambda c, k: _lib.mask_labels(mask, k, c.shape[:2]),
                                                       relu_targets, adain, wct_mode, swap5, content_colors, guided)
        ptrs, hs, ws = _image_arrays(ss)
        check(self.lib.wct_stylize_masked(self.h, c.ctypes.data_as(_lib._U8), c.shape[0], c.shape[1], m.ctypes.data_as(_lib._U8),
                                          ptrs, hs, ws, len(ss), arr, len(arr), float(alpha), flags, out.ctypes.data_as(_lib._U8)))
        return out

    # device-resident batch (what bench.py times)
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.wct_dev_alloc(self.h, int(nbytes), C.byref(p)))
        return p

    def dev_free(self, p):
        check(self.lib.wct_dev_free(self.h, p))

    def h2d(self, dst, arr):
        a = np.ascontiguousarray(arr)
        check(self.lib.wct_h2d(self.h, dst, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def d2h(self, arr, src):
        assert arr.flags['C_CONTIGUOUS']
        check(self.lib.wct_d2h(self.h, arr.ctypes.data_as(C.c_void_p), src, arr.nbytes))

    def _host_batch(self, inputs, out, enqueue, in_place=False):
        """The round trip of a host batch: a device buffer per input array and one for `out` (in_place: `out` comes back in the
        first input's buffer), h2d, enqueue(*buffers), sync(), d2h -> out.  The buffers are freed whatever happens."""
        bufs = []
        try:
            for a in inputs:
                bufs.append(self.dev_alloc(a.nbytes))
            if not in_place:
                bufs.append(self.dev_alloc(out.nbytes))
            for p, a in zip(bufs, inputs):
                self.h2d(p, a)
            enqueue(*bufs)
            self.sync()
            self.d2h(out, bufs[0] if in_place else bufs[-1])
        finally:
            for p in bufs:
                self.dev_free(p)
        return out

    def _host_batch_resized(self, raw, size, inputs, out, enqueue):
        """_host_batch for raw frames that are resized on the way in: `raw` [B][H][W][3] uint8 goes up as it is, is resized into a
        device content buffer [B][h][w][3] (resize_batch_dev), and enqueue(content buffer, *buffers of `inputs`, out buffer)
        follows on the same stream; one sync(), d2h -> out.  The buffers are freed whatever happens."""
        h, w = size
        B, hi, wi = raw.shape[:3]
        bufs = []
        try:
            for n in [raw.nbytes, B * h * w * 3] + [a.nbytes for a in inputs] + [out.nbytes]:
                bufs.append(self.dev_alloc(n))
            for p, a in zip([bufs[0]] + bufs[2:], [raw] + list(inputs)):
                self.h2d(p, a)
            self.resize_batch_dev(bufs[0], hi, wi, B, (h, w), bufs[1])
            enqueue(*bufs[1:])
            self.sync()
            self.d2h(out, bufs[-1])
        finally:
            for p in bufs:
                self.dev_free(p)
        return out

    def stylize_batch_dev(self, content_dev, hc, wc, style_dev, hs, ws, batch, relu_targets, alpha, out_dev,
                          adain=False, wct_mode='tf', swap5=False, shared_style=False, content_colors=False, guided=None):
        """B pairs resident in HBM.  shared_style: style_dev holds ONE image used for every pair (fixed-style
        video): its encoder pass, statistics and eigensystems run once per call; the frames are bit-identical
        to the ones a replicated style produces."""
        lv = _levels(relu_targets)
        arr = (C.c_int * len(lv))(*lv)
        flags = _flags(adain, wct_mode, swap5, shared_style=shared_style, content_colors=content_colors, guided=self._set_guided(guided))
        check(self.lib.wct_stylize_batch_dev(self.h, content_dev, hc, wc, style_dev, hs, ws, batch, arr, len(lv),
                                             float(alpha), flags, out_dev))

    def stylize_batch(self, contents_u8, style_u8, relu_targets, alpha=1.0, adain=False, wct_mode='tf', swap5=False,
                      content_colors=False, guided=None, resize=None):
        """Host arrays in, host array out: contents [B][H][W][3] uint8 (B <= 32); style either one image
        [Hs][Ws][3] shared by all frames or [B][Hs][Ws][3].  Returns [B][Ho][Wo][3] uint8.  resize (h, w): as in
        stylize_prepared_batch (the contents only; the style goes as it is)."""
        s = u8(style_u8)
        if resize is not None:
            hc, wc, c = check_resize(resize, contents_u8)
        else:
            c = u8(contents_u8)
            hc, wc = c.shape[1:3]
        assert c.ndim == 4 and c.shape[3] == 3 and s.ndim in (3, 4) and s.shape[-1] == 3
        shared = s.ndim == 3
        assert shared or s.shape[0] == c.shape[0]
        B = c.shape[0]
        hs, ws = s.shape[-3], s.shape[-2]
        ho, wo = self.output_size(hc, wc, relu_targets)
        out = np.empty((B, ho, wo, 3), np.uint8)
        enqueue = lambda dc, ds, do: self.stylize_batch_dev(
            dc, hc, wc, ds, hs, ws, B, relu_targets, alpha, do, adain=adain, wct_mode=wct_mode, swap5=swap5, shared_style=shared,
            content_colors=content_colors, guided=guided)
        if resize is not None:
            return self._host_batch_resized(c, (hc, wc), [s], out, enqueue)
        return self._host_batch([c, s], out, enqueue)

    # ---- decoder training (model.py:123-223) --------------------------------
    def train_step(self, relu_target, images01, step, learning_rate=1e-4, feature_weight=1.0, pixel_weight=1.0,
                   tv_weight=0.0, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """One Adam step on the decoder of `relu_target`; images01 [B][H][W][3] fp32 in [0,1].
        Returns {'feature_loss', 'pixel_loss', 'tv_loss', 'total_loss'}.  learning_rate=0 only evaluates."""
        level = _levels([relu_target])[0]
        x = f32(images01)
        assert x.ndim == 4 and x.shape[3] == 3
        out = (C.c_float * 4)()
        check(self.lib.wct_train_step(self.h, level, x.ctypes.data_as(_lib._F), x.shape[0], x.shape[1], x.shape[2],
                                      float(feature_weight), float(pixel_weight), float(tv_weight), float(learning_rate),
                                      float(beta1), float(beta2), float(epsilon), int(step), out))
        return {'feature_loss': out[0], 'pixel_loss': out[1], 'tv_loss': out[2], 'total_loss': out[3]}

    def train_grad_buffer(self, relu_target):
        """(device pointer, float count) of the decoder's contiguous gradient buffer (data-parallel all-reduce)."""
        level = _levels([relu_target])[0]
        p, n = C.c_void_p(), C.c_size_t()
        check(self.lib.wct_train_grad_buffer(self.h, level, C.byref(p), C.byref(n)))
        return p.value, n.value

    def train_apply(self, relu_target, step, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8):
        """Adam from the gradients currently in the gradient buffer (after train_step(learning_rate=0) and an
        all-reduce): the second half of a data-parallel step."""
        level = _levels([relu_target])[0]
        check(self.lib.wct_train_apply(self.h, level, float(learning_rate), float(beta1), float(beta2), float(epsilon), int(step)))

    def get_decoder(self, relu_target, grads=False):
        """[(w HWIO fp32, b)] of the decoder as it is now on the device (after training steps); with grads=True
        the gradients of the last train_step instead."""
        level = _levels([relu_target])[0]
        out = []
        for i, (_, cin, cout, _) in enumerate(p for p in decoder_plan('relu%d_1' % level) if p[0] == 'C'):
            w = np.empty((3, 3, cin, cout), np.float32)
            b = np.empty(cout, np.float32)
            wp, bp = w.ctypes.data_as(_lib._F), b.ctypes.data_as(_lib._F)
            if grads:
                check(self.lib.wct_get_decoder_layer(self.h, level, i, None, None, wp, bp))
            else:
                check(self.lib.wct_get_decoder_layer(self.h, level, i, wp, bp, None, None))
            out.append((w, b))
        return out

    # ---- measurement -------------------------------------------------------
    def prof_enable(self, on=True):
        check(self.lib.wct_prof_enable(self.h, int(on)))

    def prof_reset(self):
        check(self.lib.wct_prof_reset(self.h))

    def prof_read(self):
        n = len(_lib.PROF_CLASSES)
        ms = (C.c_double * n)()
        cnt = (C.c_longlong * n)()
        fl = (C.c_double * n)()
        by = (C.c_double * n)()
        check(self.lib.wct_prof_read(self.h, ms, cnt, fl, by))
        return {name: {'ms': ms[i], 'launches': cnt[i], 'flops': fl[i], 'bytes': by[i]}
                for i, name in enumerate(_lib.PROF_CLASSES)}

    def eig_stats(self):
        """Eigensolver statistics since the last call: {C: {'matrices', 'sweeps', 'max_sweeps'}} for the covariance
        orders C = 32 * 2^k that were solved (wct_eig_stats; synchronises the stream, cleared on read)."""
        out = (C.c_longlong * 18)()
        check(self.lib.wct_eig_stats(self.h, out))
        return {32 << k: {'matrices': out[3 * k], 'sweeps': out[3 * k + 1], 'max_sweeps': out[3 * k + 2]}
                for k in range(6) if out[3 * k]}


_default = {}


def default_context(device=0):
    """Process-wide context per device (the reference has one session per WCT object;
    the op-level functions in ops.py share this one)."""
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]
