"""`python -m wct_tf_amd.stylize_video ...`: the reference's stylize_video.py (stylize_video.py:16-160) on the
MI355X path.  Same flags.  Differences, all forced by the environment or by the hardware:

* `--in-path` may be a DIRECTORY of frames (ffmpeg is not in this image).  A video file works
  when an `ffmpeg` binary is on PATH: frames are extracted to `--tmp-dir` and the stylized frames are
  re-encoded, exactly as the reference does (stylize_video.py:73-80,136-150).  Without ffmpeg the stylized
  frames are left in `<out-path>/<video>_<style>/`.
* The reference calls `predict()` once per frame, which re-runs the style encoder, the style statistics and
  the style eigendecompositions for every frame (stylize_video.py:112-121).  Here the frames of a video go
  through `WCT.predict_frames` in batches that share ONE style: the style side runs once per batch
  (WCT_FLAG_STYLE_SHARED) and every frame is bit-identical to `predict(frame, style)`.  With
  `--keep-colors` the style image is CORAL-matched to every frame (stylize_video.py:116-119) and therefore
  differs per frame: those frames go through the per-pair batch instead.  `--content-colors` keeps the frames' colours the
  other way (luminance-only transfer, applied to the result): the style stays shared, so it goes with the prepared style,
  `--mask-path` and `--warm-start`.
* `--guided-radius R [--guided-eps E]` (the photo mode) smooths every stylized frame with a guided filter whose guide is the input
  frame (He et al., "Guided Image Filtering"): edges where the frame has them, averages where it is flat.  It runs at the end of the
  batched call, before `--content-colors`, and goes with every other option.  `--guided-guide color` guides it with the frame's
  three channels instead of their grey, which also keeps an edge between two colours of equal luminance.
* `--guided-frames T` (1 .. 3, with `--guided-radius`) extends that filter's box over the T frames on each side of a frame, against
  the flicker of frames stylized one by one: where the input stands still the stylized frames are averaged along time, where it
  moves the result follows the input.  No motion compensation.  A clip is a run of consecutive frames of one size; every frame
  equals the whole-clip filter on the plain frames of its clip whatever `--batch` is (a sliding buffer of at most 32 + `--batch`
  frames, never the whole video).  Not with `--swap5`, `--keep-colors` or `--mask-path`.  `--guided-frames-guide color` guides
  it with the frames' three channels instead of their grey (the default), which keeps an edge between two colours of equal
  luminance along time too; `--guided-guide` stays the guide of the per-frame filter and does not combine with `--guided-frames`.
* `--guided-motion global [--guided-motion-range R]` (with `--guided-frames`) runs that filter along camera motion: one global
  integer translation per frame, estimated from the input frames, shifts the window in every neighbouring frame, so a pan or a
  handheld shot is averaged along its motion, not across it.  Frames still do not depend on `--batch`.
* `--guided-upsample --guided-upsample-frames T` (1 .. 3) delivers frames stylized at `--content-size` at their own size without
  the flicker of the per-frame upsampling: the coefficients are formed over the T frames on each side of a frame of the SMALL
  clip, every frame is evaluated against itself.  `--guided-upsample-motion global [--guided-upsample-motion-range R]` shifts
  those windows along camera motion, estimated at the working size.  The buffer holds small frames (2T behind and in front of a
  chunk) and the full frames not yet delivered, never the whole video; frames do not depend on `--batch`.  Grey guide only.
* `--device-resize` (opt-in) applies `--content-size` on the device: the frames go up raw and are resized there, on the stream
  of the call that stylizes them, to the bytes Pillow's bilinear resize gives on the host -- the same frames come out.
"""
from __future__ import division, print_function

import argparse
import os
import random
import re
import shutil
import subprocess
import time

import numpy as np

from .utils import get_files, get_img, save_img, resize_to, resize_shape, center_crop, _imresize
from .wct import WCT

TMP_DIR = '_____fns_frames_%s/' % random.randint(0, 99999)


# (flags, keyword arguments): the interface of stylize_video.py:18-41, then the additions of this path
_FLAGS = [
    (('--checkpoints',), dict(nargs='+', default=None, help='one decoder checkpoint (directory or .npz) per relu target')),
    (('--relu-targets',), dict(nargs='+', required=True, help='relu layers to stylize at, in pipeline order')),
    (('--vgg-path',), dict(default='models/vgg_normalised.t7', help='encoder weights: vgg_normalised.t7 or .npz (stylize.py:19 default)')),
    (('--in-path',), dict(required=True, help='a video file (needs ffmpeg on PATH) or a directory of frames')),
    (('--out-path',), dict(required=True, help='folder the results are written to')),
    (('--style-path',), dict(default=None, help='style image, or a folder of them (one output per style)')),
    (('--tmp-dir',), dict(dest='tmp_dir', default=TMP_DIR, help='scratch folder for extracted / stylized frames')),
    (('--keep-tmp',), dict(action='store_true', default=False, help='leave the scratch folder in place')),
    (('--keep-colors',), dict(action='store_true', default=False, help='CORAL: give the style the colours of each frame first')),
    (('--content-colors',), dict(action='store_true', default=False,
                                 help='luminance-only colour preservation: every frame keeps its luminance and takes the colours '
                                      'of its input frame (the alternative to --keep-colors: not with it).  Fused into the last '
                                      'launch; with --passes > 1 applied once at the end, against the input frames')),
    (('--guided-radius',), dict(type=int, default=0, metavar='R',
                                help='guided smoothing, the photo mode: filter every frame over a (2R + 1)^2 box with its input frame '
                                     'as guide (1 .. 64; 0: off).  With --passes > 1 applied once at the end, against the input '
                                     'frames; before --content-colors')),
    (('--guided-eps',), dict(type=float, default=0.01, metavar='E',
                             help='the regulariser of --guided-radius for images in [0,1] (> 0): smaller keeps more edges')),
    (('--guided-guide',), dict(choices=['grey', 'color'], default=None,
                               help='the guide of --guided-radius: grey (the default), the grey of the input frame, or color, its three '
                                    'channels -- keeps edges between colours of equal luminance too.  Needs --guided-radius > 0')),
    (('--guided-frames',), dict(type=int, default=0, metavar='T',
                                help='temporal guided smoothing, against flicker: the box of --guided-radius also covers the T frames '
                                     'on each side of a frame (0 .. 3; 0: off), within every run of consecutive frames of one size. '
                                     'The radius is then at most 51 / 40 / 33 at T = 1 / 2 / 3.  Its guide is --guided-frames-guide '
                                     '(not --guided-guide); not with --swap5, --keep-colors or --mask-path')),
    (('--guided-frames-guide',), dict(choices=['grey', 'color'], default=None,
                                      help='the guide of --guided-frames: grey (the default), the grey of the input frames, or color, '
                                           'their three channels -- keeps edges between colours of equal luminance along time too.  '
                                           'Needs --guided-frames >= 1; goes with --guided-motion (estimated on the grey guide); not '
                                           'with --guided-upsample')),
    (('--guided-motion',), dict(choices=['global'], default=None,
                                help='run --guided-frames along camera motion: global estimates one integer translation per frame '
                                     'from the input frames (exhaustive search, steps within --guided-motion-range) and shifts the '
                                     'window in every neighbouring frame by it.  A scene cut yields an arbitrary shift, which the '
                                     'filter treats like any edge.  Needs --guided-frames >= 1.  Per-block or dense motion, sub-pixel '
                                     'shifts, rotation and zoom are not served')),
    (('--guided-motion-range',), dict(type=int, default=None, metavar='R',
                                      help='the search range of --guided-motion in pixels per frame (1 .. 16; default 8); both sides of '
                                           'a frame must be at least 4 R')),
    (('--style-size',), dict(type=int, default=0, help='short side of the style image (0: as is)')),
    (('--crop-size',), dict(type=int, default=0, help='centre-crop the style image to a square of this side (0: no)')),
    (('--content-size',), dict(type=int, default=0, help='short side of every frame (0: as is)')),
    (('--guided-upsample',), dict(action='store_true', default=False,
                                  help='stylize small, deliver at the frame\'s size (He & Sun, "Fast Guided Filter"): every raw frame '
                                       'is resized on the device to --content-size, stylized there, and upsampled against itself with '
                                       'the filter of --guided-radius / --guided-eps (in pixels of the working size); the output frames '
                                       'have the input\'s size.  Needs --guided-radius > 0 and --content-size > 0; goes with '
                                       '--content-colors, --guided-upsample-guide and --guided-upsample-frames; not with --guided-guide color, --guided-frames, '
                                       '--swap5, --keep-colors, --mask-path, --alpha-map, --warm-start or --passes > 1')),
    (('--guided-upsample-guide',), dict(choices=['grey', 'color'], default=None,
                                        help='the guide of --guided-upsample: grey (the default), the grey of the frame, or color, its '
                                             'three channels -- brings back edges between colours of equal luminance too.  Needs '
                                             '--guided-upsample')),
    (('--guided-upsample-frames',), dict(type=int, default=0, metavar='T',
                                         help='--guided-upsample with the temporal box, against flicker at full size: the coefficients '
                                              'of the upsampling are formed over the T frames on each side of a frame of the SMALL clip '
                                              '(0 .. 3; 0: off), within every run of consecutive frames of one size; every frame is then '
                                              'delivered against itself.  The radius is then at most 51 / 40 / 33 at T = 1 / 2 / 3.  Needs '
                                              '--guided-upsample; grey guide only')),
    (('--guided-upsample-motion',), dict(choices=['global'], default=None,
                                         help='run --guided-upsample-frames along camera motion: one integer translation per frame, '
                                              'estimated on the frames at the working size (steps within '
                                              '--guided-upsample-motion-range).  Needs --guided-upsample-frames >= 1')),
    (('--guided-upsample-motion-range',), dict(type=int, default=None, metavar='R',
                                               help='the search range of --guided-upsample-motion in pixels of the working size per '
                                                    'frame (1 .. 16; default 8); both sides of the working size must be at least 4 R')),
    (('--passes',), dict(type=int, default=1, help='feed the result back in this many times')),
    (('--device',), dict(default='/gpu:0', help='e.g. /gpu:0')),
    (('--alpha',), dict(type=float, default=1, help='style strength')),
    (('--concat',), dict(action='store_true', default=False, help='put the style image to the left of every frame')),
    (('--swap5',), dict(action='store_true', default=False, help='style-swap at relu5_1')),
    (('--ss-alpha',), dict(type=float, default=0.6, help='style-swap blend')),
    (('--ss-patch-size',), dict(type=int, default=3, help='style-swap patch size')),
    (('--ss-stride',), dict(type=int, default=1, help='style-swap stride')),
    (('--adain',), dict(action='store_true', default=False, help='AdaIN instead of WCT at every level')),
    (('--batch',), dict(type=int, default=16, help='frames per device batch (<= 32)')),
    (('--fps',), dict(type=int, default=30, help='frame rate of the re-encoded video (reference: 30)')),
    (('--synthetic-weights',), dict(type=int, default=None, metavar='SEED', help='seeded synthetic weights instead of files')),
    (('--wct-mode',), dict(choices=['tf', 'np'], default='tf', help='wct_tf (the graph) or wct_np semantics')),
    (('--mask-path',), dict(default=None, metavar='PATH',
                            help='spatial control: one grey label map for all frames, or a directory with one map per frame '
                                 '(matched to the frames in sorted order; the counts must agree).  Grey v picks --mask-styles image '
                                 'v * K // 256; maps are resized (nearest) to the frame.  One output folder, '
                                 '{video}_mask_{style0}+{style1}+...')),
    (('--warm-start',), dict(action='store_true',
                             help='start the content eigensolves of every batch from the last frame of the batch before it (one '
                                  'state for the whole video; frames within tolerance of the cold ones, not bit-identical).  Needs '
                                  'the prepared-style path: not with --keep-colors, --swap5, --adain or --mask-path.  Later --passes '
                                  'run cold')),
    (('--device-resize',), dict(action='store_true', default=False,
                                help='apply --content-size on the device: frames are uploaded raw and resized there (the bytes of '
                                     'the host resize); consecutive frames of one raw size are batched.  Needs --content-size > 0; not '
                                     'with --keep-colors, with --content-colors --passes > 1, or with --swap5 --ss-stride > 1 (each '
                                     'needs the resized frames on the host).  --style-size, --concat and label maps stay on the host')),
    (('--mask-styles',), dict(nargs='+', default=None, metavar='PATH',
                              help='the K style images of --mask-path, label 0 first; replaces --style-path; not with '
                                   '--keep-colors, --swap5 or --concat')),
    (('--style-masks',), dict(nargs='+', default=None, metavar='PATH',
                              help='style regions: one 8-bit grey label map per --mask-styles image (read as --mask-path is), or - for '
                                   'the whole image; frame region k takes its style from the pixels of style k labelled k')),
    (('--alpha-map',), dict(default=None, metavar='PATH',
                            help='a strength map: one 8-bit grey image for all frames, or a directory with one map per frame '
                                 '(matched to the frames in sorted order; the counts must agree), resized (bilinear) to the frame; '
                                 'white takes --alpha, black keeps the frame, greys in between.  With --style-path; not with '
                                 '--swap5, --mask-path, --keep-colors or --passes > 1')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for names, kw in _FLAGS:
        parser.add_argument(*names, **kw)
    return parser


def natural_key(path):
    """frame_2.png before frame_10.png (ffmpeg's %d numbering, stylize_video.py:76)."""
    return [int(t) if t.isdigit() else t for t in re.split(r'(\d+)', os.path.basename(path))]


def list_frames(in_dir):
    return sorted(get_files(in_dir), key=natural_key)


def check_mask_args(parser, args):
    """--mask-path / --mask-styles: the argument errors of a masked video (parser.error exits)."""
    if args.mask_path is None and args.mask_styles is None:
        if args.style_path is None:
            parser.error('--style-path is required (or --mask-path with --mask-styles)')
        return
    if args.mask_path is None or args.mask_styles is None:
        parser.error('--mask-path and --mask-styles go together')
    if args.style_path is not None:
        parser.error('--mask-styles replaces --style-path: give one or the other')
    if args.keep_colors or args.swap5 or args.concat:
        parser.error('--mask-path does not combine with --keep-colors, --swap5 or --concat')
    if len(args.mask_styles) > 8:
        parser.error('--mask-styles takes at most 8 styles')


def check_alpha_map_args(parser, args):
    """--alpha-map: what a strength map does not combine with (parser.error exits)"""
    if args.alpha_map is None:
        return
    on = [('--swap5', args.swap5), ('--mask-path', args.mask_path is not None), ('--keep-colors', args.keep_colors),
          ('--passes > 1', args.passes > 1)]
    bad = [name for name, v in on if v]
    if bad:
        parser.error('--alpha-map does not combine with %s: a strength map goes with one style, WCT or AdaIN, in one pass'
                     % ' / '.join(bad))


def check_warm_args(parser, args):
    """--warm-start: the combinations it refuses (parser.error exits)"""
    if not args.warm_start:
        return
    for flag, on in (('--keep-colors', args.keep_colors), ('--swap5', args.swap5), ('--adain', args.adain),
                     ('--mask-path', args.mask_path is not None)):
        if on:
            parser.error('--warm-start does not combine with %s' % flag)


def check_color_args(parser, args):
    """--content-colors: the combinations it refuses (parser.error exits)"""
    if not args.content_colors:
        return
    if args.keep_colors:
        parser.error('--content-colors and --keep-colors are alternatives: give one')
    if args.passes > 1 and args.swap5 and args.ss_stride != 1:
        parser.error('--content-colors with --passes > 1 needs --ss-stride 1 (a larger stride crops the frames of every pass)')


def check_guided_args(parser, args):
    """--guided-radius / --guided-eps: their ranges, and the combinations they refuse (parser.error exits)"""
    from .stylize import check_guided_args as check
    check(parser, args)
    if args.guided_radius and getattr(args, 'device_resize', False) and args.passes > 1:
        parser.error('--device-resize with --guided-radius needs --passes 1 (the stand-alone filter needs the resized frames on '
                     'the host)')
    check_guided_frames_args(parser, args)


def check_guided_frames_args(parser, args):
    """--guided-frames: its range, the radius it allows, and the combinations it refuses (parser.error exits)"""
    from ._lib import GUIDED_TIME_MAX_RADIUS
    t = getattr(args, 'guided_frames', 0)
    if not 0 <= t < len(GUIDED_TIME_MAX_RADIUS):
        parser.error('--guided-frames must be 0 (off) .. %d frames on each side, got %d' % (len(GUIDED_TIME_MAX_RADIUS) - 1, t))
    motion, search = getattr(args, 'guided_motion', None), getattr(args, 'guided_motion_range', None)
    if motion is not None and not t:
        parser.error('--guided-motion needs --guided-frames >= 1 (it shifts the windows of that filter along time)')
    if getattr(args, 'guided_frames_guide', None) is not None:
        if getattr(args, 'guided_upsample', False):
            parser.error('--guided-frames-guide does not combine with --guided-upsample: the colour guide along time is not served '
                         'under upsampling')
        if not t:
            parser.error('--guided-frames-guide needs --guided-frames >= 1 (it chooses the guide of that filter along time)')
    if search is not None:
        from ._lib import MOTION_MAX_RANGE
        if motion is None or not t:
            parser.error('--guided-motion-range needs --guided-motion with --guided-frames >= 1')
        if not 1 <= search <= MOTION_MAX_RANGE:
            parser.error('--guided-motion-range must be 1 .. %d, got %d' % (MOTION_MAX_RANGE, search))
    if not t:
        return
    if not args.guided_radius:
        parser.error('--guided-frames needs --guided-radius > 0 (it extends that filter along time)')
    if args.guided_radius > GUIDED_TIME_MAX_RADIUS[t]:
        parser.error('--guided-radius must be at most %d with --guided-frames %d, got %d' % (GUIDED_TIME_MAX_RADIUS[t], t, args.guided_radius))
    if args.guided_guide == 'color':
        parser.error('--guided-frames goes with the grey guide of --guided-guide: --guided-guide color has no form along time '
                     '(--guided-frames-guide color chooses the guide of the filter along time)')
    for flag, on in (('--swap5', args.swap5), ('--keep-colors', args.keep_colors), ('--mask-path', args.mask_path is not None)):
        if on:
            parser.error('--guided-frames does not combine with %s' % flag)


def check_upsample_time_args(parser, args):
    """--guided-upsample-frames / -motion / -motion-range: their ranges, what they need and what they refuse (parser.error exits)"""
    from ._lib import GUIDED_TIME_MAX_RADIUS, MOTION_MAX_RANGE
    t = getattr(args, 'guided_upsample_frames', 0)
    motion, search = getattr(args, 'guided_upsample_motion', None), getattr(args, 'guided_upsample_motion_range', None)
    up = getattr(args, 'guided_upsample', False)
    for flag, given in (('--guided-upsample-frames', t != 0), ('--guided-upsample-motion', motion is not None),
                        ('--guided-upsample-motion-range', search is not None)):
        if given and not up:
            parser.error('%s needs --guided-upsample (it extends that upsampling along time)' % flag)
    if not 0 <= t < len(GUIDED_TIME_MAX_RADIUS):
        parser.error('--guided-upsample-frames must be 0 (off) .. %d frames on each side, got %d' % (len(GUIDED_TIME_MAX_RADIUS) - 1, t))
    if motion is not None and not t:
        parser.error('--guided-upsample-motion needs --guided-upsample-frames >= 1 (it shifts the windows of that box along time)')
    if search is not None:
        if motion is None:
            parser.error('--guided-upsample-motion-range needs --guided-upsample-motion with --guided-upsample-frames >= 1')
        if not 1 <= search <= MOTION_MAX_RANGE:
            parser.error('--guided-upsample-motion-range must be 1 .. %d, got %d' % (MOTION_MAX_RANGE, search))
    if not t:
        return
    if args.guided_radius > GUIDED_TIME_MAX_RADIUS[t]:
        parser.error('--guided-radius must be at most %d with --guided-upsample-frames %d, got %d'
                     % (GUIDED_TIME_MAX_RADIUS[t], t, args.guided_radius))
    if getattr(args, 'guided_upsample_guide', None) == 'color':
        parser.error('--guided-upsample-frames goes with the grey guide: --guided-upsample-guide color has no form along time')


def check_resize_args(parser, args):
    """--device-resize: the combinations it refuses (parser.error exits)"""
    if not args.device_resize:
        return
    if args.content_size <= 0:
        parser.error('--device-resize applies --content-size: give --content-size > 0')
    if args.keep_colors:
        parser.error('--device-resize does not combine with --keep-colors (per-frame CORAL needs the resized frame on the host)')
    if args.content_colors and args.passes > 1:
        parser.error('--device-resize with --content-colors needs --passes 1 (the stand-alone colour op needs the resized frames '
                     'on the host)')
    if args.swap5 and args.ss_stride != 1:
        parser.error('--device-resize with --swap5 needs --ss-stride 1 (a larger stride crops the resized frames on the host)')


def device_size(args, group):
    """--device-resize: the size --content-size gives the raw frames of `group` (resize= of the predict_frames calls), else None"""
    if not getattr(args, 'device_resize', False):
        return None
    return resize_shape(group[0].shape[0], group[0].shape[1], args.content_size)


def content_colors_frames(wct_model, stylized, frames):
    """the stand-alone op on a group of frames (after --passes > 1): the luminance of `stylized` on the colours of `frames`"""
    return np.concatenate([wct_model.sess.content_colors_batch(stylized[i:i + 32], frames[i:i + 32])
                           for i in range(0, len(frames), 32)], axis=0)


def guided_frames(wct_model, stylized, frames, guided):
    """the stand-alone filter on a group of frames (after --passes > 1): `stylized` smoothed with `frames` as guides"""
    return np.concatenate([wct_model.sess.guided_filter_batch(stylized[i:i + 32], frames[i:i + 32], guided[0], guided[1],
                                                              guide=guided[2] if len(guided) > 2 else 'grey')
                           for i in range(0, len(frames), 32)], axis=0)


def smooth_clips(batches, frames_t, op, window=32):
    """--guided-frames T on a stream of batches: `batches` yields (files, plain frames [B][..], contents [B][..], per-frame extras)
    in order; a clip is a maximal run of consecutive frames of one size.  Yields the same tuples, the frames filtered along time
    within their clip -- each equal to the whole-clip op, wherever the batches were cut -- by op(plain [F], contents [F], f0, f1)
    -> the filtered frames f0 .. f1 - 1 of a resident clip of F <= `window` frames.  A frame depends on no frame further than 2T
    away, so the buffer holds one chunk of window - 4T frames, 2T frames behind it and what has arrived in front of it (2T are
    needed, except at the clip's end): never the whole video."""
    halo, step = 2 * frames_t, window - 4 * frames_t
    buf, done = [], 0                      # (file, plain, content, extra) from the oldest frame still needed; buf[:done] were yielded

    def flush(final):
        nonlocal buf, done
        while True:
            ready = len(buf) if final else len(buf) - halo          # frames whose look-ahead is there
            if ready - done < (1 if final else step):
                return
            f0, f1 = done, min(ready, done + step)
            g0, g1 = max(0, f0 - halo), min(len(buf), f1 + halo)
            outs = op(np.stack([b[1] for b in buf[g0:g1]]), np.stack([b[2] for b in buf[g0:g1]]), f0 - g0, f1 - g0)
            yield [b[0] for b in buf[f0:f1]], outs, np.stack([b[2] for b in buf[f0:f1]]), [b[3] for b in buf[f0:f1]]
            drop = max(0, f1 - halo)
            buf, done = buf[drop:], f1 - drop

    for files, plain, contents, extras in batches:
        if buf and (plain.shape[1:] != buf[-1][1].shape or contents.shape[1:] != buf[-1][2].shape):
            for item in flush(True):                                # the clip has ended
                yield item
            buf, done = [], 0
        buf.extend(zip(files, plain, contents, extras))
        for item in flush(False):
            yield item
    for item in flush(True):
        yield item


def upsample_clips(batches, frames_t, op, window=32):
    """--guided-upsample-frames T on a stream of batches, in the manner of smooth_clips: `batches` yields (files, small stylized
    frames [B][..], small contents [B][..], full contents [B][..], per-frame extras) in order; a clip is a maximal run of
    consecutive frames of one size.  Yields (files, delivered full-size frames, extras), each frame equal to the whole-clip op
    wherever the batches were cut, by op(small stylized [F], small contents [F], full contents [f1 - f0], f0, f1) -> frames
    f0 .. f1 - 1 of a resident clip of F <= `window` small frames.  The buffer holds the small frames of one chunk, 2T behind it
    and what has arrived in front of it, and the full contents of the undelivered frames only: never the whole video."""
    from .context import upsample_time_chunk
    halo = 2 * frames_t
    buf, done = [], 0                      # [file, small stylized, small content, full content or None, extra]; buf[:done] were delivered

    def flush(final):
        nonlocal buf, done
        while True:
            ready = len(buf) if final else len(buf) - halo          # frames whose look-ahead is there
            full = next(b[3] for b in buf[done:]) if done < len(buf) else None
            step = window - 4 * frames_t if full is None else min(window - 4 * frames_t, upsample_time_chunk(full.shape[0], full.shape[1], 0))
            if ready - done < (1 if final else step):
                return
            f0, f1 = done, min(ready, done + step)
            g0, g1 = max(0, f0 - halo), min(len(buf), f1 + halo)
            outs = op(np.stack([b[1] for b in buf[g0:g1]]), np.stack([b[2] for b in buf[g0:g1]]), np.stack([b[3] for b in buf[f0:f1]]),
                      f0 - g0, f1 - g0)
            yield [b[0] for b in buf[f0:f1]], outs, [b[4] for b in buf[f0:f1]]
            for b in buf[f0:f1]:
                b[3] = None                                         # delivered: only its small frames stay, as halo
            drop = max(0, f1 - halo)
            buf, done = buf[drop:], f1 - drop

    for files, plain, small, full, extras in batches:
        if buf and (plain.shape[1:] != buf[-1][1].shape or small.shape[1:] != buf[-1][2].shape or full.shape[1:] != buf[-1][5]):
            for item in flush(True):                                # the clip has ended
                yield item
            buf, done = [], 0
        buf.extend([f, p, c, C, e, C.shape] for f, p, c, C, e in zip(files, plain, small, full, extras))
        for item in flush(False):
            yield item
    for item in flush(True):
        yield item


def match_masks(mask_path, frame_files, what='label maps'):
    """the label map (or strength map) file of every frame: `mask_path` is one file for all frames, or a directory whose maps are
    matched to the frames in sorted order (natural_key) -- the counts must agree (ValueError, before any GPU work)"""
    if not os.path.isdir(mask_path):
        return [mask_path] * len(frame_files)
    maps = sorted(get_files(mask_path), key=natural_key)
    if len(maps) != len(frame_files):
        raise ValueError('%d %s in %s for %d frames' % (len(maps), what, mask_path, len(frame_files)))
    return maps


def stylize_frames_masked(wct_model, frame_files, mask_files, styles, args):
    """Yield (frame_file, stylized uint8 image) in order, every frame stylized under its own label map: consecutive same-sized
    frames go through WCT.predict_frames_masked in batches, the K styles prepared once for the whole video.  Later --passes use
    the masked call too, the maps resized to each pass's input."""
    from .stylize import load_mask, mask_labels, guided_of, prepare_style_regions
    k = len(styles)
    styles = [np.uint8(np.clip(s, 0, 255)) if s.dtype != np.uint8 else s for s in styles]
    if getattr(args, 'style_masks', None) is not None:
        prepared = prepare_style_regions(wct_model, args.mask_styles, styles, args.style_masks, args)
    else:
        prepared = [wct_model.prepare_style(s, adain=args.adain) for s in styles]
    greys = {}

    def grey_of(path):
        if path not in greys:
            if len(greys) > 64:
                greys.clear()
            greys[path] = load_mask(path)
        return greys[path]

    def load(f):
        img = get_img(f)
        if args.content_size > 0 and not getattr(args, 'device_resize', False):
            img = resize_to(img, args.content_size)
        return img

    try:
        i = 0
        while i < len(frame_files):
            first = load(frame_files[i])
            j, group = i + 1, [first]
            while j < len(frame_files) and len(group) < args.batch:
                nxt = load(frame_files[j])
                if nxt.shape != first.shape:
                    break
                group.append(nxt)
                j += 1
            frames = out = np.stack(group)
            # --content-colors: fused into a single pass; after several plain passes the op runs once, against the input frames
            colors, n = getattr(args, 'content_colors', False), max(1, args.passes)
            guided = guided_of(args)                               # --guided-radius: the same, in front of the colour op
            size = device_size(args, group)                       # --device-resize: pass 1 takes the raw frames
            for _ in range(n):
                masks = np.stack([mask_labels(grey_of(m), k, size or out.shape[1:3]) for m in mask_files[i:j]])
                out = wct_model.predict_frames_masked(out, prepared, masks, args.alpha, args.adain, batch=args.batch,
                                                      content_colors=colors and n == 1, resize=size,
                                                      guided=guided if n == 1 else None)
                size = None
            if guided and n > 1:
                out = guided_frames(wct_model, out, frames, guided)
            if colors and n > 1:
                out = content_colors_frames(wct_model, out, frames)
            for f, o in zip(frame_files[i:j], out):
                yield f, o
            i = j
    finally:
        for h in prepared:
            h.close()


def stylize_frames(wct_model, frame_files, style_img, args, alpha_files=None):
    """Yield (frame_file, stylized uint8 image) in order; consecutive same-sized frames are batched.  alpha_files: the strength map
    file of every frame (--alpha-map), or None."""
    from .stylize import load_alpha_map, strength_map, guided_of, upsample_of
    alpha_of = dict(zip(frame_files, alpha_files)) if alpha_files is not None else {}

    def strengths_of(files, shape_hw):
        """the strength maps [B][h][w] of the frames `files`, resized to the frames' (resized) size"""
        greys = {p: load_alpha_map(p) for p in {alpha_of[f] for f in files}}
        return np.stack([strength_map(greys[alpha_of[f]], shape_hw) for f in files])

    upsample = upsample_of(args)                                  # --guided-upsample: the frames go up raw, at their own size

    def load(f):
        img = get_img(f)
        if args.content_size > 0 and not getattr(args, 'device_resize', False) and upsample is None:
            img = resize_to(img, args.content_size)
        return img

    # the style is the same for every frame: its style side runs once (WCT.prepare_style), not once per batch -- the frames
    # are bit-identical.  Not with --keep-colors (the style differs per frame) or --swap5 (style-swap needs the style's patches).
    prepared = None
    if not args.keep_colors and not args.swap5:
        prepared = wct_model.prepare_style(np.uint8(np.clip(style_img, 0, 255)) if style_img.dtype != np.uint8 else style_img,
                                           adain=args.adain)

    # --warm-start: one state for the whole video, kept across frame-size groups (a covariance is C x C whatever the frame size)
    warm = wct_model.warm_state() if getattr(args, 'warm_start', False) else None

    # --content-colors: fused into a single pass; after several plain passes the op runs once, against the input frames
    colors = getattr(args, 'content_colors', False)
    guided = guided_of(args)                                      # --guided-radius: the same, in front of the colour op
    # --guided-frames T: the batches come out plain (all passes), and the filter along time and then the colour op run on a
    # sliding buffer of them (smooth_clips), so that a frame does not depend on where the batches were cut
    frames_t = getattr(args, 'guided_frames', 0)
    guided_here, colors_here = (None, False) if frames_t else (guided, colors)

    # --guided-upsample-frames T: the frames are resized and stylized plain at the working size, batch by batch, and delivered at
    # full size from a sliding buffer of small frames (upsample_clips), then the colour op: no frame depends on the batches
    up_t = getattr(args, 'guided_upsample_frames', 0) if upsample is not None else 0

    def run_small(frames, style):
        """-> (the frames stylized plain at the working size, their contents at that size)"""
        from .context import upsample_time_chunk, upsample_work_size
        frames = np.ascontiguousarray(frames, np.uint8)
        work = upsample_work_size(frames.shape[1], frames.shape[2], upsample[0])
        step = min(32, upsample_time_chunk(frames.shape[1], frames.shape[2], 0))
        small = np.concatenate([wct_model.sess.resize_batch(frames[k:k + step], work) for k in range(0, len(frames), step)], axis=0)
        return wct_model.predict_frames(small, prepared if prepared is not None else style, args.alpha, adain=args.adain,
                                        batch=args.batch), small

    def run(frames, style, files):
        """-> (the stylized frames, their contents at the size the network saw them)"""
        style = prepared if prepared is not None else style
        if upsample is not None:                              # (one pass, no warm state, no maps: check_upsample_args)
            return wct_model.predict_frames(np.ascontiguousarray(frames, np.uint8), style, args.alpha, adain=args.adain, batch=args.batch,
                                            content_colors=colors, guided_upsample=upsample), frames
        size = device_size(args, frames)
        maps = strengths_of(files, size or frames.shape[1:3]) if alpha_files is not None else None     # (one pass: check_alpha_map_args)
        out = wct_model.predict_frames(frames, style, args.alpha, args.swap5, args.ss_alpha, args.adain, batch=args.batch, warm=warm,
                                       content_colors=colors_here and args.passes <= 1, resize=size, strengths=maps,
                                       guided=guided_here if args.passes <= 1 else None)
        for _ in range(args.passes - 1):                      # later passes: plain WCT, as stylize_video.py:124-126
            out = wct_model.predict_frames(out, style, args.alpha, adain=args.adain, batch=args.batch)
        if guided_here and args.passes > 1:
            out = guided_frames(wct_model, out, frames, guided)
        if colors_here and args.passes > 1:
            out = content_colors_frames(wct_model, out, frames)
        if frames_t and size is not None:                     # --device-resize: the filter's guide is the resized frame
            frames = np.concatenate([wct_model.sess.resize_batch(frames[k:k + 32], size) for k in range(0, len(frames), 32)], axis=0)
        return out, frames

    def batches():
        """(files, stylized frames, their contents, the style of each) of every batch of consecutive same-sized frames, in order"""
        i = 0
        while i < len(frame_files):
            first = load(frame_files[i])
            group_files, group = [frame_files[i]], [first]
            i += 1
            while i < len(frame_files) and len(group) < args.batch:
                nxt = load(frame_files[i])
                if nxt.shape != first.shape:
                    break
                group_files.append(frame_files[i])
                group.append(nxt)
                i += 1
            frames = np.stack(group)
            if args.keep_colors:
                # the style differs per frame (CORAL towards each frame): per-pair batch
                from .ops import preserve_colors_np
                styles = np.stack([preserve_colors_np(style_img, f, ctx=wct_model.sess) for f in group])
                outs = wct_model.sess.stylize_batch(frames, styles, wct_model.relu_targets, alpha=args.alpha,
                                                    adain=args.adain, wct_mode=wct_model.wct_mode,
                                                    guided=guided if args.passes <= 1 else None)
                for _ in range(args.passes - 1):
                    outs = wct_model.sess.stylize_batch(outs, styles, wct_model.relu_targets, alpha=args.alpha,
                                                        adain=args.adain, wct_mode=wct_model.wct_mode)
                if guided and args.passes > 1:
                    outs = guided_frames(wct_model, outs, frames, guided)
                yield group_files, outs, frames, list(styles)
            elif up_t:
                outs, small = run_small(frames, style_img)
                yield group_files, outs, small, frames, [style_img] * len(group)
            else:
                outs, contents = run(frames, style_img, group_files)
                yield group_files, outs, contents, [style_img] * len(group)

    def smooth(plain, contents, f0, f1):
        """frames f0 .. f1 - 1 of a resident clip: the filter along time, then the colour op"""
        positions = None
        if getattr(args, 'guided_motion', None) == 'global':  # the pairs of the resident clip: halo pairs come out the same again
            positions = wct_model.sess.motion_global(contents, getattr(args, 'guided_motion_range', None) or 8)   # (on the grey guide)
        outs = wct_model.sess.guided_filter_time_range(plain, contents, guided[0], guided[1], frames_t, f0, f1, positions=positions,
                                                       guide=getattr(args, 'guided_frames_guide', None) or 'grey')
        return content_colors_frames(wct_model, outs, contents[f0:f1]) if colors else outs

    def deliver(plain, small, full, f0, f1):
        """frames f0 .. f1 - 1 of a resident clip of small frames, at full size against `full`, then the colour op"""
        positions = None
        if getattr(args, 'guided_upsample_motion', None) == 'global':
            positions = wct_model.sess.motion_global(small, getattr(args, 'guided_upsample_motion_range', None) or 8)
        outs = wct_model.sess.guided_upsample_time_range(plain, small, full, upsample[1], upsample[2], up_t, f0, f1, positions=positions)
        return content_colors_frames(wct_model, outs, full) if colors else outs

    if up_t:
        stream = ((files, outs, None, styles) for files, outs, styles in upsample_clips(batches(), up_t, deliver))
    else:
        stream = smooth_clips(batches(), frames_t, smooth) if frames_t else batches()
    for group_files, outs, _, style_per_frame in stream:
        for f, o, s in zip(group_files, outs, style_per_frame):
            if args.concat:                                   # stylize_video.py:129-132
                o = np.hstack([_imresize(s, (o.shape[0], o.shape[0])), o])
            yield f, o
    if warm is not None:
        warm.close()
    if prepared is not None:
        prepared.close()


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_mask_args(parser, args)
    from .stylize import check_style_mask_args
    check_style_mask_args(parser, args)
    check_warm_args(parser, args)
    check_color_args(parser, args)
    check_guided_args(parser, args)
    check_resize_args(parser, args)
    check_alpha_map_args(parser, args)
    from .stylize import check_upsample_args
    check_upsample_args(parser, args, extra=[('--guided-frames (use --guided-upsample-frames)', getattr(args, 'guided_frames', 0) > 0),
                                              ('--warm-start', getattr(args, 'warm_start', False))])
    check_upsample_time_args(parser, args)
    if args.synthetic_weights is None and not args.checkpoints:
        parser.error('--checkpoints is required (stylize.py:17) unless --synthetic-weights SEED is given')
    start = time.time()
    if args.keep_colors and args.swap5:
        raise SystemExit('--keep-colors with --swap5 is not batched here: use stylize.py per frame')

    ffmpeg = shutil.which('ffmpeg')
    is_video = not os.path.isdir(args.in_path)
    if is_video and ffmpeg is None:
        raise SystemExit('--in-path is a file and there is no ffmpeg on PATH: pass a directory of frames')
    in_dir = args.in_path
    if is_video:
        in_dir = os.path.join(args.tmp_dir, 'input')
        os.makedirs(in_dir, exist_ok=True)
        subprocess.check_call([ffmpeg, '-i', args.in_path, '%s/frame_%%d.png' % in_dir])
    frame_files = list_frames(in_dir)
    masked = args.mask_path is not None
    mask_files = match_masks(args.mask_path, frame_files) if masked else None      # (the count check: before any GPU work)
    alpha_files = match_masks(args.alpha_map, frame_files, 'strength maps') if args.alpha_map is not None else None
    weights = None
    if args.synthetic_weights is not None:
        from .weights import synthetic_weights
        weights = synthetic_weights(args.synthetic_weights, relu_targets=args.relu_targets)
    wct_model = WCT(checkpoints=args.checkpoints, relu_targets=args.relu_targets, vgg_path=args.vgg_path,
                    device=args.device, ss_patch_size=args.ss_patch_size, ss_stride=args.ss_stride,
                    weights=weights, wct_mode=args.wct_mode)
    style_files = [None] if masked else (get_files(args.style_path) if os.path.isdir(args.style_path) else [args.style_path])
    os.makedirs(args.out_path, exist_ok=True)

    def load_style(path):
        img = get_img(path)
        if args.style_size > 0:
            img = resize_to(img, args.style_size)
        if args.crop_size > 0:
            img = center_crop(img, args.crop_size)
        return img

    content_prefix, content_ext = os.path.splitext(os.path.basename(os.path.normpath(args.in_path)))
    count = 0
    for style_fullpath in style_files:
        if masked:
            style_prefix = 'mask_' + '+'.join(os.path.splitext(os.path.basename(p))[0] for p in args.mask_styles)
            results = stylize_frames_masked(wct_model, frame_files, mask_files, [load_style(p) for p in args.mask_styles], args)
        else:
            style_prefix = os.path.splitext(os.path.basename(style_fullpath))[0]
            results = stylize_frames(wct_model, frame_files, load_style(style_fullpath), args, alpha_files)
        out_dir = os.path.join(args.tmp_dir, 'sytlized') if is_video else \
            os.path.join(args.out_path, '{}_{}'.format(content_prefix, style_prefix))
        os.makedirs(out_dir, exist_ok=True)
        for f, stylized in results:
            out_f = os.path.join(out_dir, os.path.basename(f))
            save_img(out_f, stylized)
            count += 1
        if is_video:
            out_v = os.path.join(args.out_path, '{}_{}{}'.format(content_prefix, style_prefix, content_ext))
            subprocess.check_call([ffmpeg, '-i', '%s/frame_%%d.png' % out_dir, '-f', 'mp4', '-q:v', '0', '-vcodec', 'mpeg4',
                                   '-r', str(args.fps), '-y', out_v])
            print('Video at: %s' % out_v)
            if not args.keep_tmp:
                shutil.rmtree(out_dir)
    if is_video and not args.keep_tmp:
        shutil.rmtree(args.tmp_dir, ignore_errors=True)
    dt = time.time() - start
    print('Finished stylizing {} frames in {:.1f}s ({:.1f} frames/s incl. image I/O)'.format(count, dt, count / max(dt, 1e-9)))
    return count


if __name__ == '__main__':
    main()
