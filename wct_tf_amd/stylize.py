"""`python -m wct_tf_amd.stylize ...`: the command line of the reference's stylize.py (stylize.py:14-126) on the
MI355X path.  Flag names, defaults and the output naming `{content}_{style}{ext}` are the reference's; `--checkpoints`
takes TF checkpoint directories or .npz files (see wct.py), `--vgg-path` the .t7 or a .npz, and
`--synthetic-weights SEED` stands in when neither exists.  Under torchrun each rank takes a shard of the content
files (rank_shard); `--gpus N` without a launcher starts the N ranks itself.  `--interp-styles a b [--interp-weights wa wb]`
stylizes with a weighted mix of the styles (Li et al. 2017, sec. 4.2; the reference's README TODO).
`--mask-path M --mask-styles s0 s1 ...` stylizes each region of a grey label map with its own style (the same section,
spatial control): grey value v is label v * K // 256 of K styles.
`--style-masks m0 m1 ...` adds style regions: content region k takes its style from the pixels of style k labelled k.
`--content-colors` keeps every content's colours by luminance-only transfer (Gatys et al. 2016): the result takes its own
luminance and the content's chrominance.  Unlike `--keep-colors` (CORAL on the style) it leaves the style alone, so it goes
with prepared styles and every other option.
`--guided-radius R [--guided-eps E]` is the photo mode: the result is smoothed by a guided filter with the content as guide (He
et al., "Guided Image Filtering"; the post-step of Li et al. 2018's fast photorealistic variant) -- edges where the content has
them, averages where it is flat.  `--guided-guide color` guides it with the content's three channels where the default, `grey`,
takes their grey: it also keeps an edge between two colours of equal luminance, at about three times the filter's cost.  Not in
bands.
`--guided-upsample` (with `--guided-radius` and `--content-size`) stylizes small and delivers at the content's size: the content is
resized on the device to `--content-size`, stylized there, and the filter's coefficients are interpolated and evaluated against the
full content (He & Sun, "Fast Guided Filter"), which returns the content's edges at full sharpness.  `--guided-upsample-guide color`
does so against the content's three channels: edges between colours of equal luminance come back too."""
import argparse
import os
import time

import numpy as np

from . import utils
from .wct import WCT

# (flags, keyword arguments) -- the interface of stylize.py:16-37, then the additions of this path
_FLAGS = [
    (('--checkpoints',), dict(nargs='+', default=None, help='one decoder checkpoint (directory or .npz) per relu target')),
    (('--relu-targets',), dict(nargs='+', required=True, help='relu layers to stylize at, in pipeline order')),
    (('--vgg-path',), dict(default='models/vgg_normalised.t7', help='encoder weights: vgg_normalised.t7 or .npz (stylize.py:19 default)')),
    (('--content-path',), dict(dest='content_path', help='content image, or a folder of them')),
    (('--style-path',), dict(dest='style_path', help='style image, or a folder of them')),
    (('--out-path',), dict(dest='out_path', help='folder the results are written to')),
    (('--keep-colors',), dict(action='store_true', default=False, help='CORAL: give the style the colours of the content first')),
    (('--content-colors',), dict(action='store_true', default=False,
                                 help='luminance-only colour preservation: the result keeps its luminance and takes the colours of '
                                      'the content (the alternative to --keep-colors: not with it).  Fused into the last launch; '
                                      'with --passes > 1 applied once at the end, against the original content')),
    (('--guided-radius',), dict(type=int, default=0, metavar='R',
                                help='guided smoothing, the photo mode: filter the result over a (2R + 1)^2 box with the content as '
                                     'guide (1 .. 64; 0: off).  With --passes > 1 applied once at the end, against the original '
                                     'content; before --content-colors.  Not with --band-rows')),
    (('--guided-eps',), dict(type=float, default=0.01, metavar='E',
                             help='the regulariser of --guided-radius for images in [0,1] (> 0): smaller keeps more edges')),
    (('--guided-guide',), dict(choices=['grey', 'color'], default=None,
                               help='the guide of --guided-radius: grey (the default), the grey of the content, or color, its three '
                                    'channels -- keeps edges between colours of equal luminance too.  Needs --guided-radius > 0')),
    (('--device',), dict(default='/gpu:0', help='e.g. /gpu:0')),
    (('--style-size',), dict(type=int, default=0, help='short side of the style image (0: as is)')),
    (('--crop-size',), dict(type=int, default=0, help='centre-crop the style image to a square of this side (0: no)')),
    (('--content-size',), dict(type=int, default=0, help='short side of the content image (0: as is)')),
    (('--guided-upsample',), dict(action='store_true', default=False,
                                  help='stylize small, deliver at the content\'s size (He & Sun, "Fast Guided Filter"): the content is '
                                       'resized on the device to --content-size, stylized there, and upsampled against the full '
                                       'content with the filter of --guided-radius / --guided-eps (in pixels of the working size); the '
                                       'output has the content\'s own size.  Needs --guided-radius > 0 and --content-size > 0; goes '
                                       'with --content-colors and --guided-upsample-guide; not with --guided-guide color, --swap5, '
                                       '--keep-colors, --interp-styles, --mask-path, --alpha-map, --band-rows > 0 or --passes > 1')),
    (('--guided-upsample-guide',), dict(choices=['grey', 'color'], default=None,
                                        help='the guide of --guided-upsample: grey (the default), the grey of the content, or color, '
                                             'its three channels -- brings back edges between colours of equal luminance too.  Needs '
                                             '--guided-upsample')),
    (('--passes',), dict(type=int, default=1, help='feed the result back in this many times')),
    (('-r', '--random'), dict(type=int, default=0, help='use this many randomly chosen styles of the style folder')),
    (('--alpha',), dict(type=float, default=1, help='style strength: blend of transformed and content features')),
    (('--concat',), dict(action='store_true', default=False, help='put the style image to the left of every result')),
    (('--adain',), dict(action='store_true', default=False, help='AdaIN instead of WCT at every level')),
    (('--swap5',), dict(action='store_true', default=False, help='style-swap at relu5_1')),
    (('--ss-alpha',), dict(type=float, default=0.6, help='style-swap blend')),
    (('--ss-patch-size',), dict(type=int, default=3, help='style-swap patch size')),
    (('--ss-stride',), dict(type=int, default=1, help='style-swap stride')),
    (('--synthetic-weights',), dict(type=int, default=None, metavar='SEED', help='seeded synthetic weights instead of files')),
    (('--wct-mode',), dict(choices=['tf', 'np'], default='tf', help='wct_tf (the graph) or wct_np semantics')),
    (('--interp-styles',), dict(nargs='+', default=None, metavar='PATH',
                                help='interpolate between these style images (Li et al. 2017, sec. 4.2): one output per '
                                     'content, named {content}_{style1}+{style2}+...; not with --style-path / -r')),
    (('--interp-weights',), dict(nargs='+', type=float, default=None, metavar='W',
                                 help='one weight >= 0 per --interp-styles image, normalised to sum 1 (default: equal)')),
    (('--mask-path',), dict(default=None, metavar='PATH',
                            help='spatial control (Li et al. 2017, sec. 4.2): an 8-bit grey label map, resized (nearest) to each '
                                 'content; grey v picks --mask-styles image v * K // 256.  One output per content, named '
                                 '{content}_mask_{style0}+{style1}+...')),
    (('--mask-styles',), dict(nargs='+', default=None, metavar='PATH',
                              help='the K style images of --mask-path, label 0 first; not with --style-path / -r / '
                                   '--interp-styles / --concat')),
    (('--style-masks',), dict(nargs='+', default=None, metavar='PATH',
                              help='style regions: one 8-bit grey label map per --mask-styles image (resized, nearest, to it; read '
                                   'as --mask-path is: grey v is label v * K // 256), or - for the whole image.  Content region k then '
                                   'takes its style from the pixels of style k labelled k.  The same image and map for several k '
                                   '(one photo, one segmentation) is prepared once.  Not with --keep-colors or --swap5')),
    (('--alpha-map',), dict(default=None, metavar='PATH',
                            help='a strength map: an 8-bit grey image, resized (bilinear) to each content; white takes --alpha, '
                                 'black keeps the content, greys in between.  With --style-path; not with --swap5, '
                                 '--interp-styles, --mask-path, --keep-colors, --passes > 1 or --band-rows')),
    (('--band-rows',), dict(type=int, default=0, metavar='N',
                            help='image rows per band (a multiple of 16) of the banded call, which takes contents of any size; 0: '
                                 'only for a content past the limit of one launch (8.4 MP with relu1_1, 16.7 MP without), at the '
                                 'automatic height.  Not with --adain, --swap5, --interp-styles or --mask-path')),
    (('--gpus',), dict(type=int, default=0, metavar='N',
                       help='shard the content files over N GPUs of this node, one process per GPU: started here when no '
                            'launcher did (0: whatever the launcher set, else one GPU)')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for names, kw in _FLAGS:
        parser.add_argument(*names, **kw)
    return parser


def rank_shard(items, environ=None):
    """One process per GPU (`torchrun --nproc-per-node N -m wct_tf_amd.stylize ...`): rank r of WORLD_SIZE takes a
    contiguous shard of the content files and writes its own outputs -- independent pairs, no collective.
    Returns (shard, device or None): the device string follows LOCAL_RANK when the launcher set it."""
    env = os.environ if environ is None else environ
    world, rank = int(env.get('WORLD_SIZE', '1')), int(env.get('RANK', '0'))
    if world <= 1:
        return list(items), None
    from .dist import shard_range
    lo, hi = shard_range(len(items), world, rank)
    local = int(env.get('LOCAL_RANK', str(rank)))
    if env.get('WCT_BENCH_SHARE_GPU'):                       # dry run on a box with fewer GPUs than ranks
        import torch
        local %= max(1, torch.cuda.device_count())
    return list(items)[lo:hi], '/gpu:%d' % local


def _listing(path):
    return utils.get_files(path) if os.path.isdir(path) else [path]


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def load_style(path, args):
    """style image after --style-size / --crop-size (stylize.py:76-83)"""
    img = utils.get_img(path)
    if args.style_size > 0:
        img = utils.resize_to(img, args.style_size)
    if args.crop_size > 0:
        img = utils.center_crop(img, args.crop_size)
    return img


MAX_PREPARED = 64        # prepared styles alive at once in the --style-path loop (each keeps its image and states on the device)


def can_prepare(args):
    """may the styles of this run be prepared once (WCT.prepare_style) instead of once per content?  Not with --keep-colors
    (CORAL makes the style depend on the content) or --swap5 (style-swap needs the style's patches)."""
    return not args.keep_colors and not args.swap5


def check_color_args(parser, args):
    """--content-colors: the combinations it refuses (parser.error exits)"""
    if not args.content_colors:
        return
    if args.keep_colors:
        parser.error('--content-colors and --keep-colors are alternatives: give one')
    if args.passes > 1 and args.swap5 and args.ss_stride != 1:
        parser.error('--content-colors with --passes > 1 needs --ss-stride 1 (a larger stride crops the content of every pass)')


def check_guided_args(parser, args):
    """--guided-radius / --guided-eps / --guided-guide: their ranges (parser.error exits)"""
    from ._lib import GUIDED_MAX_RADIUS
    if getattr(args, 'guided_guide', None) is not None and not args.guided_radius > 0:
        parser.error('--guided-guide needs --guided-radius > 0 (it chooses the guide of that filter)')
    if not 0 <= args.guided_radius <= GUIDED_MAX_RADIUS:
        parser.error('--guided-radius must be 0 (off) .. %d, got %d' % (GUIDED_MAX_RADIUS, args.guided_radius))
    if not (np.isfinite(args.guided_eps) and args.guided_eps > 0):
        parser.error('--guided-eps must be > 0, got %r' % (args.guided_eps,))
    if args.guided_radius and args.passes > 1 and args.swap5 and args.ss_stride != 1:
        parser.error('--guided-radius with --passes > 1 needs --ss-stride 1 (a larger stride crops the content of every pass)')


def check_upsample_args(parser, args, extra=()):
    """--guided-upsample: what it needs and what it does not combine with (parser.error exits).  extra: further (option, given)
    pairs of the calling command line"""
    if not getattr(args, 'guided_upsample', False):
        if getattr(args, 'guided_upsample_guide', None) is not None:
            parser.error('--guided-upsample-guide needs --guided-upsample (it chooses the guide of that upsampling)')
        return
    if not args.guided_radius > 0:
        parser.error('--guided-upsample needs --guided-radius > 0 (the upsampling is that filter, in pixels of the working size)')
    if not args.content_size > 0:
        parser.error('--guided-upsample needs --content-size > 0 (the short side of the working size)')
    on = [('--guided-guide color', getattr(args, 'guided_guide', None) == 'color'), ('--swap5', args.swap5),
          ('--keep-colors', args.keep_colors), ('--interp-styles', getattr(args, 'interp_styles', None) is not None),
          ('--mask-path', getattr(args, 'mask_path', None) is not None), ('--alpha-map', getattr(args, 'alpha_map', None) is not None),
          ('--band-rows > 0', getattr(args, 'band_rows', 0) > 0), ('--passes > 1', args.passes > 1)] + list(extra)
    for flag, given in on:
        if given:
            parser.error('--guided-upsample does not combine with %s: it takes one style, WCT or AdaIN, in one pass, under the grey '
                         'guide%s' % (flag, ' (--guided-upsample-guide color chooses the guide of the upsampling)'
                                      if flag == '--guided-guide color' else ''))


def upsample_of(args):
    """(short_side, radius, eps_q) of --guided-upsample with --content-size and --guided-radius / --guided-eps -- (short_side,
    radius, eps_q, 'color') with --guided-upsample-guide color; None: off"""
    if not getattr(args, 'guided_upsample', False):
        return None
    up = (args.content_size,) + tuple(guided_of(args)[:2])
    return up + ('color',) if getattr(args, 'guided_upsample_guide', None) == 'color' else up


def guided_of(args):
    """(radius, eps_q) of --guided-radius / --guided-eps, eps in grey levels squared and at most 65025 -- (radius, eps_q, 'color')
    with --guided-guide color; None: off"""
    from ._lib import guided_eps_q, GUIDED_MAX_EPS
    r = getattr(args, 'guided_radius', 0)
    if not r:
        return None
    g = (r, min(GUIDED_MAX_EPS, guided_eps_q(getattr(args, 'guided_eps', 0.01))))
    return g + ('color',) if getattr(args, 'guided_guide', None) == 'color' else g


def _unbanded(args):
    """the options of this run that the banded call does not serve"""
    on = [('--adain', args.adain), ('--swap5', args.swap5), ('--interp-styles', args.interp_styles is not None),
          ('--mask-path', args.mask_path is not None), ('--alpha-map', getattr(args, 'alpha_map', None) is not None),
          ('--guided-radius', getattr(args, 'guided_radius', 0) != 0)]
    return [name for name, v in on if v]


def check_band_args(parser, args):
    """--band-rows: 0 or a positive multiple of 16, and none of the options the banded call does not serve (parser.error exits)"""
    if args.band_rows < 0 or args.band_rows % 16:
        parser.error('--band-rows must be 0 (automatic, only when needed) or a positive multiple of 16, got %d' % args.band_rows)
    if args.band_rows and _unbanded(args):
        parser.error('--band-rows does not combine with %s: the banded call takes whiten-colour transforms on one style'
                     % ' / '.join(_unbanded(args)))


def check_content_fits(parser, args, content, path):
    """A content past the limit of one launch runs in bands, which some options do not: a clear error, not the library's refusal"""
    if not _unbanded(args):
        return
    from .context import band_rows
    need = band_rows(content.shape[0], content.shape[1], args.relu_targets)
    if need:
        parser.error('%s is %dx%d: past the limit of one launch (a map of 2^31 bytes), it runs in bands (--band-rows, here %d), '
                     'which %s does not; try --content-size' % (path, content.shape[0], content.shape[1], need, ' / '.join(_unbanded(args))))


def run_passes(model, content, args, predict):
    """`--passes` predictions from `content`, predict(image, content_colors) -> image.  --content-colors is fused into the
    prediction of a single pass; several passes run plain (a later pass sees a stylized input, not the content) and the
    stand-alone op then runs once, against the original content -- at one pass the two routes give the same bits.
    --guided-radius is treated the same way, and runs before the colour op; only then is predict called with a third argument,
    predict(image, content_colors, guided): (radius, eps_q[, 'color']) for the single pass, None for each of several."""
    n = max(1, args.passes)
    colors = getattr(args, 'content_colors', False)
    guided = guided_of(args)
    out = content
    for _ in range(n):
        out = predict(out, colors and n == 1, guided if n == 1 else None) if guided else predict(out, colors and n == 1)
    if guided and n > 1:
        from .ops import guided_filter_np
        out = guided_filter_np(out, content, guided[0], guided[1], ctx=model.sess, **({'guide': guided[2]} if len(guided) > 2 else {}))
    if colors and n > 1:
        from .ops import content_colors_np
        out = content_colors_np(out, content, ctx=model.sess)
    return out


def check_alpha_map_args(parser, args):
    """--alpha-map: what a strength map does not combine with (parser.error exits)"""
    if args.alpha_map is None:
        return
    on = [('--swap5', args.swap5), ('--interp-styles', args.interp_styles is not None), ('--mask-path', args.mask_path is not None),
          ('--keep-colors', args.keep_colors), ('--passes > 1', args.passes > 1), ('--band-rows', getattr(args, 'band_rows', 0) != 0)]
    bad = [name for name, v in on if v]
    if bad:
        parser.error('--alpha-map does not combine with %s: a strength map goes with one style, WCT or AdaIN, in one pass on the '
                     'whole image' % ' / '.join(bad))


def load_alpha_map(path):
    """the strength map file as 8-bit grey [H][W]"""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('L'))


def strength_map(grey, shape_hw):
    """the strength map [h][w] of a grey image: resized with Pillow's bilinear filter to shape_hw"""
    from PIL import Image
    h, w = (int(v) for v in shape_hw[:2])
    g = np.asarray(grey, np.uint8)
    if g.shape != (h, w):
        g = np.array(Image.fromarray(g).resize((w, h), Image.BILINEAR))
    return np.ascontiguousarray(g)


def stylize_pair(model, content, style, args, prepared=None, alpha_grey=None):
    """one output image: optional CORAL, `--passes` predictions, optional `--concat` (stylize.py:85-110).  prepared: the
    PreparedStyle of `style` (can_prepare), or None.  alpha_grey: the grey image of --alpha-map, or None"""
    if args.keep_colors:
        from .ops import preserve_colors_np
        style = preserve_colors_np(style, content, ctx=model.sess)
    if upsample_of(args) is not None:      # (one pass, one style, the content at its own size: check_upsample_args)
        out = model.predict(content, style if prepared is None else prepared, args.alpha, adain=args.adain,
                            content_colors=getattr(args, 'content_colors', False), guided_upsample=upsample_of(args))
    elif alpha_grey is not None:           # (one pass, no swap5, no bands: check_alpha_map_args)
        out = model.predict(content, style if prepared is None else prepared, args.alpha, adain=args.adain,
                            content_colors=getattr(args, 'content_colors', False), strength=strength_map(alpha_grey, content.shape[:2]),
                            guided=guided_of(args))
    else:
        out = run_passes(model, content, args, lambda img, colors, guided=None: model.predict(
            img, style if prepared is None else prepared, args.alpha, args.swap5, args.ss_alpha, args.adain, content_colors=colors,
            band_rows=getattr(args, 'band_rows', 0) or None, guided=guided))
    if args.concat:
        side = out.shape[0]
        out = np.hstack([utils._imresize(style, (side, side)), out])
    return out


def check_interp_args(parser, args):
    """--interp-styles / --interp-weights: the argument errors of a style mix (parser.error exits)."""
    if args.interp_styles is None:
        if args.interp_weights is not None:
            parser.error('--interp-weights needs --interp-styles')
        return
    if args.style_path is not None or args.random > 0:
        parser.error('--interp-styles replaces --style-path and -r/--random: give one or the other')
    if args.swap5 and len(args.interp_styles) > 1:
        parser.error('--swap5 takes one style: style-swap is not linear in the style')
    if args.interp_weights is not None:
        if len(args.interp_weights) != len(args.interp_styles):
            parser.error('--interp-weights has %d values for %d --interp-styles' % (len(args.interp_weights), len(args.interp_styles)))
        if any(not np.isfinite(w) or w < 0 for w in args.interp_weights):
            parser.error('--interp-weights must be finite and >= 0')
        if not sum(args.interp_weights) > 0:
            parser.error('--interp-weights sum to 0')
    if len(args.interp_styles) > 8:
        parser.error('--interp-styles takes at most 8 styles')


def interp_name(content_path, style_paths):
    """output file of a style mix: {content}_{style1}+{style2}+...{ext of the content}"""
    return '%s_%s%s' % (_stem(content_path), '+'.join(_stem(p) for p in style_paths), os.path.splitext(content_path)[1])


def stylize_mix_pair(model, content, styles, args, prepared=None):
    """one output of a style mix: stylize_pair with every style taking part -- CORAL per style (--keep-colors), `--passes`
    mixes, and --concat with the K styles to the left of the result.  prepared: the PreparedStyle objects of `styles`, or None"""
    if args.keep_colors:
        from .ops import preserve_colors_np
        styles = [preserve_colors_np(s, content, ctx=model.sess) for s in styles]
    out = run_passes(model, content, args, lambda img, colors, guided=None: model.predict_mix(
        img, styles if prepared is None else prepared, args.interp_weights, args.alpha, args.adain, args.swap5, args.ss_alpha,
        content_colors=colors, guided=guided))
    if args.concat:
        side = out.shape[0]
        out = np.hstack([utils._imresize(s, (side, side)) for s in styles] + [out])
    return out


def check_mask_args(parser, args):
    """--mask-path / --mask-styles: the argument errors of spatial control (parser.error exits)."""
    if args.mask_path is None and args.mask_styles is None:
        return
    if args.mask_path is None or args.mask_styles is None:
        parser.error('--mask-path and --mask-styles go together')
    if args.style_path is not None or args.random > 0:
        parser.error('--mask-styles replaces --style-path and -r/--random: give one or the other')
    if args.interp_styles is not None:
        parser.error('--mask-path does not combine with --interp-styles')
    if args.concat:
        parser.error('--concat takes one style: not with --mask-path')
    if args.swap5 and len(args.mask_styles) > 1:
        parser.error('--swap5 takes one style: style-swap is not a per-region affine map')
    if len(args.mask_styles) > 8:
        parser.error('--mask-styles takes at most 8 styles')


def check_style_mask_args(parser, args):
    """--style-masks: the argument errors of style regions (parser.error exits)."""
    if getattr(args, 'style_masks', None) is None:
        return
    if args.mask_styles is None:
        parser.error('--style-masks needs --mask-styles (and --mask-path): one label map per style of a masked run')
    if len(args.style_masks) != len(args.mask_styles):
        parser.error('--style-masks has %d maps for %d --mask-styles (one per style; - for the whole image)'
                     % (len(args.style_masks), len(args.mask_styles)))
    if args.keep_colors:
        parser.error('--style-masks does not combine with --keep-colors (CORAL makes the style depend on the content)')
    if args.swap5:
        parser.error('--style-masks does not combine with --swap5 (style-swap needs the patches of a style image)')


def prepare_style_regions(model, style_paths, styles, mask_paths, args):
    """The K prepared styles of a run with --style-masks: style k from label k of its map (- : the whole image).  Entries with the
    same image file and the same map file are prepared together, once (WCT.prepare_style_regions).  A region too small to carry a
    style -- fewer than 2 feature pixels at some relu target -- falls back to its whole image, with one line on stderr."""
    import sys
    from .context import region_rows
    if args.keep_colors or args.swap5:
        raise ValueError('style regions do not combine with keep_colors (the style depends on the content) or swap5')
    k = len(styles)
    labels = [None if m == '-' else mask_labels(load_mask(m), k, styles[j].shape[:2]) for j, m in enumerate(mask_paths)]
    handles = [None] * k
    for j in range(k):
        if handles[j] is not None:
            continue
        if labels[j] is not None and min(region_rows(labels[j], j, r) for r in model.relu_targets) < 2:
            print('style region %d of %s is too small to carry a style: using the whole image' % (j, style_paths[j]), file=sys.stderr)
            labels[j] = None
        if labels[j] is None:
            handles[j] = model.prepare_style(styles[j], adain=args.adain)
            continue
        same = [i for i in range(j, k) if (style_paths[i], mask_paths[i]) == (style_paths[j], mask_paths[j])
                and min(region_rows(labels[j], i, r) for r in model.relu_targets) >= 2]
        if len(same) > 1:
            made = model.prepare_style_regions(styles[j], labels[j], k, adain=args.adain)
            for i, h in enumerate(made):
                if i in same:
                    handles[i] = h
                elif h is not None:
                    h.close()
        else:
            handles[j] = model.prepare_style(styles[j], adain=args.adain, region=(labels[j], j))
    return handles


def mask_name(content_path, style_paths):
    """output file of a masked stylization: {content}_mask_{style0}+{style1}+...{ext of the content}"""
    return '%s_mask_%s%s' % (_stem(content_path), '+'.join(_stem(p) for p in style_paths), os.path.splitext(content_path)[1])


def load_mask(path):
    """the label map file as 8-bit grey [H][W]"""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('L'))


def mask_labels(grey, k, shape_hw):
    """labels [h][w] of a grey map for k styles: resized (nearest) to shape_hw, then grey v -> v * k // 256 (black: style 0,
    white: style k - 1; k equal bands of grey)"""
    from PIL import Image
    h, w = (int(v) for v in shape_hw[:2])
    g = np.asarray(grey, np.uint8)
    if g.shape != (h, w):
        g = np.array(Image.fromarray(g).resize((w, h), Image.NEAREST))
    return np.uint8(g.astype(np.int32) * k // 256)


def stylize_mask_pair(model, content, grey, styles, args, prepared=None):
    """one output of spatial control: stylize_pair with a style per region -- CORAL per style (--keep-colors), and `--passes`
    masked predictions, the mask resized to each pass's input (a pass's output can be larger than its input).  prepared: the
    PreparedStyle objects of `styles` (can_prepare), or None"""
    if args.keep_colors:
        from .ops import preserve_colors_np
        styles = [preserve_colors_np(s, content, ctx=model.sess) for s in styles]
    return run_passes(model, content, args, lambda img, colors, guided=None: model.predict_masked(
        img, styles if prepared is None else prepared, mask_labels(grey, len(styles), img.shape[:2]), args.alpha, args.adain,
        args.swap5, args.ss_alpha, content_colors=colors, guided=guided))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_interp_args(parser, args)
    check_mask_args(parser, args)
    check_style_mask_args(parser, args)
    check_color_args(parser, args)
    check_guided_args(parser, args)
    check_band_args(parser, args)
    check_alpha_map_args(parser, args)
    check_upsample_args(parser, args)
    if args.synthetic_weights is None and not args.checkpoints:
        parser.error('--checkpoints is required (stylize.py:17) unless --synthetic-weights SEED is given')
    if args.gpus > 0:
        # --gpus N means N ranks: agree with a launcher's WORLD_SIZE, or start the ranks from here (dist.resolve_world)
        from .dist import resolve_world, launch_ranks
        import sys
        role = resolve_world(args.gpus, share_gpu=bool(os.environ.get('WCT_BENCH_SHARE_GPU')))
        if role[0] == 'launch':
            rc = launch_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv), module='wct_tf_amd.stylize')
            if rc:
                raise SystemExit(rc)
            return None
    t0 = time.time()
    weights = None
    if args.synthetic_weights is not None:
        from .weights import synthetic_weights
        weights = synthetic_weights(args.synthetic_weights, relu_targets=args.relu_targets)
    contents, device = rank_shard(sorted(_listing(args.content_path)))
    model = WCT(checkpoints=args.checkpoints, relu_targets=args.relu_targets, vgg_path=args.vgg_path,
                device=device or args.device, ss_patch_size=args.ss_patch_size, ss_stride=args.ss_stride,
                weights=weights, wct_mode=args.wct_mode)
    os.makedirs(args.out_path, exist_ok=True)
    written = 0
    if args.interp_styles is not None:
        mix = [load_style(p, args) for p in args.interp_styles]
        prepared = [model.prepare_style(s, adain=args.adain) for s in mix] if can_prepare(args) and contents else None
        for cpath in contents:
            content = utils.get_img(cpath)
            if args.content_size > 0:
                content = utils.resize_to(content, args.content_size)
            check_content_fits(parser, args, content, cpath)
            target = os.path.join(args.out_path, interp_name(cpath, args.interp_styles))
            utils.save_img(target, stylize_mix_pair(model, content, mix, args, prepared))
            written += 1
            print('%d: wrote %s' % (written, target))
        print('%d outputs in %.1f s' % (written, time.time() - t0))
        return written
    if args.mask_path is not None:
        grey = load_mask(args.mask_path)
        regions = [load_style(p, args) for p in args.mask_styles]
        # every style once for a folder of contents, not once per content (not with --keep-colors or --swap5: can_prepare)
        if args.style_masks is not None:                      # style regions live in handles: prepared even for one content
            prepared = prepare_style_regions(model, args.mask_styles, regions, args.style_masks, args) if contents else None
        else:
            prepared = [model.prepare_style(s, adain=args.adain) for s in regions] if can_prepare(args) and len(contents) > 1 else None
        for cpath in contents:
            content = utils.get_img(cpath)
            if args.content_size > 0:
                content = utils.resize_to(content, args.content_size)
            check_content_fits(parser, args, content, cpath)
            target = os.path.join(args.out_path, mask_name(cpath, args.mask_styles))
            utils.save_img(target, stylize_mask_pair(model, content, grey, regions, args, prepared))
            written += 1
            print('%d: wrote %s' % (written, target))
        for h in prepared or []:
            h.close()
        print('%d outputs in %.1f s' % (written, time.time() - t0))
        return written
    styles = _listing(args.style_path)
    if os.path.isdir(args.style_path) and args.random > 0:
        styles = list(np.random.choice(styles, args.random))
    # every style once, not once per content: the whole style side of every further pair (the first MAX_PREPARED styles of a
    # large folder; the others go as images, as before)
    loaded, n_prepared = {}, 0
    alpha_grey = load_alpha_map(args.alpha_map) if args.alpha_map is not None else None
    for cpath in contents:
        content = utils.get_img(cpath)
        if args.guided_upsample:           # the content goes up at its own size; the network sees --content-size
            content = np.ascontiguousarray(content, np.uint8)
        else:
            if args.content_size > 0:
                content = utils.resize_to(content, args.content_size)
            check_content_fits(parser, args, content, cpath)
        for spath in styles:
            if spath not in loaded:
                style = load_style(spath, args)
                prepare = can_prepare(args) and len(contents) > 1 and n_prepared < MAX_PREPARED
                loaded[spath] = (style, model.prepare_style(style, adain=args.adain) if prepare else None)
                n_prepared += prepare
            style, prepared = loaded[spath]
            result = stylize_pair(model, content, style, args, prepared, alpha_grey)
            target = os.path.join(args.out_path, '%s_%s%s' % (_stem(cpath), _stem(spath), os.path.splitext(cpath)[1]))
            utils.save_img(target, result)
            written += 1
            print('%d: wrote %s' % (written, target))
    print('%d outputs in %.1f s' % (written, time.time() - t0))
    return written


if __name__ == '__main__':
    main()
