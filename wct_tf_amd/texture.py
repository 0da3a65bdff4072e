"""`python -m wct_tf_amd.texture ...`: texture synthesis (Li et al. 2017, sec. 4.3) on the MI355X path -- what the reference
ships as `webcam.py --noise` (webcam.py:191-192) and as the commented-out recipe of stylize.py:95-97: a noise image goes through
the pipeline `--passes` times and comes out as a sample of the style's texture.  `--samples N` writes N samples from N
independent noise images of `--seed`; the noise is made on the device and the passes feed each other there, `--batch` samples
per call.  `--style-path` is a file, or a folder (one set of textures per style).  `--interp-styles a b [--interp-weights wa wb]`
in its place interpolates between textures (Fig. 9 of the paper).  Outputs: `{out}/{style}_texture_s{seed}_{sample}.png`, and
`{out}/{a}+{b}_texture_s{seed}_{sample}.png` for a mix.  `--tile` makes the textures seamless (every pass on a torus: the
outputs repeat without a seam; `--size` in multiples of the deepest level's stride), `--tile-preview N` also writes
`{name}_tiled.png`, the tile repeated N x N.  The model flags are those of `wct_tf_amd.stylize`."""
import argparse
import os
import time

import numpy as np

from . import utils
from .stylize import _FLAGS, _listing, _stem, load_style

_CARRIED = ('--checkpoints', '--relu-targets', '--vgg-path', '--synthetic-weights', '--wct-mode', '--device', '--style-size',
            '--crop-size', '--alpha', '--adain', '--out-path')
_NEW = [
    (('--style-path',), dict(dest='style_path', default=None, help='style image, or a folder of them (one set of textures per style)')),
    (('--size',), dict(nargs=2, type=int, default=[256, 256], metavar=('H', 'W'),
                       help='size of the noise images; the first pass can grow it to the pipeline\'s frame size')),
    (('--samples',), dict(type=int, default=1, metavar='N', help='samples 0 .. N-1 of the seed, one output each')),
    (('--seed',), dict(type=int, default=0, metavar='S', help='seed of the noise (uint32)')),
    (('--passes',), dict(type=int, default=3, metavar='P', help='times the image goes through the pipeline (1 .. 16)')),
    (('--noise-smooth',), dict(action='store_true', default=False,
                               help='smooth the noise with the 27 202 27 filter (gaussian_filter(sigma=0.5), stylize.py:95-97)')),
    (('--batch',), dict(type=int, default=16, help='samples per device call (at most 32)')),
    (('--interp-styles',), dict(nargs='+', default=None, metavar='PATH',
                                help='interpolate between the textures of these style images, in the place of --style-path')),
    (('--interp-weights',), dict(nargs='+', type=float, default=None, metavar='W',
                                 help='one weight >= 0 per --interp-styles image, normalised to sum 1 (default: equal)')),
    (('--tile',), dict(action='store_true', default=False,
                       help='seamless textures: every pass runs on a torus, so an output repeats without a seam (--size must be '
                            'multiples of the deepest level\'s stride; not with --interp-styles)')),
    (('--tile-preview',), dict(type=int, default=None, metavar='N',
                               help='with --tile: also write {name}_tiled.png, the tile repeated N x N')),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    for names, kw in _FLAGS:
        if names[0] in _CARRIED:
            parser.add_argument(*names, **kw)
    for names, kw in _NEW:
        parser.add_argument(*names, **kw)
    return parser


def check_texture_args(parser, args):
    """the argument errors of a texture run (parser.error exits)"""
    if args.interp_styles is None:
        if args.interp_weights is not None:
            parser.error('--interp-weights needs --interp-styles')
        if args.style_path is None:
            parser.error('give --style-path or --interp-styles')
    else:
        if args.style_path is not None:
            parser.error('--interp-styles replaces --style-path: give one or the other')
        if len(args.interp_styles) > 8:
            parser.error('--interp-styles takes at most 8 styles')
        if args.interp_weights is not None:
            if len(args.interp_weights) != len(args.interp_styles):
                parser.error('--interp-weights has %d values for %d --interp-styles' % (len(args.interp_weights), len(args.interp_styles)))
            if any(not np.isfinite(w) or w < 0 for w in args.interp_weights):
                parser.error('--interp-weights must be finite and >= 0')
            if not sum(args.interp_weights) > 0:
                parser.error('--interp-weights sum to 0')
    if args.tile_preview is not None:
        if not args.tile:
            parser.error('--tile-preview needs --tile')
        if args.tile_preview < 1:
            parser.error('--tile-preview must be >= 1, got %d' % args.tile_preview)
    if args.tile and args.interp_styles is not None:
        parser.error('--tile takes one style: --interp-styles runs on the single-frame mix path, which has no periodic form')
    if not 1 <= args.passes <= 16:
        parser.error('--passes must be 1 .. 16, got %d' % args.passes)
    if not 1 <= args.batch <= 32:
        parser.error('--batch must be 1 .. 32, got %d' % args.batch)
    if args.samples < 1:
        parser.error('--samples must be >= 1, got %d' % args.samples)
    if min(args.size) < 1:
        parser.error('--size must be two positive integers, got %d %d' % tuple(args.size))
    if not 0 <= args.seed < 1 << 32:
        parser.error('--seed must be a uint32, got %d' % args.seed)
    if args.out_path is None:
        parser.error('--out-path is required')


def texture_name(style_paths, seed, sample):
    """output file of a texture sample: {style}_texture_s{seed}_{sample}.png, the styles of a mix joined by +"""
    return '%s_texture_s%d_%d.png' % ('+'.join(_stem(p) for p in style_paths), seed, sample)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_texture_args(parser, args)
    if args.synthetic_weights is None and not args.checkpoints:
        parser.error('--checkpoints is required unless --synthetic-weights SEED is given')
    from .wct import WCT
    t0 = time.time()
    weights = None
    if args.synthetic_weights is not None:
        from .weights import synthetic_weights
        weights = synthetic_weights(args.synthetic_weights, relu_targets=args.relu_targets)
    model = WCT(checkpoints=args.checkpoints, relu_targets=args.relu_targets, vgg_path=args.vgg_path, device=args.device,
                weights=weights, wct_mode=args.wct_mode)
    os.makedirs(args.out_path, exist_ok=True)
    if args.interp_styles is not None:
        jobs = [(args.interp_styles, [load_style(p, args) for p in args.interp_styles], args.interp_weights)]
    else:
        jobs = [([p], load_style(p, args), None) for p in sorted(_listing(args.style_path))]
    written = 0
    for paths, style, mix_weights in jobs:
        out = model.synthesize(style, args.size, seeds=args.samples, seed=args.seed, passes=args.passes, alpha=args.alpha,
                               adain=args.adain, smooth=args.noise_smooth, batch=args.batch, weights=mix_weights, tile=args.tile)
        for sample, img in enumerate(out):
            target = os.path.join(args.out_path, texture_name(paths, args.seed, sample))
            utils.save_img(target, img)
            written += 1
            print('%d: wrote %s' % (written, target))
            if args.tile_preview is not None:
                preview = target[:-len('.png')] + '_tiled.png'
                utils.save_img(preview, np.tile(img, (args.tile_preview, args.tile_preview, 1)))
                written += 1
                print('%d: wrote %s' % (written, preview))
    print('%d outputs in %.1f s' % (written, time.time() - t0))
    return written


if __name__ == '__main__':
    main()
