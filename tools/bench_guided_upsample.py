"""Cost of guided upsampling (guided_upsample=(short_side, r, eps_q): stylize small, deliver at the content's size), in one process.

    python tools/bench_guided_upsample.py [--rounds R] [--out profiles/guided_upsample_bench.json]

Five levels, alpha 0.8, one prepared style, working size short side 512, r = 8, eps_q = 650.
Photos (4000 x 3000 and 2048 x 2048), host image in, host frame out, three routes over the same content:
  upsampled  predict(content, guided_upsample=(512, 8, 650))     resize, stylize at 512, upsample to the content's size
  full       predict(content)                                    the same build at full size (in bands past the launch limit)
  small      predict(the content resized to 512 on the host)     the 512-pixel picture alone
The op alone: guided_upsample_batch_dev on one resident 512 x 512 frame at ratios 2, 4 and 8 (1024^2, 2048^2, 4096^2), CALLS calls
between two synchronises; ms per call, and the bytes the three launches move -- per SMALL pixel s and c read twice and the 24-byte
map written (pass 1), the map read twice and the means written; per FULL pixel the content read and the frame written; the means
read once (through the cache) -- over that time.
A video: 64 frames of 1920 x 1080 at batch 8 and 32, upsampled against predict_frames(resize=the working size), ms per frame.
Every route is measured in R rounds; the routes alternate within a round (a host clock around calls that end in a device
synchronise).  Medians, and the spread (max - min) / median of each route's rounds -- the margin a difference has to exceed.
Nothing is gated on the numbers.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd import utils  # noqa: E402
from wct_tf_amd.context import upsample_work_size  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

SIDE, R, EPS_Q = 512, 8, 650
GU = (SIDE, R, EPS_Q)
PHOTOS = ((3000, 4000), (2048, 2048))
PHOTO_CALLS = 3
OP_SMALL = 512
RATIOS = (2, 4, 8)
CALLS = 20
VIDEO = (1080, 1920)
FRAMES = 64


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def big_image(seed, h, w):
    """a synthetic image of any size: a 512-pixel one tiled with mirrored repeats (no seams), plus a slow ramp"""
    base = synthetic_image(seed, 512, 512).astype(np.int32)
    tile = np.concatenate([np.concatenate([base, base[:, ::-1]], 1), np.concatenate([base[::-1], base[::-1, ::-1]], 1)], 0)
    img = np.tile(tile, ((h + 1023) // 1024, (w + 1023) // 1024, 1))[:h, :w]
    ramp = (np.arange(w)[None, :, None] * 40 // w) - 20
    return np.clip(img + ramp, 0, 255).astype(np.uint8)


def measure(routes, rounds, per):
    for fn in routes.values():
        fn()                                   # the warm-up of every route
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed_ms(fn) / per)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'guided_upsample_bench.json'))
    ap.add_argument('--skip', nargs='*', default=[], choices=['photos', 'op', 'video'])
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    handle = model.prepare_style(synthetic_image(2000, SIDE, SIDE))
    res = {'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'short_side': SIDE, 'radius': R, 'eps_q': EPS_Q, 'cases': {}}

    if 'photos' not in args.skip:
        for h, w in PHOTOS:
            content = big_image(1000, h, w)
            work = upsample_work_size(h, w, SIDE)
            small = utils._imresize(content, work)

            def rep(fn):
                return lambda: [fn() for _ in range(PHOTO_CALLS)]

            routes = {'upsampled': rep(lambda: model.predict(content, handle, 0.8, guided_upsample=GU)),
                      'full': rep(lambda: model.predict(content, handle, 0.8)),
                      'small': rep(lambda: model.predict(small, handle, 0.8))}
            ms = measure(routes, rounds, PHOTO_CALLS)
            case = {'working_size': list(work), 'unit': 'ms per image, host image in, host frame out', 'calls_per_timing': PHOTO_CALLS}
            for k, v in ms.items():
                case[k + '_ms'] = round(float(np.median(v)), 3)
                case[k + '_spread'] = spread(v)
            case['upsampled_over_small'] = round(case['upsampled_ms'] / case['small_ms'], 3)
            case['full_over_upsampled'] = round(case['full_ms'] / case['upsampled_ms'], 3)
            res['cases']['photo_%dx%d' % (w, h)] = case
            print((h, w), case, flush=True)

    if 'op' not in args.skip:
        s, c = synthetic_image(3000, OP_SMALL, OP_SMALL), synthetic_image(3001, OP_SMALL, OP_SMALL)
        op_case = {'small': [OP_SMALL, OP_SMALL], 'calls_per_timing': CALLS}
        bufs = {}
        try:
            ds, dc = ctx.dev_alloc(s.nbytes), ctx.dev_alloc(c.nbytes)
            bufs['s'], bufs['c'] = ds, dc
            ctx.h2d(ds, s)
            ctx.h2d(dc, c)
            routes = {}
            for ratio in RATIOS:
                n = OP_SMALL * ratio
                full = big_image(3002, n, n)
                df, do = ctx.dev_alloc(full.nbytes), ctx.dev_alloc(full.nbytes)
                bufs['f%d' % ratio], bufs['o%d' % ratio] = df, do
                ctx.h2d(df, full)

                def op(n=n, df=df, do=do):
                    for _ in range(CALLS):
                        ctx.guided_upsample_batch_dev(ds, OP_SMALL, OP_SMALL, dc, OP_SMALL, OP_SMALL, df, n, n, 1, R, EPS_Q, do)
                    ctx.sync()
                routes[ratio] = op
            ms = measure(routes, rounds, CALLS)
        finally:
            for p in bufs.values():
                ctx.dev_free(p)
        for ratio in RATIOS:
            n = OP_SMALL * ratio
            nbytes = OP_SMALL * OP_SMALL * (2 * 3 + 2 * 3 + 24 + 2 * 24 + 24 + 24) + n * n * 6
            med = float(np.median(ms[ratio]))
            op_case['ratio%d_full' % ratio] = [n, n]
            op_case['ratio%d_bytes' % ratio] = nbytes
            op_case['ratio%d_ms_per_call' % ratio] = round(med, 4)
            op_case['ratio%d_spread' % ratio] = spread(ms[ratio])
            op_case['ratio%d_GBps' % ratio] = round(nbytes / (med * 1e-3) / 1e9, 1)
        res['cases']['op_one_resident_frame'] = op_case
        print('op', op_case, flush=True)

    if 'video' not in args.skip:
        h, w = VIDEO
        base = big_image(4000, h, w + FRAMES * 4)
        video = np.stack([base[:, 4 * i:4 * i + w] for i in range(FRAMES)])             # a pan of 4 pixels per frame
        work = upsample_work_size(h, w, SIDE)
        for batch in (8, 32):
            routes = {'upsampled': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided_upsample=GU),
                      'small': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, resize=work)}
            ms = measure(routes, rounds, FRAMES)
            case = {'frame': [h, w], 'working_size': list(work), 'frames': FRAMES, 'unit': 'ms per frame, host frames in, host frames out'}
            for k, v in ms.items():
                case[k + '_ms_per_frame'] = round(float(np.median(v)), 4)
                case[k + '_spread'] = spread(v)
            case['upsampled_extra_ms_per_frame'] = round(case['upsampled_ms_per_frame'] - case['small_ms_per_frame'], 4)
            res['cases']['video64_1080p_batch%d' % batch] = case
            print(batch, case, flush=True)

    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
