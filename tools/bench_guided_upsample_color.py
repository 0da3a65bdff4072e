"""Cost of guided upsampling under the colour guide against the grey guide, in one process.

    python tools/bench_guided_upsample_color.py [--rounds R] [--out profiles/guided_upsample_color_bench.json]

The protocol of tools/bench_guided_upsample.py: five levels, alpha 0.8, one prepared style, working size short side 512, r = 8,
eps_q = 650; every route measured in R rounds, the routes alternating within a round (a host clock around calls that end in a
device synchronise); medians, and the spread (max - min) / median of each route's rounds -- the margin a difference has to exceed.
Photos (2048 x 2048 and 4000 x 3000), host image in, host frame out: predict(content, guided_upsample=(512, 8, 650, guide)) with
  guide 'color' and 'grey'.
The op alone: guided_upsample_batch_dev on one resident 512 x 512 frame at ratios 2, 4 and 8 under either guide, CALLS calls between
  two synchronises; ms per call, and the bytes the three launches move over that time -- per SMALL pixel s and c read twice and the
  map written (pass 1), the map read twice and the means written, the means read once (through the cache); per FULL pixel the
  content read and the frame written.  The map is 24 B per small pixel under the grey guide and 48 B under the colour guide.
The colour op on 32 resident frames of 512 x 512 at ratio 2, ms per call and per frame.
The kernels' own times come from a kernel trace in a run of its own (--trace-run: the three launches CALLS times at each ratio and
nothing else; run it under rocprofv3 --kernel-trace --stats).
Nothing is gated on the numbers.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from bench_guided_upsample import CALLS, EPS_Q, OP_SMALL, PHOTO_CALLS, R, RATIOS, SIDE, big_image, measure, spread  # noqa: E402
from wct_tf_amd.context import upsample_work_size  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

PHOTOS = ((2048, 2048), (3000, 4000))
GUIDES = ('color', 'grey')
MAP = {'grey': 24, 'color': 48}
BATCH = 32


def op_bytes(small, n, guide, frames=1):
    m = MAP[guide]
    return frames * (small * small * (2 * 3 + 2 * 3 + m + 2 * m + m + m) + n * n * 6)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'guided_upsample_color_bench.json'))
    ap.add_argument('--skip', nargs='*', default=[], choices=['photos', 'op', 'batch'])
    ap.add_argument('--trace-run', action='store_true', help='only the colour op at each ratio, for a kernel trace; writes nothing')
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    res = {'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'short_side': SIDE, 'radius': R, 'eps_q': EPS_Q, 'cases': {}}

    if not args.trace_run and 'photos' not in args.skip:
        handle = model.prepare_style(synthetic_image(2000, SIDE, SIDE))
        for h, w in PHOTOS:
            content = big_image(1000, h, w)
            routes = {g: (lambda g=g: [model.predict(content, handle, 0.8, guided_upsample=(SIDE, R, EPS_Q, g)) for _ in range(PHOTO_CALLS)])
                      for g in GUIDES}
            ms = measure(routes, rounds, PHOTO_CALLS)
            case = {'working_size': list(upsample_work_size(h, w, SIDE)), 'unit': 'ms per image, host image in, host frame out',
                    'calls_per_timing': PHOTO_CALLS}
            for g, v in ms.items():
                case[g + '_ms'] = round(float(np.median(v)), 3)
                case[g + '_spread'] = spread(v)
            case['color_over_grey'] = round(case['color_ms'] / case['grey_ms'], 4)
            res['cases']['photo_%dx%d' % (w, h)] = case
            print((h, w), case, flush=True)
        handle.close()

    s, c = synthetic_image(3000, OP_SMALL, OP_SMALL), synthetic_image(3001, OP_SMALL, OP_SMALL)
    bufs = []

    def resident(a):
        p = ctx.dev_alloc(a.nbytes)
        bufs.append(p)
        ctx.h2d(p, a)
        return p

    try:
        if args.trace_run or 'op' not in args.skip:
            ds, dc = resident(s), resident(c)
            routes = {}
            for ratio in RATIOS:
                n = OP_SMALL * ratio
                df = resident(big_image(3002, n, n))
                do = ctx.dev_alloc(n * n * 3)
                bufs.append(do)
                for g in (('color',) if args.trace_run else GUIDES):
                    def op(n=n, df=df, do=do, g=g):
                        for _ in range(CALLS):
                            ctx.guided_upsample_batch_dev(ds, OP_SMALL, OP_SMALL, dc, OP_SMALL, OP_SMALL, df, n, n, 1, R, EPS_Q, do, guide=g)
                        ctx.sync()
                    routes[(ratio, g)] = op
            if args.trace_run:
                for fn in routes.values():
                    fn()
                return
            ms = measure(routes, rounds, CALLS)
            op_case = {'small': [OP_SMALL, OP_SMALL], 'calls_per_timing': CALLS}
            for (ratio, g), v in ms.items():
                n, med = OP_SMALL * ratio, float(np.median(v))
                key = 'ratio%d_%s' % (ratio, g)
                op_case[key + '_bytes'] = op_bytes(OP_SMALL, n, g)
                op_case[key + '_ms_per_call'] = round(med, 4)
                op_case[key + '_spread'] = spread(v)
                op_case[key + '_GBps'] = round(op_bytes(OP_SMALL, n, g) / (med * 1e-3) / 1e9, 1)
            res['cases']['op_one_resident_frame'] = op_case
            print('op', op_case, flush=True)

        if 'batch' not in args.skip:
            n = OP_SMALL * 2
            sb = np.stack([np.roll(s, 7 * i, 1) for i in range(BATCH)])
            cb = np.stack([np.roll(c, 7 * i, 1) for i in range(BATCH)])
            full = big_image(3002, n, n)
            fb = np.stack([np.roll(full, 14 * i, 1) for i in range(BATCH)])
            dsb, dcb, dfb = resident(sb), resident(cb), resident(fb)
            dob = ctx.dev_alloc(fb.nbytes)
            bufs.append(dob)

            def batch_op(g):
                for _ in range(CALLS):
                    ctx.guided_upsample_batch_dev(dsb, OP_SMALL, OP_SMALL, dcb, OP_SMALL, OP_SMALL, dfb, n, n, BATCH, R, EPS_Q, dob, guide=g)
                ctx.sync()
            ms = measure({g: (lambda g=g: batch_op(g)) for g in GUIDES}, rounds, CALLS)
            case = {'frames': BATCH, 'small': [OP_SMALL, OP_SMALL], 'full': [n, n], 'calls_per_timing': CALLS,
                    'workspace_bytes_color': BATCH * OP_SMALL * OP_SMALL * 96}
            for g, v in ms.items():
                med = float(np.median(v))
                case[g + '_ms_per_call'] = round(med, 4)
                case[g + '_ms_per_frame'] = round(med / BATCH, 4)
                case[g + '_spread'] = spread(v)
                case[g + '_GBps'] = round(op_bytes(OP_SMALL, n, g, BATCH) / (med * 1e-3) / 1e9, 1)
            res['cases']['op_32_resident_frames'] = case
            print('batch', case, flush=True)
    finally:
        for p in bufs:
            ctx.dev_free(p)
        ctx.close()

    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
