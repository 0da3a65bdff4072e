"""Cost of guided smoothing with the colour guide (guided=(r, eps_q, 'color')) beside the grey guide and the plain call, in a video,
and of the two ops alone, in one process.

    python tools/bench_guided_color.py [--rounds R] [--out profiles/guided_color_bench.json]

64 frames of 512 x 512, five levels, alpha 0.8, one prepared style, at batch 8 and batch 32.  Seven routes over the same frames:
  plain      predict_frames on the prepared style                            (the floor: the same build's unflagged call)
  grey_r     the same call with guided=(r, 650) for r = 4, 16, 64            (guided.hip: two more launches per batch)
  color_r    the same call with guided=(r, 650, 'color')                     (guided_color.hip: 21 sums and a 3 x 3 solve per pixel)
Each route is measured in R rounds of one pass over the video (a host clock around calls that end in a device synchronise); the
routes alternate within a round.  Per batch size: the median ms per frame of each, each over plain, colour over grey in the extra
time, and the spread of each route's rounds, (max - min) / median -- the margin a difference has to exceed.  The colour frames
are checked once against the stand-alone op on the plain ones (they must be equal).
The ops alone: 32 frames of 512 x 512 resident on the device, guided_filter_batch_dev in place, CALLS calls between two
synchronises, alternating over guide and r in the same rounds; ms per call, and the bytes the two launches move (per pixel: s
and c read twice -- the entering and the leaving row of the running sums --, the map of 24 or 48 bytes written once and read
twice, c read and the frame written) over that time.  Nothing is gated on the numbers.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512
FRAMES = 64
RADII = (4, 16, 64)
GUIDES = ('grey', 'color')
EPS_Q = 650
OP_FRAMES = 32
CALLS = 20
MAP_BYTES = {'grey': 24, 'color': 48}


def op_bytes_per_pixel(guide):
    return 2 * 3 + 2 * 3 + 3 * MAP_BYTES[guide] + 3 + 3     # s twice, c twice (pass 1); the map once out, twice in; c and out (pass 2)


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'guided_color_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    style = synthetic_image(2000, S, S)
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(FRAMES)])
    handle = model.prepare_style(style)

    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'video_frames': FRAMES, 'eps_q': EPS_Q,
           'unit': 'ms per frame, host clock around blocking calls over all %d frames' % FRAMES, 'cases': {}}
    for batch in (8, 32):
        routes = {'plain': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch)}
        for r in RADII:
            routes['grey_r%d' % r] = lambda r=r: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=(r, EPS_Q))
            routes['color_r%d' % r] = lambda r=r: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=(r, EPS_Q, 'color'))
        first = {k: fn() for k, fn in routes.items()}                          # also the warm-up of every route
        same = all(bool(np.array_equal(first['color_r%d' % r][i:i + 32],
                                       ctx.guided_filter_batch(first['plain'][i:i + 32], video[i:i + 32], r, EPS_Q, guide='color')))
                   for r in RADII for i in range(0, FRAMES, 32))
        differs = all(not np.array_equal(first['color_r%d' % r], first['grey_r%d' % r]) for r in RADII)
        del first
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn) / FRAMES)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        case = {'color_flagged_equals_op_on_plain': same, 'color_differs_from_grey': differs}
        for k in routes:
            case[k + '_ms_per_frame'] = round(med[k], 4)
            case[k + '_spread'] = spread(ms[k])
            if k != 'plain':
                case[k + '_over_plain'] = round(med[k] / med['plain'], 4)
                case[k + '_extra_ms_per_frame'] = round(med[k] - med['plain'], 4)
        res['cases']['video64_batch%d' % batch] = case
        print(batch, case, flush=True)

    # the ops alone on resident frames
    frames = video[:OP_FRAMES]
    ds, dc = ctx.dev_alloc(frames.nbytes), ctx.dev_alloc(frames.nbytes)
    keys = [(g, r) for r in RADII for g in GUIDES]
    try:
        ctx.h2d(ds, frames[::-1])
        ctx.h2d(dc, frames)

        def op(g, r):
            for _ in range(CALLS):
                ctx.guided_filter_batch_dev(ds, S, S, dc, S, S, OP_FRAMES, r, EPS_Q, ds, guide=g)
            ctx.sync()

        for k in keys:
            op(*k)
        ms = {k: [] for k in keys}
        for _ in range(rounds):
            for k in keys:
                ms[k].append(timed_ms(lambda: op(*k)) / CALLS)
    finally:
        ctx.dev_free(ds)
        ctx.dev_free(dc)
    op_case = {'frames': OP_FRAMES, 'calls_per_timing': CALLS,
               'bytes_per_pixel': {g: op_bytes_per_pixel(g) for g in GUIDES}}
    for g, r in keys:
        med = float(np.median(ms[g, r]))
        op_case['%s_r%d_ms_per_call' % (g, r)] = round(med, 4)
        op_case['%s_r%d_ms_per_frame' % (g, r)] = round(med / OP_FRAMES, 5)
        op_case['%s_r%d_spread' % (g, r)] = spread(ms[g, r])
        op_case['%s_r%d_GBps' % (g, r)] = round(OP_FRAMES * S * S * op_bytes_per_pixel(g) / (med * 1e-3) / 1e9, 1)
    for r in RADII:
        op_case['color_over_grey_r%d' % r] = round(op_case['color_r%d_ms_per_call' % r] / op_case['grey_r%d_ms_per_call' % r], 4)
    res['cases']['op_32_resident_frames'] = op_case
    print('op', op_case, flush=True)
    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
