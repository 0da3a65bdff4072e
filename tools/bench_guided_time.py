"""Cost of temporal guided smoothing (guided_frames=T) in a video, and of the op alone, in one process.

    python tools/bench_guided_time.py [--rounds R] [--out profiles/guided_time_bench.json]

The op alone: 32 frames of 512 x 512 resident on the device, guided_filter_time_batch_dev on the whole clip in place at T = 1, 2, 3
and r = 4, 16, 33, beside guided_filter_batch_dev (the 2-D op) at the same r, CALLS calls between two synchronises; the routes
alternate within a round.  ms per call, each T over the 2-D op, and the spread of each route's rounds, (max - min) / median --
the margin a difference has to exceed.  Every route's output (one out-of-place call on the same frames) is checked equal to the
NumPy oracle of tests/.
A 64-frame video of 512 x 512, five levels, alpha 0.8, one prepared style, at batch 8 and batch 32, r = 4:
  plain       predict_frames on the prepared style
  fused_t0    guided=(4, 650): the per-frame filter at the end of every batch, on the device (T = 0)
  frames_t1/3 guided=(4, 650), guided_frames=1 / 3: the plain frames come back to the host, go up again in chunks with halos
              through the filter along time, and come back
  filter_t1/3 that second trip alone (ops.guided_filter_time_np on the plain frames): upload, kernels, download
ms per frame of each (a host clock around calls that end in a device synchronise), and for T = 1 and 3 how the extra cost over
`plain` splits into the kernels (the op alone, per frame, at the same r and T) and the rest: the extra host round trip.  The
frames of every timed route are checked equal to the op applied to the plain frames.  Nothing is gated on the numbers.  Writes one
JSON file and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import guided_oracle  # noqa: E402
import guided_time_oracle  # noqa: E402
from wct_tf_amd.ops import guided_filter_time_np  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512
FRAMES = 64
RADII = (4, 16, 33)
TS = (1, 2, 3)
VIDEO_R = 4
EPS_Q = 650
OP_FRAMES = 32
CALLS = 10


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def bench_op(ctx, frames, rounds):
    """the op alone on resident frames -> the JSON case"""
    s = frames[::-1].copy()
    ds, dc, do = ctx.dev_alloc(s.nbytes), ctx.dev_alloc(frames.nbytes), ctx.dev_alloc(s.nbytes)
    routes = [(r, t) for r in RADII for t in (0,) + TS]
    try:
        ctx.h2d(dc, frames)

        def call(r, t, out):
            if t == 0:
                ctx.guided_filter_batch_dev(ds, S, S, dc, S, S, OP_FRAMES, r, EPS_Q, out)
            else:
                ctx.guided_filter_time_batch_dev(ds, S, S, dc, S, S, OP_FRAMES, r, EPS_Q, t, 0, OP_FRAMES, out)

        same = {}
        got = np.empty_like(s)
        for r, t in routes:                                                   # the check, out of place on the same frames
            ctx.h2d(ds, s)
            call(r, t, do)
            ctx.sync()
            ctx.d2h(got, do)
            want = guided_oracle.guided_filter(s, frames, r, EPS_Q) if t == 0 else guided_time_oracle.guided_filter_time(s, frames, r, EPS_Q, t)
            same['r%d_t%d' % (r, t)] = bool(np.array_equal(got, want))
            print('op check', r, t, same['r%d_t%d' % (r, t)], flush=True)

        def op(r, t):
            for _ in range(CALLS):
                call(r, t, ds)
            ctx.sync()

        ctx.h2d(ds, s)
        for r, t in routes:
            op(r, t)                                                          # warm-up
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k in routes:
                ms[k].append(timed_ms(lambda: op(*k)) / CALLS)
    finally:
        for p in (ds, dc, do):
            ctx.dev_free(p)
    case = {'frames': OP_FRAMES, 'calls_per_timing': CALLS, 'equals_oracle': same}
    for r, t in routes:
        med = float(np.median(ms[r, t]))
        name = 'r%d_t%d' % (r, t)
        case[name + '_ms_per_call'] = round(med, 4)
        case[name + '_ms_per_frame'] = round(med / OP_FRAMES, 5)
        case[name + '_spread'] = spread(ms[r, t])
        if t:
            case[name + '_over_2d'] = round(med / float(np.median(ms[r, 0])), 3)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guided_time_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(FRAMES)])
    handle = model.prepare_style(synthetic_image(2000, S, S))
    g = (VIDEO_R, EPS_Q)

    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'video_frames': FRAMES, 'eps_q': EPS_Q,
           'video_radius': VIDEO_R, 'unit': 'ms, host clock around blocking calls', 'cases': {}}
    op_case = bench_op(ctx, video[:OP_FRAMES], rounds)
    res['cases']['op_32_resident_frames'] = op_case
    print('op', op_case, flush=True)

    for batch in (8, 32):
        plain = model.predict_frames(video, handle, alpha=0.8, batch=batch)
        routes = {'plain': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch),
                  'fused_t0': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=g)}
        for t in (1, 3):
            routes['frames_t%d' % t] = lambda t=t: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=g, guided_frames=t)
            routes['filter_t%d' % t] = lambda t=t: guided_filter_time_np(plain, video, VIDEO_R, EPS_Q, t, ctx=ctx)
        first = {k: fn() for k, fn in routes.items()}                          # also the warm-up of every route
        same = bool(np.array_equal(first['plain'], plain)) and all(
            bool(np.array_equal(first['fused_t0'][i:i + 32], ctx.guided_filter_batch(plain[i:i + 32], video[i:i + 32], *g)))
            for i in range(0, FRAMES, 32)) and all(bool(np.array_equal(first['frames_t%d' % t], first['filter_t%d' % t])) for t in (1, 3))
        del first
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn) / FRAMES)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        case = {'routes_equal_the_op_on_plain': same}
        for k in routes:
            case[k + '_ms_per_frame'] = round(med[k], 4)
            case[k + '_spread'] = spread(ms[k])
        case['fused_t0_extra_ms_per_frame'] = round(med['fused_t0'] - med['plain'], 4)
        for t in (1, 3):
            extra = med['frames_t%d' % t] - med['plain']
            kernels = op_case['r%d_t%d_ms_per_frame' % (VIDEO_R, t)]
            case['frames_t%d_extra_ms_per_frame' % t] = round(extra, 4)
            case['frames_t%d_kernels_ms_per_frame' % t] = kernels
            case['frames_t%d_round_trip_ms_per_frame' % t] = round(extra - kernels, 4)
        res['cases']['video64_batch%d' % batch] = case
        print(batch, case, flush=True)
    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
