"""Cost of temporal guided smoothing along camera motion: the filter beside the op without motion, the estimator alone, and the
video route, in one process.

    python tools/bench_guided_motion.py [--rounds R] [--out profiles/guided_motion_bench.json]

The filter: 32 frames of 512 x 512 resident on the device, guided_filter_motion_batch_dev on the whole clip in place under a zig-zag
of +-(2, 6) steps, beside guided_filter_time_batch_dev at the same (r, T), CALLS calls between two synchronises; the routes
alternate within a round.  ms per call, the ratio, and the spread of each route's rounds, (max - min) / median -- the margin a
difference has to exceed.  Each (r, T) is checked equal to the NumPy oracle of tests/ on the first 8 frames as a clip of their own.
The estimator: motion_global_batch_dev on the same 32 resident contents (a camera that pans by (1, 3) px per frame over one image)
at R = 4, 8, 16; every call blocks on its result, so a timing is CALLS calls.  The positions are checked against the true pan, and
against the oracle on the first 3 frames.
A 64-frame video of 512 x 512 of that pan, five levels, alpha 0.8, one prepared style, batch 32, r = 4, T = 2:
  plain        predict_frames on the prepared style
  frames_t2    guided=(4, 650), guided_frames=2: the filter along time without motion
  motion_t2    the same with guided_motion='global': the estimate (one more upload of the contents), then the filter along it
  estimate     ops.motion_global_np on the 64 contents alone: upload, kernels, the 8 F byte result
  filter_t2    ops.guided_filter_time_np(positions=...) on the plain frames alone
ms per frame of each (a host clock around calls that end in a device synchronise).  The frames of motion_t2 are checked equal to
filter_t2.  Nothing is gated on the numbers.  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import guided_motion_oracle as oracle  # noqa: E402
from wct_tf_amd.ops import guided_filter_time_np, motion_global_np  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512
FRAMES = 64
ROUTES = ((4, 1), (4, 2), (16, 2), (33, 3))
SEARCHES = (4, 8, 16)
VIDEO_R, VIDEO_T = 4, 2
EPS_Q = 650
OP_FRAMES = 32
CALLS = 10
PAN = (1, 3)


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def bench_filter(ctx, frames, rounds):
    """the filter alone on resident frames, with and without motion -> the JSON case"""
    s = frames[::-1].copy()
    pos = oracle.positions_of([(2, 6) if f % 2 == 0 else (-2, -6) for f in range(OP_FRAMES - 1)])
    ds, dc, do = ctx.dev_alloc(s.nbytes), ctx.dev_alloc(frames.nbytes), ctx.dev_alloc(s.nbytes)
    try:
        ctx.h2d(dc, frames)
        ctx.h2d(ds, s)

        def call(r, t, moving, out, n=OP_FRAMES):
            if moving:
                ctx.guided_filter_motion_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, t, pos[:n], 0, n, out)
            else:
                ctx.guided_filter_time_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, t, 0, n, out)

        same = {}
        got = np.empty_like(s[:8])
        for r, t in ROUTES:                                                   # the check: the first 8 frames as a clip, out of place
            call(r, t, True, do, 8)
            ctx.sync()
            ctx.d2h(got, do)
            same['r%d_t%d' % (r, t)] = bool(np.array_equal(got, oracle.guided_filter_motion(s[:8], frames[:8], r, EPS_Q, t, pos[:8])))
            print('filter check', r, t, same['r%d_t%d' % (r, t)], flush=True)

        def op(r, t, moving):
            for _ in range(CALLS):
                call(r, t, moving, ds)
            ctx.sync()

        keys = [(r, t, m) for r, t in ROUTES for m in (False, True)]
        for k in keys:
            op(*k)                                                            # warm-up
        ms = {k: [] for k in keys}
        for _ in range(rounds):
            for k in keys:
                ms[k].append(timed_ms(lambda: op(*k)) / CALLS)
    finally:
        for p in (ds, dc, do):
            ctx.dev_free(p)
    case = {'frames': OP_FRAMES, 'calls_per_timing': CALLS, 'steps': 'zig-zag +-(2, 6)', 'equals_oracle_on_8_frames': same}
    for r, t in ROUTES:
        still, moving = float(np.median(ms[r, t, False])), float(np.median(ms[r, t, True]))
        name = 'r%d_t%d' % (r, t)
        case[name + '_time_ms_per_call'] = round(still, 4)
        case[name + '_motion_ms_per_call'] = round(moving, 4)
        case[name + '_time_spread'] = spread(ms[r, t, False])
        case[name + '_motion_spread'] = spread(ms[r, t, True])
        case[name + '_motion_over_time'] = round(moving / still, 3)
    return case


def bench_estimator(ctx, contents, true_pos, rounds):
    """the estimator alone on resident contents -> the JSON case"""
    dc = ctx.dev_alloc(contents.nbytes)
    try:
        ctx.h2d(dc, contents)
        case = {'frames': OP_FRAMES, 'calls_per_timing': CALLS, 'pan': list(PAN)}
        got = {R: ctx.motion_global_batch_dev(dc, S, S, OP_FRAMES, R) for R in SEARCHES}        # also the warm-up
        case['finds_the_pan'] = {str(R): bool(np.array_equal(got[R], true_pos)) for R in SEARCHES}
        case['equals_oracle_on_3_frames'] = {str(R): bool(np.array_equal(got[R][:3], oracle.estimate_positions(contents[:3], R)))
                                             for R in SEARCHES}
        print('estimator check', case['finds_the_pan'], case['equals_oracle_on_3_frames'], flush=True)
        ms = {R: [] for R in SEARCHES}

        def op(R):
            for _ in range(CALLS):
                ctx.motion_global_batch_dev(dc, S, S, OP_FRAMES, R)

        for _ in range(rounds):
            for R in SEARCHES:
                ms[R].append(timed_ms(lambda: op(R)) / CALLS)
    finally:
        ctx.dev_free(dc)
    for R in SEARCHES:
        med = float(np.median(ms[R]))
        diffs = (OP_FRAMES - 1) * (2 * R + 1) ** 2 * (S // 2) * (S // 2)        # an upper count: the border cuts a few
        case['R%d_ms_per_call' % R] = round(med, 4)
        case['R%d_spread' % R] = spread(ms[R])
        case['R%d_byte_differences' % R] = diffs
        case['R%d_giga_differences_per_s' % R] = round(diffs / med / 1e6, 1)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guided_motion_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    scene = synthetic_image(3000, S + PAN[0] * FRAMES, S + PAN[1] * FRAMES)
    video = np.stack([scene[PAN[0] * f:PAN[0] * f + S, PAN[1] * f:PAN[1] * f + S] for f in range(FRAMES)])
    true_pos = oracle.positions_of([(-PAN[0], -PAN[1])] * (FRAMES - 1))
    handle = model.prepare_style(synthetic_image(2000, S, S))
    g = (VIDEO_R, EPS_Q)

    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'video_frames': FRAMES, 'eps_q': EPS_Q,
           'video_radius': VIDEO_R, 'video_frames_t': VIDEO_T, 'unit': 'ms, host clock around blocking calls', 'cases': {}}
    res['cases']['filter_32_resident_frames'] = bench_filter(ctx, video[:OP_FRAMES], rounds)
    print('filter', res['cases']['filter_32_resident_frames'], flush=True)
    res['cases']['estimator_32_resident_frames'] = bench_estimator(ctx, video[:OP_FRAMES], true_pos[:OP_FRAMES], rounds)
    print('estimator', res['cases']['estimator_32_resident_frames'], flush=True)

    batch = 32
    plain = model.predict_frames(video, handle, alpha=0.8, batch=batch)
    routes = {'plain': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch),
              'frames_t2': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=g, guided_frames=VIDEO_T),
              'motion_t2': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, guided=g, guided_frames=VIDEO_T,
                                                        guided_motion='global'),
              'estimate': lambda: motion_global_np(video, 8, ctx=ctx),
              'filter_t2': lambda: guided_filter_time_np(plain, video, VIDEO_R, EPS_Q, VIDEO_T, ctx=ctx, positions=true_pos)}
    first = {k: fn() for k, fn in routes.items()}                              # also the warm-up of every route
    case = {'estimate_finds_the_pan': bool(np.array_equal(first['estimate'], true_pos)),
            'motion_t2_equals_filter_t2': bool(np.array_equal(first['motion_t2'], first['filter_t2'])),
            'motion_t2_differs_from_frames_t2': not np.array_equal(first['motion_t2'], first['frames_t2'])}
    del first
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed_ms(fn) / FRAMES)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k in routes:
        case[k + '_ms_per_frame'] = round(med[k], 4)
        case[k + '_spread'] = spread(ms[k])
    case['frames_t2_extra_ms_per_frame'] = round(med['frames_t2'] - med['plain'], 4)
    case['motion_t2_extra_ms_per_frame'] = round(med['motion_t2'] - med['plain'], 4)
    case['motion_over_frames_t2_extra_ms_per_frame'] = round(med['motion_t2'] - med['frames_t2'], 4)
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
