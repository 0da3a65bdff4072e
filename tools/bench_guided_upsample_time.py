"""Cost of temporal guided upsampling (guided_upsample_frames=T: the box across frames where the coefficients are formed), in one process.

    python tools/bench_guided_upsample_time.py [--rounds R] [--video-rounds R] [--out profiles/guided_upsample_time_bench.json]

The op alone: 32 resident small frames of 512 x 512, frames [6, 26) delivered at 1024 x 1024 and at 1080 x 1920;
guided_upsample_time_batch_dev at T = 1 / 2 / 3 with r = 4 and at (r, T) = (33, 3), without positions and under a +-(2, 6) zig-zag, CALLS
calls between two synchronises.  In the same rounds, on the same frames:
  a  guided_upsample_batch_dev on the 20 delivered frames (T = 0)
  b  guided_filter_time_batch_dev on frames [6, 26) of the small clip
  c  guided_filter_motion_batch_dev on the same, under the same positions
Per delivered frame the op does strictly less than a + b (a + c under motion): one pass 1 fewer, and the means in place of pass 2.
So its median must not exceed that sum by more than the spread of the rounds (the largest max - min of the routes involved, in
ms); `within_work_count` says whether it does not.
A video: 64 synthetic frames of 1080 x 1920, working size short side 512, five levels, one prepared style, host frames in, host
frames out, ms per frame:
  time_T      predict_frames(guided_upsample=(512, 4, 650), guided_upsample_frames=T), T = 1 and 3
  per_frame   predict_frames(guided_upsample=(512, 4, 650)): the per-frame upsampling, which flickers
  full_T      predict_frames(guided=(16, 650), guided_frames=T): stylized at full size and filtered along time there (the radius in
              full pixels that 4 small pixels are), the only way to this result before
and the upload of one full frame (the new route sends each twice: for the resize, and for the upsampling).
Every route is measured in R rounds; the routes alternate within a round (a host clock around calls that end in a device
synchronise).  Medians, and the spread (max - min) / median of each route's rounds.  Writes one JSON file and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd.context import Context, upsample_work_size  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

EPS_Q = 650
SMALL, CLIP, F0, F1 = 512, 32, 6, 26
FULLS = ((1024, 1024), (1080, 1920))
PARAMS = ((4, 1), (4, 2), (4, 3), (33, 3))                 # (r, T)
CALLS = 5
VIDEO, FRAMES, SIDE, R_SMALL, R_FULL = (1080, 1920), 64, 512, 4, 16


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


def bench_op(ctx, rounds):
    rng = np.random.default_rng(3000)
    c = np.stack([synthetic_image(3000 + f, SMALL, SMALL) for f in range(4)])[np.arange(CLIP) % 4]
    c = np.clip(c.astype(np.int32) + rng.integers(-3, 4, c.shape), 0, 255).astype(np.uint8)
    s = np.clip(c[..., ::-1].astype(np.int32) + rng.integers(-20, 21, c.shape), 0, 255).astype(np.uint8)
    zig = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum([[2 * (-1) ** f, 6 * (-1) ** f] for f in range(CLIP - 1)], 0)]).astype(np.int32)
    n = F1 - F0
    out = {'small': [SMALL, SMALL], 'clip_frames': CLIP, 'delivered': [F0, F1], 'calls_per_timing': CALLS, 'eps_q': EPS_Q,
           'unit': 'ms per call (20 delivered frames)', 'sizes': {}}
    ds, dc, dt = ctx.dev_alloc(s.nbytes), ctx.dev_alloc(c.nbytes), ctx.dev_alloc(s.nbytes)
    try:
        ctx.h2d(ds, s)
        ctx.h2d(dc, c)
        s0 = ds.value + F0 * SMALL * SMALL * 3
        c0 = dc.value + F0 * SMALL * SMALL * 3
        for hf, wf in FULLS:
            full = np.stack([big_image(3100 + k, hf, wf) for k in range(2)])[np.arange(n) % 2]
            df, do = ctx.dev_alloc(full.nbytes), ctx.dev_alloc(full.nbytes)
            try:
                ctx.h2d(df, full)

                def rep(fn):
                    def run():
                        for _ in range(CALLS):
                            fn()
                        ctx.sync()
                    return run

                routes = {}
                for r, t in PARAMS:
                    key = 'r%d_T%d' % (r, t)
                    routes[key + '_a'] = rep(lambda r=r: ctx.guided_upsample_batch_dev(s0, SMALL, SMALL, c0, SMALL, SMALL, df, hf, wf, n, r, EPS_Q, do))
                    routes[key + '_b'] = rep(lambda r=r, t=t: ctx.guided_filter_time_batch_dev(ds, SMALL, SMALL, dc, SMALL, SMALL, CLIP, r, EPS_Q,
                                                                                             t, F0, F1, dt))
                    routes[key + '_c'] = rep(lambda r=r, t=t: ctx.guided_filter_motion_batch_dev(ds, SMALL, SMALL, dc, SMALL, SMALL, CLIP, r, EPS_Q,
                                                                                               t, zig, F0, F1, dt))
                    routes[key + '_still'] = rep(lambda r=r, t=t: ctx.guided_upsample_time_batch_dev(
                        ds, SMALL, SMALL, dc, SMALL, SMALL, df, hf, wf, CLIP, r, EPS_Q, t, F0, F1, do))
                    routes[key + '_motion'] = rep(lambda r=r, t=t: ctx.guided_upsample_time_batch_dev(
                        ds, SMALL, SMALL, dc, SMALL, SMALL, df, hf, wf, CLIP, r, EPS_Q, t, F0, F1, do, positions=zig))
                ms = measure(routes, rounds, CALLS)
            finally:
                ctx.dev_free(df)
                ctx.dev_free(do)
            size = {}
            for r, t in PARAMS:
                key = 'r%d_T%d' % (r, t)
                med = {k: float(np.median(ms[key + '_' + k])) for k in ('a', 'b', 'c', 'still', 'motion')}
                rng_ms = {k: max(ms[key + '_' + k]) - min(ms[key + '_' + k]) for k in med}
                case = {k + '_ms': round(v, 4) for k, v in med.items()}
                case.update({k + '_spread': spread(ms[key + '_' + k]) for k in med})
                for mode, other in (('still', 'b'), ('motion', 'c')):
                    total, margin = med['a'] + med[other], max(rng_ms['a'], rng_ms[other], rng_ms[mode])
                    case[mode + '_sum_ms'] = round(total, 4)
                    case[mode + '_margin_ms'] = round(margin, 4)
                    case[mode + '_over_sum'] = round(med[mode] / total, 4)
                    case[mode + '_within_work_count'] = bool(med[mode] <= total + margin)
                case['still_ms_per_delivered_frame'] = round(med['still'] / n, 4)
                case['motion_ms_per_delivered_frame'] = round(med['motion'] / n, 4)
                size[key] = case
                print((hf, wf), key, case, flush=True)
            out['sizes']['%dx%d' % (hf, wf)] = size
    finally:
        for p in (ds, dc, dt):
            ctx.dev_free(p)
    return out


def bench_video(rounds):
    from wct_tf_amd.wct import WCT
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    handle = model.prepare_style(synthetic_image(2000, SIDE, SIDE))
    h, w = VIDEO
    base = big_image(4000, h, w + FRAMES * 4)
    video = np.stack([base[:, 4 * i:4 * i + w] for i in range(FRAMES)])             # a pan of 4 pixels per frame
    gu = (SIDE, R_SMALL, EPS_Q)
    routes = {'per_frame': lambda: model.predict_frames(video, handle, alpha=0.8, batch=16, guided_upsample=gu)}
    for t in (1, 3):
        routes['time_T%d' % t] = lambda t=t: model.predict_frames(video, handle, alpha=0.8, batch=16, guided_upsample=gu, guided_upsample_frames=t)
        routes['full_T%d' % t] = lambda t=t: model.predict_frames(video, handle, alpha=0.8, batch=16, guided=(R_FULL, EPS_Q), guided_frames=t)
    buf = ctx.dev_alloc(video[:16].nbytes)
    try:
        def upload():
            ctx.h2d(buf, video[:16])
            ctx.sync()
        routes_up = {'upload': upload}
        up = measure(routes_up, max(rounds, 5), 16)
    finally:
        ctx.dev_free(buf)
    ms = measure(routes, rounds, FRAMES)
    case = {'frame': [h, w], 'working_size': list(upsample_work_size(h, w, SIDE)), 'frames': FRAMES, 'levels': len(RELU_TARGETS), 'alpha': 0.8,
            'batch': 16, 'rounds': rounds, 'radius_small': R_SMALL, 'radius_full': R_FULL, 'eps_q': EPS_Q,
            'unit': 'ms per frame, host frames in, host frames out'}
    for k, v in ms.items():
        case[k + '_ms_per_frame'] = round(float(np.median(v)), 4)
        case[k + '_spread'] = spread(v)
    case['upload_full_frame_ms'] = round(float(np.median(up['upload'])), 4)
    case['upload_full_frame_spread'] = spread(up['upload'])
    for t in (1, 3):
        case['time_T%d_extra_over_per_frame_ms' % t] = round(case['time_T%d_ms_per_frame' % t] - case['per_frame_ms_per_frame'], 4)
        case['full_T%d_over_time_T%d' % (t, t)] = round(case['full_T%d_ms_per_frame' % t] / case['time_T%d_ms_per_frame' % t], 3)
    handle.close()
    ctx.close()
    print('video', case, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--video-rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'guided_upsample_time_bench.json'))
    ap.add_argument('--skip', nargs='*', default=[], choices=['op', 'video'])
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    res = {'rounds': rounds, 'cases': {}}
    if 'op' not in args.skip:
        ctx = Context(0)
        try:
            res['cases']['op_20_of_32_resident_frames'] = bench_op(ctx, rounds)
        finally:
            ctx.close()
    if 'video' not in args.skip:
        res['cases']['video64_1080p'] = bench_video(max(3, args.video_rounds))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
