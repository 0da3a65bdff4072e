"""Cost of temporal guided smoothing with the colour guide: the op with and without motion beside the 2-D colour op and the grey
temporal op on the same frames, in one process.

    python tools/bench_guided_color_time.py [--rounds R] [--out profiles/guided_color_time_bench.json]

32 frames of 512 x 512 resident on the device, every route on the whole clip in place, CALLS calls between two synchronises; the
routes alternate within a round.  At each (r, T) of ROUTES:
  color_time    guided_filter_time_batch_dev(guide='color'): null positions
  color_motion  guided_filter_motion_batch_dev(guide='color') under a zig-zag of +-(2, 6) steps
  color_2d      guided_filter_batch_dev(guide='color') at the same radius: the per-frame colour op
  grey_time     guided_filter_time_batch_dev at the same (r, T): the grey temporal op
ms per call, the ratios, and the spread of each route's rounds, (max - min) / median -- the margin a difference has to exceed.
Each (r, T) is checked equal to the NumPy oracle of tests/ on the first 4 frames as a clip of their own, with and without motion.
Nothing is gated on the numbers.  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import guided_color_time_oracle as oracle  # noqa: E402
import guided_motion_oracle as gm  # noqa: E402
from wct_tf_amd.context import Context  # noqa: E402
from wct_tf_amd.weights import synthetic_image  # noqa: E402

S = 512
ROUTES = ((4, 1), (4, 2), (4, 3), (33, 3))
KINDS = ('color_time', 'color_motion', 'color_2d', 'grey_time')
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


def bench(ctx, frames, rounds):
    s = frames[::-1].copy()
    pos = gm.positions_of([(2, 6) if f % 2 == 0 else (-2, -6) for f in range(OP_FRAMES - 1)])
    ds, dc, do = ctx.dev_alloc(s.nbytes), ctx.dev_alloc(frames.nbytes), ctx.dev_alloc(s.nbytes)
    try:
        ctx.h2d(dc, frames)
        ctx.h2d(ds, s)

        def call(r, t, kind, out, n=OP_FRAMES):
            if kind == 'color_time':
                ctx.guided_filter_time_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, t, 0, n, out, guide='color')
            elif kind == 'color_motion':
                ctx.guided_filter_motion_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, t, pos[:n], 0, n, out, guide='color')
            elif kind == 'color_2d':
                ctx.guided_filter_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, out, guide='color')
            else:
                ctx.guided_filter_time_batch_dev(ds, S, S, dc, S, S, n, r, EPS_Q, t, 0, n, out)

        same = {}
        got = np.empty_like(s[:4])
        for r, t in ROUTES:                                                   # the check: the first 4 frames as a clip, out of place
            for kind, p in (('color_time', None), ('color_motion', pos[:4])):
                call(r, t, kind, do, 4)
                ctx.sync()
                ctx.d2h(got, do)
                name = 'r%d_t%d_%s' % (r, t, kind)
                same[name] = bool(np.array_equal(got, oracle.guided_filter(s[:4], frames[:4], r, EPS_Q, t, p)))
                print('check', name, same[name], flush=True)

        def op(r, t, kind):
            for _ in range(CALLS):
                call(r, t, kind, ds)
            ctx.sync()

        keys = [(r, t, k) for r, t in ROUTES for k in KINDS]
        for k in keys:
            op(*k)                                                            # warm-up
        ms = {k: [] for k in keys}
        for _ in range(rounds):
            for k in keys:
                ms[k].append(timed_ms(lambda: op(*k)) / CALLS)
    finally:
        for p in (ds, dc, do):
            ctx.dev_free(p)
    case = {'frames': OP_FRAMES, 'calls_per_timing': CALLS, 'steps': 'zig-zag +-(2, 6)', 'equals_oracle_on_4_frames': same}
    for r, t in ROUTES:
        name = 'r%d_t%d' % (r, t)
        med = {k: float(np.median(ms[r, t, k])) for k in KINDS}
        for k in KINDS:
            case['%s_%s_ms_per_call' % (name, k)] = round(med[k], 4)
            case['%s_%s_spread' % (name, k)] = spread(ms[r, t, k])
        case[name + '_color_motion_over_color_time'] = round(med['color_motion'] / med['color_time'], 3)
        case[name + '_color_time_over_color_2d'] = round(med['color_time'] / med['color_2d'], 3)
        case[name + '_color_time_over_grey_time'] = round(med['color_time'] / med['grey_time'], 3)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'guided_color_time_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    ctx = Context(0)
    scene = synthetic_image(3000, S + PAN[0] * OP_FRAMES, S + PAN[1] * OP_FRAMES)
    video = np.stack([scene[PAN[0] * f:PAN[0] * f + S, PAN[1] * f:PAN[1] * f + S] for f in range(OP_FRAMES)])
    res = {'frame': [S, S], 'rounds': rounds, 'eps_q': EPS_Q, 'unit': 'ms, host clock around blocking calls', 'cases': {}}
    res['cases']['filter_32_resident_frames'] = bench(ctx, video, rounds)
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
