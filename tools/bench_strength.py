"""Cost of a strength map: predict_frames(strengths=maps) against plain predict_frames, in one process.

    python tools/bench_strength.py [--rounds R] [--out profiles/strength_bench.json]

64 frames at 512 x 512, five levels, one prepared style, alpha 0.8, host frames in and host frames out; one smooth map per
frame.  Two cases: device batches of 8 and of 32 frames.  Each case is measured in R >= 7 rounds; a round times the plain call
and the strength call one after the other (a host clock around calls that end in a device synchronise), the side that goes
first changing from round to round, so the two alternate in time and see the same neighbours.  Per case and side: the median over the rounds in ms per FRAME, the ratio strength / plain,
and the spread of each side's rounds, (max - min) / median -- the margin a difference has to exceed.  An all-255 map at alpha = 1
must give the plain frames (checked once per case).  With --classes the per-class device times of one call of each side
(wct_prof_read) are recorded too.  No threshold: the ratio is the finding.  Writes one JSON file and prints it.
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

S, FRAMES = 512, 64


def smooth_map(seed):
    f = np.random.default_rng(seed).standard_normal((S // 8, S // 8))
    for _ in range(4):
        f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
    f = np.kron((f - f.min()) / (f.max() - f.min()), np.ones((8, 8)))
    return np.uint8(np.round(f * 255))


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def classes_ms(model, fn):
    model.sess.prof_enable(True)
    model.sess.prof_reset()
    fn()
    out = {k: round(v['ms'], 3) for k, v in model.sess.prof_read().items() if v['launches']}
    model.sess.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--classes', action='store_true', help='also record per-class device times of one call of every side')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'strength_bench.json'))
    args = ap.parse_args()
    rounds = max(7, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(FRAMES)])
    maps = np.stack([smooth_map(4000 + i) for i in range(FRAMES)])
    ones = np.full((S, S), 255, np.uint8)
    handle = model.prepare_style(synthetic_image(2000, S, S))
    res = {'frames': FRAMES, 'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds,
           'unit': 'ms per frame, host frames in and out, host clock around blocking calls', 'cases': {}}
    for b in (8, 32):
        sides = {
            'plain': lambda: model.predict_frames(video, handle, alpha=0.8, batch=b),
            'strength': lambda: model.predict_frames(video, handle, alpha=0.8, batch=b, strengths=maps),
        }
        first = {n: fn() for n, fn in sides.items()}                          # also the warm-up of every shape
        anchor = bool(np.array_equal(model.predict_frames(video[:b], handle, alpha=1, batch=b, strengths=ones),
                                     model.predict_frames(video[:b], handle, alpha=1, batch=b)))
        t = {n: [] for n in sides}
        for r in range(rounds):                                              # the side that goes first alternates as well
            for n in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
                t[n].append(timed_ms(sides[n]) / FRAMES)
        med = {n: float(np.median(v)) for n, v in t.items()}
        case = {n + '_ms': round(v, 3) for n, v in med.items()}
        case.update(strength_over_plain=round(med['strength'] / med['plain'], 4),
                    plain_spread=round((max(t['plain']) - min(t['plain'])) / med['plain'], 4),
                    strength_spread=round((max(t['strength']) - min(t['strength'])) / med['strength'], 4),
                    rounds_ms={n: [round(v, 3) for v in t[n]] for n in t}, all_255_at_alpha_1_is_plain=anchor, frames_differ=bool(not np.array_equal(first['plain'], first['strength'])))
        if args.classes:
            case['classes_ms_per_call'] = {n: classes_ms(model, fn) for n, fn in sides.items()}
        res['cases']['batch%d' % b] = case
        print('batch%d' % b, case, flush=True)
    handle.close()
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
