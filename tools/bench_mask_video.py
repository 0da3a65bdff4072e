"""Cost of a masked video: the batched handle-based call against the per-frame loops, in one process.

    python tools/bench_mask_video.py [--rounds R] [--out profiles/mask_video_bench.json]

Cases, five levels, 512 x 512 frames, alpha 0.8: K = 2 (left / right at 3/8 | 5/8, the split DESIGN 4.6 uses) and K = 4
(quadrants), each over B = 8 and B = 32 frames that share one label map.  Three sides per case:

  loop_images   per frame predict_masked with the K style IMAGES (the baseline: what exists without this feature);
  loop_handles  per frame predict_masked with K prepared styles (what the handles bring);
  batch         ONE predict_frames_masked call over the B frames with the K prepared styles (what batching adds).

Each case is measured in R rounds; a round times the three sides one after the other (a host clock around calls that end in
a device synchronise), so they alternate in time and see the same neighbours.  Per case and side: the median over the rounds
in ms per FRAME, the ratios to the baseline, and the spread of the baseline rounds, (max - min) / median -- the margin a
difference has to exceed.  The frames of the three sides are compared once (they must be equal).  With --classes the
per-class times of one call of each side (wct_prof_read) are recorded too.  Writes one JSON file and prints it.
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


def masks_for(k):
    m = np.zeros((S, S), np.uint8)
    if k == 2:
        m[:, S * 3 // 8:] = 1
    else:
        m[:S // 2, S // 2:] = 1
        m[S // 2:, :S // 2] = 2
        m[S // 2:, S // 2:] = 3
    return m


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
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--classes', action='store_true', help='also record per-class device times of one call of every side')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'mask_video_bench.json'))
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    styles = [synthetic_image(2000 + k, S, S) for k in range(4)]
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(32)])
    handles = [model.prepare_style(s) for s in styles]
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds,
           'unit': 'ms per frame, host clock around blocking calls', 'cases': {}}
    for k in (2, 4):
        mask = masks_for(k)
        for b in (8, 32):
            frames = video[:b]
            sides = {
                'loop_images': lambda: [model.predict_masked(f, styles[:k], mask, alpha=0.8) for f in frames],
                'loop_handles': lambda: [model.predict_masked(f, handles[:k], mask, alpha=0.8) for f in frames],
                'batch': lambda: model.predict_frames_masked(frames, handles[:k], mask, alpha=0.8, batch=b),
            }
            first = {n: np.stack(fn()) for n, fn in sides.items()}             # also the warm-up of every shape
            same = bool(np.array_equal(first['loop_images'], first['loop_handles']) and np.array_equal(first['loop_images'], first['batch']))
            t = {n: [] for n in sides}
            for _ in range(rounds):
                for n, fn in sides.items():
                    t[n].append(timed_ms(fn) / b)
            med = {n: float(np.median(v)) for n, v in t.items()}
            base = med['loop_images']
            spread = (max(t['loop_images']) - min(t['loop_images'])) / base
            case = {n + '_ms': round(v, 3) for n, v in med.items()}
            case.update(loop_handles_over_baseline=round(med['loop_handles'] / base, 4), batch_over_baseline=round(med['batch'] / base, 4),
                        baseline_spread=round(spread, 4), batch_spread=round((max(t['batch']) - min(t['batch'])) / med['batch'], 4),
                        frames_equal=same, not_slower=bool(med['batch'] <= base * (1 + spread)))
            if args.classes:
                case['classes_ms_per_call'] = {n: classes_ms(model, fn) for n, fn in sides.items()}
            res['cases']['k%d_batch%d' % (k, b)] = case
            print('k%d_batch%d' % (k, b), case, flush=True)
    for h in handles:
        h.close()
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
