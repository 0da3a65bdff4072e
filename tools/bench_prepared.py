"""Cost of the style side: every image-based call against its twin with prepared styles (WCT.prepare_style), in one process.

    python tools/bench_prepared.py [--rounds R] [--calls N] [--out profiles/prepared_bench.json]

Cases, five levels, 512 x 512, alpha 0.8: predict (one pair per call); predict_mix at K = 2 and K = 4; a 64-frame video
through predict_frames at batch 8 and batch 32, where the image-based call already shares one style per batch.

Each case is measured in R rounds; a round times N calls with images (a host clock around calls that end in a device
synchronise), then N calls with handles, so the two alternate in time and see the same neighbours.  Per case: the median
over the rounds for each, their ratio, and the spread of the image-based rounds, (max - min) / median -- the margin a
difference has to exceed.  The frames of the two are compared once (they must be equal).  Writes one JSON file and
prints it.
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


def per_call_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()                                   # blocking: every call ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10, help='calls per round (single-frame cases; a video case is one call)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'prepared_bench.json'))
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    content = synthetic_image(1000, S, S)
    styles = [synthetic_image(2000 + k, S, S) for k in range(4)]
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(FRAMES)])
    handles = [model.prepare_style(s) for s in styles]
    # name: (image-based call, handle-based call, calls per round)
    cases = {
        'predict': (lambda: model.predict(content, styles[0], alpha=0.8), lambda: model.predict(content, handles[0], alpha=0.8), args.calls),
        'predict_mix_k2': (lambda: model.predict_mix(content, styles[:2], [1, 2], alpha=0.8),
                           lambda: model.predict_mix(content, handles[:2], [1, 2], alpha=0.8), args.calls),
        'predict_mix_k4': (lambda: model.predict_mix(content, styles, [1, 2, 3, 4], alpha=0.8),
                           lambda: model.predict_mix(content, handles, [1, 2, 3, 4], alpha=0.8), args.calls),
        'video64_batch8': (lambda: model.predict_frames(video, styles[0], alpha=0.8, batch=8),
                           lambda: model.predict_frames(video, handles[0], alpha=0.8, batch=8), 1),
        'video64_batch32': (lambda: model.predict_frames(video, styles[0], alpha=0.8, batch=32),
                            lambda: model.predict_frames(video, handles[0], alpha=0.8, batch=32), 1),
    }
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'calls_per_round': args.calls,
           'video_frames': FRAMES, 'unit': 'ms per call, host clock around blocking calls (a video call: all %d frames)' % FRAMES,
           'cases': {}}
    for name, (with_images, with_handles, calls) in cases.items():
        same = bool(np.array_equal(with_images(), with_handles()))            # also the warm-up of both shapes
        with_images()
        with_handles()
        img, hnd = [], []
        for _ in range(rounds):
            img.append(per_call_ms(with_images, calls))
            hnd.append(per_call_ms(with_handles, calls))
        mi, mh = float(np.median(img)), float(np.median(hnd))
        res['cases'][name] = {'images_ms': round(mi, 3), 'handles_ms': round(mh, 3), 'handles_over_images': round(mh / mi, 4),
                              'images_spread': round((max(img) - min(img)) / mi, 4), 'handles_spread': round((max(hnd) - min(hnd)) / mh, 4),
                              'frames_equal': same, 'not_slower': bool(mh <= mi * (1 + (max(img) - min(img)) / mi))}
        print(name, res['cases'][name], flush=True)
    t0 = time.perf_counter()
    h = model.prepare_style(styles[1])
    res['prepare_style_ms'] = round((time.perf_counter() - t0) * 1e3, 3)
    h.close()
    for h in handles:
        h.close()
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
