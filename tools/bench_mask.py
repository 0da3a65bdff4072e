"""Cost of spatial control: WCT.predict against WCT.predict_masked at K = 1, 2 and 4, five levels, 512 x 512 frames.

    python tools/bench_mask.py [--iters N] [--warmup W]

K = 1 takes an all-zero mask, K = 2 the left and right halves, K = 4 the quadrants.  Each call is timed with device events on
the context's stream (warm-up, then the median of N >= 5); a profiled call of each case then splits the time by kernel class
(wct_prof_read).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from bench_mix import timed, profiled  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    iters = max(5, args.iters)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    content = synthetic_image(1000, S, S)
    styles = [synthetic_image(2000 + k, S, S) for k in range(4)]
    halves = np.zeros((S, S), np.uint8)
    halves[:, S // 2:] = 1
    quads = np.uint8(2 * (np.arange(S)[:, None] >= S // 2) + (np.arange(S)[None, :] >= S // 2))
    cases = {'predict': lambda: model.predict(content, styles[0], alpha=0.8),
             'predict_masked_k1': lambda: model.predict_masked(content, styles[:1], np.zeros((S, S), np.uint8), alpha=0.8),
             'predict_masked_k2': lambda: model.predict_masked(content, styles[:2], halves, alpha=0.8),
             'predict_masked_k4': lambda: model.predict_masked(content, styles, quads, alpha=0.8)}
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'iters': iters, 'ms': {}, 'classes_ms': {}}
    for name, fn in cases.items():
        res['ms'][name] = round(timed(ctx, fn, iters, args.warmup), 3)
    for name, fn in cases.items():
        res['classes_ms'][name] = profiled(ctx, fn)
    for k in (1, 2, 4):
        res['k%d_over_predict' % k] = round(res['ms']['predict_masked_k%d' % k] / res['ms']['predict'], 3)
    ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
