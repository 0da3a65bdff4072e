"""Cost of a style mix: WCT.predict against WCT.predict_mix at K = 2 and 4, five levels, 512 x 512 frames.

    python tools/bench_mix.py [--iters N] [--warmup W]

Each call is timed with device events on the context's stream (warm-up, then the median of N >= 5); a profiled call of
each case then splits the time by kernel class (wct_prof_read).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512


def timed(ctx, fn, iters, warmup):
    stream = torch.cuda.ExternalStream(ctx.stream_handle())
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def profiled(ctx, fn):
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        fn()
        rec = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    return {k: round(v['ms'], 3) for k, v in rec.items() if v['launches']}


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
    cases = {'predict': lambda: model.predict(content, styles[0], alpha=0.8),
             'predict_mix_k2': lambda: model.predict_mix(content, styles[:2], alpha=0.8),
             'predict_mix_k4': lambda: model.predict_mix(content, styles, alpha=0.8)}
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'iters': iters, 'ms': {}, 'classes_ms': {}}
    for name, fn in cases.items():
        res['ms'][name] = round(timed(ctx, fn, iters, args.warmup), 3)
    for name, fn in cases.items():
        res['classes_ms'][name] = profiled(ctx, fn)
    res['k2_over_predict'] = round(res['ms']['predict_mix_k2'] / res['ms']['predict'], 3)
    res['k4_over_predict'] = round(res['ms']['predict_mix_k4'] / res['ms']['predict'], 3)
    ctx.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
