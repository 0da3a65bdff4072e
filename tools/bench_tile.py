"""Seamless textures: what the wrap-around halos cost next to a plain texture, in one process.

    python tools/bench_tile.py [--rounds R] [--out profiles/tile_bench.json]

32 samples of 512 x 512, five levels, alpha 1, on one prepared style, at 1 and at 3 passes.  Two calls on the same noise:
  tile    Context.texture_prepared_wrap_batch: every encoder and decoder on the map extended by its halo, the transform on the tile
  plain   Context.texture_prepared_batch: the reflect-padded chain (it cannot produce a tile; it is the yardstick, not a competitor)
From pixel counts alone the halo costs (512 + 192)^2 / 512^2 = 1.9x at relu5_1, 1.4x at relu4_1 and 1.13x at relu1_1 .. relu3_1
in the encoders, about the same in the decoders, and nothing in the transforms.  Each call is measured in R rounds (a host clock
around calls that end in a device synchronise); the two alternate within a round, after one warm-up of each.  Per pass count: the
median ms of each, tile / plain, and the spread of each call's rounds, (max - min) / median.  Nothing is gated on the numbers.
Writes one JSON file and prints it.
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
SAMPLES = 32
SEED = 1


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: the call ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'tile_bench.json'))
    args = ap.parse_args()
    rounds = max(7, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    handle = model.prepare_style(synthetic_image(2000, S, S))
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 1, 'samples': SAMPLES, 'rounds': rounds,
           'unit': 'ms per call of %d samples, host clock around blocking calls' % SAMPLES, 'cases': {}}
    for passes in (1, 3):
        routes = {'tile': lambda: ctx.texture_prepared_wrap_batch(S, S, SAMPLES, SEED, 0, handle, RELU_TARGETS, passes=passes),
                  'plain': lambda: ctx.texture_prepared_batch(S, S, SAMPLES, SEED, 0, handle, RELU_TARGETS, passes=passes)}
        shapes = {k: list(fn().shape) for k, fn in routes.items()}              # also the warm-up of both
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        res['cases']['passes%d' % passes] = {
            'tile_ms': round(med['tile'], 3), 'plain_ms': round(med['plain'], 3), 'tile_over_plain': round(med['tile'] / med['plain'], 4),
            'tile_spread': round(spread['tile'], 4), 'plain_spread': round(spread['plain'], 4),
            'tile_rounds_ms': [round(v, 3) for v in ms['tile']], 'plain_rounds_ms': [round(v, 3) for v in ms['plain']],
            'shapes': shapes}
        print(passes, res['cases']['passes%d' % passes], flush=True)
    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
