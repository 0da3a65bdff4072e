"""Texture synthesis: the device pass chain against the host loop it replaces, in one process.

    python tools/bench_texture.py [--rounds R] [--out profiles/texture_bench.json]

32 samples of 512 x 512, five levels, alpha 1, on one prepared style, at 1 and at 3 passes.  Two routes to the same 32 frames:
  chain   Context.texture_prepared_batch: the noise made on the device, the passes feeding each other in device memory, one
          download of the last pass
  host    what the package offered before: NumPy noise (np.random's uint8 integers, webcam.py:192) uploaded once, predict_frames
          on the handle once per pass, the frames through the host between passes
Each route is measured in R rounds (a host clock around calls that end in a device synchronise); the routes alternate within a
round, after one warm-up of each.  Per pass count: the median ms of each route, chain / host, the spread of each route's rounds,
(max - min) / median -- the margin a difference has to exceed -- and the NumPy noise alone.  The chain's frames are checked once
against the host loop on the same noise (they must be equal).  Nothing is gated on the numbers.  Writes one JSON file and prints
it.
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
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def numpy_noise():
    return np.random.default_rng(SEED).integers(0, 256, (SAMPLES, S, S, 3), np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'texture_bench.json'))
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    handle = model.prepare_style(synthetic_image(2000, S, S))

    def host_loop(frames, passes):
        for _ in range(passes):
            frames = model.predict_frames(frames, handle, batch=SAMPLES)
        return frames

    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 1, 'samples': SAMPLES, 'rounds': rounds,
           'unit': 'ms per call of %d samples, host clock around blocking calls' % SAMPLES, 'cases': {}}
    for passes in (1, 3):
        routes = {'chain': lambda: ctx.texture_prepared_batch(S, S, SAMPLES, SEED, 0, handle, RELU_TARGETS, passes=passes),
                  'host': lambda: host_loop(numpy_noise(), passes)}
        chained = routes['chain']()                                             # also the warm-up of both
        routes['host']()
        rule_noise = np.stack([ctx.texture_noise(S, S, SEED, i) for i in range(SAMPLES)])
        same = bool(np.array_equal(chained, host_loop(rule_noise, passes)))
        ms = {k: [] for k in routes}
        noise_ms = []
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn))
            noise_ms.append(timed_ms(numpy_noise))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        res['cases']['passes%d' % passes] = {
            'chain_ms': round(med['chain'], 3), 'host_ms': round(med['host'], 3), 'chain_over_host': round(med['chain'] / med['host'], 4),
            'chain_spread': round(spread['chain'], 4), 'host_spread': round(spread['host'], 4),
            'numpy_noise_ms': round(float(np.median(noise_ms)), 3),
            'chain_rounds_ms': [round(v, 3) for v in ms['chain']], 'host_rounds_ms': [round(v, 3) for v in ms['host']],
            'chain_not_slower_than_host_beyond_spread': bool(med['chain'] <= med['host'] * (1 + max(spread.values()))),
            'chain_equals_host_loop': same}
        print(passes, res['cases']['passes%d' % passes], flush=True)
    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
