"""Banded stylization (Context.stylize_prepared_banded): what the bands cost, measured on one MI355X.

    python tools/bench_banded.py [--rounds R] [--out profiles/banded_bench.json]

Five levels on a prepared style, alpha 1, host clock around blocking calls (host image in, host frame out: the transfers are the
same in every route).
(a) a 4000 x 3000 content, which the whole-image call refuses, at band_rows 512 / 1024 / 2048 / automatic;
(b) a 2048 x 2048 content, which it takes: banded (automatic: one band per level; and 256 / 512 rows) against whole.
The routes of a case alternate within a round, after one warm-up of each; per route the median of the rounds and their spread,
(max - min) / median -- the margin a difference has to exceed.  (b) also checks that the banded frames equal the whole one.
No figure is a gate: the automatic height's cap (BAND_ROWS_CAP, csrc/banded.hip) is set from (a)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: the call ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def tiled(seed, h, w, tile=500):
    """an h x w image from one seeded tile (a 12 MP synthetic_image is seconds of NumPy)"""
    t = synthetic_image(seed, tile, tile)
    return np.ascontiguousarray(np.tile(t, (-(-h // tile), -(-w // tile), 1))[:h, :w])


def measure(routes, rounds):
    frames = {k: fn() for k, fn in routes.items()}                     # the warm-up of each, and its frame
    ms = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            ms[k].append(timed_ms(fn))
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = {'ms': round(med, 3), 'spread': round((max(v) - min(v)) / med, 4), 'rounds_ms': [round(x, 3) for x in v]}
    return out, frames


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'banded_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ctx = model.sess
    handle = model.prepare_style(synthetic_image(2000, 512, 512))
    res = {'levels': len(RELU_TARGETS), 'alpha': 1, 'rounds': rounds, 'unit': 'ms per frame, host clock around blocking calls', 'cases': {}}

    big = tiled(1000, 4000, 3000)
    auto = ctx.band_rows(4000, 3000, RELU_TARGETS)
    routes = {'band_rows_%d' % r: (lambda r=r: ctx.stylize_prepared_banded(big, handle, RELU_TARGETS, band_rows=r)) for r in (512, 1024, 2048)}
    routes['automatic'] = lambda: ctx.stylize_prepared_banded(big, handle, RELU_TARGETS, band_rows=0)
    out, frames = measure(routes, rounds)
    first = next(iter(frames.values()))
    res['cases']['4000x3000'] = {'automatic_band_rows': auto, 'routes': out,
                                 'frames_equal_across_band_rows': bool(all(np.array_equal(f, first) for f in frames.values()))}
    print(json.dumps(res['cases']['4000x3000']), flush=True)

    mid = tiled(1001, 2048, 2048)
    routes = {'whole': lambda: ctx.stylize_prepared(mid, handle, RELU_TARGETS),
              'banded_one_band': lambda: ctx.stylize_prepared_banded(mid, handle, RELU_TARGETS, band_rows=0)}
    for r in (256, 512):
        routes['banded_%d' % r] = lambda r=r: ctx.stylize_prepared_banded(mid, handle, RELU_TARGETS, band_rows=r)
    out, frames = measure(routes, rounds)
    for k in out:
        out[k]['over_whole'] = round(out[k]['ms'] / out['whole']['ms'], 4)
    res['cases']['2048x2048'] = {'routes': out, 'banded_equals_whole': bool(all(np.array_equal(f, frames['whole']) for f in frames.values()))}
    print(json.dumps(res['cases']['2048x2048']), flush=True)

    handle.close()
    ctx.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
