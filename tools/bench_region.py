"""Cost of style regions, in one process: preparing K regions of one image together against K whole-image handles, and a masked
frame on region handles against the same frame on whole-image handles.

    python tools/bench_region.py [--rounds R] [--out profiles/region_bench.json]

One 512 x 512 style, five levels, its label map K vertical bands of equal width (K = 2, 4).
  prepare_regions   prepare_style_regions(style, map, K): one upload, one encoder pass, one partition per level, K states per level
  prepare_whole     K x prepare_style(style): K uploads, K encoder passes, K states per level (what a user had before: a style per
                    region, each a whole image)
  prepare_single    K x prepare_style(style, region=(map, k)): K encoder passes and K partitions (the single-region entry point)
Each is timed with the handles closed again inside the timing (a host clock around blocking calls).
  masked_regions / masked_whole   predict_masked of one 512 x 512 content, its mask K bands the other way, alpha 0.8, on the region
                    handles and on the whole-image handles: the content side is the same code, so the two should agree within the
                    spread (the style keys differ -- n_k rows against h w -- and with them the content's partial-sum layout).
R rounds, the routes alternating within a round, after one warm-up each; medians and spreads, (max - min) / median.  Nothing is
gated on the numbers.  Writes one JSON file and prints it.
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


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return round((max(v) - min(v)) / float(np.median(v)), 4)


def close_all(handles):
    for h in handles:
        if h is not None:
            h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'region_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    style = synthetic_image(2000, S, S)
    content = synthetic_image(1000, S, S)
    res = {'style': [S, S], 'content': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds,
           'unit': 'ms, host clock around blocking calls', 'cases': {}}
    for k in (2, 4):
        smap = np.ascontiguousarray(np.broadcast_to(np.uint8(np.arange(S) * k // S)[None, :], (S, S)))
        mask = np.ascontiguousarray(smap.T)
        routes = {
            'prepare_regions': lambda: close_all(model.prepare_style_regions(style, smap, k)),
            'prepare_whole': lambda: close_all([model.prepare_style(style) for _ in range(k)]),
            'prepare_single': lambda: close_all([model.prepare_style(style, region=(smap, j)) for j in range(k)]),
        }
        regions = model.prepare_style_regions(style, smap, k)
        whole = [model.prepare_style(style) for _ in range(k)]
        routes['masked_regions'] = lambda: model.predict_masked(content, regions, mask, alpha=0.8)
        routes['masked_whole'] = lambda: model.predict_masked(content, whole, mask, alpha=0.8)
        for fn in routes.values():             # the warm-up of every route (and the states the masked calls need)
            fn()
        ms = {name: [] for name in routes}
        for _ in range(rounds):
            for name, fn in routes.items():
                ms[name].append(timed_ms(fn))
        close_all(regions + whole)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        case = {'rows_relu5_1': [int(v) * (S // 16) for v in np.bincount(smap[0, ::16], minlength=k)]}
        for name in routes:
            case[name + '_ms'] = round(med[name], 3)
            case[name + '_spread'] = spread(ms[name])
        case['prepare_regions_over_whole'] = round(med['prepare_regions'] / med['prepare_whole'], 4)
        case['prepare_regions_over_single'] = round(med['prepare_regions'] / med['prepare_single'], 4)
        case['masked_regions_over_whole'] = round(med['masked_regions'] / med['masked_whole'], 4)
        res['cases']['K%d' % k] = case
        print(k, case, flush=True)
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
