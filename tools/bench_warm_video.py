"""Video warm start against the cold path on a slowly varying sequence, in one process.

    python tools/bench_warm_video.py [--rounds R] [--out profiles/warm_video_bench.json]

Sequence: 64 frames at 512 x 512, (1 - t) synthetic_image(a) + t synthetic_image(b) rounded to uint8, t stepping by 1 / 64; five
levels, one prepared style, alpha 0.8.  A second sequence has a hard cut: from frame 32 on the frames blend two unrelated images.

Per sequence and batch size (1 and 8) the whole video runs R rounds, each round cold and then warm (a fresh state per round), so
the two alternate in time and see the same neighbours.  Recorded: the median ms per frame of each (host clock around blocking
calls), their ratio, the spread of the cold rounds, (max - min) / median -- the margin a difference has to exceed -- and the
eigensolver's sweeps per matrix and level from eig_stats; for batch 1 also the sweeps per frame and level (the cost of the cut
shows at frame 32).  Writes one JSON file and prints it.
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


def blend(a, b, ts):
    x, y = np.float64(synthetic_image(a, S, S)), np.float64(synthetic_image(b, S, S))
    return [np.uint8(np.rint((1 - t) * x + t * y)) for t in ts]


def run(model, video, handle, batch, warm):
    """(ms per frame, {C: sweeps per matrix}) of one pass over the video"""
    model.sess.eig_stats()
    state = model.warm_state() if warm else None
    t0 = time.perf_counter()
    model.predict_frames(video, handle, alpha=0.8, batch=batch, warm=state)      # blocking per batch
    ms = (time.perf_counter() - t0) * 1e3 / len(video)
    st = model.sess.eig_stats()
    if state is not None:
        state.close()
    return ms, {str(c): round(v['sweeps'] / v['matrices'], 3) for c, v in sorted(st.items())}


def per_frame_sweeps(model, video, handle, warm):
    """batch 1: the sweeps of every frame's solves, per channel count"""
    state = model.warm_state() if warm else None
    out = []
    model.sess.eig_stats()
    for f in video:
        model.predict(f, handle, alpha=0.8, warm=state)
        out.append({str(c): v['sweeps'] for c, v in sorted(model.sess.eig_stats().items())})
    if state is not None:
        state.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'warm_video_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    ts = [i / FRAMES for i in range(FRAMES)]
    videos = {'blend': np.stack(blend(3000, 3001, ts)),
              'hard_cut_at_32': np.stack(blend(3000, 3001, ts[:32]) + blend(3002, 3003, ts[32:]))}
    handle = model.prepare_style(synthetic_image(2000, S, S))
    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'video_frames': FRAMES,
           'unit': 'ms per frame, host clock around blocking calls; sweeps per matrix by channel count (two levels have 512)', 'cases': {}}
    for name, video in videos.items():
        for batch in (1, 8):
            run(model, video[:8], handle, batch, False)                           # warm-up of both paths at this shape
            run(model, video[:8], handle, batch, True)
            cold, warm = [], []
            for _ in range(rounds):
                cold.append(run(model, video, handle, batch, False))
                warm.append(run(model, video, handle, batch, True))
            mc, mw = float(np.median([c[0] for c in cold])), float(np.median([w[0] for w in warm]))
            spread = (max(c[0] for c in cold) - min(c[0] for c in cold)) / mc
            res['cases']['%s_batch%d' % (name, batch)] = {
                'cold_ms_per_frame': round(mc, 3), 'warm_ms_per_frame': round(mw, 3), 'warm_over_cold': round(mw / mc, 4),
                'cold_spread': round(spread, 4), 'warm_faster_beyond_spread': bool(mw < mc * (1 - spread)),
                'cold_sweeps_per_matrix': cold[-1][1], 'warm_sweeps_per_matrix': warm[-1][1]}
            print(name, batch, res['cases']['%s_batch%d' % (name, batch)], flush=True)
        res['cases'][name + '_batch1']['cold_sweeps_per_frame'] = per_frame_sweeps(model, video, handle, False)
        res['cases'][name + '_batch1']['warm_sweeps_per_frame'] = per_frame_sweeps(model, video, handle, True)
    handle.close()
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({k: {m: v[m] for m in ('cold_ms_per_frame', 'warm_ms_per_frame', 'warm_over_cold', 'cold_spread')}
                      for k, v in res['cases'].items()}))


if __name__ == '__main__':
    main()
