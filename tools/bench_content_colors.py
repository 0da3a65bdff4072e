"""Cost of keeping the content's colours in a video: luminance-only transfer (--content-colors) against no colour preservation
and against the CORAL route (--keep-colors), in one process.

    python tools/bench_content_colors.py [--rounds R] [--out profiles/content_colors_bench.json]

64 frames of 512 x 512, five levels, alpha 0.8, at batch 8 and batch 32.  Three routes over the same frames:
  plain    predict_frames on a prepared style                                   (no colour preservation: the floor)
  colors   the same call with content_colors=True                               (one byte-stream launch swapped for another)
  coral    what stylize_video --keep-colors does: preserve_colors_np(style, frame) per frame, then the per-pair
           stylize_batch -- a style encoder pass and style eigensolves per frame
Each route is measured in R rounds of one pass over the video (a host clock around calls that end in a device synchronise);
the routes alternate within a round.  Per batch size: the median ms per frame of each, colors / plain, coral / colors, and the
spread of the plain rounds, (max - min) / median -- the margin a difference has to exceed.  The flagged frames are checked
once against the stand-alone op on the plain ones (they must be equal).  Nothing is gated on the numbers.  Writes one JSON
file and prints it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from wct_tf_amd.ops import preserve_colors_np  # noqa: E402
from wct_tf_amd.wct import WCT  # noqa: E402
from wct_tf_amd.weights import RELU_TARGETS, synthetic_image, synthetic_weights  # noqa: E402

S = 512
FRAMES = 64


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()                                       # blocking: every call inside ends in a device synchronise
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'content_colors_bench.json'))
    args = ap.parse_args()
    rounds = max(3, args.rounds)
    model = WCT(None, RELU_TARGETS, None, weights=synthetic_weights(42))
    style = synthetic_image(2000, S, S)
    video = np.stack([synthetic_image(3000 + i, S, S) for i in range(FRAMES)])
    handle = model.prepare_style(style)

    def coral(batch):
        outs = []
        for i in range(0, FRAMES, batch):
            group = video[i:i + batch]
            styles = np.stack([preserve_colors_np(style, f, ctx=model.sess) for f in group])
            outs.append(model.sess.stylize_batch(group, styles, RELU_TARGETS, alpha=0.8))
        return np.concatenate(outs, axis=0)

    res = {'frame': [S, S], 'levels': len(RELU_TARGETS), 'alpha': 0.8, 'rounds': rounds, 'video_frames': FRAMES,
           'unit': 'ms per frame, host clock around blocking calls over all %d frames' % FRAMES, 'cases': {}}
    for batch in (8, 32):
        routes = {'plain': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch),
                  'colors': lambda: model.predict_frames(video, handle, alpha=0.8, batch=batch, content_colors=True),
                  'coral': lambda: coral(batch)}
        plain, flagged = routes['plain'](), routes['colors']()                 # also the warm-up of both
        routes['coral']()
        same = all(bool(np.array_equal(flagged[i:i + 32], model.sess.content_colors_batch(plain[i:i + 32], video[i:i + 32])))
                   for i in range(0, FRAMES, 32))
        ms = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                ms[k].append(timed_ms(fn) / FRAMES)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res['cases']['video64_batch%d' % batch] = {
            'plain_ms_per_frame': round(med['plain'], 4), 'colors_ms_per_frame': round(med['colors'], 4),
            'coral_ms_per_frame': round(med['coral'], 4), 'colors_over_plain': round(med['colors'] / med['plain'], 4),
            'coral_over_colors': round(med['coral'] / med['colors'], 4),
            'plain_spread': round((max(ms['plain']) - min(ms['plain'])) / med['plain'], 4),
            'colors_spread': round((max(ms['colors']) - min(ms['colors'])) / med['colors'], 4),
            'coral_spread': round((max(ms['coral']) - min(ms['coral'])) / med['coral'], 4),
            'flagged_equals_op_on_plain': same}
        print(batch, res['cases']['video64_batch%d' % batch], flush=True)
    handle.close()
    model.sess.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
